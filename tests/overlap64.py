"""What an overlap query (mi_overlap_batch, World.overlap) must report, built from the oracle alone: "a trigger you ask once".

expectation(): given a fresh OracleWorld twin of the world (a raycast_util.CastWorld instantiated into it), every query volume is added
as a trigger entity at its world pose (pos, rot) with that one collider.  After one step_internal(1e-9, 1), world_colliders() yields
the world records and boxes of the candidates and of the volumes, bit for bit as the step builds them.  Per volume:
  1. the candidates by the candidate rule: colliders of alive bodies, with `static` those of entities without a rigid body, never a
     force-field or trigger collider, not the bodies b with b - excludeFirst < excludeCount in uint32 arithmetic;
  2. the inclusive box test, in numpy on the float32 boxes: not (amax < bmin or amin > bmax) on every axis;
  3. oracle.overlap_ordered on the two world records, operand A the record of the lower collider type (after promotion), of equal
     types the volume;
  4. ascending indices, their count, truncation at max_hits, zeros behind.
A query is switched off (all zero) when enabled == 0, its mount is no body or a deleted one, type >= 6, the hull index names no
geometry, or its world box is not finite.

A mounted volume's world pose is composed in float32 in the order of csrc/mi_common.h (compose32: rotation = mountRot * rot, position =
mountRot * pos + mountPos, the quaternion sandwich product); compose64 is its float64 reading."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geom64 as g  # noqa: E402

STATIC_BODY = 0xFFFFFFFF
SPHERE, CAPSULE, CYLINDER, AABB, OBB, HULL = range(6)
SHAPE_WORDS = (4, 7, 7, 6, 10, 8)   # the words mi_add_collider reads per type
QUERY_DTYPE = np.dtype([("shape", "<f4", 10), ("type", "<u4"), ("enabled", "<u4"), ("pos", "<f4", 3), ("mount", "<u4"), ("rot", "<f4", 4),
                        ("excludeFirst", "<u4"), ("excludeCount", "<u4"), ("reserved", "<u4", 2)])
IDENT = (0.0, 0.0, 0.0, 1.0)


def query(ctype, shape, pos=(0, 0, 0), rot=IDENT, mount=STATIC_BODY, exclude_first=0, exclude_count=0, enabled=1):
    q = np.zeros(1, QUERY_DTYPE)
    q["shape"][0, :len(shape)] = shape
    q["type"], q["enabled"], q["pos"], q["rot"], q["mount"] = ctype, enabled, pos, rot, mount
    q["excludeFirst"], q["excludeCount"] = exclude_first, exclude_count
    return q


def queries(items):
    return np.concatenate(items) if len(items) else np.zeros(0, QUERY_DTYPE)


# ---- pose composition ----------------------------------------------------------------------------------------------------------
def _qmul32(a, b):
    f = np.float32
    a, b = np.asarray(a, f), np.asarray(b, f)
    av, bv = a[0:3], b[0:3]
    w = f(f(a[3] * b[3]) - f(f(f(av[0] * bv[0]) + f(av[1] * bv[1])) + f(av[2] * bv[2])))
    cr = np.array([f(f(av[1] * bv[2]) - f(av[2] * bv[1])), f(f(av[2] * bv[0]) - f(av[0] * bv[2])), f(f(av[0] * bv[1]) - f(av[1] * bv[0]))], f)
    v = ((av * b[3]).astype(f) + (bv * a[3]).astype(f)).astype(f) + cr
    return np.array([v[0], v[1], v[2], w], f)


def _rotate32(q, v):
    q = np.asarray(q, np.float32)
    conj = np.array([-q[0], -q[1], -q[2], q[3]], np.float32)
    return _qmul32(_qmul32(q, np.array([v[0], v[1], v[2], 0], np.float32)), conj)[0:3]


def compose32(mount_pos, mount_rot, pos, rot):
    """(world position, world rotation) in float32, the operations in the order of csrc/mi_common.h"""
    return (_rotate32(mount_rot, np.asarray(pos, np.float32)) + np.asarray(mount_pos, np.float32)).astype(np.float32), _qmul32(mount_rot, rot)


def compose64(mount_pos, mount_rot, pos, rot):
    """The same composition in float64 on the float32 inputs as given (the mount's quaternion is not renormalised: the sandwich product
    scales by |q|^2, and so does this reading)."""
    mq, q = np.asarray(mount_rot, np.float64), np.asarray(rot, np.float64)
    n2 = float(mq @ mq)
    R = g.quat_to_matrix(mq / np.sqrt(n2)) * n2
    w = mq[3] * q[3] - mq[0:3] @ q[0:3]
    v = mq[0:3] * q[3] + q[0:3] * mq[3] + np.cross(mq[0:3], q[0:3])
    return R @ np.asarray(pos, np.float64) + np.asarray(mount_pos, np.float64), np.array([v[0], v[1], v[2], w])


# ---- the expectation ---------------------------------------------------------------------------------------------------------
class Expected:
    """summary [n, 4] uint32 = numOverlaps, numWritten, valid, 0; colliders, bodies [n, max_hits]; all [n] lists of every overlapping
    (collider, body); shapes [n, 20] float32 = the world shapes; boxpass [n] lists of the candidates that pass the box test"""

    def __init__(self, n, max_hits):
        self.summary = np.zeros((n, 4), np.uint32)
        self.colliders, self.bodies = np.zeros((n, max_hits), np.uint32), np.zeros((n, max_hits), np.uint32)
        self.all, self.boxpass = [[] for _ in range(n)], [[] for _ in range(n)]
        self.shapes = np.zeros((n, 20), np.float32)

    def blocks(self):
        """[n, 4 + 2 * max_hits] uint32: the bytes of dOut"""
        n, m = self.colliders.shape
        out = np.zeros((n, 4 + 2 * m), np.uint32)
        out[:, :4], out[:, 4::2], out[:, 5::2] = self.summary, self.colliders, self.bodies
        return out


def world_pose(q, poses):
    if q["mount"] == STATIC_BODY:
        return q["pos"].copy(), q["rot"].copy()
    m = int(q["mount"])
    return compose32(poses[m, 0:3], poses[m, 3:7], q["pos"], q["rot"])


def _switched_off(q, cw, num_bodies):
    t = int(q["type"])
    if q["enabled"] == 0 or t >= 6:
        return True
    m = int(q["mount"])
    if m != STATIC_BODY and (m >= num_bodies or m in cw.dead):
        return True
    if t == HULL and not (q["shape"][7] >= 0 and q["shape"][7] < len(cw.hulls)):
        return True
    return not (np.isfinite(q["shape"][:SHAPE_WORDS[t]]).all() and np.isfinite(q["pos"]).all() and np.isfinite(q["rot"]).all())


def expectation(orc, o, cw, qs, max_hits, static=True, poses=None):
    """orc: the oracle module; o: a FRESH OracleWorld that cw (raycast_util.CastWorld) was instantiated into (it is stepped here);
    qs: QUERY_DTYPE array; poses [num bodies, 7] float32: the bodies' current poses instead of the described ones."""
    o.use_hull_geometries()
    nb = len(cw.bodies)
    described = np.array([np.concatenate([p, r]) for p, r in cw.bodies], np.float32).reshape(nb, 7)
    cur = described if poses is None else np.asarray(poses, np.float32)
    if poses is not None and nb:
        o.write_state(cur, o.velocities())
    first = o.num_colliders
    index = {}
    for k, q in enumerate(qs):
        if _switched_off(q, cw, nb):
            continue
        p, r = world_pose(q, cur)
        if not (np.isfinite(p).all() and np.isfinite(r).all()):
            continue
        t = o.add_trigger(p, r)
        index[k] = o.add_trigger_collider(t, int(q["type"]), q["shape"][:SHAPE_WORDS[int(q["type"])]])
    o.step_internal(1e-9, 1)
    cols, aabbs = o.world_colliders()
    cand = [(i, STATIC_BODY if c["body"] is None else c["body"]) for i, c in enumerate(cw.colliders)
            if c["zone"] == 0 and ((c["body"] is None and static) or (c["body"] is not None and c["body"] not in cw.dead))]
    ci = np.array([i for i, _ in cand], np.int64)
    cb = np.array([b for _, b in cand], np.uint32)
    e = Expected(len(qs), max_hits)
    for k, q in enumerate(qs):
        if k not in index:
            continue
        v = index[k]
        box = aabbs[v]
        if not (np.isfinite(box).all() and (box[0:3] <= box[3:6]).all()):
            continue
        e.shapes[k, 0:10] = cols["shape"][v]
        e.shapes[k, 10:11].view(np.uint32)[0] = cols["type"][v]
        e.shapes[k, 12:15], e.shapes[k, 16:19] = box[0:3], box[3:6]
        e.summary[k, 2] = 1
        if not len(ci):
            continue
        excluded = (cb != STATIC_BODY) & ((cb - np.uint32(q["excludeFirst"])).astype(np.uint32) < np.uint32(q["excludeCount"]))
        cbox = aabbs[ci]
        meet = ~((cbox[:, 3:6] < box[0:3]) | (cbox[:, 0:3] > box[3:6])).any(axis=1) & ~excluded
        idx, bod = ci[meet], cb[meet]
        e.boxpass[k] = [int(i) for i in idx]
        vt = int(cols["type"][v])
        pairs = np.array([(v, i) if vt <= int(cols["type"][i]) else (i, v) for i in idx], np.uint32).reshape(-1, 2)
        hit = orc.overlap_ordered(cols, pairs) if len(pairs) else np.zeros(0, bool)
        e.all[k] = [(int(i), int(b)) for i, b, h in zip(idx, bod, hit) if h]
        m = min(len(e.all[k]), max_hits)
        e.summary[k, 0], e.summary[k, 1] = len(e.all[k]), m
        for j in range(m):
            e.colliders[k, j], e.bodies[k, j] = e.all[k][j]
    e.cols, e.aabbs = cols, aabbs
    return e


# ---- the worlds the CPU and the GPU tests share ---------------------------------------------------------------------------------
def battery_world(pairing):
    """(CastWorld, queries) of zone64's battery for one pairing: body k with its collider (index k), query k = the zone's collider at the
    zone entity's pose, world space.  The bodies of zone64.build_scene(pairing, "trigger") in the same order, without the triggers."""
    import raycast_util as ru
    import zone64 as z
    cw = ru.CastWorld()
    for v, t in z.hull_geometries():
        cw.add_hull(v, t)
    cases = z.battery()[pairing]
    for c in cases:
        cw.add_collider(cw.add_body(c.body_pos, c.body_rot), c.body[0], c.body[1])
    return cw, queries([query(c.zone[0], c.zone[1], c.zone_pos, c.zone_rot) for c in cases])


RANDOM_SEED = 20261023   # the first seed from 20261020 on for which test_overlap64_cpu.py::test_random_world_is_not_vacuous holds


def random_volumes(seed=RANDOM_SEED, n=64, num_bodies=290):
    """n volumes of all six types for raycast_util.random_world (300 colliders in the cube [-10, 10]^3 over a static ground box at
    y = -10.5 .. -11.5): type k % 6 at scales from 0.3 (most touch nothing) to 10 (many overlaps); every 4th AABB keeps the identity
    rotation and stays an AABB, the others turn into OBBs; volumes 6 .. 11 sit on the ground box, one of each type; volume 0 is a box
    that holds the whole world; every 5th is mounted on a body, every 7th excludes a random body range (one wraps around 2^32)."""
    import ray64 as r64
    import raycast_util as ru
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        kind = k % 6
        scale = float((0.3, 2.0, 6.0, 10.0)[(k // 6) % 4])
        shape = r64._local_shape(kind, scale=scale, q=ru._random_quat(rng), offset=rng.uniform(-0.2, 0.2, 3), hull=(k // 6) % 2)
        pos = rng.uniform(-9, 9, 3)
        rot = ru._random_quat(rng)
        if kind == AABB and (k // 6) % 4 != 1:
            rot = IDENT
        if 6 <= k < 12:
            pos[1] = -10.2
        mount, ef, ec = STATIC_BODY, 0, 0
        if k % 5 == 4:
            mount, pos = int(rng.integers(0, num_bodies)), rng.uniform(-2, 2, 3)
        if k % 7 == 3:
            ef, ec = int(rng.integers(0, num_bodies)), int(rng.integers(1, 120))
        if k == 17:
            ef, ec = 0xFFFFFFF0, 0x40   # bodies 2^32 - 16 .. 2^32 - 1 (none) and 0 .. 47
        out.append(query(kind, shape, pos, rot, mount, ef, ec))
    out[0] = query(AABB, (-40, -40, -40, 40, 40, 40))
    return queries(out)


def hand_world():
    """(CastWorld, names): 8 unit spheres on bodies 0 .. 7 along x at x = 0, 3, 6, ... (body 5 deleted), a static box under them, a
    static sphere at x = 30, a force-field sphere and a trigger box around everything.  Colliders 0 .. 7, 8 (box), 9 (far sphere), 10, 11."""
    import raycast_util as ru
    cw = ru.CastWorld()
    for k in range(8):
        cw.add_collider(cw.add_body((3.0 * k, 0.0, 0.0)), SPHERE, (0, 0, 0, 1.0))
    cw.dead.add(5)
    cw.add_static(AABB, (-2, -1, -2, 24, 0, 2), pos=(0.0, -1.5, 0.0))
    cw.add_static(SPHERE, (0, 0, 0, 1.0), pos=(30.0, 0.0, 0.0))
    cw.add_static(SPHERE, (0, 0, 0, 50.0), pos=(0.0, 0.0, 0.0), zone=ru.ZONE_FORCE_FIELD)
    cw.add_static(AABB, (-50, -50, -50, 50, 50, 50), pos=(0.0, 0.0, 0.0), zone=ru.ZONE_TRIGGER)
    return cw
