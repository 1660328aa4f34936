"""What a contact query (mi_contact_query_batch, World.contact_query) must report, built from the oracle alone: "a collider you ask once".

expectation() is overlap64.expectation with oracle.narrowphase_ordered in place of overlap_ordered: given a fresh OracleWorld twin of the
world (a raycast_util.CastWorld instantiated into it), every query volume is added as a trigger entity at its world pose with that one
collider.  After one step_internal(1e-9, 1), world_colliders() yields the world records and boxes of the candidates and of the volumes,
bit for bit as the step builds them.  Per volume:
  1. the candidates by overlap's candidate rule (alive bodies, with `static` the entities without a rigid body, never a zone collider,
     not the excluded body range in uint32 arithmetic);
  2. the inclusive box test in numpy on the float32 boxes;
  3. oracle.narrowphase_ordered on the two world records, operand A the record of the lower collider type (after promotion), of equal
     types the volume; a contact is a pair with count > 0;
  4. the sign rule: where the collider was A the three sign bits of the normal are flipped, points and depths stay verbatim;
  5. ascending collider indices, truncation at max_hits, zeros behind; the deepest contact = the largest |depth| over all contacts, ties
     to the lower collider index (0xFFFFFFFF, 0xFFFFFFFF, 0 without a contact).
The query dtype, the pose composition and the switched-off rule are overlap64's."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geom64 as g  # noqa: E402
import overlap64 as o64  # noqa: E402

STATIC_BODY = o64.STATIC_BODY
SUMMARY_DTYPE = np.dtype([("numContacts", "<u4"), ("numWritten", "<u4"), ("valid", "<u4"), ("reserved0", "<u4"),
                          ("deepestCollider", "<u4"), ("deepestBody", "<u4"), ("deepestDepth", "<f4"), ("reserved1", "<u4")])
RECORD_DTYPE = np.dtype([("collider", "<u4"), ("body", "<u4"), ("count", "<u4"), ("reserved", "<u4"), ("normal", "<f4", 3), ("maxDepth", "<f4"),
                         ("points", "<f4", (4, 4))])


class Expected:
    """summary [n] SUMMARY_DTYPE; records [n, max_hits] RECORD_DTYPE; all [n] lists of every contact's record (untruncated, ascending);
    ordered [n] lists of (A, B, contacts as the narrowphase gave them, volume is A) per candidate that passed the box test, A and B
    indices into cols; shapes [n, 20]; cols, aabbs: the oracle twin's world colliders with the volumes behind the world's"""

    def __init__(self, n, max_hits):
        self.summary, self.records = np.zeros(n, SUMMARY_DTYPE), np.zeros((n, max_hits), RECORD_DTYPE)
        self.all, self.ordered = [[] for _ in range(n)], [[] for _ in range(n)]
        self.shapes = np.zeros((n, 20), np.float32)

    def blocks(self):
        """[n, 8 + 24 * max_hits] uint32: the bytes of dOut"""
        n, m = self.records.shape
        out = np.zeros((n, 8 + 24 * m), np.uint32)
        out[:, :8] = self.summary.view(np.uint32).reshape(n, 8)
        if m:
            out[:, 8:] = self.records.view(np.uint32).reshape(n, 24 * m)
        return out


def record_of(collider, body, contacts, volume_is_a):
    """One RECORD_DTYPE record from the narrowphase's contacts of a pair (CONTACT_DTYPE [count], count >= 1)"""
    r = np.zeros((), RECORD_DTYPE)
    r["collider"], r["body"], r["count"] = collider, body, len(contacts)
    n = contacts["normal"][0].astype(np.float32).copy()
    if not volume_is_a:
        n = (n.view(np.uint32) ^ np.uint32(0x80000000)).view(np.float32)
    r["normal"] = n
    r["maxDepth"] = np.abs(contacts["depth"]).max()
    for k, c in enumerate(contacts):
        r["points"][k, 0:3], r["points"][k, 3] = c["point"], c["depth"]
    return r


def expectation(orc, o, cw, qs, max_hits, static=True, poses=None):
    """orc: the oracle module; o: a FRESH OracleWorld that cw (raycast_util.CastWorld) was instantiated into (it is stepped here);
    qs: overlap64.QUERY_DTYPE array; poses [num bodies, 7] float32: the bodies' current poses instead of the described ones."""
    o.use_hull_geometries()
    nb = len(cw.bodies)
    described = np.array([np.concatenate([p, r]) for p, r in cw.bodies], np.float32).reshape(nb, 7)
    cur = described if poses is None else np.asarray(poses, np.float32)
    if poses is not None and nb:
        o.write_state(cur, o.velocities())
    index = {}
    for k, q in enumerate(qs):
        if o64._switched_off(q, cw, nb):
            continue
        p, r = o64.world_pose(q, cur)
        if not (np.isfinite(p).all() and np.isfinite(r).all()):
            continue
        t = o.add_trigger(p, r)
        index[k] = o.add_trigger_collider(t, int(q["type"]), q["shape"][:o64.SHAPE_WORDS[int(q["type"])]])
    o.step_internal(1e-9, 1)
    cols, aabbs = o.world_colliders()
    cand = [(i, STATIC_BODY if c["body"] is None else c["body"]) for i, c in enumerate(cw.colliders)
            if c["zone"] == 0 and ((c["body"] is None and static) or (c["body"] is not None and c["body"] not in cw.dead))]
    ci = np.array([i for i, _ in cand], np.int64)
    cb = np.array([b for _, b in cand], np.uint32)
    e = Expected(len(qs), max_hits)
    e.cols, e.aabbs = cols, aabbs
    todo = []   # (query, collider, body, A, B, volume is A)
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
        e.summary["valid"][k] = 1
        e.summary["deepestCollider"][k] = e.summary["deepestBody"][k] = 0xFFFFFFFF
        if not len(ci):
            continue
        excluded = (cb != STATIC_BODY) & ((cb - np.uint32(q["excludeFirst"])).astype(np.uint32) < np.uint32(q["excludeCount"]))
        cbox = aabbs[ci]
        meet = ~((cbox[:, 3:6] < box[0:3]) | (cbox[:, 0:3] > box[3:6])).any(axis=1) & ~excluded
        vt = int(cols["type"][v])
        for i, b in zip(ci[meet], cb[meet]):
            va = vt <= int(cols["type"][i])
            todo.append((k, int(i), int(b), v if va else int(i), int(i) if va else v, va))
    if todo:
        contacts, counts = orc.narrowphase_ordered(cols, np.array([(t[3], t[4]) for t in todo], np.uint32))
        start = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
        for n, (k, i, b, A, B, va) in enumerate(todo):
            c = contacts[start[n]:start[n + 1]].copy()
            e.ordered[k].append((A, B, c, va))
            if len(c):
                e.all[k].append(record_of(i, b, c, va))
    for k in range(len(qs)):
        recs = e.all[k]   # ascending: the candidates were met in index order
        m = min(len(recs), max_hits)
        e.summary["numContacts"][k], e.summary["numWritten"][k] = len(recs), m
        for j in range(m):
            e.records[k, j] = recs[j]
        best = None
        for r in recs:
            if best is None or r["maxDepth"] > best["maxDepth"]:
                best = r
        if best is not None:
            e.summary["deepestCollider"][k], e.summary["deepestBody"][k], e.summary["deepestDepth"][k] = best["collider"], best["body"], best["maxDepth"]
    return e


# ---- the worlds the CPU and the GPU tests share ---------------------------------------------------------------------------------
def scene_world(scene):
    """A raycast_util.CastWorld with the hulls, bodies and colliders of a scenes.Scene whose colliders all ride on bodies, same indices"""
    import raycast_util as ru
    cw = ru.CastWorld()
    for v, t in scene.hulls:
        cw.add_hull(v, t)
    for pos, rot, *_ in scene.bodies:
        cw.add_body(pos, rot)
    for body, ctype, shape, *_ in scene.colliders:
        cw.add_collider(body, ctype, shape)
    return cw


def battery_world(index):
    """(name, scene, cases, CastWorld, queries) of geom64.narrow_battery()[index] in both roles: query 2 k is collider a of case k as the
    volume, at its body's pose and blind to that body, in the world that holds b; query 2 k + 1 is collider b as the volume, blind to its
    body, in the world that holds a.  (The cases stand apart by more than their sizes: a volume's box meets its partner's alone.)"""
    name, scene, cases = g.narrow_battery()[index]
    cw = scene_world(scene)
    qs = []
    for c in cases:
        for me in (c["a"], c["b"]):
            body, ctype, shape = scene.colliders[me][0:3]
            pos, rot = scene.bodies[body][0:2]
            qs.append(o64.query(ctype, shape, pos, rot, exclude_first=body, exclude_count=1))
    return name, scene, cases, cw, o64.queries(qs)


def manifolds_of(e):
    """([(A, B, contacts)] with count > 0, [(A, B)] of every ordered pair asked) for geom64.check_manifolds on e.cols"""
    manifolds, asked = [], []
    for pairs in e.ordered:
        for A, B, c, _ in pairs:
            asked.append((A, B))
            if len(c):
                manifolds.append((A, B, c))
    return manifolds, asked
