"""What a whole-world ray cast (mi_raycast_batch, World.raycast) must report, built from ray64: the float64 reading of the reference's
ray tests, applied to every candidate collider of a world, with the cast's own hit rule on top.

A ray is [8] = origin, maxT, direction, enabled.  A candidate's test is ray64.reference_hit in the collider's frame (the body's pose, or
the static pose); it counts if 0 <= t <= maxT; the smallest t wins, of equal t the lowest collider index.  Colliders of deleted bodies,
force-field and trigger colliders are no candidates, static colliders only when asked for.

CastWorld describes a world once, for the device (mi.World), the oracle (OracleWorld) and the expectation alike."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray64 as r64  # noqa: E402

STATIC_BODY = 0xFFFFFFFF
ZONE_NONE, ZONE_FORCE_FIELD, ZONE_TRIGGER = 0, 2, 3


class CastExpected:
    """hit; collider, body (STATIC_BODY for a static collider), t of the closest hit; decided: float32 cannot flip the answer."""

    def __init__(self):
        self.hit, self.collider, self.body, self.t, self.decided = False, None, None, None, True
        self.frame = None           # (position, rotation) of the winning collider's frame, float64
        self.size = None            # its shape's size


class CastWorld:
    """bodies [(position, rotation)], colliders in index order [dict(body | None, type, shape10, pos, rot, zone)], hulls, dead bodies."""

    def __init__(self):
        self.bodies, self.colliders, self.hulls, self.dead = [], [], [], set()

    # ---- description ----
    def add_hull(self, vertices, triangles):
        self.hulls.append((np.asarray(vertices, np.float32), np.asarray(triangles, np.uint32)))
        return len(self.hulls) - 1

    def add_body(self, pos, rot=r64.IDENT):
        self.bodies.append((np.asarray(pos, np.float32), np.asarray(rot, np.float32)))
        return len(self.bodies) - 1

    def _shape(self, shape):
        s = np.zeros(10, np.float32)
        s[:len(shape)] = shape
        return s

    def add_collider(self, body, ctype, shape):
        self.colliders.append(dict(body=body, type=ctype, shape=self._shape(shape), pos=None, rot=None, zone=ZONE_NONE))
        return len(self.colliders) - 1

    def add_static(self, ctype, shape, pos=(0, 0, 0), rot=r64.IDENT, zone=ZONE_NONE):
        self.colliders.append(dict(body=None, type=ctype, shape=self._shape(shape), pos=np.asarray(pos, np.float32), rot=np.asarray(rot, np.float32), zone=zone))
        return len(self.colliders) - 1

    def add_scene(self, scene, offset=(0, 0, 0)):
        """A ray64.Scene, moved by `offset`; returns its body indices in this world."""
        off = np.asarray(offset, np.float64)
        hull_ids = [self.add_hull(v, t) for v, t in scene.hulls]
        ids = [self.add_body((p.astype(np.float64) + off).astype(np.float32), q) for p, q in scene.bodies]
        for b, t, s in scene.colliders:
            s = s.copy()
            if t == r64.HULL:
                s[7] = hull_ids[int(s[7])]
            self.add_collider(ids[b], t, s)
        self.dead.update(ids[b] for b in scene.dead)
        return ids

    # ---- the same world on the device or in the oracle ----
    def instantiate(self, world, zones=True):
        """zones=False leaves the force-field and trigger colliders out (their collider indices must then come last)."""
        for v, t in self.hulls:
            world.add_hull_geometry(v, t)
        for p, q in self.bodies:
            world.add_body(p, q, gravity_factor=0.0, linear_damping=0.0, angular_damping=0.0)
        field = trigger = None
        for i, c in enumerate(self.colliders):
            if c["zone"] == ZONE_NONE and c["body"] is not None:
                got = world.add_collider(c["body"], c["type"], c["shape"], r64.MATERIAL)
            elif c["zone"] == ZONE_NONE:
                got = world.add_static_collider(c["type"], c["shape"], r64.MATERIAL, pos=c["pos"], rot=c["rot"])
            elif not zones:
                assert all(d["zone"] != ZONE_NONE for d in self.colliders[i:])
                continue
            elif c["zone"] == ZONE_FORCE_FIELD:
                field = world.add_force_field((0.0, 5.0, 0.0), pos=c["pos"], rot=c["rot"])
                got = world.add_force_field_collider(field, c["type"], c["shape"])
            else:
                trigger = world.add_trigger(pos=c["pos"], rot=c["rot"])
                got = world.add_trigger_collider(trigger, c["type"], c["shape"])
            assert got == i, (got, i)
        for b in sorted(self.dead):
            world.delete_body(b)
        return world

    # ---- expectation ----
    def _prepared(self, i):
        """(ray64 Shape, local centre, bounding radius about it) of collider i, built once"""
        c = self.colliders[i]
        if "_prepared" not in c:
            shape = r64.shape_from_record(c["type"], c["shape"], self.hulls)
            c["_prepared"] = (shape,) + _bounding_sphere(c["type"], c["shape"], shape)
        return c["_prepared"]

    def candidates(self, static=True, poses=None):
        """[(collider, body | STATIC_BODY, prepared shape, position, rotation)]; poses [n, 7]: the bodies' current poses instead of the described ones"""
        out = []
        for i, c in enumerate(self.colliders):
            if c["zone"] != ZONE_NONE:
                continue
            if c["body"] is None:
                if static:
                    out.append((i, STATIC_BODY, self._prepared(i), c["pos"], c["rot"]))
            elif c["body"] not in self.dead:
                p, q = self.bodies[c["body"]] if poses is None else (poses[c["body"], 0:3], poses[c["body"], 3:7])
                out.append((i, c["body"], self._prepared(i), p, q))
        return out

    def expect(self, ray, static=True, poses=None):
        return expect_cast(ray, self.candidates(static, poses))


def _bounding_sphere(ctype, s, shape):
    """(centre in the collider's frame, radius) of a ball that holds the shape with room to spare (a hull's size is measured from its
    vertex mean, not from its position: twice the size covers every type)"""
    s = r64._f64(s)
    centre = {r64.SPHERE: s[0:3], r64.CAPSULE: 0.5 * (s[0:3] + s[3:6]), r64.CYLINDER: 0.5 * (s[0:3] + s[3:6]), r64.AABB: 0.5 * (s[0:3] + s[3:6]), r64.OBB: s[4:7], r64.HULL: s[4:7]}[ctype]
    return centre, 2.0 * float(shape.size)


def expect_cast(ray, candidates):
    e = CastExpected()
    ray = r64._f64(ray)
    o, max_t, d, enabled = ray[0:3], ray[3], ray[4:7], ray[7]
    if enabled == 0.0:
        return e                                                 # R7
    dl = float(np.linalg.norm(d))
    hits = []
    for c, body, (shape, centre, radius), pos, rot in candidates:
        pos, R = r64._f64(pos), r64.quat_to_matrix(r64._f64(rot))
        # a collider whose bounding ball the ray's LINE (hits behind the origin included) passes at more than half a radius cannot be hit, and
        # is more than its own size from being hit: nothing to decide
        rel = pos + R @ centre - o
        if dl > 0 and float(np.linalg.norm(rel - (rel @ d) * d / (dl * dl))) > 1.5 * radius:
            continue
        t, margin = r64.reference_hit(shape, R.T @ (o - pos), R.T @ d)
        rounding = 64 * r64.F32_EPS * (float(np.abs(o).max()) + float(np.abs(pos).max()) + shape.size) / shape.size     # as ray64.expect
        if margin <= r64.DECIDED_MARGIN + rounding:
            e.decided = False
        if t is None:
            continue
        # the cast's window [0, maxT]: a distance the rules set to exactly 0 (R1, R4) is in; one that rounding can carry over an end is undecided
        for end in (0.0, max_t):
            if math.isfinite(end) and not (t == 0.0 and end == 0.0) and abs(t - end) * dl <= (r64.DECIDED_MARGIN + rounding) * shape.size:
                e.decided = False
        if 0.0 <= t <= max_t:
            hits.append((t, c, body, pos, r64._f64(rot), shape.size))
    if not hits:
        return e
    hits.sort(key=lambda h: (h[0], h[1]))                        # R8
    t, c, body, pos, rot, size = hits[0]
    for t2, c2, *_ in hits[1:]:
        if t2 != t and abs(t2 - t) <= 1e-4 * (1 + abs(t)):
            e.decided = False                                    # two colliders nearly as close: float32 may order them the other way
    e.hit, e.collider, e.body, e.t, e.frame, e.size = True, c, body, t, (pos, rot), size
    return e


# ---------------------------------------------------------------------------------------------------------------------------
# The battery, every scene in one world
# ---------------------------------------------------------------------------------------------------------------------------
def _reach(case):
    """(centre, radius of the ball that holds the case's colliders, its ray's origin and the ray up to maxT; maxT): maxT reaches
    1.1 x as far as the farthest point of any of the scene's colliders."""
    pts, rad = [], []
    for b, t, s in case.scene.colliders:
        centre, radius = _bounding_sphere(t, s, r64.shape_from_record(t, s, case.scene.hulls))
        pts.append(r64._world_point(case.scene.bodies[b], centre))
        rad.append(radius)
    o, d = r64._f64(case.ray[0:3]), r64._f64(case.ray[4:7])
    far = max([float(np.linalg.norm(p - o)) + r for p, r in zip(pts, rad)] + [1.0])
    max_t = 1.1 * far / float(np.linalg.norm(d))
    centre = o
    radius = max([float(np.linalg.norm(p - centre)) + r for p, r in zip(pts, rad)] + [max_t * float(np.linalg.norm(d))])
    return centre, radius, max_t


def battery_world(cases):
    """(CastWorld, rays [n, 8] with maxT in slot 3, body indices per case).  Case i is moved by a whole number of metres into a ball of
    its own (see _reach); the balls sit on cubic grids, one grid per size class, so that the small cases stay near the origin."""
    reach = [_reach(c) for c in cases]
    spot, edge = {}, 0.0
    for lo, hi in ((0.0, 10.0), (10.0, 40.0), (40.0, math.inf)):       # a cubic grid per size class, the grids side by side towards -x
        members = [i for i, (_, r, _) in enumerate(reach) if lo < r <= hi]
        if not members:
            continue
        cell = 2.0 * math.ceil(max(reach[i][1] for i in members) + 1.0)
        side = math.ceil(len(members) ** (1.0 / 3.0) - 1e-9)
        for k, i in enumerate(members):
            spot[i] = np.array([edge - cell * (k % side + 0.5), cell * ((k // side) % side - 0.5 * side + 0.5), cell * (k // (side * side) - 0.5 * side + 0.5)])
        edge -= cell * side
    cw, rays, ids = CastWorld(), [], []
    for i, c in enumerate(cases):
        centre, _, max_t = reach[i]
        off = np.round(spot[i] - centre)
        ids.append(cw.add_scene(c.scene, off))
        r = c.ray.copy()
        r[0:3] = (r64._f64(c.ray[0:3]) + off).astype(np.float32)
        r[3] = np.float32(max_t)
        rays.append(r)
    return cw, np.stack(rays), ids


def single_world(case):
    """One case in a world of its own, unmoved."""
    cw = CastWorld()
    cw.add_scene(case.scene)
    return cw


def with_max_t(ray, max_t):
    r = np.array(ray, np.float32)
    r[3] = max_t
    return r


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def point_from(ray, t, pos, rot):
    """rot * (lo + t * ld) + pos in float32 numpy, the operations in the order of mi_common.h (quaternion sandwich products)."""
    f = np.float32

    def qmul(a, b):
        av, bv = a[0:3], b[0:3]
        w = f(f(a[3] * b[3]) - f(f(f(av[0] * bv[0]) + f(av[1] * bv[1])) + f(av[2] * bv[2])))
        cr = np.array([f(f(av[1] * bv[2]) - f(av[2] * bv[1])), f(f(av[2] * bv[0]) - f(av[0] * bv[2])), f(f(av[0] * bv[1]) - f(av[1] * bv[0]))], f)
        v = (av * b[3] + bv * a[3]).astype(f) + cr
        return np.array([v[0], v[1], v[2], w], f)

    def rotate(q, v):
        conj = np.array([-q[0], -q[1], -q[2], q[3]], f)
        return qmul(qmul(q, np.array([v[0], v[1], v[2], 0], f)), conj)[0:3]

    ray, pos, rot = np.asarray(ray, f), np.asarray(pos, f), np.asarray(rot, f)
    conj = np.array([-rot[0], -rot[1], -rot[2], rot[3]], f)
    lo, ld = rotate(conj, (ray[0:3] - pos).astype(f)), rotate(conj, ray[4:7])
    return (rotate(rot, (lo + f(t) * ld).astype(f)) + pos).astype(f)


# ---------------------------------------------------------------------------------------------------------------------------
# A seeded random world
# ---------------------------------------------------------------------------------------------------------------------------
RANDOM_SEED = 20261018


def _random_quat(rng):
    q = rng.normal(size=4)
    return (q / np.linalg.norm(q)).astype(np.float32)


def random_world(seed=RANDOM_SEED, num_bodies=290, num_rays=2048):
    """(CastWorld, rays [num_rays, 8]).  300 colliders of all six types (ray64._local_shape at scales 0.5 .. 1.5, every 29th body with a
    second one) on randomly posed bodies in the cube [-10, 10]^3, two of them deleted; a 60 m static ground box under the cube and
    three static boxes in it; last, so that a world without them has the same indices, a force-field sphere and a trigger box around
    the centre, where most rays pass.  Half the origins are in the cube, half 25 .. 40 m from its centre looking at a point in it;
    every fourth ray has a finite maxT, every 97th is disabled."""
    rng = np.random.default_rng(seed)
    cw = CastWorld()
    hulls = [cw.add_hull(*r64.TETRA), cw.add_hull(*r64.BRICK)]
    for j in range(num_bodies):
        b = cw.add_body(rng.uniform(-10, 10, 3), _random_quat(rng))
        for k in range(2 if j % 29 == 0 else 1):
            kind = (j + k) % 6
            cw.add_collider(b, kind, r64._local_shape(kind, scale=float(rng.uniform(0.5, 1.5)), q=_random_quat(rng), offset=rng.uniform(-0.3, 0.3, 3), hull=hulls[(j // 6) % 2]))
    cw.dead.update((7, 120))
    cw.add_static(r64.AABB, (-30, -1, -30, 30, 0, 30), pos=(0.0, -10.5, 0.0))
    for k in range(3):
        cw.add_static(r64.OBB if k == 1 else r64.AABB, r64._local_shape(r64.OBB if k == 1 else r64.AABB, scale=3.0), pos=rng.uniform(-8, 8, 3), rot=_random_quat(rng))
    cw.add_static(r64.SPHERE, (0, 0, 0, 5.0), pos=(0.5, 0.0, -0.5), zone=ZONE_FORCE_FIELD)
    cw.add_static(r64.AABB, (-6, -6, -6, 6, 6, 6), pos=(-1.0, 1.0, 0.0), zone=ZONE_TRIGGER)
    rays = np.zeros((num_rays, 8), np.float32)
    for i in range(num_rays):
        if i % 2 == 0:
            o = rng.uniform(-10, 10, 3)
            d = rng.normal(size=3)
        else:
            u = rng.normal(size=3)
            o = u / np.linalg.norm(u) * rng.uniform(25, 40)
            d = rng.uniform(-9, 9, 3) - o
        rays[i, 0:3], rays[i, 4:7] = o, d / np.linalg.norm(d)
        rays[i, 3] = rng.uniform(2, 30) if i % 4 == 3 else np.inf
        rays[i, 7] = 0.0 if i % 97 == 96 else 1.0
    return cw, rays


def oracle_casts(oracle, cw, rays):
    """[(pushed body | None, distance)] of the oracle's test_physics_interaction, one call per enabled ray, against the same bodies
    (no zone colliders); the accumulators are taken back after every push, as ray64.run_whole_world does."""
    w = cw.instantiate(oracle.OracleWorld(), zones=False)
    out = []
    for r in rays:
        if r[7] == 0.0:
            out.append((None, 0.0))
            continue
        pushed = w.test_physics_interaction(r[0:3], r[4:7], 1.0)
        dist = w.last_interaction_distance()
        if pushed is not None:
            acc = np.array(w.accumulators()[pushed], np.float32)
            w.apply_force_torque(pushed, -acc[0:3], -acc[3:6])
        out.append((pushed, dist))
    return out
