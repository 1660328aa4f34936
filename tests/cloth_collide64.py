"""What the cloth's projection pass (mi_cloth_set_collision, csrc/k_cloth_collide.hip) must compute: the rule of include/mi_physics.h read
in float64 on proximity64.local64, its float32 restatement on proximity64.world32 in the header's operation order, the battery both are
held to, and the expectation of one internal step that the GPU tests compare the device with, byte for byte.

The reading is mi_proximity's; only the projection is stated here.  All six shapes are convex, so for a single collider the float64
signed distance of the projected point p' is the thickness: measure() reports how far the float32 rule is from that, per collider type,
relative to 1 + the largest |coordinate| of p'.  E_F32 holds the figures (test_cloth_collide64_cpu.py holds the table to its own
measurement within 1.5 x either way; DESIGN.md, "Cloth collision", quotes it); the device's tolerance is 4 x the figure."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geom64 as g64  # noqa: E402
import proximity64 as p64  # noqa: E402

f = np.float32
_v, _dot, _cross, _len, _rot, _conj = p64._v, p64._dot, p64._cross, p64._len, p64._rot, p64._conj
SPHERE, CAPSULE, CYLINDER, AABB, OBB, HULL = range(6)
STATIC_BODY, TERRAIN_COLLIDER, NO_CONTACT = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF

# |d64(p') - thickness| / (1 + max |p'|) of the float32 rule over the battery, per collider type (measure())
E_F32 = {
    "aabb": 3.2e-08,
    "capsule": 2.1e-08,
    "cylinder": 3.6e-08,
    "hull": 3.0e-08,
    "obb": 3.5e-08,
    "sphere": 2.8e-08,
}


def tolerance(type_name, p):
    """What the device's p' may miss the thickness by, in metres: 4 x the measured figure at the scale of p."""
    return 4.0 * E_F32[type_name] * (1.0 + float(np.abs(np.asarray(p, np.float64)).max()))


# ---------------------------------------------------------------------------------------------------------------------------
# The projection: float32 in the header's order, and float64
# ---------------------------------------------------------------------------------------------------------------------------
def surface_velocity32(lin, ang, c, pos, rot, local_cog):
    """vs = v_b + cross(w_b, c - cog_b), cog_b = pos_b + rot_b * localCOG_b"""
    cog = _v(_v(pos) + _rot(_v(rot), _v(local_cog)))
    return _v(_v(lin) + _cross(_v(ang), _v(_v(c) - cog)))


def project32(p, v, thickness, friction, d, n, vs):
    """(p', v') of one particle from its reading (d, n) and the surface velocity vs; v' is v itself (same bytes) unless un < 0."""
    p, v, n, vs, thickness, friction, d = _v(p), _v(v), _v(n), _v(vs), f(thickness), f(friction), f(d)
    push = f(thickness - d)
    p1 = _v(p + _v(n * push))
    u = _v(v - vs)
    un = _dot(u, n)
    if not un < 0:
        return p1, v
    u = _v(u - _v(n * un))
    jn, lt = f(-un), _len(u)
    if friction > 0:
        fj = f(friction * jn)
        s = f(f(1) - f(fj / lt)) if lt > fj else f(0)
        u = _v(u * s)
    return p1, _v(vs + u)


def project64(p, v, thickness, friction, d, n, vs):
    p, v, n, vs = (np.asarray(x, np.float64) for x in (p, v, n, vs))
    p1 = p + n * (thickness - d)
    u = v - vs
    un = float(np.dot(u, n))
    if not un < 0:
        return p1, v
    u = u - n * un
    jn, lt = -un, float(np.linalg.norm(u))
    if friction > 0:
        u = u * ((1.0 - friction * jn / lt) if lt > friction * jn else 0.0)
    return p1, vs + u


def distance64(ctype, shape10, hulls, pos, rot, point):
    """float64 signed distance of a world point (given in any precision) to one posed collider"""
    R = g64.quat_to_matrix(p64._f64(rot))
    return p64.local64(ctype, shape10, hulls, R.T @ (np.asarray(point, np.float64) - p64._f64(pos)))[0]


# ---------------------------------------------------------------------------------------------------------------------------
# The battery: points inside, on, and within the thickness of all six shapes, with four kinds of velocity
# ---------------------------------------------------------------------------------------------------------------------------
def _hull_box(hx, hy, hz):
    v = np.array([[x, y, z] for x in (-hx, hx) for y in (-hy, hy) for z in (-hz, hz)], np.float32)
    t = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.uint32)
    return v, t


HULLS = [_hull_box(0.7, 0.4, 0.5)]
THICKNESS = 0.125
COLLIDERS = [   # (type, shape10, pos, rot)
    (SPHERE, (0.1, -0.2, 0.05, 0.8, 0, 0, 0, 0, 0, 0), (1.0, 2.0, -3.0), (0.18257419, 0.36514837, 0.54772256, 0.73029674)),
    (CAPSULE, (0.0, -0.5, 0.0, 0.0, 0.5, 0.0, 0.3, 0, 0, 0), (-2.0, 1.5, 0.5), (0.5, -0.5, 0.5, 0.5)),
    (CYLINDER, (0.0, -0.4, 0.0, 0.0, 0.4, 0.0, 0.5, 0, 0, 0), (4.0, 0.5, 2.0), (0.0, 0.38268343, 0.0, 0.92387953)),
    (AABB, (-0.5, -0.4, -0.6, 0.5, 0.4, 0.6, 0, 0, 0, 0), (0.5, 3.0, 6.0), (0.0, 0.0, 0.0, 1.0)),
    (OBB, (0.25881905, 0.0, 0.0, 0.96592583, 0.1, 0.0, -0.1, 0.6, 0.3, 0.45), (-5.0, 2.5, -1.0), (0.0, 0.0, 0.38268343, 0.92387953)),
    (HULL, (0.0, 0.25881905, 0.0, 0.96592583, 0.0, 0.1, 0.0, 0.0, 0, 0), (7.0, 1.0, -4.0), (0.36514837, 0.18257419, -0.54772256, 0.73029674)),
]
VELOCITY_KINDS = ("resting", "approaching", "separating", "sliding")


class Case:
    def __init__(self, ctype, where, kind, point, velocity, friction):
        self.ctype, self.where, self.kind, self.point, self.velocity, self.friction = ctype, where, kind, np.asarray(point, np.float32), np.asarray(velocity, np.float32), friction


def battery(per_shape=24, seed=7):
    """Points at signed distances in [-0.2, thickness) of each collider (a third inside, a third on the surface to within 2e-5 m, a third
    in the shell), each with a resting, an approaching, a separating and a sliding velocity, without and with friction.  The points on
    the surface sit on its inner side: outside a box, cylinder or hull by less than a few float32 ulps of the coordinates, mi_proximity's
    n = unit(p - c) is a quotient of two rounding errors, in float32 as in any precision (a limit the projection inherits)."""
    rng = np.random.default_rng(seed)
    cases = []
    for ctype, shape, pos, rot in COLLIDERS:
        R = g64.quat_to_matrix(p64._f64(rot))
        made = 0
        for _ in range(200 * per_shape):
            if made == per_shape:
                break
            local = rng.uniform(-1.2, 1.2, 3)
            d, c, n, margin, size = p64.local64(ctype, shape, HULLS, local)
            if not (np.linalg.norm(n) > 0.5 and margin > 1e-3 * size):
                continue
            where = ("inside", "on", "within")[made % 3]
            target = {"inside": -rng.uniform(0.01, 0.2), "on": -rng.uniform(1e-5, 2e-5), "within": rng.uniform(0.01, THICKNESS - 0.01)}[where]
            q = local + n * (target - d)
            d2, c2, n2, margin2, _ = p64.local64(ctype, shape, HULLS, q)
            # moved across a branch of the rule (past the centre, to another face)?  (on the surface the margin is |d| itself: inside and
            # outside meet there and agree)
            if abs(d2 - target) > 1e-9 or (where != "on" and not margin2 > 1e-3 * size) or p64.angle(n, n2) > 1e-6:
                continue
            world, nw = R @ q + p64._f64(pos), R @ n2
            t = np.cross(nw, rng.normal(size=3)); t /= np.linalg.norm(t)
            for kind, vel in zip(VELOCITY_KINDS, (np.zeros(3), -2.0 * nw + 1.5 * t, 1.0 * nw + 0.5 * t, 1.2 * t)):
                for friction in (0.0, 0.4):
                    cases.append(Case(ctype, where, kind, world, vel, friction))
            made += 1
        assert made == per_shape, (ctype, made)
    return cases


def run32(case, vs=(0, 0, 0)):
    """The float32 rule on one case against its own collider: (d, c, n, p', v')"""
    ctype, shape, pos, rot = COLLIDERS[case.ctype]
    d, c, n = p64.world32(ctype, shape, HULLS, pos, rot, case.point)
    p1, v1 = project32(case.point, case.velocity, THICKNESS, case.friction, d, n, vs)
    return d, c, n, p1, v1


def run64(case, vs=(0, 0, 0)):
    ctype, shape, pos, rot = COLLIDERS[case.ctype]
    R = g64.quat_to_matrix(p64._f64(rot))
    d, c, n, _, _ = p64.local64(ctype, shape, HULLS, R.T @ (p64._f64(case.point) - p64._f64(pos)))
    p1, v1 = project64(p64._f64(case.point), p64._f64(case.velocity), THICKNESS, case.friction, d, R @ n, np.asarray(vs, np.float64))
    return d, R @ c + p64._f64(pos), R @ n, p1, v1


def measure():
    """{type name: largest |d64(p') - thickness| / (1 + max |p'|)} of the float32 rule over the battery"""
    worst = {}
    for case in battery():
        ctype, shape, pos, rot = COLLIDERS[case.ctype]
        p1 = run32(case)[3]
        dev = abs(distance64(ctype, shape, HULLS, pos, rot, p1.astype(np.float64)) - THICKNESS) / (1.0 + float(np.abs(p1).max()))
        name = p64.TYPE_NAMES[ctype]
        worst[name] = max(worst.get(name, 0.0), dev)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# One internal step: what a world with collision on must hold, from its twin that stepped with collision off
# ---------------------------------------------------------------------------------------------------------------------------
def expect_step(twin, cloth, fixed, thickness, friction=0.0, static=True, terrain=False, exclude=(0, 0)):
    """(positions, velocities, contacts, readings) the projection pass makes of the twin's cloth state: mi_proximity_host at the twin's
    particle positions with the flags and exclusion range mapped as the header says, the twin's body poses, velocities and local
    centres of gravity, and project32.  fixed: bool [n], the particles with invMass == 0."""
    pos, vel = twin.cloth_state(cloth)
    n = len(pos)
    readings = twin.proximity(pos, radius=thickness, exclude_first=np.full(n, exclude[0], np.uint32), exclude_count=np.full(n, exclude[1], np.uint32),
                              static=static, count=False, terrain=terrain)
    tf, bv, lcog = twin.transforms(), twin.velocities(), twin.mass_properties()[:, 0:3]
    out_p, out_v, contacts = pos.copy(), vel.copy(), np.full(n, NO_CONTACT, np.uint32)
    for i in range(n):
        r = readings[i]
        if fixed[i] or not r["found"] or not np.any(r["normal"] != 0):
            continue
        body = int(r["body"])
        vs = np.zeros(3, f) if body == STATIC_BODY else surface_velocity32(bv[body, 0:3], bv[body, 3:6], r["point"], tf[body, 0:3], tf[body, 3:7], lcog[body])
        out_p[i], out_v[i] = project32(pos[i], vel[i], thickness, friction, r["distance"], r["normal"], vs)
        contacts[i] = r["collider"]
    return out_p, out_v, contacts, readings


def fixed_mask(grid_x, grid_y):
    """the locked upper row of mi_add_cloth"""
    m = np.zeros(grid_x * grid_y, bool)
    m[:grid_x] = True
    return m
