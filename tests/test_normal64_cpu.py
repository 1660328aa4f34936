"""tests/normal64.py, the float64 reading of mi_raycast_sensors' hit normal, held to closed forms; the share of the batteries whose normal
float32 cannot flip; and the distance between the rule in float32 numpy and in float64 per family (normal64.MEASURED_ANGLE, the
device's tolerance base), printed next to its bound.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normal64 as n64  # noqa: E402
import ray64 as r64  # noqa: E402
import raycast_util as rcu  # noqa: E402
import terrain_ray64 as t64  # noqa: E402

CASES = n64.battery()
INF = np.float32(np.inf)


def _one(kind, shape, ray, hulls=(), body=((0, 0, 0), r64.IDENT)):
    """Expected of one collider on one body for a world ray"""
    return n64.case_expect(r64.Case("closed-form", "x", r64.Scene([body], [(0, kind, shape)], hulls), ray))


# ---- closed forms -----------------------------------------------------------------------------------------------------------------------
def test_head_on_sphere_has_the_negated_direction():
    for d in ((1, 0, 0), (0.3, -0.5, 0.8), (-1, 2, 0.5)):
        dn = np.asarray(d, np.float64) / np.linalg.norm(d)
        e = _one(r64.SPHERE, (0, 0, 0, 0.5), r64.ray(np.array([1.0, 2.0, 3.0]) - 4 * dn, dn), body=((1, 2, 3), r64.Q_BODY))
        assert e.hit and e.decided and abs(e.t - 3.5) < 1e-6
        assert np.abs(e.normal + r64._f64(r64._unit32(dn))).max() < 1e-6, (e.normal, dn)


def test_axis_aligned_rays_hit_each_box_face():
    for kind, shape in ((r64.AABB, (-1, -0.5, -0.75, 1, 0.5, 0.75)), (r64.OBB, (0, 0, 0, 1, 0, 0, 0, 1, 0.5, 0.75))):
        for axis in range(3):
            for sign in (1.0, -1.0):
                o = np.array([0.2, 0.1, -0.15])
                o[axis] = 5.0 * sign
                d = np.zeros(3)
                d[axis] = -sign
                e = _one(kind, shape, r64.ray(o, d, unit=False))
                want = -d
                assert e.hit and e.decided and np.array_equal(e.normal, want), (kind, axis, sign, e.normal)
    # a rotated body: the face normal is the body's rotated axis
    R = r64.quat_to_matrix(r64.Q_BODY)
    e = _one(r64.AABB, (-1, -0.5, -0.75, 1, 0.5, 0.75), r64.ray(R @ np.array([0.2, 5.0, 0.1]), R @ np.array([0.0, -1.0, 0.0])), body=((0, 0, 0), r64.Q_BODY))
    assert e.hit and e.decided and np.abs(e.normal - R[:, 1]).max() < 1e-12


def test_cap_and_side_of_a_cylinder():
    cyl = (0, -1, 0, 0, 1, 0, 0.5)
    e = _one(r64.CYLINDER, cyl, r64.ray((0.1, 3, 0.1), (0.05, -1, 0.02)))
    assert e.hit and e.decided and np.array_equal(e.normal, [0, 1, 0])
    e = _one(r64.CYLINDER, cyl, r64.ray((0.2, -3, -0.1), (0, 1, 0), unit=False))
    assert e.hit and e.decided and np.array_equal(e.normal, [0, -1, 0])
    e = _one(r64.CYLINDER, cyl, r64.ray((-3, 0.2, 0.3), (1, 0, 0), unit=False))
    z = float(np.float32(0.3))                                                              # the side: radial through the hit point
    assert e.hit and e.decided and np.abs(e.normal - np.array([-math.sqrt(0.25 - z * z), 0, z]) / 0.5).max() < 1e-12, e.normal
    e = _one(r64.CYLINDER, cyl, r64.ray((1.2, 2.2, 0), (-1, -1, 0)))                      # onto the cap from outside the radius: the side test misses, the cap is hit
    assert e.hit and np.array_equal(e.normal, [0, 1, 0])
    e = _one(r64.CYLINDER, cyl, r64.ray((0.5 - 2, 1 + 2, 0), (1, -1, 0)))                 # the rim: both branches are within reach
    assert not e.decided and len(e.alternatives) == 2
    # capsule: the cylinder part is radial, the end spheres are spherical, continuous across the seam
    cap = (0, -1, 0, 0, 1, 0, 0.5)
    e = _one(r64.CAPSULE, cap, r64.ray((-3, 0.4, 0.0), (1, 0, 0), unit=False))
    assert e.hit and e.decided and np.abs(e.normal - np.array([-1.0, 0, 0])).max() < 1e-12
    e = _one(r64.CAPSULE, cap, r64.ray((0.0, 4, 0.0), (0, -1, 0), unit=False))
    assert e.hit and e.decided and np.abs(e.normal - np.array([0, 1.0, 0])).max() < 1e-12
    e = _one(r64.CAPSULE, cap, r64.ray((-3, 1.3, 0.0), (1, 0, 0), unit=False))
    y = float(np.float32(1.3)) - 1.0
    assert e.hit and e.decided and np.abs(e.normal - np.array([-math.sqrt(0.25 - y * y), y, 0]) / 0.5).max() < 1e-12, e.normal


def test_exact_ties_in_float32():
    """dc == ds on a cylinder's rim goes to the side, equal axes of a box to the lowest: the float32 restatement on exact inputs"""
    ident = ((0, 0, 0), r64.IDENT)
    cyl = np.zeros(10, np.float32)
    cyl[:7] = (0, -1, 0, 0, 1, 0, 0.5)
    n = n64.rule32(r64.CYLINDER, cyl, (), np.array([0.5, 3, 0, np.inf, 0, -1, 0, 1], np.float32), *ident, 2.0)
    assert np.array_equal(n, [1, 0, 0]), n
    box = np.zeros(10, np.float32)
    box[:6] = (-1, -0.5, -0.75, 1, 0.5, 0.75)
    n = n64.rule32(r64.AABB, box, (), np.array([3, 1.5, 2.25, np.inf, -1, -0.5, -0.75, 1], np.float32), *ident, 2.0)
    assert np.array_equal(n, [1, 0, 0]), n
    e = _one(r64.CYLINDER, (0, -1, 0, 0, 1, 0, 0.5), np.array([0.5, 3, 0, 1000, 0, -1, 0, 1], np.float32))
    assert e.hit and e.t == 2.0 and not e.decided and np.array_equal(e.normal, [1, 0, 0]) and len(e.alternatives) == 2


def test_each_tetra_face():
    v, tri = r64.TETRA
    for f, (i, j, k) in enumerate(tri):
        a, b, c = (v[m].astype(np.float64) for m in (i, j, k))
        n = np.cross(b - a, c - a)
        n /= np.linalg.norm(n)
        centre = (a + b + c) / 3.0
        assert n @ centre > 0, "the triangles face outwards"
        e = _one(r64.HULL, (0, 0, 0, 1, 0, 0, 0, 0), r64.ray(centre + 3.0 * n + np.array([0.01, -0.02, 0.015]), -n), hulls=[r64.TETRA])
        assert e.hit and e.decided and np.abs(e.normal - n).max() < 1e-12, (f, e.normal, n)
        # from inside the ray leaves through the face: the same outward normal, not flipped towards the ray
        e = _one(r64.HULL, (0, 0, 0, 1, 0, 0, 0, 0), r64.ray(0.1 * centre, n), hulls=[r64.TETRA])
        assert e.hit and np.abs(e.normal - n).max() < 1e-12, (f, e.normal, n)


def test_a_miss_has_a_zero_normal():
    e = _one(r64.SPHERE, (0, 0, 0, 0.5), r64.ray((-4, 2, 0), (1, 0, 0), unit=False))
    assert not e.hit and not np.any(e.normal)


def test_sphere_centre_and_inside():
    e = _one(r64.SPHERE, (0, 0, 0, 0.5), r64.ray((0, 0, 0), (1, 0, 0), unit=False))
    assert e.hit and e.t == 0.0 and not np.any(e.normal) and not e.decided          # at the centre the rule gives zero
    e = _one(r64.SPHERE, (0, 0, 0, 0.5), r64.ray((0, 0.25, 0), (1, 0, 0), unit=False))
    assert e.hit and e.t == 0.0 and e.decided and np.array_equal(e.normal, [0, 1, 0])   # inside: from the centre to the origin


def _flat(h):
    return t64.Terrain(1, 24.0, (-12.0, -2.0, -12.0), 6.0, {(0, 0): np.full((t64.VERTS, t64.VERTS), h, np.uint16)})


def test_terrain_flat_and_tilted():
    e = n64.terrain_expect(_flat(20000), t64.make_ray((1.03, 9.0, -2.07), (0.2, -1.0, 0.1)))
    assert e.hit and e.decided and np.array_equal(e.normal, [0, 1, 0])
    e = n64.terrain_expect(_flat(20000), t64.make_ray((1.03, -9.0, -2.07), (0.2, 1.0, 0.1)))
    assert e.hit and e.decided and np.array_equal(e.normal, [0, 1, 0]), "from below: the same normal, y > 0"
    # a plane h = gx * 100 + gz * 50 (uint16 steps per vertex): normal ~ (-dh/dx, 1, -dh/dz)
    gz, gx = np.meshgrid(np.arange(t64.VERTS), np.arange(t64.VERTS), indexing="ij")
    T = t64.Terrain(1, 24.0, (-12.0, -2.0, -12.0), 6.0, {(0, 0): (gx * 100 + gz * 50).astype(np.uint16)})
    hs, cell = 6.0 / 65535.0, 24.0 / 128
    want = np.array([-100 * hs / cell, 1.0, -50 * hs / cell])
    want /= np.linalg.norm(want)
    for ray in (t64.make_ray((1.03, 9.0, -2.07), (0.2, -1.0, 0.1)), t64.down(-3.3, 4.41)):
        e = n64.terrain_expect(T, ray)
        assert e.hit and e.decided and np.abs(e.normal - want).max() < 1e-12 and e.normal[1] > 0, (e.normal, want)
        assert np.abs(n64.terrain_triangle_normal32(T, e.triangle).astype(np.float64) - want).max() < 4 * r64.F32_EPS


# ---- the batteries ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def expected():
    return [n64.case_expect(c) for c in CASES]


def test_the_battery_is_mostly_decided(expected):
    hits = [(c, e) for c, e in zip(CASES, expected) if e.hit]
    undecided = [c.id for c, e in hits if not e.decided]
    print("%d cases, %d hit, %d of them undecided: %s" % (len(CASES), len(hits), len(undecided), undecided))
    assert all(c.knife_edge for c, e in hits if not e.decided), [c.id for c, e in hits if not e.decided and not c.knife_edge]
    assert len(hits) - len(undecided) >= 0.9 * len(hits)
    for kind in range(6):
        assert any(e.decided and rcu.single_world(c).colliders[e.collider]["type"] == kind for c, e in hits), r64.TYPE_NAMES[kind]
    fams = {c.family for c in CASES}
    assert {"normal-cap-inside-radius", "normal-box-faces", "normal-capsule-parts", "normal-far-cylinder"} <= fams
    faces = {tuple(np.round(rcu.single_world(c).bodies[0][1], 3)) + tuple(np.round(r64.quat_to_matrix(r64.Q_BODY).T @ e.normal, 2))
             for c, e in hits if c.family == "normal-box-faces" and c.name.startswith("aabb")}
    assert len(faces) == 6, faces


def test_the_terrain_battery_is_mostly_decided():
    layouts, cases = n64.terrain_battery()
    got = [(c, n64.terrain_expect(layouts[c.layout], c.ray)) for c in cases]
    hits = [(c, e) for c, e in got if e.hit]
    undecided = [c.family for c, e in hits if not e.decided]
    print("%d cases, %d hit, %d of them undecided: %s" % (len(cases), len(hits), len(undecided), undecided))
    assert len(hits) >= 60 and len(hits) - len(undecided) >= 0.9 * len(hits)
    assert all(e.normal[1] > 0 for c, e in hits)
    layouts, edges = n64.terrain_knife_edges()
    assert len(edges) >= 40 and {c.family for c in edges} == set(n64.TERRAIN_KNIFE_EDGE)


# ---- float32 against float64 ----------------------------------------------------------------------------------------------------------------
def test_float32_rule_within_the_measured_bounds(oracle, expected):
    """t32: the distance the oracle reports for the case in a world of its own, where the oracle's closest hit is the expected
    collider's body in front of the ray; elsewhere (the cast and testPhysicsInteraction differ by design: a cap disk behind the origin)
    the float64 distance rounded to float32."""
    run = r64.run_whole_world(CASES, oracle.OracleWorld, lambda w: w.accumulators(), lambda w: w.last_interaction_distance())
    worst, unit = {}, 0.0
    for c, e, (pushed, _, _, dist) in zip(CASES, expected, run):
        if not (e.hit and e.decided):
            continue
        t32 = np.float32(dist) if (pushed == e.body and dist >= 0.0) else np.float32(e.t)
        n32 = n64.case_normal32(c, e, t32).astype(np.float64)
        worst[c.family] = max(worst.get(c.family, 0.0), float(np.linalg.norm(n32 - e.normal)))
        unit = max(unit, abs(float(np.linalg.norm(n32)) - 1.0))
    print("float32 rule against float64, per family: measured | table | bound")
    for f in sorted(worst):
        print("    %-28s %.3g | %s | %s" % (f, worst[f], n64.MEASURED_ANGLE.get(f), n64.bound(f) if f in n64.MEASURED_ANGLE else None))
    assert set(worst) == set(n64.MEASURED_ANGLE), set(worst) ^ set(n64.MEASURED_ANGLE)
    for f, w in worst.items():
        assert w <= n64.bound(f), (f, w, n64.bound(f))
    assert unit <= 4 * r64.F32_EPS, unit


def test_float32_terrain_normal_within_the_measured_bounds():
    layouts, cases = n64.terrain_battery()
    worst = {}
    for c in cases:
        T = layouts[c.layout]
        e = n64.terrain_expect(T, c.ray)
        if not e.decided:
            continue
        n32 = n64.terrain_triangle_normal32(T, e.triangle).astype(np.float64)
        worst[c.family] = max(worst.get(c.family, 0.0), float(np.linalg.norm(n32 - e.normal)))
        assert abs(float(np.linalg.norm(n32)) - 1.0) <= 4 * r64.F32_EPS
    print("float32 terrain normal against float64, per family: measured | table")
    for f in sorted(worst):
        print("    %-28s %.3g | %s" % (f, worst[f], n64.MEASURED_TERRAIN_ANGLE.get(f)))
    assert set(worst) == set(n64.MEASURED_TERRAIN_ANGLE), set(worst) ^ set(n64.MEASURED_TERRAIN_ANGLE)
    for f, w in worst.items():
        assert w <= n64.terrain_bound(f), (f, w)
