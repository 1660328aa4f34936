"""The CPU oracle's collision detection against the float64 geometry of tests/geom64.py (no GPU).

Known-answer tests pin geom64 itself to closed forms; the batteries then hold the oracle's broadphase to a brute-force pair set
and every manifold it reports to float64 bounds (see geom64.check_manifolds).  Bounds are printed next to what was measured."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geom64 as g  # noqa: E402
from parity_util import pair_set  # noqa: E402


def f32(*x):
    """the values as the float32 records hold them (closed forms below are evaluated on exactly what geom64 sees)"""
    return [float(np.float32(v)) for v in x]


def rec(t, shape):
    r = {"type": t, "shape": np.zeros(10, np.float32)}
    r["shape"][:len(shape)] = shape
    return g.shape_from_record(r)


def test_kat_sphere_sphere():
    for c2, r1, r2 in (((3.0, 0.0, 0.0), 1.0, 1.5), ((0.5, -2.0, 1.0), 0.25, 0.75), ((0.0, 0.0, 7.0), 2.0, 2.0)):
        c2, (r1, r2) = f32(*c2), f32(r1, r2)
        d, n, err = g.signed_depth(rec(g.SPHERE, (0, 0, 0, r1)), rec(g.SPHERE, (*c2, r2)))
        exact = r1 + r2 - math.sqrt(sum(x * x for x in c2))
        assert abs(d - exact) <= 1e-9 and err <= 1e-9
        assert np.allclose(n, np.array(c2) / np.linalg.norm(c2), atol=1e-9)


def test_kat_axis_aligned_boxes():
    for lo2, hi2 in (((0.5, -1, -1), (3, 1, 1)), ((-1, 0.9, -1), (1, 2, 1)), ((2.25, 0, 0), (3, 1, 1)), ((-0.25, -0.5, 0.75), (0.25, 0.5, 1.75))):
        lo2, hi2 = f32(*lo2), f32(*hi2)
        A, B = rec(g.AABB, (-1, -1, -1, 1, 1, 1)), rec(g.AABB, (*lo2, *hi2))
        d, n, err = g.signed_depth(A, B)
        ov = np.minimum(1.0, np.array(hi2, float)) - np.maximum(-1.0, np.array(lo2, float))
        exact = ov.min() if ov.min() >= 0 else -math.sqrt(float((np.minimum(ov, 0) ** 2).sum()))
        assert abs(d - exact) <= 1e-9, (lo2, d, exact)


def test_kat_parallel_capsules():
    for dx, h1, h2, r1, r2, dy in ((0.7, 1.0, 0.5, 0.4, 0.5, 0.3), (1.2, 1.0, 1.0, 0.5, 0.5, 0.0), (0.0, 1.0, 2.0, 0.1, 0.2, 0.0), (0.3, 0.5, 0.5, 0.2, 0.2, 1.5)):
        A, B = rec(g.CAPSULE, (0, -h1, 0, 0, h1, 0, r1)), rec(g.CAPSULE, (dx, dy - h2, 0, dx, dy + h2, 0, r2))
        (dx, h1, r1, r2), (b0, b1) = f32(dx, h1, r1, r2), f32(dy - h2, dy + h2)
        gap_y = max(0.0, b0 - h1, -h1 - b1)
        exact = r1 + r2 - math.hypot(dx, gap_y)
        d, n, err = g.signed_depth(A, B)
        assert abs(d - exact) <= 1e-9, (dx, dy, d, exact)


def test_kat_sphere_box_centre_outside():
    q = (0.2, -0.3, 0.1, 0.927)
    for local, r in (((1.4, 0.2, -0.1), 0.5), ((1.3, 1.2, 0.0), 0.6), ((1.1, 0.9, 0.8), 0.3), ((-2.0, -2.0, -2.0), 0.1)):
        he = np.array(f32(1.0, 0.8, 0.6))
        r = f32(r)[0]
        for B in (rec(g.AABB, (*(-he), *he)), rec(g.OBB, (*q, 0, 0, 0, *he))):
            rot = np.eye(3) if B.kind == g.AABB else g.quat_to_matrix(np.float32(q))
            c = np.array(f32(*(rot @ np.array(local))))
            loc = rot.T @ c
            dist = float(np.linalg.norm(loc - np.clip(loc, -he, he)))
            d, n, err = g.signed_depth(rec(g.SPHERE, (*c, r)), B)
            assert abs(d - (r - dist)) <= 1e-9, (local, B.kind, d, r - dist)
            assert abs(float(g.point_signed_distance(B, c[None])[0]) - dist) <= 1e-12


def test_kat_cylinder_against_closed_forms():
    """The approximate (cylinder) depths against closed forms: parallel cylinders side by side and end on end, a cylinder on a box
    face, and a cylinder lying on a box: the stated error bound holds."""
    cases = [(rec(g.CYLINDER, (0, -1, 0, 0, 1, 0, 0.5)), rec(g.CYLINDER, (0.875, -0.5, 0, 0.875, 1.5, 0, 0.5)), 0.125),
             (rec(g.CYLINDER, (0, -1, 0, 0, 1, 0, 0.5)), rec(g.CYLINDER, (0.125, 0.9375, 0, 0.125, 2.9375, 0, 0.3125)), 0.0625),
             (rec(g.CYLINDER, (0, -1, 0, 0, 1, 0, 0.5)), rec(g.AABB, (-2, 0.75, -2, 2, 3, 2)), 0.25),
             (rec(g.CYLINDER, (-1, 0, 0, 1, 0, 0, 0.5)), rec(g.AABB, (-2, 0.4375, -2, 2, 3, 2)), 0.0625),
             (rec(g.CYLINDER, (-1, 0, 0, 1, 0, 0, 0.5)), rec(g.AABB, (-2, 0.75, -2, 2, 3, 2)), -0.25),
             (rec(g.CYLINDER, (0, -1, 0, 0, 1, 0, 0.5)), rec(g.SPHERE, (1.5, 1.5, 0, 0.75)), 0.75 - math.hypot(1.0, 0.5))]
    worst = 0.0
    for A, B, exact in cases:
        d, n, err = g.signed_depth(A, B)
        worst = max(worst, abs(d - exact))
        assert abs(d - exact) <= err, (d, exact, err)
    print("cylinder depth: worst |float64 - closed form| = %.3g (stated bound %.3g x (1 + size))" % (worst, g.CYLINDER_DEPTH_ERR_REL))


def test_kat_point_distances():
    cyl = rec(g.CYLINDER, (0, -1, 0, 0, 1, 0, 0.5))
    p = np.array([[0.0, 0.0, 0.0], [0.8, 0.0, 0.0], [0.0, 1.5, 0.0], [0.8, 1.4, 0.0], [0.2, 0.9, 0.0]])
    assert np.allclose(g.point_signed_distance(cyl, p), [-0.5, 0.3, 0.5, 0.5, -0.1], atol=1e-12)
    box = rec(g.OBB, (0, 0, 0, 1, 0, 0, 0, 1, 2, 3))
    assert np.allclose(g.point_signed_distance(box, np.array([[0, 0, 0], [2, 0, 0], [2, 3, 0], [0.5, 0, 0]])), [-1, 1, 1.4142135623730951, -0.5], atol=1e-12)


def _oracle_step(oracle, scene):
    w = scene.instantiate(oracle.OracleWorld())
    w.use_hull_geometries()
    w.step_internal(1e-9, 1)
    return w


def _tie_excused(aabbs, extra, axis):
    i = (extra & np.uint64(0xFFFFFFFF)).astype(np.int64); j = (extra >> np.uint64(32)).astype(np.int64)
    return (aabbs[i, 3 + axis] == aabbs[j, axis]) | (aabbs[j, 3 + axis] == aabbs[i, axis])


@pytest.mark.parametrize("index", range(3))
def test_oracle_broadphase_against_brute_force(oracle, index):
    """The oracle's sort-and-sweep pair set on the grid-edge worlds against the brute-force inclusive set: equal, except the pairs
    whose endpoints tie on the sorting axis, which the reference's sweep drops (parity_util.follow_step); those are counted."""
    name, scene, expect = g.broad_battery()[index]
    w = _oracle_step(oracle, scene)
    cols, aabbs = w.world_colliders()
    brute = g.brute_force_pairs(aabbs)
    got = pair_set(w.pairs())
    assert len(np.setdiff1d(got, brute)) == 0
    missing = np.setdiff1d(brute, got)
    ties = _tie_excused(aabbs, missing, w.sorting_axis()[0])
    print("%s: %d colliders, %d brute-force pairs, oracle misses %d (expected %d), all endpoint ties: %s" % (name, len(cols), len(brute), len(missing), expect["ties"], bool(ties.all())))
    assert ties.all() and len(missing) == expect["ties"]


def _run_narrow_world(oracle, scene, cases):
    w = _oracle_step(oracle, scene)
    cols, aabbs = w.world_colliders()
    cpairs, counts = w.collisions()
    contacts, _, _ = w.contacts()
    start = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    manifolds = [(a, b, contacts[start[i]:start[i + 1]]) for i, (a, b) in enumerate(cpairs) if counts[i]]
    return cols, g.check_manifolds(cols, scene.hulls, manifolds, [(c["a"], c["b"]) for c in cases])


def print_report(name, report, misses):
    for fam, r in sorted(report.items()):
        print("%s %s: %d manifolds; depth - bound <= %.3g (tol <= %.3g); point outside its depth by <= %.3g (tol); |n|-1 <= %.3g (1e-5); quirks asserted in shape: "
              "%d signed AABB depths, %d sphere centres inside a box, %d points at the reference's cylinder-cap / parallel-axes formula, %d tube-box clipping manifolds, "
              "%d parallel-flag SAT depths (face axes only); deepest float64 overlap without a manifold %.3g"
              % (name, fam, r["manifolds"], r["depth_excess"], r["max_tol"], r["point_excess"], r["normal_err"], r["aabb_signed"], r["sphere_inside_box"],
                 r.get("formula_points", 0), r.get("tube_box_clip", 0), r.get("sat_parallel", 0), r.get("missed_depth", float("nan"))))
    if misses:
        print("%s: %d coincident-centre GJK pairs without a manifold (quirk)" % (name, len(misses)))


@pytest.mark.parametrize("pair", ["%s-%s" % p for p in g.TYPE_PAIRS])
def test_oracle_narrowphase_against_float64(oracle, pair):
    """Every manifold the oracle reports on the narrowphase battery meets the float64 bounds: finite, unit normal within 1e-5,
    largest depth <= float64 depth + tol, every point within its depth + tol
    of both shapes, and a manifold wherever float64 finds an overlap > tol (tol = 1e-5 (1 + |coord| / 1 m) + the float64 value's
    stated error).  The reference's quirks are asserted in their exact shape: AABB-AABB depths signed and their points on
    centreA + radiusA - depth / 2, a sphere centre inside a box giving depth = radius along the box's +y (check_manifolds), and no
    manifold from GJK for two centrally symmetric shapes with coincident centres (assert_misses_are_gjk_coincident), sphere /
    capsule-end vs cylinder-cap points along the unnormalised normal and parallel capsule-tube points midway between the axes (at
    the reference's formula, restated in float64), tube-box contacts of the clipping branch on EPA's tilted reference plane, and
    the SAT's face-only depth when two box axes are within 0.99 (bounded by the face-only float64 depth)."""
    idx = [i for i, p in enumerate(g.TYPE_PAIRS) if "%s-%s" % p == pair][0]
    name, scene, cases = g.narrow_battery()[idx]
    oracle.stats_reset()
    cols, (report, failures, misses) = _run_narrow_world(oracle, scene, cases)
    print_report(name, report, misses)
    st = oracle.stats()
    print(name, "oracle GJK/EPA marks:", st, "caps: 64 iterations, 128 triangles, 160 edges, 32 border edges")
    assert not failures, failures[:10]
    g.assert_misses_are_gjk_coincident(misses, cols, scene.hulls)
    assert st["epa_out_of_memory"] == 0
    assert st["gjk_max_iters"] < 64 and st["epa_max_triangles"] < 128 and st["epa_max_edges"] < 160 and st["epa_max_border"] < 32
