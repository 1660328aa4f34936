"""proximity64 itself: the float64 reading against closed forms and against geom64.point_signed_distance, the battery's classification,
and the measured float32 table the device test takes its tolerances from.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geom64 as g64  # noqa: E402
import proximity64 as p64  # noqa: E402
import ray64 as r64  # noqa: E402


def _shape(*v):
    s = np.zeros(10, np.float32); s[:len(v)] = v
    return s


def test_closed_forms():
    hulls = [r64.BRICK]
    I = (0.0, 0.0, 0.0, 1.0)
    checks = [
        # (type, shape, point, d, c, n)
        (p64.SPHERE, _shape(1, 2, 3, 0.5), (1, 2, 5), 1.5, (1, 2, 3.5), (0, 0, 1)),
        (p64.SPHERE, _shape(1, 2, 3, 0.5), (1, 2.25, 3), -0.25, (1, 2.5, 3), (0, 1, 0)),
        (p64.CAPSULE, _shape(0, 0, 0, 0, 2, 0, 0.5), (3, 1, 0), 2.5, (0.5, 1, 0), (1, 0, 0)),
        (p64.CAPSULE, _shape(0, 0, 0, 0, 2, 0, 0.5), (0, 5, 0), 2.5, (0, 2.5, 0), (0, 1, 0)),
        (p64.CAPSULE, _shape(1, 1, 1, 1, 1, 1, 0.5), (1, 1, 3), 1.5, (1, 1, 1.5), (0, 0, 1)),
        (p64.CYLINDER, _shape(0, 0, 0, 0, 2, 0, 1), (0.25, 1.75, 0), -0.25, (0.25, 2, 0), (0, 1, 0)),
        (p64.CYLINDER, _shape(0, 0, 0, 0, 2, 0, 1), (0.875, 1, 0), -0.125, (1, 1, 0), (1, 0, 0)),
        (p64.CYLINDER, _shape(0, 0, 0, 0, 2, 0, 1), (4, 6, 0), 5.0, (1, 2, 0), (0.6, 0.8, 0)),
        (p64.CYLINDER, _shape(0, 0, 0, 0, 2, 0, 1), (0.5, -3, 0), 3.0, (0.5, 0, 0), (0, -1, 0)),
        (p64.AABB, _shape(-1, -2, -3, 1, 2, 3), (0.5, 0, 0), -0.5, (1, 0, 0), (1, 0, 0)),
        (p64.AABB, _shape(-1, -2, -3, 1, 2, 3), (4, 6, 3), 5.0, (1, 2, 3), (0.6, 0.8, 0)),
        (p64.OBB, _shape(*I, 1, 1, 1, 1, 2, 3), (1, 1, 4.5), 0.5, (1, 1, 4), (0, 0, 1)),
        (p64.HULL, _shape(*I, 0, 0, 0, 0), (0, 0.25, 0), -0.25, (0, 0.5, 0), (0, 1, 0)),
        (p64.HULL, _shape(*I, 0, 0, 0, 0), (4, 4.5, 0.75), 5.0, (1, 0.5, 0.75), (0.6, 0.8, 0)),
        (p64.HULL, _shape(*I, 0, 0, 0, 0), (0.5, 0, 2.75), 2.0, (0.5, 0, 0.75), (0, 0, 1)),
    ]
    for ctype, s, p, d, c, n in checks:
        got = p64.local64(ctype, s, hulls, np.array(p, np.float64))
        assert abs(got[0] - d) <= 1e-12 and np.allclose(got[1], c, atol=1e-12, rtol=0) and np.allclose(got[2], n, atol=1e-12, rtol=0), (ctype, p, got)
        f32 = p64.local32(ctype, s, hulls, np.array(p, np.float32))
        assert abs(float(f32[0]) - d) <= 1e-6 and np.allclose(f32[1], c, atol=1e-6) and np.allclose(f32[2], n, atol=1e-6), (ctype, p, f32)


def test_point_and_normal_agree_with_geom64_distance():
    """c is on the surface (geom64 says distance 0 there), |p - c| = |d|, and p - c = d n, for every candidate of every battery query."""
    cw, cases = p64.battery()
    cands = p64.candidates(cw)
    rng = np.random.default_rng(5)
    for col, body, ctype, shape10, pos, rot in cands:
        shape = g64.shape_from_record({"type": ctype, "shape": shape10}, cw.hulls)
        for p in shape.center + rng.normal(size=(6, 3)) * shape.size * np.array([[0.2], [0.5], [1.0], [2.0], [4.0], [0.05]]):
            d, c, n, margin, size = p64.local64(ctype, shape10, cw.hulls, p)
            assert d == float(g64.point_signed_distance(shape, p[None])[0])
            scale = 1.0 + size + float(np.abs(p).max())
            assert abs(float(g64.point_signed_distance(shape, c[None])[0])) <= 1e-12 * scale, (col, p)
            assert abs(float(np.linalg.norm(p - c)) - abs(d)) <= 1e-12 * scale, (col, p)
            if margin > 1e-9 * size:
                assert float(np.linalg.norm((p - c) - d * n)) <= 1e-12 * scale and abs(float(np.linalg.norm(n)) - 1.0) <= 1e-12, (col, p)


def test_battery_is_classified_and_under_the_cap():
    cw, cases = p64.battery()
    clear, ties, undecided = p64.classify()
    assert len(cases) >= 150 and len(clear) + len(ties) + len(undecided) == len(cases)
    assert len(undecided) <= p64.UNDECIDED_CAP * len(cases)
    assert all(cases[i].family.startswith(p64.UNDECIDED_FAMILIES) for i in undecided)
    assert all(cases[i].tie[0] for i in ties)
    families = {c.family for c in cases}
    for need in ("outside", "inside", "tie-surface", "tie-centre", "edge-rim", "vertex-corner", "vertex-hull", "edge-hull", "degenerate-capsule", "outside-1cm", "outside-30m",
                 "outside@1e3", "outside@-1e3", "tie-radius-zero", "radius-inf", "radius-negative", "tie-colliders"):
        assert need in families, need
    types = {e.type for e in p64.battery_expected() if e.found}
    assert types == set(range(6))


def test_float32_restatement_decides_like_float64_on_clear_cases():
    cw, cases = p64.battery()
    clear, _, _ = p64.classify()
    cands = p64.candidates(cw)
    for i in clear:
        c, e = cases[i], p64.battery_expected()[i]
        got = [(p64.world32(ct, s, cw.hulls, pos, rot, c.point)[0], col) for col, body, ct, s, pos, rot in cands]
        within = sorted((d, col) for d, col in got if d <= c.radius)
        assert len(within) == e.within and (not within or within[0][1] == e.collider), c.id


def test_measured_float32_table():
    """proximity64.E_F32 is the measurement, within 1.5 x either way (figures below an eighth of an ulp are not held from below)."""
    measured = p64.measure_f32()
    print({k: tuple(float("%.3g" % v) for v in m) for k, m in sorted(measured.items())})
    assert set(measured) == set(p64.E_F32)
    for fam, m in measured.items():
        for got, stated in zip(m, p64.E_F32[fam]):
            assert got <= 1.5 * stated and (got >= stated / 1.5 or stated <= 0.125 * p64.F32_EPS), (fam, m, p64.E_F32[fam])
        assert all(t >= 4 * p64.F32_EPS for t in p64.tolerance(fam))
