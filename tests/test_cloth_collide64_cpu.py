"""The cloth's projection rule (include/mi_physics.h, "Cloth collision") on the CPU: the float32 restatement of cloth_collide64.py against
its float64 reading and against the closed forms, and the measured deviation table the GPU tests take their tolerance from.  Needs no GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloth_collide64 as c64  # noqa: E402
import proximity64 as p64  # noqa: E402

f = np.float32


def test_battery_covers_every_shape_place_and_velocity():
    cases = c64.battery()
    seen = {(c.ctype, c.where, c.kind, c.friction > 0) for c in cases}
    assert len(seen) == 6 * 3 * 4 * 2
    for c in cases:
        d = c64.run64(c)[0]
        assert d <= c64.THICKNESS and {"inside": d < -0.005, "on": abs(d) < 1e-4, "within": d > 0.005}[c.where], (c.ctype, c.where, d)


def test_float32_rule_follows_float64():
    """position and velocity of the float32 restatement against the float64 reading of the rule, on every case"""
    for c in c64.battery():
        d32, _, n32, p32, v32 = c64.run32(c)
        d64, _, n64, p1, v1 = c64.run64(c)
        assert abs(float(d32) - d64) <= 4e-6 and p64.angle(n32, n64) <= 2e-5, (c.ctype, c.where)
        assert np.abs(p32 - p1).max() <= 4e-6 * (1.0 + np.abs(p1).max()), (c.ctype, c.where, c.kind)
        assert np.abs(v32 - v1).max() <= 2e-4, (c.ctype, c.where, c.kind, v32, v1)   # (|v| <= 2.5 times the normal's 2e-5)


def test_deviation_table_is_the_measurement():
    """All six shapes are convex: the float64 distance of p' is the thickness.  The table of cloth_collide64.py is held to the measured
    deviation within 1.5 x either way (the GPU tests take 4 x the table)."""
    measured = c64.measure()
    print("\n".join("%-9s %.2e (table %.2e)" % (k, v, c64.E_F32[k]) for k, v in sorted(measured.items())))
    assert set(measured) == set(c64.E_F32)
    for name, dev in measured.items():
        assert c64.E_F32[name] / 1.5 <= dev <= c64.E_F32[name] * 1.5, (name, dev, c64.E_F32[name])


def test_point_inside_a_sphere_lands_at_radius_plus_thickness():
    centre, r, t = np.array([0.5, -1.0, 2.0], f), f(0.75), f(0.125)
    for p in ([0.6, -1.1, 2.2], [0.5, -0.4, 2.0], [0.9, -1.4, 1.8]):
        d, c, n = p64.world32(c64.SPHERE, (0, 0, 0, r, 0, 0, 0, 0, 0, 0), [], centre, (0, 0, 0, 1), p)
        assert d < 0
        p1, _ = c64.project32(p, (0, 0, 0), t, 0.0, d, n, (0, 0, 0))
        assert abs(np.linalg.norm(p1.astype(np.float64) - centre) - (float(r) + float(t))) <= 4 * p64.F32_EPS * 4.0


def test_point_above_a_box_face_keeps_its_tangential_coordinates():
    box = (-1.0, -0.5, -2.0, 1.0, 0.5, 2.0, 0, 0, 0, 0)
    for p in ([0.3, 0.55, -1.2], [0.3, 0.45, -1.2], [-0.9, 0.6, 1.9]):
        d, c, n = p64.world32(c64.AABB, box, [], (0, 0, 0), (0, 0, 0, 1), p)
        p1, _ = c64.project32(p, (0, 0, 0), 0.125, 0.0, d, n, (0, 0, 0))
        assert p1[0] == f(p[0]) and p1[2] == f(p[2]) and abs(float(p1[1]) - 0.625) <= 2 * p64.F32_EPS


def test_velocity_rule_closed_forms():
    n, t = np.array([0.0, 1.0, 0.0], f), 0.125
    v = np.array([1.5, -2.0, 0.5], f)
    # zero friction keeps u - n un
    _, v1 = c64.project32((0, 0, 0), v, t, 0.0, 0.1, n, (0, 0, 0))
    assert np.array_equal(v1, np.array([1.5, 0.0, 0.5], f))
    # friction >= lt / jn stops the particle relative to the surface (also a moving one)
    lt_over_jn = np.hypot(1.5, 0.5) / 2.0
    _, v1 = c64.project32((0, 0, 0), v, t, lt_over_jn * 1.0001, 0.1, n, (0, 0, 0))
    assert np.array_equal(v1, np.zeros(3, f))
    vs = np.array([0.25, 0.5, -1.0], f)
    _, v1 = c64.project32((0, 0, 0), v, t, 10.0, 0.1, n, vs)
    assert np.array_equal(v1, vs)
    # less friction scales the tangential part
    _, v1 = c64.project32((0, 0, 0), v, t, 0.25, 0.1, n, (0, 0, 0))
    s = 1.0 - 0.25 * 2.0 / np.hypot(1.5, 0.5)
    assert np.allclose(v1, [1.5 * s, 0.0, 0.5 * s], rtol=1e-6, atol=0)
    # a separating particle and a NaN keep their velocity, byte for byte; the position is still pushed
    for vel in (np.array([1.0, 2.0, 3.0], f), np.array([np.nan, 1.0, 0.0], f), np.array([1.0, 0.0, -1.0], f)):
        p1, v1 = c64.project32((1, 2, 3), vel, t, 0.5, 0.1, n, (0, 0, 0))
        assert v1.tobytes() == vel.tobytes() and np.array_equal(p1, np.array([1.0, 2.025, 3.0], f))


def test_surface_velocity_of_a_spinning_body():
    """vs = v_b + cross(w_b, c - (pos + rot * localCOG)): a body spinning about y through its centre of gravity"""
    vs = c64.surface_velocity32((1, 0, 0), (0, 2, 0), (3.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0, 0, 0, 1), (1.0, 0.5, 0.0))
    assert np.allclose(vs, [1.0, 0.0, -2.0], atol=1e-6)     # c - cog = (1, .5, 0); cross((0, 2, 0), (1, .5, 0)) = (0, 0, -2)
