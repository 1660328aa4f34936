"""cloth64.py against closed forms, and the oracle's cloth (oracle/ocloth.h) against cloth64.py one step at a time: every case of the
battery in colour order, the grids up to 27 x 19 in the reference's storage order, setWorldPositionOfFixedVertices, the battery's own
condition, and the two measurements cloth64.py records (the deviation table and colour order against storage order).  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloth64 as c64  # noqa: E402

STEPS = 40
CHECKPOINTS = (0, 1, 5, 6, 9, 19, 29, 39)   # the step before which the state is read; steps 0 and 5 are the ones taken at the two boundary dt values


# ---------------------------------------------------------------------------------------------------------------------------
# Closed forms for cloth64 itself
# ---------------------------------------------------------------------------------------------------------------------------
def _flat(gx=4, gy=5, width=1.2, height=1.5, **kw):
    c = c64.Cloth64(width, height, gx, gy, 2.0, **kw)
    return c, c.p0.copy(), np.zeros((c.n, 3), np.float32)


@pytest.mark.parametrize("gravity_factor", [1.0, 0.0, -1.0])
@pytest.mark.parametrize("damping", [0.0, 0.3, 50.0])
@pytest.mark.parametrize("dt", [1.0 / 120.0, 1.0 / 30.0, float(c64.DT_EDGE)])
def test_free_particle_without_iterations(gravity_factor, damping, dt):
    """(0, 0, 0), no wind: v = g dt gf / (1 + dt damping), and p has moved by g dt gf dt"""
    c, p, v = _flat(damping=damping, gravity_factor=gravity_factor)
    dt = float(np.float32(dt))
    p1, v1 = c64.step64(c, p, v, None, (0, 0, 0), dt)
    g = c64.GRAVITY_F32 * dt * gravity_factor
    free = np.arange(c.n) >= c.gx
    assert np.allclose(v1[free], [0.0, g / (1.0 + dt * float(np.float32(damping))), 0.0], rtol=1e-14, atol=0)
    assert np.allclose(p1[free] - p[free], [0.0, g * dt, 0.0], rtol=0, atol=1e-15)


@pytest.mark.parametrize("iterations", c64.MIXES)
@pytest.mark.parametrize("order", ["colour", "storage"])
def test_locked_particles_stay(iterations, order):
    c, p, v = _flat()
    rng = np.random.default_rng(3)
    p[c.gx:] += rng.normal(0, 0.05, (c.n - c.gx, 3)).astype(np.float32)
    p1, v1 = c64.step64(c, p, v, c64.WIND, iterations, 1.0 / 60.0, order)
    assert np.array_equal(p1[:c.gx], p[:c.gx].astype(np.float64)) and not np.any(v1[:c.gx])
    assert np.abs(p1[c.gx:] - p[c.gx:]).max() > 1e-4


def test_wind_on_a_flat_sheet():
    """two triangles per cell, each with |normal| = cell area x 2 / 2 ... summed: 2 x width x height x the wind along the normal"""
    c, p, _ = _flat(gx=7, gy=5, width=2.0, height=1.5)
    total = c64.wind_forces64(c, p.astype(np.float64), c64.WIND).sum(axis=0)
    normal = np.array([0.0, -1.0, 0.0])   # cross(bl - tl, tr - tl) of the sheet as built: it lies in the xz plane
    wind_normal = float(np.dot(np.asarray(c64.WIND, np.float32).astype(np.float64), normal))
    assert np.allclose(total, 2.0 * float(c.width) * float(c.height) * wind_normal * normal, rtol=1e-6, atol=1e-12)   # (width / height are float32, the cells sum to them within that)
    assert not np.any(c64.wind_forces64(c, p.astype(np.float64), None))


@pytest.mark.parametrize("order", ["colour", "storage"])
def test_one_stretched_constraint(order):
    """two free particles of equal mass at stiffness 1: one position solve takes length L to 2 L r^2 / (r^2 + L^2)"""
    c = c64.Cloth64(1.0, 1.0, 2, 2, 4.0, stiffness=1.0, damping=0.0, gravity_factor=0.0)
    lower = (c.a == 2) & (c.b == 3)   # the stretch constraint of the free row; drop the others
    c.a, c.b, c.rest, c.rest32, c.ims, c.ims32, c.colour = (x[lower] for x in (c.a, c.b, c.rest, c.rest32, c.ims, c.ims32, c.colour))
    c.colours = [np.nonzero(c.colour == k)[0] for k in range(12)]
    r, L = float(c.rest[0]), 1.375
    p = c.p0.copy(); p[3, 0] = p[2, 0] + np.float32(L)
    p1, v1 = c64.step64(c, p, np.zeros((4, 3), np.float32), None, (0, 1, 0), 1.0 / 60.0, order)
    assert math.isclose(np.linalg.norm(p1[3] - p1[2]), 2.0 * L * r * r / (r * r + L * L), rel_tol=1e-14)
    assert np.allclose(p1[2] + p1[3], p[2].astype(np.float64) + p[3], atol=1e-15)   # equal masses: the middle stays
    assert np.allclose(v1[2], (p1[2] - p[2]) / float(np.float32(1.0 / 60.0)), rtol=1e-12)


@pytest.mark.parametrize("gx", [4, 5])
@pytest.mark.parametrize("rot", [(0.18257419, 0.36514837, 0.54772256, 0.73029674), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)])
def test_rigid_bar_move_preserves_distances(gx, rot):
    c, p, _ = _flat(gx=gx)
    rng = np.random.default_rng(5)
    p[c.gx:] += rng.normal(0, 0.1, (c.n - c.gx, 3)).astype(np.float32)
    q = c64.set_fixed64(c, p, (1.0, 2.0, -3.0), rot, True)
    lower0, lower1 = p[c.gx:].astype(np.float64), q[c.gx:]
    d0 = np.linalg.norm(lower0[:, None] - lower0[None], axis=2); d1 = np.linalg.norm(lower1[:, None] - lower1[None], axis=2)
    assert np.abs(d1 - d0).max() < 1e-6   # the quaternion is a float32 one: unit to 1e-7
    assert np.abs(np.linalg.norm(q[c.gx - 1] - q[0]) - float(c.width)) < 1e-6
    still = c64.set_fixed64(c, p, (1.0, 2.0, -3.0), rot, False)
    assert np.array_equal(still[c.gx:], lower0) and np.array_equal(still[:c.gx], q[:c.gx])


def test_colours_are_conflict_free_and_edges_are_what_the_battery_says():
    for gx, gy, w, h in c64.GRIDS:
        c = c64.Cloth64(w, h, gx, gy, 1.0)   # asserts the uniqueness per colour
        assert sum(len(k) for k in c.colours) == len(c.a) == (gx - 1) * gy + gx * (gy - 1) + 2 * (gx - 1) * (gy - 1) + max(gx - 2, 0) * gy + gx * max(gy - 2, 0)
        cell = (w / (gx - 1), h / (gy - 1))
        assert max(cell) / min(cell) <= 4.0 and min(cell) ** 2 > 2e-5   # near-square cells, rest lengths far above the 1e-5 branch
    assert not len(c64.Cloth64(0.5, 0.4, 2, 2, 1.0).colours[8]) and not len(c64.Cloth64(0.5, 0.4, 2, 2, 1.0).colours[10])
    three = c64.Cloth64(1.0, 1.2, 3, 3, 1.0)
    assert len(three.colours[8]) == 3 and not len(three.colours[9]) and len(three.colours[10]) == 3 and not len(three.colours[11])
    cases = c64.battery()
    assert len(cases) == len(c64.GRIDS) * len(c64.MIXES)
    for lds in (True, False):   # every value with both kernel variants
        mine = [k for k in cases if (k.n <= c64.LDS_PARTICLE_LIMIT) == lds]
        assert {k.gravity_factor for k in mine} == set(c64.GRAVITY_FACTORS) and {k.damping for k in mine} == set(c64.DAMPINGS)
        assert {k.stiffness for k in mine} == set(c64.STIFFNESSES) and {k.wind for k in mine} == {None, c64.WIND_IN_PLANE, c64.WIND, c64.WIND_STRONG}
        assert {k.dt for k in mine} == {1.0 / 120.0, 1.0 / 30.0} and any(max(abs(x) for x in k.pos) > 90 for k in mine)
    assert sorted(c64.world_order()) == list(range(len(c64.GRIDS)))
    assert {float(c64.step_dt(1.0 / 120.0, k)) for k in range(12)} == {float(np.float32(1.0 / 120.0)), float(c64.DT_EDGE), float(c64.DT_ABOVE)}


# ---------------------------------------------------------------------------------------------------------------------------
# The oracle against the reading
# ---------------------------------------------------------------------------------------------------------------------------
def _run(oracle, mix, grids, colour_order, order):
    """The oracle's world of one mix, free for STEPS steps; at each checkpoint step64 from the oracle's state before the step against its
    state after.  Returns [(case, step, class, position deviation, velocity deviation)] and the largest speed seen."""
    w, cases, ids = c64.build_world(oracle.OracleWorld, mix, grids, colour_order)
    readings = [k.cloth64() for k in cases]
    rows, speed, finite = [], 0.0, True
    for step in range(STEPS):
        dt = c64.step_dt(cases[0], step)
        before = [w.cloth_state(i) for i in ids] if step in CHECKPOINTS else None
        w.step_internal(float(dt), 4)
        after = [w.cloth_state(i) for i in ids]
        for p, v in after:
            finite = finite and bool(np.isfinite(p).all() and np.isfinite(v).all())
            speed = max(speed, float(np.abs(v).max()))
        if before is None:
            continue
        for case, reading, (p0, v0), (p1, v1) in zip(cases, readings, before, after):
            p64, v64 = c64.step64(reading, p0, v0, case.wind, case.iterations, dt, order)
            dp, dv = c64.deviation(p1, v1, p64, v64, case.iterations, dt)
            rows.append((case, step, c64.mix_class(case.iterations), dp, dv))
    return rows, speed, finite


_cache = {}


def _colour_run(oracle, mix):
    if mix not in _cache:
        _cache[mix] = _run(oracle, mix, None, True, "colour")
    return _cache[mix]


def _worst(rows):
    table = {}
    for case, step, cls, dp, dv in rows:
        p, v = table.get(cls, (0.0, 0.0))
        table[cls] = (max(p, dp), max(v, dv))
    return table


@pytest.mark.parametrize("mix", range(len(c64.MIXES)))
def test_battery_stays_finite_and_slow(oracle, mix):
    """the battery's condition: over the steps the tests run, the oracle's own trajectory of every case is finite and below MAX_SPEED"""
    rows, speed, finite = _colour_run(oracle, mix)
    print("mix %s: largest |v| component %.3g m/s" % (c64.MIXES[mix], speed))
    assert finite and speed < c64.MAX_SPEED


@pytest.mark.parametrize("mix", range(len(c64.MIXES)))
def test_oracle_step_in_colour_order(oracle, mix):
    """every grid: the oracle's float32 step within 1.5 x the table of step64 from the same state, at every checkpoint"""
    rows, _, _ = _colour_run(oracle, mix)
    assert len(rows) == len(c64.GRIDS) * len(CHECKPOINTS)
    for case, step, cls, dp, dv in rows:
        ep, ev = c64.E_F32[cls]
        assert dp <= 1.5 * ep and dv <= 1.5 * ev, "%s step %d (%s): positions %.3g of %.3g units, velocities %.3g of %.3g" % (case.name, step, cls, dp, ep, dv, ev)


@pytest.mark.parametrize("mix", range(len(c64.MIXES)))
def test_oracle_step_in_storage_order(oracle, mix):
    """the reference's own order, on the grids up to 27 x 19: the oracle with colour order off against the sequential float64 loop"""
    rows, speed, finite = _run(oracle, mix, list(range(len(c64.STORAGE_ORDER_GRIDS))), False, "storage")
    assert finite and speed < c64.MAX_SPEED
    for case, step, cls, dp, dv in rows:
        ep, ev = c64.E_F32[cls]
        assert dp <= 1.5 * ep and dv <= 1.5 * ev, "%s step %d (%s): positions %.3g of %.3g units, velocities %.3g of %.3g" % (case.name, step, cls, dp, ep, dv, ev)


def test_deviation_table(oracle):
    """cloth64.E_F32 is this measurement: within 1.5 x either way, class by class"""
    rows = [r for mix in range(len(c64.MIXES)) for r in _colour_run(oracle, mix)[0]]
    measured = _worst(rows)
    for cls in sorted(c64.E_F32):
        print("%-10s measured positions %.3g velocities %.3g   E_F32 %.3g %.3g" % ((cls,) + measured[cls] + c64.E_F32[cls]))
    assert set(measured) == set(c64.E_F32)
    for cls, (ep, ev) in c64.E_F32.items():
        mp, mv = measured[cls]
        assert ep / 1.5 <= mp <= ep * 1.5 and ev / 1.5 <= mv <= ev * 1.5, cls


def test_colour_order_against_storage_order(oracle):
    """120 free steps of mix (2, 3, 1) on the grids up to 52 x 45: how far apart the two Gauss-Seidel orders of the oracle end"""
    mix = c64.MIXES.index((2, 3, 1))
    grids = list(range(len(c64.ORDER_GRIDS)))
    worlds = [c64.build_world(oracle.OracleWorld, mix, grids, order) for order in (True, False)]
    for step in range(120):
        for w, _, _ in worlds:
            w.step_internal(float(c64.step_dt(worlds[0][1][0], step)), 4)
    worst = 0.0
    for i in worlds[0][2]:
        pc, ps = worlds[0][0].cloth_state(i)[0], worlds[1][0].cloth_state(i)[0]
        assert np.isfinite(pc).all() and np.isfinite(ps).all()
        worst = max(worst, float(np.linalg.norm(pc.astype(np.float64) - ps, axis=1).max()))
    print("colour order against storage order after 120 steps: %.4g m (cloth64.ORDER_DISTANCE %.4g)" % (worst, c64.ORDER_DISTANCE))
    assert c64.ORDER_DISTANCE / 2.0 <= worst <= c64.ORDER_DISTANCE * 2.0


# ---------------------------------------------------------------------------------------------------------------------------
# setWorldPositionOfFixedVertices
# ---------------------------------------------------------------------------------------------------------------------------
HALF_TURN_Y = (0.0, 1.0, 0.0, 0.0)
MOVES = [((1.5, 2.0, -0.5), (0.36514837, -0.18257419, 0.54772256, 0.73029674)), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)), ((-2.0, 1.0, 3.0), HALF_TURN_Y),
         ((96.0, -40.0, 12.0), (0.18257419, 0.36514837, 0.54772256, 0.73029674))]


def _fixed_rows(oracle):
    rows = []
    for gx, gy in ((4, 5), (5, 4), (32, 16), (27, 19)):
        for move_rigid in (True, False):
            for pos, rot in MOVES:
                for moving in (False, True):   # from the construction pose, and from a cloth that has swung for ten steps
                    w = oracle.OracleWorld(); c64.far_body(w)
                    c = w.add_cloth(1.2, 1.5, gx, gy, 2.0)
                    w.set_cloth_iterations(2, 3, 1); w.set_cloth_colour_order(True)
                    if moving:
                        w.cloth_set_fixed_vertices(c, (0.5, 1.0, 0.0), (0.25881905, 0.0, 0.0, 0.96592583), True)
                        for _ in range(10):
                            w.step_internal(1.0 / 60.0, 4)
                    p0, _ = w.cloth_state(c)
                    w.cloth_set_fixed_vertices(c, pos, rot, move_rigid)
                    p1, v1 = w.cloth_state(c)
                    p64 = c64.set_fixed64(c64.Cloth64(1.2, 1.5, gx, gy, 2.0), p0, pos, rot, move_rigid)
                    unit = c64.EPS32 * max(1.0, float(np.abs(p64).max()))
                    rows.append(((gx, gy, move_rigid, rot, moving), float(np.abs(p1.astype(np.float64) - p64).max()) / unit))
    return rows


def test_fixed_vertices(oracle):
    """the oracle right after the call against set_fixed64: even and odd gridX, both modes, a generic rotation, the identity, a half turn
    about y (the antiparallel branch of rotateFromTo: the rows below the bar turn about z, not y), near the origin and far off"""
    rows = _fixed_rows(oracle)
    worst = max(d for _, d in rows)
    print("setWorldPositionOfFixedVertices: measured %.3g units (cloth64.E_F32_FIXED %.3g)" % (worst, c64.E_F32_FIXED))
    for what, d in rows:
        assert d <= 1.5 * c64.E_F32_FIXED, (what, d)
    assert c64.E_F32_FIXED / 1.5 <= worst
    # the half turn took the antiparallel branch: a cloth in its construction pose turned about y would have its free rows at +z of the
    # bar; turned about z they stay at -z
    c = c64.Cloth64(1.2, 1.5, 4, 5, 2.0)
    q = c64.set_fixed64(c, c.p0, (0.0, 0.0, 0.0), HALF_TURN_Y, True)
    assert np.allclose(q[c.gx:, 2], c.p0[c.gx:, 2], atol=1e-6) and np.allclose(q[c.gx:, 0], -c.p0[c.gx:, 0].astype(np.float64), atol=1e-6)
