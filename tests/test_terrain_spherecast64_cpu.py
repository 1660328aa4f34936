"""terrain_spherecast64.py against closed forms, its float32 restatement against its float64 reading, the iteration budget and the
battery's margins (no GPU)."""
import collections
import math

import numpy as np
import pytest

import spherecast64 as s64
import terrain_ray64 as t64
import terrain_spherecast64 as ts
from test_terrain_prox64_cpu import CELL, _chunk


def _level(units):
    return -2.0 + units * 6.0 / 65535.0


def test_vertical_drop_on_a_flat_chunk():
    T = _chunk(lambda x, z: 3.0)
    h = _level(round(3.0 / 6.0 * 65535.0))
    for y, r, L in ((5.0, 0.3, 1.0), (2.5, 0.0, 2.0), (9.0, 1.5, 0.25)):
        e = ts.expect(T, (0.3, y, 0.4), (0.0, -L, 0.0), r, np.inf)
        r = float(np.float32(r))
        assert e.kind == "hit" and e.t == pytest.approx((y - h - r) / L, abs=2e-9 / L) and e.cos == pytest.approx(1.0)
    assert ts.expect(T, (0.3, 5.0, 0.4), (0.0, -1.0, 0.0), 0.3, 1.0).kind == "miss"
    under = float(np.float32(h - 3.0))
    assert ts.expect(T, (0.3, under, 0.4), (0.0, 1.0, 0.0), 0.3, np.inf).t == pytest.approx(h - under - float(np.float32(0.3)), abs=2e-9)     # from below: the sheet has two sides
    assert ts.expect(T, (0.3, h + 0.2, 0.4), (1.0, 0.0, 0.0), 0.3, np.inf).kind == "touch"


def test_drop_on_a_tilted_plane():
    step = 40
    T = _chunk(lambda x, z: (20000 + step * x) * 6.0 / 65535.0)
    slope = step * 6.0 / 65535.0 / CELL
    ny = 1.0 / math.sqrt(1.0 + slope * slope)
    for x, r in ((0.3, 0.25), (-4.1, 0.8)):
        hx = _level(20000 + step * (float(np.float32(x)) + 12.0) / CELL)
        e = ts.expect(T, (x, 6.0, 0.4), (0.0, -1.0, 0.0), r, np.inf)
        r = float(np.float32(r))
        assert e.t == pytest.approx(((6.0 - hx) * ny - r) / ny, abs=1e-8) and e.cos == pytest.approx(ny, abs=1e-7)


def test_landing_on_a_ridge_edge_and_on_a_peak():
    roof = _chunk(lambda x, z: 1.0 + 2.0 - abs(x - 64) * 0.05)                # a ridge along z at x = 64
    crest = -2.0 + round((3.0) / 6.0 * 65535.0) * 6.0 / 65535.0
    e = ts.expect(roof, (0.0, 6.0, 0.4), (0.0, -1.0, 0.0), 0.5, np.inf)      # centred over the ridge: the edge is touched first
    assert e.t == pytest.approx(6.0 - crest - 0.5, abs=1e-8) and e.cos == pytest.approx(1.0)
    off = 0.1                                                                # beside it, still on the edge: the distance to the ridge line
    e = ts.expect(roof, (off, 6.0, 0.4), (0.0, -1.0, 0.0), 0.5, np.inf)
    assert e.t == pytest.approx(6.0 - crest - math.sqrt(0.25 - np.float32(off).astype(np.float64) ** 2), abs=1e-8)
    spike = _chunk(lambda x, z: 1.5 + (1.5 if (x, z) == (64, 64) else 0.0))
    apex = -2.0 + round(3.0 / 6.0 * 65535.0) * 6.0 / 65535.0
    e = ts.expect(spike, (0.0, 6.0, 0.0), (0.0, -1.0, 0.0), 0.4, np.inf)
    assert e.t == pytest.approx(6.0 - apex - 0.4, abs=1e-8)


def test_radius_zero_is_the_ray_casts_t():
    layouts, cases = t64.battery()
    checked = 0
    for c in cases[::3]:
        T = layouts[c.layout]
        r = T.expect(c.ray)
        if not (r.hit and r.t_decided) or c.ray[7] == 0 or not c.family.startswith(("vertical-interior", "slanted", "from-below", "far-origin")):
            continue
        e = ts.expect(T, c.ray[0:3], c.ray[4:7], 0.0, c.ray[3])
        assert e.t is not None and e.t == pytest.approx(r.t, abs=1e-6), (c.family, c.ray)
        checked += 1
    assert checked >= 10


def test_battery_is_not_vacuous_and_the_restatement_agrees(capsys):
    layouts, cases = ts.battery()
    done = ts.battery_done()
    assert 140 <= len(cases) <= 190
    fam = collections.Counter(c.family for c in cases)
    assert all(fam[k] >= 4 for k in ts.FAMILIES), fam
    undecided = [c.family for c, (e, _, _) in zip(cases, done) if not e.decided]
    assert len(undecided) <= 0.1 * len(cases) and set(undecided) <= set(ts.KNIFE_EDGE), undecided
    kinds = collections.Counter(e.kind for e, _, _ in done)
    assert kinds["hit"] >= 100 and kinds["miss"] >= 10 and kinds["touch"] >= 8
    for c, (e, ids, (got, _)) in zip(cases, done):
        if e.decided:
            assert (got is not None) == (e.kind in ("hit", "touch")), (c.layout, c.family, c.origin)
            if e.kind == "touch":
                assert got[1] == 0 and got[3] <= e.tol
    measured = ts.measure_f32()
    with capsys.disabled():
        print("\nterrain sphere cast, float32 restatement against float64 (t, point, normal, gap):")
        for k in sorted(measured):
            print('    "%s": (%.2g, %.2g, %.2g, %.2g),' % ((k,) + measured[k]))
    assert set(measured) == set(ts.E_F32)
    for k, row in measured.items():
        for got, table in zip(row, ts.E_F32[k]):
            assert table / 1.5 - 1e-12 <= got <= table * 1.5 + 1e-12, (k, row, ts.E_F32[k])


def test_the_iteration_budget_holds(capsys):
    """no unresolved cast in the battery or in seeded random casts; the recorded maxima (10 000 casts, measure_iterations(10000)) leave
    SC_MAX_ITER its room.  The suite runs 400 of the 10 000: the full run takes minutes of numpy float32."""
    worst_b, worst_r, unresolved = ts.measure_iterations(400)
    with capsys.disabled():
        print("\nterrain sphere cast, most samples: battery %d, 400 random casts %d, unresolved %d" % (worst_b, worst_r, unresolved))
    assert unresolved == 0
    assert worst_b == ts.MAX_ITER_BATTERY and worst_r <= ts.MAX_ITER_RANDOM
    assert 2 * max(ts.MAX_ITER_BATTERY, ts.MAX_ITER_RANDOM) <= s64.SC_MAX_ITER


def test_the_stop_against_the_proximity_reading(capsys):
    x = ts.cross_check32()
    applies = [v for v in x.values() if v[1]]
    with capsys.disabled():
        print("\ncast stop against proximity there: %d cases, %d with the winner the nearest triangle; worst difference %.3g ulps (those), %.3g ulps (the rest)"
              % (len(x), len(applies), max(v[0] for v in applies), max([v[0] for v in x.values() if not v[1]] or [0.0])))
    assert len(applies) >= 20
    assert max(v[0] for v in applies) == ts.CROSS_CHECK_ULPS and all(v[2] for v in applies)


def test_the_golden_fixture_is_current():
    fresh, stored = ts.golden_arrays(), ts.load_golden()
    assert set(fresh) == set(stored)
    for k in fresh:
        np.testing.assert_array_equal(fresh[k], stored[k], err_msg=k)
