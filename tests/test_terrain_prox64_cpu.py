"""terrain_prox64.py against closed forms, its float32 restatement against its float64 reading, and the battery's margins (no GPU)."""
import collections
import math

import numpy as np
import pytest

import terrain_prox64 as tp
import terrain_ray64 as t64

CELL = 24.0 / 128


def _chunk(fn):
    """one 24 m chunk at (-12, -2, -12), amplitude 6, heights fn(gx, gz) in metres over the corner, quantised exactly where fn allows"""
    gz, gx = np.meshgrid(np.arange(129), np.arange(129), indexing="ij")
    h = np.round(np.vectorize(fn)(gx, gz) / 6.0 * 65535.0)
    return t64.Terrain(1, 24.0, (-12.0, -2.0, -12.0), 6.0, {(0, 0): h.astype(np.uint16)})


def test_flat_chunk_reads_height_over_it():
    T = _chunk(lambda x, z: 3.0)
    h = -2.0 + round(3.0 / 6.0 * 65535.0) * 6.0 / 65535.0
    for y, x, z in ((2.5, 0.3, 0.4), (1.2, -7.1, 5.5), (0.5, 3.3, 3.3), (-1.5, 0.0, 0.0)):
        e = tp.expect(T, (x, y, z), np.inf)
        assert e.found and e.d == pytest.approx(np.float32(y) - h, abs=1e-12)
        assert e.below == (y < h)
        np.testing.assert_allclose(e.point, (np.float32(x), h, np.float32(z)), atol=1e-12)
        np.testing.assert_allclose(e.normal, (0, 1, 0), atol=1e-9)      # up on either side: out of the solid
    assert not tp.expect(T, (0.3, h + 0.5, 0.4), 0.25).found
    assert tp.expect(T, (0.3, h - 5.0, 0.4), 0.0).found                    # below: within for every radius


def test_tilted_plane_reads_along_the_normal():
    step = 40                                                            # height units per cell in x: exact in uint16
    T = _chunk(lambda x, z: (20000 + step * x) * 6.0 / 65535.0)
    slope = step * 6.0 / 65535.0 / CELL
    ny = 1.0 / math.sqrt(1.0 + slope * slope)
    for x, z, dy in ((0.3, 0.4, 0.8), (-3.7, 2.2, 0.1), (5.05, -6.6, -0.6)):
        hx = -2.0 + (20000 + step * (float(np.float32(x)) + 12.0) / CELL) * 6.0 / 65535.0
        y = float(np.float32(hx + dy))
        e = tp.expect(T, (x, y, z), np.inf)
        assert e.d == pytest.approx((float(y) - hx) * ny, abs=1e-9)
        np.testing.assert_allclose(e.normal, np.array([-slope, 1.0, 0.0]) * ny, atol=1e-7)


def test_single_raised_vertex_apex_and_edges():
    H = 1.5
    T = _chunk(lambda x, z: 1.5 + (H if (x, z) == (64, 64) else 0.0))
    base = -2.0 + round(1.5 / 6.0 * 65535.0) * 6.0 / 65535.0
    apex = np.array([0.0, -2.0 + round(3.0 / 6.0 * 65535.0) * 6.0 / 65535.0, 0.0])
    e = tp.expect(T, (0.0, apex[1] + 0.7, 0.0), np.inf)                    # straight over the apex: the vertex region
    assert e.d == pytest.approx(np.float32(apex[1] + 0.7) - apex[1], abs=1e-9) and not e.tri_decided
    np.testing.assert_allclose(e.point, apex, atol=1e-12)
    # beside the spike, over the edge from the apex to the vertex (65, 64): the distance to that segment, by hand
    foot = np.array([CELL, base, 0.0])
    p = np.array([0.12, base + 1.4, 0.0], np.float32).astype(np.float64)
    s = np.clip(np.dot(p - apex, foot - apex) / np.dot(foot - apex, foot - apex), 0, 1)
    by_hand = np.linalg.norm(p - (apex + s * (foot - apex)))
    e = tp.expect(T, p, np.inf)
    assert 0 < s < 1 and e.d == pytest.approx(by_hand, abs=1e-9)
    np.testing.assert_allclose(e.point, apex + s * (foot - apex), atol=1e-9)


def test_outside_the_footprint_is_never_below():
    T = t64.one_chunk()
    e = tp.expect(T, (-13.0, -1.9, 0.0), np.inf)                           # lower than the rim beside it
    assert e.found and not e.below and e.d > 0 and math.isinf(e.margins["sign"])


def test_battery_is_not_vacuous():
    layouts, cases = tp.battery()
    ex = tp.battery_expected()
    assert 140 <= len(cases) <= 170
    fam = collections.Counter(c.family for c in cases)
    assert all(fam[k] >= 6 for k in tp.FAMILIES), fam
    decided = sum(e.decided for e in ex)
    assert decided >= 0.9 * len(cases), (decided, len(cases))
    assert {c.family for c, e in zip(cases, ex) if not e.decided} <= {"surface"}
    by = lambda pred: collections.Counter(c.family for c, e in zip(cases, ex) if pred(c, e))
    below, lost = by(lambda c, e: e.below), by(lambda c, e: e.decided and not e.found)
    assert below["below-shallow"] == fam["below-shallow"] and below["below-deep"] == fam["below-deep"] and below["rim-outside"] == 0
    assert lost["radius"] >= 4 and by(lambda c, e: e.found)["radius"] >= 4                      # the radius cuts on both sides
    deep = [e for c, e in zip(cases, ex) if c.family == "below-deep"]
    assert all(e.found and -e.d > float(c.radius) for c, e in zip(cases, ex) if c.family == "below-deep") and deep
    # the valley's nearest triangle is not one of the column's; the ridge's closest point is a vertex or an edge (several triangles tie)
    assert sum(not e.tri_decided for c, e in zip(cases, ex) if c.family == "ridge-peak") >= 8
    elsewhere = 0
    for c, e in zip(cases, ex):
        if c.family == "valley":
            T = layouts[c.layout]
            _, _, cx, cz, _ = t64_triangle(e.tri, T.cpd)
            own = (int((float(c.point[0]) - float(T.corner[0])) / T.cell) % 128, int((float(c.point[2]) - float(T.corner[2])) / T.cell) % 128)
            elsewhere += (cx, cz) != own
    assert elsewhere >= fam["valley"] // 2, elsewhere


def t64_triangle(triangle, cpd):
    which, cell, chunk = triangle & 1, (triangle >> 1) & 16383, triangle >> 15
    return chunk % cpd, chunk // cpd, cell & 127, cell >> 7, which


def test_restatement_agrees_and_table_is_current(capsys):
    layouts, cases = tp.battery()
    for c, e, got in zip(cases, tp.battery_expected(), tp.battery_restated()):
        if not e.decided:
            continue
        assert (got is not None) == e.found, (c.family, c.point)
        if e.found:
            assert bool(got[0] < 0) == e.below
            if e.tri_decided:
                assert got[3] == e.tri
    measured = tp.measure_f32()
    with capsys.disabled():
        print("\nterrain proximity, float32 restatement against float64 (distance / M, point / M, angle x distance / M):")
        for k in sorted(measured):
            print('    "%s": (%.2g, %.2g, %.2g),' % ((k,) + measured[k]))
    for k, row in measured.items():
        for got, table in zip(row, tp.E_F32[k]):
            assert table / 1.5 - 1e-12 <= got <= table * 1.5 + 1e-12, (k, row, tp.E_F32[k])


def test_the_golden_fixture_is_current():
    fresh, stored = tp.golden_arrays(), tp.load_golden()
    assert set(fresh) == set(stored)
    for k in fresh:
        np.testing.assert_array_equal(fresh[k], stored[k], err_msg=k)
