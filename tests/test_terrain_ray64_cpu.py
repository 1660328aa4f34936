"""tests/terrain_ray64.py against closed forms, the share of its battery it leaves undecided, the triangle id round trip, and the
float32 rounding it measures per family (the table of DESIGN.md, "Whole-world ray casts": the terrain)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import terrain_ray64 as t64  # noqa: E402

import directx_renderer_kurth_amd as mi  # noqa: E402


def _flat(h=30000, cpd=1):
    return t64.Terrain(cpd, 24.0, (-12.0, -2.0, -12.0), 6.0, {(x, z): np.full((129, 129), h, np.uint16) for x in range(cpd) for z in range(cpd)})


def _rays(seed, n=40):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        o = np.array([rng.uniform(-11, 11), rng.uniform(5, 9), rng.uniform(-11, 11)])
        d = np.array([0.0, -1.0, 0.0]) if k % 3 == 0 else np.array([rng.uniform(-0.3, 0.3), -1.0, rng.uniform(-0.3, 0.3)])
        out.append(t64.make_ray(o, d))
    return out


def test_flat_terrain():
    T = _flat()
    y = -2.0 + 30000 * (6.0 / 65535.0)
    hits = 0
    for r in _rays(1):
        e = T.expect(r)
        o, d = r[0:3].astype(np.float64), r[4:7].astype(np.float64)
        t = (y - o[1]) / d[1]
        q = o + t * d
        if abs(q[0]) < 11.9 and abs(q[2]) < 11.9:
            hits += 1
            assert e.hit and e.hit_decided and abs(e.t - t) <= 1e-12 * (1 + t), (r, e.t, t)
    assert hits >= 30
    up = T.expect(t64.make_ray((0.1, -5.0, 0.2), (0.05, 1.0, 0.0)))          # both faces count
    assert up.hit and abs(up.t - (y + 5.0) / (1.0 / np.linalg.norm([0.05, 1.0]))) <= 1e-6
    assert not T.expect(t64.make_ray((0.1, 5.0, 0.2), (0.0, 1.0, 0.0))).hit     # away from it
    assert not T.expect(t64.make_ray((0.1, 5.0, 0.2), (0.0, -1.0, 0.0), max_t=1.0)).hit


def test_terrain_linear_in_x():
    """h = 1000 + 300 * column: both triangles of every cell lie in one plane, the answer is a ray-plane hit"""
    H = np.tile((1000 + 300 * np.arange(129)).astype(np.uint16), (129, 1))
    T = t64.Terrain(1, 24.0, (-12.0, -2.0, -12.0), 6.0, {(0, 0): H})
    hs, cell = 6.0 / 65535.0, 24.0 / 128
    n = np.array([-300 * hs / cell, 1.0, 0.0])
    n /= np.linalg.norm(n)
    a = np.array([-12.0, -2.0 + 1000 * hs, -12.0])
    for r in _rays(2):
        o, d = r[0:3].astype(np.float64), r[4:7].astype(np.float64)
        t = -(n @ o - n @ a) / (n @ d)
        q = o + t * d
        if abs(q[0]) < 11.9 and abs(q[2]) < 11.9:
            e = T.expect(r)
            assert e.hit and e.hit_decided and abs(e.t - t) <= 1e-10 * (1 + t), (r, e.t, t)


def test_vertical_rays_on_vertices_give_the_vertex_height():
    T = t64.one_chunk()
    for gx, gz in [(0, 0), (128, 128), (0, 77), (64, 64), (5, 9), (127, 1), (128, 40)]:
        x, z = T.vertex_xz(gx, gz)
        e = T.expect(t64.down(x, z))
        assert e.hit and e.t_decided and abs((10.0 - e.t) - T.height(gx, gz)) <= 1e-12, (gx, gz, e.t)
        assert e.triangle == min(e.ties) and len(e.ties) >= 1
        inner = 0 < gx < 128 and 0 < gz < 128
        assert len(e.ties) == (6 if inner else len(e.ties)) and not e.triangle_decided   # on a vertex no triangle holds the point with room to spare


def test_the_battery_is_mostly_decided():
    layouts, cases = t64.battery()
    assert 140 <= len(cases) <= 180, len(cases)
    live = [c for c in cases if c.family != "off"]
    exp = [layouts[c.layout].expect(c.ray) for c in live]
    undecided = [c for c, e in zip(live, exp) if not e.t_decided]
    print("%d rays, %d hit, %d without a decided t: %s" % (len(live), sum(e.hit for e in exp), len(undecided), sorted({c.family for c in undecided})))
    assert len(undecided) <= 0.1 * len(cases), len(undecided)
    assert not [c for c in undecided if c.family in t64.VERTICAL]
    assert sum(e.hit and e.triangle_decided for e in exp) >= len(cases) // 3
    assert sum(e.hit and e.t_decided and not e.triangle_decided for e in exp) >= 20
    assert sum((not e.hit) and e.hit_decided for e in exp) >= 8
    for c in cases:
        if c.family == "off":
            e = layouts[c.layout].expect(c.ray)
            assert not e.hit and e.hit_decided


def test_triangle_id_round_trip():
    rng = np.random.default_rng(3)
    for cpd in (1, 2, 7, 256):
        for _ in range(50):
            X, Z, cx, cz, which = int(rng.integers(cpd)), int(rng.integers(cpd)), int(rng.integers(128)), int(rng.integers(128)), int(rng.integers(2))
            tid = mi.heightmap_triangle_id(cpd, X, Z, cx, cz, which)
            assert tid == t64.triangle_id(cpd, X, Z, cx, cz, which) and 0 <= tid < 2 ** 32
            assert mi.heightmap_triangle(tid, cpd) == (X, Z, cx, cz, which)
    assert mi.heightmap_triangle_id(362, 1, 361, 127, 127, 1) < 0xFFFFFFFE   # 131 044 chunks: the largest square layout below 131 071


def test_float32_rounding_per_family():
    """The table.  Sanity only: the derivation in k_raycast_terrain.hip bounds the residual of t's formula by 20 eps M / |n . d|."""
    k = t64.measure()
    print("family                 |t32 - t64| |n.d| / M   (in eps)")
    for family in sorted(k):
        print("%-22s %.3e   %.2f" % (family, k[family], k[family] / t64.F32_EPS))
    assert all(v <= 20 * t64.F32_EPS for v in k.values()), k
    assert sum(v > 0 for v in k.values()) >= 6


def test_vertex_and_edge_heights_in_float32():
    """A rehearsal of the watertight test on the CPU: on vertices and axis edges the restated t gives origin.y - t = the bilinear
    mi_heightmap_height_at (restated in float32) within the tolerance the device is held to."""
    T = t64.scene_layout()
    k = max(v for f, v in t64.measure().items() if f in t64.VERTICAL)
    worst = 0.0
    for gx4 in range(124 * 4, 132 * 4 + 1, 3):
        for gz4 in range(60 * 4, 68 * 4 + 1, 5):
            if gx4 % 4 and gz4 % 4:
                continue
            x, z = float(T.corner[0]) + gx4 * 0.25 * T.cell, float(T.corner[2]) + gz4 * 0.25 * T.cell
            r = t64.down(x, z)
            e = T.expect(r)
            assert e.hit and e.t_decided
            for tri in e.ties:
                t32 = float(t64.triangle_t32(T, r, tri))
                err = abs((10.0 - t32) - t64.height_at32(T, x, z))
                worst = max(worst, err / t64.tolerance(k, e))
    print("worst |origin.y - t32 - height_at32| / tolerance: %.3f" % worst)
    assert worst <= 1.0
