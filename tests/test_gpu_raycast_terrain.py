"""mi_raycast_batch with MI_RAY_TERRAIN / World.raycast(terrain=True): the heightmap's triangles as ray-cast candidates.  The walk
against brute force in all 32 bytes of every record; the device against the float64 reading of tests/terrain_ray64.py within the
rounding that file measures; watertight vertical rays; terrain together with colliders; the flag; launch shapes and the life of the
tile table."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch  # before libmi_physics.so is loaded: the process then uses torch's HIP runtime for both

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import terrain_ray64 as t64  # noqa: E402

pytestmark = pytest.mark.gpu

MI_OK = 0
RAY_STATIC, RAY_BRUTE_FORCE, RAY_TERRAIN = 1, 2, 4
LAYOUTS, CASES = t64.battery()
FAR_CORNER = (1000.0, 990.0, -1048.0)


def _raw(w, rays, flags, num_rays=None, extra=0, sentinel=-7.5):
    """(status, records [len(rays) + extra, 8] as uint32) of mi_raycast_batch called with num_rays; the buffer holds `sentinel` before"""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    n = len(rays) if num_rays is None else num_rays
    dev = torch.device("cuda", torch.cuda.current_device())
    ext = torch.cuda.ExternalStream(w.device_state().stream or 0, device=dev)
    with torch.cuda.stream(ext):
        d_rays = torch.from_numpy(rays).to(dev)
        d_out = torch.full((len(rays) + extra, 8), sentinel, dtype=torch.float32, device=dev)
        code = w.lib.mi_raycast_batch(w.w, ctypes.c_uint32(n), ctypes.c_void_p(d_rays.data_ptr()), ctypes.c_uint32(flags), ctypes.c_void_p(d_out.data_ptr()))
        ext.synchronize()
        out = d_out.cpu().numpy()
    return code, np.ascontiguousarray(out).view(np.uint32)


def _cast(w, rays, flags):
    code, rec = _raw(w, rays, flags)
    assert code == MI_OK, code
    return rec


def _walk_equals_brute(w, rays, static=True):
    """The records [n, 8] uint32 of the walk, after checking that brute force gives the same 32 bytes per record"""
    base = RAY_TERRAIN | (RAY_STATIC if static else 0)
    walk, brute = _cast(w, rays, base), _cast(w, rays, base | RAY_BRUTE_FORCE)
    same = (walk == brute).all(axis=1)
    assert same.all(), (np.flatnonzero(~same)[:8].tolist(), rays[~same][:4], walk[~same][:4], brute[~same][:4])
    assert not np.isnan(walk[:, [0, 4, 5, 6]].view(np.float32)).any(), "a NaN reached a record"
    return walk


def _fields(rec):
    return rec[:, 0].view(np.float32), rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4:7].view(np.float32), rec[:, 7]


def _world(mi, T):
    return T.instantiate(mi.World())


def _battery_rays(name):
    return np.stack([c.ray for c in CASES if c.layout == name])


def _shifted(rays, T, corner):
    out = rays.copy()
    out[:, 0:3] = (rays[:, 0:3].astype(np.float64) + (np.asarray(corner, np.float64) - T.corner.astype(np.float64))).astype(np.float32)
    return out


def _must_hit(T, rays):
    """Rays that cannot miss: straight down, unlimited, switched on, from above the terrain's box, at least a cell inside the x/z extent of a chunk that has heights"""
    lo, hi = T.box()
    out = np.zeros(len(rays), bool)
    for i, r in enumerate(rays):
        if r[7] != 0.0 and r[4] == 0.0 and r[6] == 0.0 and r[5] < 0.0 and np.isinf(r[3]) and r[1] > hi[1] + 0.01:
            fx, fz = (float(r[0]) - lo[0]) / float(T.chunk_size), (float(r[2]) - lo[2]) / float(T.chunk_size)
            inside = 0.01 < fx < T.cpd - 0.01 and 0.01 < fz < T.cpd - 0.01
            out[i] = inside and (int(fx), int(fz)) in T.chunks and not T.near_rim(float(r[0]), float(r[2]), T.cell, T.cell)
    return out


@pytest.fixture(scope="module")
def measured():
    return t64.measure()


# ---- 1: the walk against brute force -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one-chunk", "scene"])
def test_walk_equals_brute_force(mi, measured, name):
    T = LAYOUTS[name]
    w = _world(mi, T)
    rays = np.concatenate([_battery_rays(name), t64.random_rays(T, 300, seed=7 + len(name))])
    rec = _walk_equals_brute(w, rays)
    must = _must_hit(T, rays)
    assert must.sum() >= 15 and rec[must, 3].all(), (int(must.sum()), np.flatnonzero(must & (rec[:, 3] == 0))[:8])
    assert (rec[rays[:, 7] == 0.0] == 0).all()
    assert (rec[rec[:, 3] == 1, 1] == t64.TERRAIN_COLLIDER).all() and (rec[rec[:, 3] == 1, 2] == t64.STATIC_BODY).all()
    # mi_heightmap_update: only the corner and the amplitude change; the table of uint16 heights is still good and the cast sees the new placement
    w.heightmap_update(FAR_CORNER, 5.0)
    far = T.moved(FAR_CORNER, 5.0)
    far_rays = np.concatenate([_shifted(_battery_rays(name), T, FAR_CORNER), t64.random_rays(far, 300, seed=11)])
    rec_far = _walk_equals_brute(w, far_rays)
    must = _must_hit(far, far_rays)
    assert must.sum() >= 15 and rec_far[must, 3].all(), (int(must.sum()), np.flatnonzero(must & (rec_far[:, 3] == 0))[:8])
    k = max(v for f, v in measured.items() if f in t64.VERTICAL)
    probes = np.stack([t64.down(*far.vertex_xz(gx, gz), y=1000.0) for gx, gz in ((40, 50), (0, 0), (128, 77), (17, 128), (101, 3))])
    t = _fields(_walk_equals_brute(w, probes))[0]
    for r, ti in zip(probes, t):
        e = far.expect(r)
        assert e.hit and e.t_decided and abs(float(ti) - e.t) <= t64.tolerance(k, e), (r, float(ti), e.t, t64.tolerance(k, e))
    w.close()


# ---- 2: the device against the float64 reading ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one-chunk", "scene"])
def test_device_against_float64(mi, measured, name):
    T = LAYOUTS[name]
    cases = [c for c in CASES if c.layout == name]
    w = _world(mi, T)
    rec = _walk_equals_brute(w, np.stack([c.ray for c in cases]))
    t, col, body, hit, point, tri = _fields(rec)
    checked_t = checked_tri = 0
    for i, c in enumerate(cases):
        e = T.expect(c.ray)
        if c.family == "off":
            assert not rec[i].any(), (c.family, rec[i])
            continue
        if e.hit_decided:
            assert bool(hit[i]) == e.hit, (c.family, c.ray, int(hit[i]), e.hit, e.t)
        if not hit[i]:
            assert not rec[i].any(), (c.family, "a miss is all zero")
            continue
        assert col[i] == t64.TERRAIN_COLLIDER and body[i] == t64.STATIC_BODY and 0.0 <= t[i] <= c.ray[3], (c.family, rec[i])
        if not e.t_decided:
            continue
        tol = t64.tolerance(measured[c.family], e)
        o, d = c.ray[0:3].astype(np.float64), c.ray[4:7].astype(np.float64)
        err_t = abs(float(t[i]) - e.t)
        err_p = float(np.abs(point[i].astype(np.float64) - (o + e.t * d)).max())
        tol_p = tol * float(np.abs(d).max()) + 2 * t64.F32_EPS * e.m
        print("%-9s %-18s t %.9g (float64 %.9g) error %.3g bound %.3g; point error %.3g bound %.3g; triangle %d %s" % (name, c.family, t[i], e.t, err_t, tol, err_p, tol_p, tri[i], e.ties))
        assert err_t <= tol, (c.family, c.ray, float(t[i]), e.t, err_t, tol)
        assert err_p <= tol_p, (c.family, c.ray, point[i], err_p, tol_p)
        assert int(tri[i]) in e.ties, (c.family, int(tri[i]), e.ties)
        checked_t += 1
        if e.triangle_decided:
            assert int(tri[i]) == e.triangle
            checked_tri += 1
    assert checked_t >= len(cases) // 2 and checked_tri >= len(cases) // 4, (checked_t, checked_tri)
    w.close()


# ---- 3: watertight vertical rays -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seam", ["x", "z"])
def test_vertical_rays_are_watertight(mi, measured, seam):
    """33 x 33 vertical rays at quarter-cell steps over 8 x 8 cells across a chunk seam: vertices, axis edges, diagonals (u + v = 1 at
    0.25 + 0.75 and 0.5 + 0.5) and interiors, all on exactly representable coordinates."""
    T = LAYOUTS["scene"]
    w = _world(mi, T)
    gx4 = np.arange(33) + 4 * (124 if seam == "x" else 60)
    gz4 = np.arange(33) + 4 * (60 if seam == "x" else 124)
    pts = [(a, b) for b in gz4 for a in gx4]
    rays = np.stack([t64.down(float(T.corner[0]) + a * 0.25 * T.cell, float(T.corner[2]) + b * 0.25 * T.cell) for a, b in pts])
    rec = _walk_equals_brute(w, rays)
    t, col, body, hit, point, tri = _fields(rec)
    assert hit.all(), np.flatnonzero(hit == 0)[:8]
    k = max(v for f, v in measured.items() if f in t64.VERTICAL)
    checked, worst = 0, 0.0
    for i, (a, b) in enumerate(pts):
        if a % 4 and b % 4:
            continue
        e = T.expect(rays[i])
        assert e.hit and e.t_decided
        tol = t64.tolerance(k, e)
        h = w.heightmap_height_at(float(rays[i, 0]), float(rays[i, 2]))
        err = abs((10.0 - float(t[i])) - h)
        worst = max(worst, err / tol)
        assert abs(float(t[i]) - e.t) <= tol and err <= tol, (a, b, float(t[i]), e.t, h, tol)
        assert int(tri[i]) in e.ties
        checked += 1
    print("seam %s: %d rays on vertices and axis edges, worst |origin.y - t - height_at| / tolerance %.3f" % (seam, checked, worst))
    assert checked >= 33 * 9 * 2 - 81
    w.close()


# ---- 4: terrain together with colliders ----------------------------------------------------------------------------------------------------
def _grid_rays(lo, hi, n, y, direction=(0.0, -1.0, 0.0)):
    xs = np.linspace(lo, hi, n)
    return np.stack([t64.make_ray((x + 0.013, y, z - 0.021), direction) for z in xs for x in xs])


def test_terrain_and_colliders(mi):
    from directx_renderer_kurth_amd import scenes
    s = scenes.terrain(n=120)
    w = s.instantiate(mi.World())
    for _ in range(4):
        w.step_internal(s.dt)
    only = _world(mi, LAYOUTS["scene"])                       # the same heightmap and no collider at all
    rays = np.concatenate([_grid_rays(-21.0, 9.0, 28, 30.0), _grid_rays(-21.0, 9.0, 12, 12.0, (0.3, -1.0, 0.2))])
    both = _walk_equals_brute(w, rays)
    plain = _cast(w, rays, RAY_STATIC)
    ground = _walk_equals_brute(only, rays)
    assert ground[:, 3].sum() >= 0.8 * len(rays), "a world with a heightmap and no collider answers"   # (9 % of the grid lies over the hole)
    assert not _cast(only, rays, RAY_STATIC).any()
    tp, tg = plain[:, 0].view(np.float32), ground[:, 0].view(np.float32)
    terrain_wins = (ground[:, 3] == 1) & ((plain[:, 3] == 0) | (tg < tp))
    collider_wins = (plain[:, 3] == 1) & ~terrain_wins
    assert collider_wins.sum() >= 20 and terrain_wins.sum() >= 100, (int(collider_wins.sum()), int(terrain_wins.sum()))
    assert (both[collider_wins] == plain[collider_wins]).all(), "a ray whose winner is a collider: the plain cast's record, byte for byte"
    assert not both[collider_wins, 7].any() and (both[collider_wins, 1] != t64.TERRAIN_COLLIDER).all()
    assert (both[terrain_wins] == ground[terrain_wins]).all(), "a ray whose winner is the ground: the record of the terrain alone"
    neither = ~terrain_wins & ~collider_wins
    assert not both[neither].any()
    # a collider in front stops the terrain pass early: what lies behind the collider's t is not reported
    assert (both[collider_wins, 0].view(np.float32) <= tg[collider_wins])[ground[collider_wins, 3] == 1].all()
    w.close()
    only.close()


# ---- 5: the flag ---------------------------------------------------------------------------------------------------------------------------
def test_flag_handling(mi):
    from directx_renderer_kurth_amd import scenes
    s = scenes.terrain(n=120)
    with_map = s.instantiate(mi.World())
    s.heightmap = None
    without = s.instantiate(mi.World())
    rays = _grid_rays(-21.0, 9.0, 20, 30.0)
    for brute in (0, RAY_BRUTE_FORCE):
        plain = _cast(without, rays, RAY_STATIC | brute)
        assert plain[:, 3].sum() >= 10
        assert (_cast(with_map, rays, RAY_STATIC | brute) == plain).all(), "without the flag the terrain is invisible"
        assert (_cast(without, rays, RAY_STATIC | RAY_TERRAIN | brute) == plain).all(), "with the flag and no heightmap: the plain cast"
    t, col, body, hit, point, tri = with_map.raycast(rays, terrain=True)
    assert tri.dtype == np.uint32 and (tri[col != t64.TERRAIN_COLLIDER] == 0).all() and (col == t64.TERRAIN_COLLIDER).sum() >= 100
    X, Z, cx, cz, which = with_map.heightmap_triangle(int(tri[col == t64.TERRAIN_COLLIDER][0]))
    assert 0 <= X < 2 and 0 <= Z < 2 and 0 <= cx < 128 and 0 <= cz < 128 and which in (0, 1)
    assert len(with_map.raycast(rays)) == 5
    dev_out = with_map.raycast(torch.from_numpy(rays).cuda(), terrain=True)
    assert (dev_out.cpu().numpy().view(np.uint32)[:, 7] == tri).all()
    with_map.close()
    without.close()


# ---- 6: launch shapes and the life of the tile table ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [RAY_TERRAIN, RAY_TERRAIN | RAY_BRUTE_FORCE], ids=["walk", "brute-force"])
@pytest.mark.parametrize("num_rays", [1, 63, 64, 65, 130])
def test_launch_shapes(mi, num_rays, flags):
    T = LAYOUTS["one-chunk"]
    w = _world(mi, T)
    rays = _vertical_grid(T, 12)[:130]
    rays[1::3] = t64.random_rays(T, 130, seed=5)[1::3]
    want = _cast(w, rays, RAY_TERRAIN | RAY_BRUTE_FORCE)
    assert want[0::3, 3].all() and want[2::3, 3].all()
    code, out = _raw(w, rays, flags, num_rays=num_rays, extra=64)
    assert code == MI_OK
    assert (out[num_rays:] == np.float32(-7.5).view(np.uint32)).all(), "records past the last ray were written"
    assert (out[:num_rays] == want[:num_rays]).all()
    w.close()


def _vertical_grid(T, n=24):
    lo, hi = T.box()
    xs = np.linspace(lo[0] + 0.4, hi[0] - 0.4, n)
    return np.stack([t64.down(float(x), float(z)) for z in xs for x in xs])


def test_a_cast_changes_nothing(mi):
    """The next steps (poses and velocities, and with them the terrain contacts that made them) are bit-equal to those of a world that never cast."""
    from directx_renderer_kurth_amd import scenes
    s = scenes.terrain(n=60)
    a, b = s.instantiate(mi.World()), s.instantiate(mi.World())
    rays = _grid_rays(-21.0, 9.0, 12, 30.0)
    for _ in range(40):
        a.step_internal(s.dt)
        b.step_internal(s.dt)
    for step in range(3):
        assert _walk_equals_brute(a, rays)[:, 3].sum() >= 100
        a.step_internal(s.dt)
        b.step_internal(s.dt)
        assert np.array_equal(a.transforms().view(np.uint32), b.transforms().view(np.uint32)) and np.array_equal(a.velocities().view(np.uint32), b.velocities().view(np.uint32)), step
    a.close()
    b.close()


def test_the_next_cast_sees_new_heights(mi):
    """Vertical rays, and flat ones (0.2 down per metre) from 1 m above the terrain's box: over a tile they keep within 0.4 m in height, so
    a table left over from other heights makes the walk pass the tile by."""
    T = LAYOUTS["one-chunk"]
    w = _world(mi, T)
    top = float(T.corner[1]) + float(T.amplitude)
    flat_rays = _grid_rays(-11.0, 4.0, 12, top + 1.0, (1.0, -0.2, 0.0))
    rays = np.concatenate([_vertical_grid(T), flat_rays])
    before = _walk_equals_brute(w, rays)
    assert before[:24 * 24, 3].all()
    flat = t64.Terrain(1, T.chunk_size, T.corner, T.amplitude, {(0, 0): np.full((129, 129), 65535, np.uint16)})
    w.heightmap_set_chunk(0, 0, flat.chunks[(0, 0)])          # the tile table is stale now: the old heights end far below the new surface
    after = _walk_equals_brute(w, rays)
    assert after[:, 3].all(), "every ray meets the plane y = top inside the chunk"
    assert np.abs(after[:24 * 24, 0].view(np.float32) - (10.0 - top)).max() <= 1e-5
    assert np.abs(after[24 * 24:, 0].view(np.float32) - 1.0 / (0.2 / np.hypot(1.0, 0.2))).max() <= 1e-4
    # snapshot -> restore: the restored world builds its own table
    r = mi.World.restore(w.snapshot())
    assert (_walk_equals_brute(r, rays) == after).all()
    r.close()
    w.heightmap_set_chunk(0, 0, T.chunks[(0, 0)])
    assert (_walk_equals_brute(w, rays) == before).all()
    w.close()
