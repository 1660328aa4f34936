"""mi_proximity with MI_PROX_TERRAIN / World.proximity(terrain=True): the heightmap as one more candidate, the solid under its surface.
The walk against brute force in every byte on the `terrain` scene with bodies lying on it; the device against tests/terrain_prox64.py's
float32 restatement bit for bit and against its float64 reading within 4 x the rounding measured there; the flag off and a world
without a heightmap (the bytes of the call without the flag), a heightmap-only world; colliders and terrain together; the two entries at
the launch shapes and the life of the min / max table; the triangle id."""
import os
import sys

import numpy as np
import pytest
import torch  # before libmi_physics.so is loaded: the process then uses torch's HIP runtime for both

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import terrain_prox64 as tp  # noqa: E402
import terrain_ray64 as t64  # noqa: E402

pytestmark = pytest.mark.gpu

STATIC_BODY, TERRAIN = 0xFFFFFFFF, 0xFFFFFFFE
INF = np.float32(np.inf)
SPHERE = 0
MATERIAL = (0.1, 0.8, 1.0)


def _ids(r):
    return r["reserved"].view(np.uint32)


@pytest.fixture(scope="module")
def settled(mi):
    """the `terrain` scene after 60 steps: its bodies lie on and near the ground"""
    from directx_renderer_kurth_amd import scenes
    sc = scenes.terrain()
    w = sc.instantiate(mi.World())
    for _ in range(60):
        w.step(sc.dt)
    yield w
    w.close()


def _random_queries(mi, w, n, seed):
    rng = np.random.default_rng(seed)
    T = t64.scene_layout()
    lo, hi = T.box()
    rec = np.zeros(n, mi.PROXIMITY_QUERY_DTYPE)
    pts = lo + (hi - lo) * rng.uniform(-0.1, 1.1, (n, 3))
    pts[:, 1] = lo[1] + (hi[1] - lo[1]) * rng.uniform(-0.5, 1.6, n)
    rec["point"], rec["mount"], rec["enabled"] = pts, STATIC_BODY, 1
    rec["radius"] = rng.choice([0.0, 0.1, 0.5, 2.0, 8.0, np.inf], n)
    # a third of the queries ride on a body (points within a metre of it), half of those blind to a range of bodies around the carrier
    nb = w.num_bodies
    mounted = np.flatnonzero(np.arange(n) % 3 == 0)
    rec["mount"][mounted] = rng.integers(0, nb, len(mounted))
    rec["point"][mounted] = rng.uniform(-1.0, 1.0, (len(mounted), 3))
    ex = mounted[::2]
    rec["excludeFirst"][ex] = np.maximum(rec["mount"][ex].astype(np.int64) - 2, 0)
    rec["excludeCount"][ex] = 5
    rec["enabled"][::97] = 0
    rec["mount"][5::211] = nb + 7                    # no such body: off
    return rec


@pytest.mark.parametrize("count", [True, False])
@pytest.mark.parametrize("static", [True, False])
def test_walk_equals_brute_force_in_every_byte(mi, settled, count, static):
    rec = _random_queries(mi, settled, 2000, 11)
    walk = settled.proximity(rec, static=static, count=count, terrain=True)
    found = walk[walk["found"] != 0]
    on_terrain = int((found["collider"] == TERRAIN).sum())
    assert on_terrain >= 0.5 * len(found) and len(found) - on_terrain >= 0.05 * len(found), (len(found), on_terrain)
    assert int((found["distance"] < 0).sum()) >= 100 and int((found["distance"] > 0).sum()) >= 100
    brute = settled.proximity(rec, static=static, count=count, terrain=True, brute_force=True)
    assert walk.tobytes() == brute.tobytes()
    if not count:
        assert not walk["numWithin"].any()


@pytest.fixture(scope="module")
def battery_answers(mi):
    """(golden arrays, the device's readings) of terrain_prox64's battery, each layout in a heightmap-only world.  The float64 readings and
    the restatement come from tests/golden/terrain_prox64.npz, which test_terrain_prox64_cpu.py holds to a fresh computation."""
    g = tp.load_golden()
    out = np.zeros(len(g["point"]), mi.PROXIMITY_READING_DTYPE)
    for name, T in tp.layouts().items():
        w = T.instantiate(mi.World())
        idx = np.flatnonzero(g["layout"] == name)
        out[idx] = w.proximity(g["point"][idx], g["radius"][idx], terrain=True)
        assert out[idx].tobytes() == w.proximity(g["point"][idx], g["radius"][idx], terrain=True, brute_force=True).tobytes()
        w.close()
    return g, out


def test_device_equals_the_float32_restatement(mi, battery_answers):
    """terrain_point.h on the device and terrain_prox64's numpy float32 in its order: the same bits, on every case of the battery"""
    g, got = battery_answers
    assert len(got) >= 140
    for i, r in enumerate(got):
        where = (g["layout"][i], g["family"][i], g["point"][i])
        if not g["found32"][i]:
            assert r.tobytes() == bytes(48), where
            continue
        assert r["found"] == 1 and r["collider"] == TERRAIN and r["body"] == STATIC_BODY and r["numWithin"] == 1, where
        mine = np.concatenate([[r["distance"]], r["point"], r["normal"]]).astype(np.float32)
        assert mine.tobytes() == g["answer32"][i].tobytes(), where + (mine, g["answer32"][i])
        assert int(_ids(r)) == int(g["triangle32"][i]), where


def test_device_against_float64(mi, battery_answers):
    """decided cases: found as the reading says; distance, point and normal within 4 x the family's measured rounding; the sign; the
    triangle where it is decided"""
    g, got = battery_answers
    checked = 0
    for i, r in enumerate(got):
        where = (g["layout"][i], g["family"][i], g["point"][i])
        if not g["decided"][i]:
            continue
        assert bool(r["found"]) == bool(g["found"][i]), where
        if not g["found"][i]:
            assert r.tobytes() == bytes(48)
            continue
        e = tp.Reading()
        e.d, e.d_f, e.m, e.point, e.normal = float(g["d"][i]), float(g["d_f"][i]), float(g["m"][i]), g["c"][i], g["n"][i]
        tol = tp.tolerance(str(g["family"][i]))
        err = tp.errors(e, r["distance"], r["point"], r["normal"])
        assert all(a <= b for a, b in zip(err, tol)), where + (err, tol)
        assert bool(r["distance"] < 0) == bool(g["below"][i])
        if g["tri_decided"][i]:
            assert int(_ids(r)) == int(g["tri"][i])
        checked += 1
    assert checked >= 120


def test_flag_off_and_no_heightmap_change_no_byte(mi, settled):
    rec = _random_queries(mi, settled, 512, 12)
    plain = settled.proximity(rec)
    assert not (plain["collider"] == TERRAIN).any() and not _ids(plain).any()
    assert settled.proximity(rec, terrain=False).tobytes() == plain.tobytes()
    # a world without a heightmap: the flag does nothing
    w = mi.World()
    b = w.add_body((0.0, 1.0, 0.0), gravity_factor=0.0)
    w.add_collider(b, SPHERE, (0, 0, 0, 0.5), MATERIAL)
    pts = np.array([(0.0, 2.0, 0.0), (3.0, 1.0, 0.0), (0.0, 1.0, 0.0)], np.float32)
    assert w.proximity(pts, terrain=True).tobytes() == w.proximity(pts).tobytes()
    assert w.proximity(pts, terrain=True, brute_force=True).tobytes() == w.proximity(pts, brute_force=True).tobytes()
    w.close()


def test_a_heightmap_only_world_answers(mi):
    T = t64.one_chunk()
    w = T.instantiate(mi.World())
    pts = np.array([(0.3, 5.0, 0.4), (0.3, -1.9, 0.4), (40.0, 0.0, 0.0)], np.float32)
    r, wp = w.proximity(pts, terrain=True, world_points=True)
    assert (r["found"] == 1).all() and (r["collider"] == TERRAIN).all() and (r["body"] == STATIC_BODY).all() and (r["numWithin"] == 1).all()
    assert r["distance"][0] > 0 and r["distance"][1] < 0 and r["distance"][2] > 27.0
    np.testing.assert_array_equal(wp[:, 0:3], pts)
    assert not w.proximity(pts).view(np.uint8).any()                       # and nothing without the flag
    assert not w.proximity(pts, radius=-1.0, terrain=True).view(np.uint8).any()
    assert not w.proximity(pts, radius=np.nan, terrain=True).view(np.uint8).any()
    nan = w.proximity(np.array([(np.nan, 0.0, 0.0)], np.float32), terrain=True)
    assert not nan.view(np.uint8).any()
    w.close()


def test_colliders_and_terrain_together(mi):
    T = t64.one_chunk()
    w = T.instantiate(mi.World())
    h = float(t64.height_at32(T, 0.3, 0.4))
    ball = w.add_body((0.3, h + 0.5, 0.4), gravity_factor=0.0)              # a sphere resting on the ground
    w.add_collider(ball, SPHERE, (0, 0, 0, 0.5), MATERIAL)
    centre, beside = (0.3, h + 0.5, 0.4), (3.3, float(t64.height_at32(T, 3.3, 0.4)) + 0.2, 0.4)
    r = w.proximity(np.array([centre, beside], np.float32), radius=2.0, terrain=True)
    assert r["collider"][0] != TERRAIN and r["body"][0] == ball and r["distance"][0] == np.float32(-0.5) and r["numWithin"][0] == 2
    assert r["collider"][1] == TERRAIN and 0.0 < r["distance"][1] <= 0.2 + 1e-6 and r["numWithin"][1] == 1
    # without counting the same winners and no count
    r0 = w.proximity(np.array([centre, beside], np.float32), radius=2.0, terrain=True, count=False)
    assert (r0["collider"] == r["collider"]).all() and not r0["numWithin"].any()
    # an excluded carrier still sees the ground: mounted at the ball's centre, blind to the ball
    r = w.proximity(np.zeros((1, 3), np.float32), radius=2.0, mount=ball, exclude_first=ball, exclude_count=1, terrain=True)
    assert r["collider"][0] == TERRAIN and r["numWithin"][0] == 1 and abs(float(r["distance"][0]) - 0.5) < 0.05
    # a metre under the surface: the terrain is within radius 0 (the distance is along the slope's normal, so less than the metre)
    below = w.proximity(np.array([(0.3, h - 1.0, 0.4)], np.float32), radius=0.0, terrain=True)
    assert below["collider"][0] == TERRAIN and -1.0 <= below["distance"][0] < -0.5 and below["normal"][0][1] > 0
    w.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_host_entry_equals_device_entry(mi, settled, n):
    rec = _random_queries(mi, settled, 129, 13)[:n]
    host, wp_h = settled.proximity(rec, terrain=True, world_points=True)
    dev, wp_d = settled.proximity(rec, terrain=True, world_points=True, device=True)
    assert host.tobytes() == dev.tobytes() and wp_h.tobytes() == wp_d.tobytes()


def test_the_life_of_the_table(mi):
    T = t64.one_chunk()
    w = T.instantiate(mi.World())
    b = w.add_body((5.0, 6.0, 5.0))
    w.add_collider(b, SPHERE, (0, 0, 0, 0.3), MATERIAL)
    pts = np.array([(0.3, 3.0, 0.4), (-5.5, 2.0, 6.1), (2.0, -1.0, -3.0)], np.float32)

    def ask(world):
        walk = world.proximity(pts, terrain=True, count=False, exclude_first=0, exclude_count=1)
        assert walk.tobytes() == world.proximity(pts, terrain=True, count=False, exclude_first=0, exclude_count=1, brute_force=True).tobytes()
        return walk
    first = ask(w)
    rays = np.array([[0.3, 9.0, 0.4, np.inf, 0.0, -1.0, 0.0, 1.0]], np.float32)
    assert w.raycast(rays, terrain=True)[3][0] == 1                          # a ray cast in between uses the same table
    assert ask(w).tobytes() == first.tobytes()
    flat = np.full((129, 129), 30000, np.uint16)
    w.heightmap_set_chunk(0, 0, flat)                                        # new heights: the table is rebuilt
    second = ask(w)
    level = -2.0 + 30000 * 6.0 / 65535.0
    np.testing.assert_allclose(second["distance"], pts[:, 1] - level, atol=1e-5)
    w.heightmap_update((-12.0, -1.0, -12.0), 6.0)                            # the corner moves up a metre: no rebuild needed
    third = ask(w)
    np.testing.assert_allclose(third["distance"], second["distance"] - 1.0, atol=1e-5)
    w.step(1.0 / 120.0)
    assert ask(w).tobytes() == third.tobytes()
    twin = mi.World.restore(w.snapshot())
    assert ask(twin).tobytes() == third.tobytes()
    twin.close()
    w.close()


def test_the_triangle_id_names_the_cell_that_holds_the_point(mi, battery_answers):
    g, got = battery_answers
    lay = tp.layouts()
    seen = 0
    for i, r in enumerate(got):
        if not r["found"]:
            continue
        T = lay[str(g["layout"][i])]
        X, Z, cx, cz, which = mi.heightmap_triangle(int(_ids(r)), T.cpd)
        assert (X, Z) in T.chunks
        a, b, cc = (np.asarray(v, np.float64) for v in tp.vertices32(T, int(_ids(r)))[0:3])
        p = r["point"].astype(np.float64)
        # the reported point lies on that triangle: on its plane and inside its cell's extent, to a few ulps of the coordinates
        n = np.cross(b - a, cc - a); n /= np.linalg.norm(n)
        slack = 16 * tp.F32_EPS * T.magnitude(p)
        assert abs(np.dot(p - a, n)) <= slack
        x0, z0 = float(T.corner[0]) + (X * 128 + cx) * T.cell, float(T.corner[2]) + (Z * 128 + cz) * T.cell
        assert x0 - slack <= p[0] <= x0 + T.cell + slack and z0 - slack <= p[2] <= z0 + T.cell + slack
        seen += 1
    assert seen >= 130
