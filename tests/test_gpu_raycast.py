"""mi_raycast_batch / World.raycast: rays against the whole world through the device BVH.  The battery of tests/ray64.py bit for bit
against the oracle and within the measured bounds against float64 (raycast_util holds the expectation); the tree against the brute-
force path, all 32 bytes of every record; degenerate trees; launch shapes; the life of a cast between pushes and steps."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch  # before libmi_physics.so is loaded: the process then uses torch's HIP runtime for both

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray64 as r64  # noqa: E402
import raycast_util as rcu  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = r64.ray_battery()
MI_OK, MI_ERR_INVALID_ARGUMENT = 0, 2
RAY_STATIC, RAY_BRUTE_FORCE = 1, 2
INF = np.float32(np.inf)


def _bound(family):
    """(t, torque) bound of a family; a family ray64 has no measurement for (it holds undecided cases only) gets what ray64 calls well conditioned"""
    return r64.bound(family) if family in r64.MEASURED else (r64.WELL_CONDITIONED, r64.WELL_CONDITIONED)


def _records(w, rays, static=True, brute_force=False):
    """The raw records [n, 8] float32 of one cast"""
    t, col, body, hit, point = w.raycast(rays, static=static, brute_force=brute_force)
    rec = np.zeros((len(t), 8), np.float32)
    rec[:, 0] = t
    rec[:, 1:4] = np.stack([col, body, hit], axis=1).astype(np.uint32).view(np.float32)
    rec[:, 4:7] = point
    return rec


def _cast_both(w, rays, static=True):
    """(t, collider, body, hit, point) through the tree, after checking that the brute-force path gives the same 32 bytes per record"""
    tree = w.raycast(rays, static=static)
    brute = w.raycast(rays, static=static, brute_force=True)
    for a, b, name in zip(tree, brute, ("t", "collider", "body", "hit", "point")):
        same = rcu.bits(a) == rcu.bits(b) if a.dtype == np.float32 else a == b
        assert np.all(same), (name, np.argwhere(~same)[:8].tolist(), a[~same][:8], b[~same][:8])
    return tree


def _check_against_expectation(cw, rays, got, static=True, poses=None, t_bound=None, need_decided=None):
    """Decided rays: hit, collider, body as expected, t within the bound (default: the worst of the posed families)."""
    t, col, body, hit, point = got
    bound = t_bound if t_bound is not None else max(r64.bound("posed-" + n)[0] for n in r64.TYPE_NAMES)
    decided = 0
    for i, r in enumerate(rays):
        e = cw.expect(r, static=static, poses=poses)
        if not e.decided:
            continue
        decided += 1
        assert bool(hit[i]) == e.hit, (i, r, int(hit[i]), e.hit, e.collider, e.t)
        if not e.hit:
            assert not np.any(rcu.bits(point[i])) and t[i] == 0 and col[i] == 0 and body[i] == 0, (i, "a miss is all zero")
            continue
        assert (int(col[i]), int(body[i])) == (e.collider, e.body), (i, r, int(col[i]), int(body[i]), e.collider, e.body, float(t[i]), e.t)
        err = abs(float(t[i]) - e.t) / (1 + abs(e.t))
        assert err <= bound, (i, float(t[i]), e.t, err, bound)
    assert decided >= (len(rays) if need_decided is None else need_decided), (decided, len(rays))


# ---- 1, 2: the battery, every case in a world of its own --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def battery(mi, oracle):
    """Per case: the oracle's (pushed body, distance), the cast's record with flags = 0 and maxT = inf, and the float64 expectation."""
    orc = r64.run_whole_world(CASES, oracle.OracleWorld, lambda w: w.accumulators(), lambda w: w.last_interaction_distance())
    got = [None] * len(CASES)
    for scene, idx in r64.scenes_of(CASES):
        w = mi.World()
        scene.instantiate(w)
        rays = np.stack([rcu.with_max_t(CASES[i].ray, INF) for i in idx])
        t, col, body, hit, point = w.raycast(rays, static=False)
        for k, i in enumerate(idx):
            got[i] = (float(t[k]), int(col[k]), int(body[k]), int(hit[k]), point[k].copy(), np.float32(t[k]))
        w.close()
    return [dict(case=c, oracle=(o[0], o[3]), got=g, expect=rcu.single_world(c).expect(rcu.with_max_t(c.ray, INF), static=False)) for c, o, g in zip(CASES, orc, got)]


def test_battery_is_the_oracle_bit_for_bit(battery):
    """Where the oracle's closest hit is in front of the ray: the same body, and t with the oracle's bits (the axis-antiparallel family,
    whose cylinder frame goes through libm's sinf / cosf, within its measured bound instead); the undecided knife edges included."""
    checked = 0
    for r in battery:
        c, (pushed, dist), (t, col, body, hit, point, t32) = r["case"], r["oracle"], r["got"]
        if pushed is None or dist < 0.0:
            continue
        checked += 1
        assert hit == 1 and body == pushed, (c.id, hit, body, pushed)
        if c.family == r64.ANTIPARALLEL:
            assert abs(t - dist) / (1 + abs(dist)) <= _bound(c.family)[0], (c.id, t, dist)
        else:
            assert rcu.bits(t32) == rcu.bits(np.float32(dist)), (c.id, t, dist)
    assert checked >= 60, checked


def test_battery_hit_points(battery):
    """point = rot * (lo + t * ld) + pos: recomputed in float32 numpy within 2 ulp of the coordinate magnitude, and against float64 (the
    same expression with the cast's own t: the point's formation, not t, is what the torque bound measures) within the family's torque
    bound scaled by 1 + that magnitude."""
    checked = 0
    for r in battery:
        c, (t, col, body, hit, point, t32) = r["case"], r["got"]
        if not hit:
            assert not np.any(rcu.bits(point)), c.id
            continue
        checked += 1
        pos, rot = c.scene.bodies[body]
        want32 = rcu.point_from(c.ray, t32, pos, rot)
        o, d = r64._f64(c.ray[0:3]), r64._f64(c.ray[4:7])
        want64 = o + float(t32) * d
        mag = max(float(np.abs(o).max()), float(np.abs(r64._f64(pos)).max()), float(np.abs(want64).max()))
        e32 = float(np.abs(point.astype(np.float64) - want32.astype(np.float64)).max())
        e64 = float(np.abs(point.astype(np.float64) - want64).max())
        print("%-60s point error %.3g (2 ulp: %.3g), against float64 %.3g (bound %.3g)" % (c.id, e32, 2.0 ** -22 * mag, e64, _bound(c.family)[1] * (1 + mag)))
        assert e32 <= 2.0 ** -22 * mag, (c.id, point, want32)
        assert e64 <= _bound(c.family)[1] * (1 + mag), (c.id, point, want64)
    assert checked >= 60, checked


def test_battery_against_float64(battery):
    """Decided cases: hit, collider and body of raycast_util's expectation (the cases whose reference answer lies behind the ray
    included: there the cast misses or reports what is in front), t within the family's bound."""
    decided = 0
    for r in battery:
        c, e, (t, col, body, hit, point, t32) = r["case"], r["expect"], r["got"]
        if not e.decided:
            assert c.knife_edge, c.id
            continue
        decided += 1
        assert bool(hit) == e.hit, (c.id, hit, e.hit, t, e.t)
        if e.hit:
            assert (col, body) == (e.collider, e.body), (c.id, col, body, e.collider, e.body)
            err = abs(t - e.t) / (1 + abs(e.t))
            print("%-60s t %.9g (float64 %.9g) error %.3g bound %.3g" % (c.id, t, e.t, err, _bound(c.family)[0]))
            assert err <= _bound(c.family)[0], (c.id, t, e.t, err)
        else:
            assert (t, col, body) == (0.0, 0, 0) and not np.any(rcu.bits(point)), c.id
    assert decided >= 0.85 * len(battery)
    behind = [r for r in battery if r["oracle"][0] is not None and r["oracle"][1] < 0.0]
    assert len(behind) >= 3 and all(not r["got"][3] or r["got"][0] >= 0.0 for r in behind)


# ---- 3: the tree against brute force ------------------------------------------------------------------------------------------------------
def test_tree_equals_brute_force_on_the_battery_world(mi):
    """Every case in a ball of its own, maxT from the case's extent.  Against float64 the bound is the family's plus what moving the
    case costs: origin and position are rounded at the coordinates M they were moved to (half an ulp each) and subtracted, 2 more
    roundings at that size follow in the body's frame: 4 * eps * M on t's scale of 1 + |t|."""
    cw, rays, ids = rcu.battery_world(CASES)
    w = cw.instantiate(mi.World())
    got = _cast_both(w, rays)
    for i, c in enumerate(CASES):
        moved = 4 * r64.F32_EPS * float(np.abs(rays[i, 0:3]).max())
        _check_against_expectation(cw, rays[i:i + 1], tuple(g[i:i + 1] for g in got), t_bound=_bound(c.family)[0] + moved, need_decided=0)
        if got[3][i]:
            assert int(got[2][i]) in ids[i], (c.id, int(got[2][i]), ids[i])   # every case keeps to itself
    assert sum(cw.expect(r).decided for r in rays) >= len(rays) // 2
    rays_inf = rays.copy()
    rays_inf[:, 3] = INF
    _cast_both(w, rays_inf)
    w.close()


@pytest.fixture(scope="module")
def random_world():
    return rcu.random_world()


@pytest.mark.parametrize("static", [True, False], ids=["static", "bodies-only"])
def test_tree_equals_brute_force_on_a_random_world(mi, random_world, static):
    cw, rays = random_world
    w = cw.instantiate(mi.World())
    t, col, body, hit, point = _cast_both(w, rays, static=static)
    zone = [i for i, c in enumerate(cw.colliders) if c["zone"] != rcu.ZONE_NONE]
    dead_colliders = [i for i, c in enumerate(cw.colliders) if c["body"] in cw.dead]
    assert not np.any(np.isin(col[hit == 1], zone + dead_colliders)), "a zone collider or a deleted body was hit"
    assert not np.any(hit[rays[:, 7] == 0.0]) and np.all(t[hit == 1] <= rays[hit == 1, 3]) and np.all(t[hit == 1] >= 0)
    assert np.any(body[hit == 1] == rcu.STATIC_BODY) == static
    assert hit.sum() >= len(rays) // (3 if static else 4), int(hit.sum())
    w.close()


def test_random_world_against_the_oracle(mi, oracle, random_world):
    """static=False: the oracle has the same bodies and one test_physics_interaction per ray.  Where its closest hit lies in
    [0, maxT]: the same body and the bits of t; where it is beyond maxT or there is none: a miss.  A ray is not comparable only when
    the oracle's closest hit is behind it; with RANDOM_SEED that is 1 ray of 2048 (checked on the CPU), and at least 90 % must be."""
    cw, rays = random_world
    orc = rcu.oracle_casts(oracle, cw, rays)
    w = cw.instantiate(mi.World())
    t, col, body, hit, point = w.raycast(rays, static=False)
    comparable = 0
    for i, (pushed, dist) in enumerate(orc):
        if pushed is not None and dist < 0.0:
            continue
        comparable += 1
        if pushed is not None and dist <= rays[i, 3]:
            assert hit[i] == 1 and int(body[i]) == pushed and rcu.bits(t[i]) == rcu.bits(np.float32(dist)), (i, int(hit[i]), int(body[i]), pushed, float(t[i]), dist)
        else:
            assert hit[i] == 0, (i, int(body[i]), float(t[i]), pushed, dist)
    assert comparable >= 0.9 * len(rays), comparable
    w.close()


# ---- 4: degenerate trees ----------------------------------------------------------------------------------------------------------------
def _down(x, z, max_t=INF, y=5.0, enabled=1.0):
    return np.array([x, y, z, max_t, 0, -1, 0, enabled], np.float32)


def _along_x(y, z, x=-5.0, max_t=INF):
    return np.array([x, y, z, max_t, 1, 0, 0, 1], np.float32)


def _slant(x, y, z, slope=1.0, max_t=INF):
    """towards +x and downwards through (x, y, z), from 2 further back"""
    d = np.array([1.0, -slope, 0.0]) / math.hypot(1.0, slope)
    return r64.ray(np.array([x, y, z]) - 2.0 * d, d, strength=max_t)


S1 = (0, 0, 0, 0.5)


def _degenerate(name):
    """(CastWorld, rays, number of rays that must be decided (None: all))"""
    cw = rcu.CastWorld()
    if name == "bodies-without-colliders":
        for k in range(3):
            cw.add_body((1.5 * k, 0, 0))
        return cw, np.stack([_down(0.1, 0.0), _along_x(0.1, 0.0)]), None
    if name == "only-zone-colliders":
        cw.add_body((0, 0, 0))
        cw.add_static(r64.SPHERE, (0, 0, 0, 2.0), zone=rcu.ZONE_TRIGGER)
        cw.add_static(r64.AABB, (-1, -1, -1, 1, 1, 1), pos=(0.5, 0, 0), zone=rcu.ZONE_FORCE_FIELD)
        return cw, np.stack([_down(0.1, 0.0), _along_x(0.1, 0.0)]), None
    if name in ("one", "two", "three"):
        n = ("one", "two", "three").index(name) + 1
        for k in range(n):
            cw.add_collider(cw.add_body((1.5 * k, 0, 0)), (r64.SPHERE, r64.OBB, r64.CAPSULE)[k], r64._local_shape((r64.SPHERE, r64.OBB, r64.CAPSULE)[k], offset=(0, 0, 0)))
        rays = [_down(1.5 * k + 0.05, 0.02) for k in range(3)] + [_along_x(0.03, 0.02), _along_x(0.03, 0.02, max_t=3.0), _along_x(0.03, 0.02, x=9.0), _down(-3.0, 0.0)]
        return cw, np.stack(rays), None
    if name == "65-spheres-one-centre":
        for k in range(65):
            cw.add_collider(cw.add_body((1.0, 2.0, 3.0)), r64.SPHERE, S1)
        return cw, np.stack([_down(1.1, 3.05, y=9.0), _along_x(2.1, 3.05), _along_x(2.1, 3.05, max_t=2.0), _down(4.0, 3.0)]), None
    if name == "64-spheres-on-a-line":
        for k in range(64):
            cw.add_collider(cw.add_body((1.25 * k, 0, 0)), r64.SPHERE, S1)
        rays = [_down(1.25 * k + 0.1, 0.05) for k in range(0, 64, 7)] + [_along_x(0.1, 0.05), _along_x(0.1, 0.05, x=100.0), _along_x(0.1, 0.05, x=30.2), _down(0.625, 0.0)]
        return cw, np.stack(rays), None
    if name == "64-spheres-in-a-plane":
        for k in range(64):
            cw.add_collider(cw.add_body((1.25 * (k % 8), 0, 1.25 * (k // 8))), r64.SPHERE, S1)
        rays = [_down(1.25 * (k % 8) + 0.1, 1.25 * (k // 8) - 0.05) for k in range(0, 64, 5)] + [_along_x(0.1, 2.55), _along_x(0.1, 2.55, x=4.0), _down(0.625, 0.625)]
        return cw, np.stack(rays), None
    if name == "1cm-sphere-next-to-a-100m-box":
        cw.add_static(r64.AABB, (-50, -50, -50, 50, 50, 50), pos=(0.0, -50.0, 0.0))            # top face at y = 0
        cw.add_collider(cw.add_body((0.25, 0.02, 0.25)), r64.SPHERE, (0, 0, 0, 0.005))
        rays = [_down(0.251, 0.249, y=1.0), _down(0.251, 0.249, y=2.0, max_t=1.7), _down(0.27, 0.25, y=1.0), _slant(0.25, 0.02, 0.2505, slope=0.5), _slant(0.25, 0.02, 0.28, slope=0.5),
                _along_x(-10.0, 3.0, x=-200.0), _down(40.0, -40.0, y=300.0)]
        return cw, np.stack(rays), None
    if name == "coordinates-of-1e3":
        base = np.array([1000.0, -1000.0, 1000.0])
        cw.add_hull(*r64.TETRA)
        for kind in range(6):
            cw.add_collider(cw.add_body(base + np.array([3.0 * kind, 0, 0]), r64.Q_BODY), kind, r64._local_shape(kind))
        cw.add_static(r64.AABB, (-20, -1, -20, 20, 0, 20), pos=base + np.array([7.5, -3.0, 0.0]))
        rays = []
        for kind in range(6):
            centre = r64._world_point(cw.bodies[kind], (0.3, -0.2, 0.1))
            rays.append(r64.ray(centre + np.array([-5, 0.1, 0.1]), (1, -0.02, -0.01), strength=INF))
            rays.append(r64.ray(centre + np.array([0.05, 6.0, 0.02]), (0.01, -1, 0.02), strength=INF))
        rays.append(r64.ray(base + np.array([-4.0, 5.0, 1.0]), (0, -1, 0), strength=INF, unit=False))
        rays.append(r64.ray(base + np.array([-4.0, 5.0, 1.0]), (0, 1, 0), strength=INF, unit=False))      # away from everything
        return cw, np.stack(rays), 9
    raise ValueError(name)


DEGENERATE = ["bodies-without-colliders", "only-zone-colliders", "one", "two", "three", "65-spheres-one-centre", "64-spheres-on-a-line", "64-spheres-in-a-plane",
              "1cm-sphere-next-to-a-100m-box", "coordinates-of-1e3"]


@pytest.mark.parametrize("name", DEGENERATE)
def test_degenerate_trees(mi, name):
    cw, rays, need = _degenerate(name)
    w = cw.instantiate(mi.World())
    got = _cast_both(w, rays)
    t_bound = r64.bound("far-1e3")[0] if name == "coordinates-of-1e3" else None
    if name == "1cm-sphere-next-to-a-100m-box":
        # the reference's sphere test takes the root of b * b - c, two numbers of size m^2 (m: origin to centre, up to 2.25 here) whose
        # difference is at most r^2 = 2.5e-5: 4 roundings of m^2 move t by 4 eps m^2 / (2 * the root) >= r / 2 for these rays
        # through the middle), on the scale of 1 + t with t >= 0.97
        t_bound = max(r64.bound("posed-" + n)[0] for n in r64.TYPE_NAMES) + 4 * r64.F32_EPS * 2.25 ** 2 / 0.005 / 1.97
    _check_against_expectation(cw, rays, got, t_bound=t_bound, need_decided=need)
    t, col, body, hit, point = got
    if name in ("bodies-without-colliders", "only-zone-colliders"):
        assert not np.any(hit)
    else:
        assert np.any(hit == 1) and np.any(hit == 0)
    if name == "65-spheres-one-centre":
        assert list(col[hit == 1]) == [0, 0] and list(hit) == [1, 1, 0, 0]        # the tie goes to the lowest index; maxT = 2 ends before the sphere
    if name == "1cm-sphere-next-to-a-100m-box":
        assert list(col) == [1, 0, 0, 1, 0, 0, 0] and list(hit) == [1, 0, 1, 1, 1, 1, 1]        # the sphere where a ray meets it first, else the box under it
    w.close()


# ---- 5: launch shapes -------------------------------------------------------------------------------------------------------------------
def _row_world(n=130):
    cw = rcu.CastWorld()
    hulls = [cw.add_hull(*r64.TETRA), cw.add_hull(*r64.BRICK)]
    for j in range(n):
        kind = j % 6
        cw.add_collider(cw.add_body((3.0 * j, 0, 0)), kind, r64._local_shape(kind, offset=(0, 0, 0), hull=hulls[(j // 6) % 2]))
    return cw


def _row_rays():
    """Down onto body i (every 5th of them disabled), or slanting through it from the side (every 3rd of those with a maxT that ends 0.5 before it)"""
    return np.stack([_down(3.0 * i + 0.05, 0.02, enabled=float(i % 5 != 3)) if i % 2 == 0 else _slant(3.0 * i, 0.03, 0.02, max_t=(1.0 if i % 3 == 0 else INF)) for i in range(130)])


def _raw_cast(w, rays, num_rays, flags, extra=64, sentinel=-7.5):
    """(status code, records [len(rays) + extra, 8]) of mi_raycast_batch called with num_rays; the buffer holds `sentinel` before"""
    dev = torch.device("cuda", torch.cuda.current_device())
    ext = torch.cuda.ExternalStream(w.device_state().stream or 0, device=dev)
    with torch.cuda.stream(ext):
        d_rays = torch.from_numpy(np.ascontiguousarray(rays, np.float32)).to(dev)
        d_out = torch.full((len(rays) + extra, 8), sentinel, dtype=torch.float32, device=dev)
        code = w.lib.mi_raycast_batch(w.w, ctypes.c_uint32(num_rays), ctypes.c_void_p(d_rays.data_ptr()), ctypes.c_uint32(flags), ctypes.c_void_p(d_out.data_ptr()))
        ext.synchronize()
        out = d_out.cpu().numpy()
    return code, out


@pytest.mark.parametrize("flags", [RAY_STATIC, RAY_STATIC | RAY_BRUTE_FORCE], ids=["tree", "brute-force"])
@pytest.mark.parametrize("num_rays", [1, 63, 64, 65, 130])
def test_launch_shapes(mi, num_rays, flags):
    cw = _row_world()
    w = cw.instantiate(mi.World())
    rays = _row_rays()
    code, out = _raw_cast(w, rays, num_rays, flags)
    assert code == MI_OK
    assert np.all(out[num_rays:] == -7.5), "records past the last ray were written"
    rec = out[:num_rays]
    got = (rec[:, 0], rec[:, 1].view(np.uint32), rec[:, 2].view(np.uint32), rec[:, 3].view(np.uint32), rec[:, 4:7])
    assert not np.any(rcu.bits(rec[:, 7])), "reserved is 0"
    assert set(np.unique(got[3])) <= {0, 1}
    _check_against_expectation(cw, rays[:num_rays], got, need_decided=num_rays - num_rays // 8)
    w.close()


def test_no_rays_and_null_pointers(mi):
    cw = _row_world(8)
    w = cw.instantiate(mi.World())
    rays = np.stack([_down(3.0 * i + 0.05, 0.02) for i in range(4)])
    code, out = _raw_cast(w, rays, 0, RAY_STATIC)
    assert code == MI_OK and np.all(out == -7.5), "numRays = 0 writes nothing"
    assert w.lib.mi_raycast_batch(w.w, ctypes.c_uint32(0), None, ctypes.c_uint32(0), None) == MI_OK
    dev = torch.device("cuda", torch.cuda.current_device())
    buf = torch.zeros((4, 8), dtype=torch.float32, device=dev)
    assert w.lib.mi_raycast_batch(w.w, ctypes.c_uint32(4), None, ctypes.c_uint32(0), ctypes.c_void_p(buf.data_ptr())) == MI_ERR_INVALID_ARGUMENT
    assert w.lib.mi_raycast_batch(w.w, ctypes.c_uint32(4), ctypes.c_void_p(buf.data_ptr()), ctypes.c_uint32(0), None) == MI_ERR_INVALID_ARGUMENT
    assert w.lib.mi_raycast_batch(None, ctypes.c_uint32(4), ctypes.c_void_p(buf.data_ptr()), ctypes.c_uint32(0), ctypes.c_void_p(buf.data_ptr())) == MI_ERR_INVALID_ARGUMENT
    assert w.raycast(rays)[3].tolist() == [1, 1, 1, 1], "the world is still usable after a rejected call"
    w.close()


def test_device_tensor_in_place(mi):
    """A torch tensor on the device is cast in place and comes back as one [n, 8] tensor of records"""
    cw = _row_world(8)
    w = cw.instantiate(mi.World())
    rays = np.stack([_down(3.0 * i + 0.05, 0.02) for i in range(8)])
    want = _records(w, rays)
    out = w.raycast(torch.from_numpy(rays).cuda())
    assert isinstance(out, torch.Tensor) and out.shape == (8, 8) and out.is_cuda
    assert np.array_equal(rcu.bits(out.cpu().numpy()), rcu.bits(want))
    w.close()


# ---- 6: life cycle ------------------------------------------------------------------------------------------------------------------------
def _falling_spheres(mi, n=48):
    """n spheres in a 3 m grid, some resting on a static ground box, under gravity"""
    cw = rcu.CastWorld()
    for k in range(n):
        cw.add_collider(cw.add_body((3.0 * (k % 8), 0.5 + 0.7 * (k % 3), 3.0 * (k // 8))), r64.SPHERE, S1)
    cw.add_static(r64.AABB, (-30, -1, -30, 30, 0, 30))
    w = mi.World()
    for p, q in cw.bodies:
        w.add_body(p, q)
    for c in cw.colliders[:-1]:
        w.add_collider(c["body"], c["type"], c["shape"], r64.MATERIAL)
    w.add_static_collider(r64.AABB, cw.colliders[-1]["shape"], r64.MATERIAL)
    return cw, w


def _sphere_rays(cw):
    return np.stack([_down(float(p[0]) + 0.1, float(p[2]) - 0.05, y=6.0) for p, _ in cw.bodies])


def test_a_cast_changes_nothing(mi):
    """No accumulator is written, and the next steps are bit-equal to those of a world that never cast."""
    (cw, a), (_, b) = _falling_spheres(mi), _falling_spheres(mi)
    rays = _sphere_rays(cw)
    for step in range(3):
        assert a.raycast(rays)[3].all()
        assert a.raycast(rays, brute_force=True)[3].all()
        assert not np.any(a.accumulators())
        a.step_internal(1.0 / 120.0, 8)
        b.step_internal(1.0 / 120.0, 8)
        assert np.array_equal(rcu.bits(a.transforms()), rcu.bits(b.transforms())) and np.array_equal(rcu.bits(a.velocities()), rcu.bits(b.velocities())), step
    a.close()
    b.close()


def test_hits_follow_the_stepped_poses(mi):
    cw, w = _falling_spheres(mi)
    for _ in range(30):
        w.step_internal(1.0 / 120.0, 8)
    rays = _sphere_rays(cw)                   # the spheres fell straight down: the rays still pass 0.11 from their centres
    got = _cast_both(w, rays)
    poses = w.transforms()
    assert np.abs(poses[:48, 1] - np.array([p[1] for p, _ in cw.bodies])).max() > 0.05, "nothing moved"
    _check_against_expectation(cw, rays, got, poses=poses, t_bound=r64.bound("sphere")[0])
    assert list(got[2]) == list(range(48))
    w.close()


def test_the_next_cast_sees_every_change(mi):
    cw = _row_world(6)
    w = cw.instantiate(mi.World())
    rays = np.stack([_down(3.0 * i + 0.05, 0.02) for i in range(8)])
    _check_against_expectation(cw, rays, _cast_both(w, rays))
    w.step_internal(1.0 / 120.0, 4)            # the state now lives on the device (no gravity: nothing moves)
    # set_transform: body 1 moves to x = 18, where ray 6 finds it
    w.set_transform(1, (18.0, 0.0, 0.0), r64.IDENT)
    cw.bodies[1] = (np.array([18.0, 0, 0], np.float32), r64.IDENT)
    got = _cast_both(w, rays)
    _check_against_expectation(cw, rays, got)
    assert list(got[3]) == [1, 0, 1, 1, 1, 1, 1, 0] and got[2][6] == 1
    # a new body with a collider of a new hull geometry at x = 21
    g = w.add_hull_geometry(*r64.BRICK)
    assert g == cw.add_hull(*r64.BRICK)
    b = w.add_body((21.0, 0, 0), gravity_factor=0.0, linear_damping=0.0, angular_damping=0.0)
    assert b == cw.add_body((21.0, 0, 0))
    assert w.add_collider(b, r64.HULL, (0, 0, 0, 1, 0, 0, 0, g), r64.MATERIAL) == cw.add_collider(b, r64.HULL, (0, 0, 0, 1, 0, 0, 0, g))
    got = _cast_both(w, rays)
    _check_against_expectation(cw, rays, got)
    assert got[3][7] == 1 and got[2][7] == b and abs(got[0][7] - 4.5) <= 1e-6
    # delete_body
    w.delete_body(2)
    cw.dead.add(2)
    got = _cast_both(w, rays)
    _check_against_expectation(cw, rays, got)
    assert list(got[3]) == [1, 0, 0, 1, 1, 1, 1, 1]
    w.close()


def test_a_cast_between_a_push_and_the_step_leaves_the_push(mi):
    def world():
        w = mi.World()
        for k in range(3):
            w.add_collider(w.add_body((3.0 * k, 0, 0), gravity_factor=0.0, linear_damping=0.0, angular_damping=0.0), r64.SPHERE, S1, r64.MATERIAL)
        return w
    a, b = world(), world()
    pushes = np.stack([r64.ray((3.0 * k, 5.0, 0.0), (0, -1, 0), 300.0 + 100 * k, unit=False) for k in range(3)])
    for w in (a, b):
        assert list(w.test_physics_interaction_batch(pushes, 0, 1)) == [1, 2, 3]
    before = a.accumulators()
    assert a.raycast(np.stack([_down(3.0 * k, 0.0) for k in range(3)]))[3].all()
    assert np.array_equal(rcu.bits(a.accumulators()), rcu.bits(before)) and np.any(before)
    for w in (a, b):
        w.step_internal(1.0 / 120.0, 1)
    assert np.array_equal(rcu.bits(a.velocities()), rcu.bits(b.velocities())) and np.all(a.velocities()[:, 1] < 0)
    a.close()
    b.close()
