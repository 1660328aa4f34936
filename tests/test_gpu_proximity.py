"""mi_proximity / World.proximity: the nearest surface and the overlap count around a point.  The tree against brute force in every
byte (battery, a random world with a random exclusion range per query, trees of 1 .. 3 candidates, equal Morton keys, the pruning
boundary); the device against tests/proximity64.py within 4 x the float32 figures measured there, the decision itself exact; mounted
points against the float64 transform; exclusion against a twin world whose bodies were deleted; the two entry points; launch shapes;
the life of a call between steps, pose writes, deletions and ray casts; the façade's nearestSurface / countWithin."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # before libmi_physics.so is loaded: the process then uses torch's HIP runtime for both

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geom64 as g64  # noqa: E402
import proximity64 as p64  # noqa: E402
import ray64 as r64  # noqa: E402
import raycast_util as rcu  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI_OK = 0
PROX_STATIC, PROX_BRUTE_FORCE, PROX_COUNT = 1, 2, 4
STATIC_BODY = 0xFFFFFFFF
INF = np.float32(np.inf)
EPS = p64.F32_EPS
SENTINEL = -7.5
QUERY = np.dtype([("point", "<f4", 3), ("radius", "<f4"), ("mount", "<u4"), ("excludeFirst", "<u4"), ("excludeCount", "<u4"), ("enabled", "<u4")])
READING = np.dtype([("distance", "<f4"), ("collider", "<u4"), ("body", "<u4"), ("found", "<u4"), ("point", "<f4", 3), ("numWithin", "<u4"),
                    ("normal", "<f4", 3), ("reserved", "<f4")])


# ---- calling ----------------------------------------------------------------------------------------------------------------------------
def _queries(points, radius=INF, mount=STATIC_BODY, first=0, count=0, enabled=1):
    points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    rec = np.zeros(len(points), QUERY)
    rec["point"], rec["radius"], rec["mount"], rec["excludeFirst"], rec["excludeCount"], rec["enabled"] = points, radius, mount, first, count, enabled
    return rec


def _stream(w):
    dev = torch.device("cuda", torch.cuda.current_device())
    return dev, torch.cuda.ExternalStream(w.device_state().stream or 0, device=dev)


def _raw(w, rec, flags, n=None, extra=0, world_points=True):
    """(status, readings [len + extra, 12] uint32, world points [len + extra, 4] uint32) of mi_proximity called with n queries; both
    buffers hold SENTINEL before"""
    n = len(rec) if n is None else n
    dev, ext = _stream(w)
    with torch.cuda.stream(ext):
        d_in = torch.from_numpy(np.ascontiguousarray(rec).view(np.float32).reshape(-1, 8).copy()).to(dev)
        d_out = torch.full((len(rec) + extra, 12), SENTINEL, dtype=torch.float32, device=dev)
        d_wp = torch.full((len(rec) + extra, 4), SENTINEL, dtype=torch.float32, device=dev)
        code = w.lib.mi_proximity(w.w, ctypes.c_uint32(n), ctypes.c_void_p(d_in.data_ptr()), ctypes.c_uint32(flags), ctypes.c_void_p(d_out.data_ptr()),
                                  ctypes.c_void_p(d_wp.data_ptr()) if world_points else None)
        ext.synchronize()
        out, wp = d_out.cpu().numpy(), d_wp.cpu().numpy()
    return code, np.ascontiguousarray(out).view(np.uint32), np.ascontiguousarray(wp).view(np.uint32)


def _ask(w, rec, flags):
    code, out, wp = _raw(w, rec, flags)
    assert code == MI_OK, code
    return out, wp


def _readings(out):
    return np.ascontiguousarray(out).view(READING).reshape(-1)


def _same(a, b, what):
    same = (a == b).all(axis=1)
    assert same.all(), (what, np.flatnonzero(~same)[:8].tolist(), a[~same][:3], b[~same][:3])


def _check_records(out):
    r = _readings(out)
    assert set(np.unique(r["found"])) <= {0, 1}
    assert not out[r["found"] == 0].any(), "nothing within: the whole record is zero"
    assert not out[:, 11].any()
    ln = np.linalg.norm(r["normal"][r["found"] == 1].astype(np.float64), axis=1)
    assert np.all((np.abs(ln - 1.0) <= 4 * EPS) | (ln == 0.0)), ln[np.abs(ln - 1.0) > 4 * EPS][:8]


def _tree_equals_brute(w, rec, what, expect_found=True):
    seen = 0
    for static in (0, PROX_STATIC):
        for count in (0, PROX_COUNT):
            tree, wp = _ask(w, rec, static | count)
            brute, wp2 = _ask(w, rec, static | count | PROX_BRUTE_FORCE)
            _same(tree, brute, (what, static, count))
            _same(wp, wp2, (what, "world points"))
            _check_records(tree)
            r = _readings(tree)
            assert count or not r["numWithin"].any()
            assert not count or np.all(r["numWithin"][r["found"] == 1] >= 1)
            seen += int(r["found"].sum())
    assert seen > 0 or not expect_found, what
    return _readings(tree)


@pytest.fixture(scope="module")
def battery():
    cw, cases = p64.battery()
    return cw, cases, _queries([c.point for c in cases], [c.radius for c in cases])


@pytest.fixture(scope="module")
def random_world():
    cw, rays = rcu.random_world()
    rng = np.random.default_rng(11)
    n = 768
    rec = _queries(rays[:n, 0:3], rng.choice(np.array([0.5, 2.0, 5.0, 40.0, np.inf], np.float32), n), first=rng.integers(0, 290, n), count=rng.choice([0, 1, 5, 40, 400], n))
    rec["enabled"][::97] = 0
    return cw, rec


# ---- 1: the tree is brute force ------------------------------------------------------------------------------------------------------------
def test_tree_equals_brute_force_on_the_battery(mi, battery):
    cw, cases, rec = battery
    w = cw.instantiate(mi.World())
    _tree_equals_brute(w, rec, "battery")
    w.close()


def test_tree_equals_brute_force_with_a_random_range_per_query(mi, random_world):
    cw, rec = random_world
    w = cw.instantiate(mi.World())
    r = _tree_equals_brute(w, rec, "random")
    assert 0.3 < r["found"].mean() < 1.0 and r["numWithin"].max() > 100
    inside = r["distance"][r["found"] == 1] < 0
    assert inside.any() and not inside.all()
    w.close()


@pytest.mark.parametrize("n", [1, 2, 3])
def test_tree_equals_brute_force_with_few_candidates(mi, n):
    cw = rcu.CastWorld()
    for k in range(n):
        cw.add_collider(cw.add_body((3.0 * k, 1.0, -2.0 * k), r64.Q_BODY), k % 6, r64._local_shape(k % 6))
    cw.add_static(r64.AABB, (-30, -1, -30, 30, 0, 30), pos=(0.0, -10.0, 0.0))   # with MI_PROX_STATIC one more
    rng = np.random.default_rng(n)
    rec = _queries(rng.uniform(-6, 8, (130, 3)), rng.choice(np.array([1.0, 4.0, np.inf], np.float32), 130))
    w = cw.instantiate(mi.World())
    _tree_equals_brute(w, rec, n)
    only = _readings(_ask(w, _queries(rng.uniform(-6, 8, (64, 3)), first=0, count=n), PROX_COUNT)[0])   # every body excluded, no statics: nothing left
    assert not only["found"].any()
    w.close()


def test_tree_equals_brute_force_with_equal_morton_keys(mi):
    """24 colliders of all types whose boxes share one centre (the keys tie, the sorted position separates them), and 8 copies of one record"""
    cw = rcu.CastWorld()
    hull = cw.add_hull(*r64.BRICK)
    for k in range(24):
        cw.add_collider(cw.add_body((1.0, 2.0, 3.0), r64.IDENT), k % 6, r64._local_shape(k % 6, scale=0.5 + 0.1 * k, offset=(0, 0, 0), q=r64.IDENT, hull=hull))
    for k in range(8):
        cw.add_collider(cw.add_body((1.0, 2.0, 3.0), r64.IDENT), r64.SPHERE, (0, 0, 0, 0.25))
    rng = np.random.default_rng(3)
    rec = _queries(np.array([1.0, 2.0, 3.0]) + rng.normal(size=(192, 3)) * rng.choice([0.05, 0.5, 3.0], (192, 1)), rng.choice(np.array([0.0, 1.0, np.inf], np.float32), 192))
    w = cw.instantiate(mi.World())
    _tree_equals_brute(w, rec, "one centre")
    w.close()


@pytest.mark.parametrize("base,far", [(1e3, 2e4), (0.0, 3e3)], ids=["at+1e3", "at-origin"])
def test_tree_equals_brute_force_at_the_pruning_boundary(mi, base, far):
    """Small colliders, queries along the axes from far away, the radius set to the reported distance itself and to the float32 on
    either side of it: the collider's box then lies at the pruning bound to within the rounding of d in the collider's frame
    (a few ulps of |p - pos|, more than the box's pad).  Without slack some of these nodes are skipped."""
    cw = rcu.CastWorld()
    rng = np.random.default_rng(17)
    centres = []
    for k in range(3):
        pos = np.array([base, base, base]) + 2.0 * np.eye(3)[k] + rng.uniform(-0.5, 0.5, 3)
        cw.add_collider(cw.add_body(pos, r64.Q_BODY), r64.SPHERE, (0.3, -0.2, 0.1, 0.05))
        centres.append(r64._world_point(cw.bodies[-1], (0.3, -0.2, 0.1)))
    pts = []
    for i in range(384):
        u = np.zeros(3); u[i % 3] = 1.0 if (i // 3) % 2 else -1.0
        pts.append(centres[i % 3] + u * far * rng.uniform(0.3, 1.0) + rng.uniform(-0.02, 0.02, 3) * (1.0 - np.abs(u)))
    w = cw.instantiate(mi.World())
    d = _readings(_ask(w, _queries(pts), PROX_BRUTE_FORCE)[0])
    assert d["found"].all()
    radius = np.concatenate([d["distance"], np.nextafter(d["distance"], -INF), np.nextafter(d["distance"], INF)])
    rec = _queries(np.concatenate([pts, pts, pts]), radius)
    r = _tree_equals_brute(w, rec, "boundary")
    n = len(pts)
    assert r["found"][:n].all() and not r["found"][n:2 * n].any() and r["found"][2 * n:].all()
    assert np.array_equal(r["collider"][:n], d["collider"])
    w.close()


# ---- 2: the device against proximity64 ----------------------------------------------------------------------------------------------------
def test_battery_against_float64(mi, battery):
    cw, cases, rec = battery
    clear, ties, undecided = p64.classify()
    expected = p64.battery_expected()
    w = cw.instantiate(mi.World())
    r = _readings(_ask(w, rec, PROX_STATIC | PROX_COUNT)[0])
    w.close()
    worst = {}
    for i in clear:
        c, e, g = cases[i], expected[i], r[i]
        assert bool(g["found"]) == e.found, c.id
        if not e.found:
            assert not g.tobytes().strip(b"\0"), c.id
            continue
        assert g["collider"] == e.collider and g["body"] == e.body and g["numWithin"] == e.within, (c.id, g, e.collider, e.within)
        fam = p64.family_of(c, e)
        err = p64.errors(e, g["distance"], g["point"], g["normal"])
        worst[fam] = tuple(max(a, b) for a, b in zip(worst.get(fam, (0, 0, 0)), err))
        assert all(a <= t for a, t in zip(err, p64.tolerance(fam))), (c.id, err, p64.tolerance(fam))
    print({k: tuple(float("%.3g" % x) for x in v) for k, v in sorted(worst.items())})
    for i in ties:
        c, e, g = cases[i], expected[i], r[i]
        reason, winner, fields = c.tie
        if winner is None:
            assert not g.tobytes().strip(b"\0"), c.id
            continue
        assert g["found"] == 1 and g["collider"] == winner, (c.id, reason, g)
        tol = p64.tolerance(p64.TYPE_NAMES[cw.colliders[winner]["type"]] + ("@1e3" if float(np.abs(c.point).max()) > 500.0 else ""))
        if "distance" in fields:
            # at a surface d is the difference of two lengths of the shape's size, each rounded there: the family's figure relative to
            # 1 + |d| + size (on the clear cases |d| is of the shape's size itself)
            size = p64.local64(cw.colliders[winner]["type"], cw.colliders[winner]["shape"], cw.hulls, np.zeros(3))[4]
            assert abs(float(g["distance"]) - e.d) <= tol[0] * (1 + abs(e.d) + size), (c.id, g["distance"], e.d)
        if "point" in fields and e.collider == winner:
            assert np.linalg.norm(g["point"].astype(np.float64) - e.point) <= tol[1] * (1 + np.linalg.norm(e.point)), c.id
        if "normal" in fields and e.collider == winner:
            assert p64.angle(g["normal"], e.normal) <= tol[2], c.id
        if "within" in fields and e.margin_radius >= p64.CLEAR_MARGIN:
            assert g["numWithin"] == e.within, (c.id, g["numWithin"], e.within)
    for i in undecided:   # the answer is one of the rule's: the point is on the winner's surface at the reported distance
        c, e, g = cases[i], expected[i], r[i]
        assert g["found"] == 1 and g["collider"] == e.collider and abs(float(g["distance"]) - e.d) <= 1e-5 * (1 + abs(e.d)), (c.id, g)


def test_device_equals_the_float32_restatement(mi, battery):
    """point_tests.h on the device and proximity64's numpy float32 in its order: the same bits on the battery"""
    cw, cases, rec = battery
    w = cw.instantiate(mi.World())
    r = _readings(_ask(w, rec, PROX_STATIC | PROX_COUNT)[0])
    w.close()
    cands = {c[0]: c for c in p64.candidates(cw)}
    for c, g in zip(cases, r):
        if g["found"]:
            _, _, ctype, shape10, pos, rot = cands[int(g["collider"])]
            d, point, normal = p64.world32(ctype, shape10, cw.hulls, pos, rot, c.point)
            assert np.array_equal(np.float32(d), g["distance"]) and np.array_equal(point, g["point"]) and np.array_equal(normal, g["normal"]), (c.id, d, point, normal, g)


# ---- 3: mounts -----------------------------------------------------------------------------------------------------------------------------
def test_mounted_points(mi, random_world):
    cw, _ = random_world
    rng = np.random.default_rng(23)
    n = 256
    mounts = rng.integers(0, 290, n).astype(np.uint32)
    mounts[::8] = STATIC_BODY
    local = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    local[::8] = rng.uniform(-10, 10, (n // 8, 3))
    rec = _queries(local, 5.0, mount=mounts)
    w = cw.instantiate(mi.World())
    out, wp = _ask(w, rec, PROX_STATIC | PROX_COUNT)
    wpf = wp.view(np.float32)
    dead = np.isin(mounts, sorted(cw.dead))
    assert dead.any() and not out[dead].any() and not wp[dead].any()
    assert np.array_equal(wp[::8, 0:3], local[::8].view(np.uint32)), "a MI_STATIC_BODY mount passes bit for bit"
    for i in np.flatnonzero(~dead):
        assert wpf[i, 3] == 5.0
        if mounts[i] != STATIC_BODY:
            p, q = cw.bodies[mounts[i]]
            want = p64._f64(p) + g64.quat_to_matrix(p64._f64(q)) @ p64._f64(local[i])
            assert np.abs(wpf[i, 0:3] - want).max() <= 16 * EPS * (np.abs(p).max() + np.abs(local[i]).max()), (i, wpf[i], want)
            assert np.array_equal(wpf[i, 0:3], p64.mount32(p, q, local[i]))
    again, _ = _ask(w, _queries(wpf[:, 0:3], 5.0, enabled=(~dead).astype(np.uint32)), PROX_STATIC | PROX_COUNT)   # the reading is that of the world point
    _same(out, again, "mounted against world-space")
    w.close()


# ---- 4: exclusion ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("brute", [0, PROX_BRUTE_FORCE], ids=["tree", "brute"])
def test_exclusion_is_a_twin_world_without_the_bodies(mi, random_world, brute):
    cw, rec = random_world
    rec = rec.copy()
    rec["excludeFirst"], rec["excludeCount"] = 40, 25
    w = cw.instantiate(mi.World())
    got, _ = _ask(w, rec, PROX_STATIC | PROX_COUNT | brute)
    for b in range(40, 65):
        if b not in cw.dead:
            w.delete_body(b)
    rec["excludeCount"] = 0
    twin, _ = _ask(w, rec, PROX_STATIC | PROX_COUNT | brute)
    _same(got, twin, "excluded against deleted")
    w.close()


def test_a_sensor_inside_its_carrier_sees_through_it(mi):
    w = mi.World()
    carrier = w.add_body((0.0, 2.0, 0.0), r64.Q_BODY, gravity_factor=0.0)
    w.add_collider(carrier, r64.SPHERE, (0, 0, 0, 0.5), r64.MATERIAL)
    wall = w.add_static_collider(r64.AABB, (-1, -1, -1, 1, 1, 1), r64.MATERIAL, pos=(3.0, 2.0, 0.0))
    own = _readings(_ask(w, _queries([(0, 0, 0)], mount=carrier), PROX_STATIC | PROX_COUNT)[0])[0]
    assert own["collider"] == 0 and own["distance"] == np.float32(-0.5) and own["numWithin"] == 2
    out = _readings(_ask(w, _queries([(0, 0, 0)], mount=carrier, first=carrier, count=1), PROX_STATIC | PROX_COUNT)[0])[0]
    assert out["collider"] == wall and out["body"] == STATIC_BODY and out["numWithin"] == 1
    assert abs(float(out["distance"]) - 2.0) <= 8 * EPS and np.abs(out["point"] - [2, 2, 0]).max() <= 8 * EPS and np.abs(out["normal"] - [-1, 0, 0]).max() <= 4 * EPS
    w.close()


# ---- 5: entry points -------------------------------------------------------------------------------------------------------------------------
def test_host_entry_equals_device_entry(mi, random_world):
    cw, rec = random_world
    w = cw.instantiate(mi.World())
    for kw in (dict(), dict(static=False, count=False), dict(brute_force=True)):
        host, hp = w.proximity(rec.view(mi.PROXIMITY_QUERY_DTYPE), world_points=True, **kw)
        dev, dp = w.proximity(rec.view(mi.PROXIMITY_QUERY_DTYPE), world_points=True, device=True, **kw)
        assert host.tobytes() == dev.tobytes() and hp.tobytes() == dp.tobytes(), kw
        assert host.dtype == mi.PROXIMITY_READING_DTYPE and host["found"].any()
    d_in = torch.from_numpy(rec.view(np.float32).reshape(-1, 8).copy()).cuda()
    t = w.proximity(d_in)
    torch.cuda.synchronize()
    assert t.cpu().numpy().tobytes() == w.proximity(rec.view(mi.PROXIMITY_QUERY_DTYPE)).tobytes()
    plain = w.proximity(rec["point"][:16], 5.0)
    assert plain.tobytes() == w.proximity(_queries(rec["point"][:16], 5.0).view(mi.PROXIMITY_QUERY_DTYPE)).tobytes()
    del d_in, t
    w.close()


# ---- 6: launch shapes ------------------------------------------------------------------------------------------------------------------------
def _row_world(mi, n=130):
    w = mi.World()
    for k in range(n):
        w.add_collider(w.add_body((2.0 * k, 1.0, 0.0), r64.IDENT, gravity_factor=0.0), r64.SPHERE, (0, 0, 0, 0.5), r64.MATERIAL)
    return w, _queries([(2.0 * k, 2.0, 0.0) for k in range(n)], 1.0)


@pytest.mark.parametrize("flags", [PROX_COUNT, PROX_COUNT | PROX_BRUTE_FORCE], ids=["tree", "brute-force"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_launch_shapes(mi, n, flags):
    w, rec = _row_world(mi)
    code, out, wp = _raw(w, rec, flags, n=n)
    assert code == MI_OK
    r = _readings(out[:n])
    assert np.array_equal(r["collider"], np.arange(n)) and r["found"].all() and np.all(r["numWithin"] == 1) and np.abs(r["distance"] - 0.5).max() <= 4 * EPS
    assert np.all(out[n:].view(np.float32) == SENTINEL) and np.all(wp[n:].view(np.float32) == SENTINEL), "nothing is written past the last query"
    w.close()


def test_no_queries_and_null_pointers(mi):
    w, rec = _row_world(mi, 4)
    assert w.lib.mi_proximity(w.w, ctypes.c_uint32(0), None, ctypes.c_uint32(PROX_COUNT), None, None) == MI_OK
    assert w.lib.mi_proximity_host(w.w, ctypes.c_uint32(0), None, ctypes.c_uint32(0), None, None) == MI_OK
    assert len(w.proximity(np.zeros((0, 3), np.float32), 1.0)) == 0 and len(w.proximity(np.zeros((0, 3), np.float32), 1.0, device=True)) == 0
    code, out, wp = _raw(w, rec, PROX_COUNT, n=0)
    assert code == MI_OK and np.all(out.view(np.float32) == SENTINEL)
    code, out, wp = _raw(w, rec, PROX_COUNT, world_points=False)
    assert code == MI_OK and _readings(out)["found"].all() and np.all(wp.view(np.float32) == SENTINEL)
    assert w.lib.mi_proximity(w.w, ctypes.c_uint32(4), None, ctypes.c_uint32(0), None, None) != MI_OK
    w.close()
    empty = mi.World()
    e = empty.proximity([(0.0, 0.0, 0.0)], np.inf, world_points=True)
    assert not e[0].tobytes().strip(b"\0") and np.array_equal(e[1], [[0, 0, 0, np.inf]])
    empty.close()


# ---- 7: life ---------------------------------------------------------------------------------------------------------------------------------
def _carriers(mi, gravity=1.0):
    """Pairs of spheres 2 m apart along x, the pairs 4 m apart along z, over a ground box far below; body 2k carries a point at its centre
    that does not see its carrier"""
    w = mi.World()
    for k in range(6):
        for side in range(2):
            b = w.add_body((2.0 * side, 3.0 + 0.5 * k, 4.0 * k), r64.Q_BODY if side == 0 else r64.IDENT, gravity_factor=gravity, linear_damping=0.0, angular_damping=0.0)
            w.add_collider(b, r64.SPHERE, (0, 0, 0, 0.5), r64.MATERIAL)
    w.add_static_collider(r64.AABB, (-30, -1, -30, 30, 0, 30), r64.MATERIAL, pos=(0.0, -40.0, 0.0))
    mounts = 2 * np.arange(6)
    return w, _queries(np.zeros((6, 3)), 3.0, mount=mounts, first=mounts, count=1)


def test_a_query_changes_nothing(mi):
    w, rec = _carriers(mi)
    twin, _ = _carriers(mi)
    for x in (w, twin):
        x.step_internal(1.0 / 120.0, 4)
        x.apply_force_torque(3, (1.0, 2.0, 3.0), (0.5, 0.0, 0.0))
    snap, acc = w.snapshot(), w.accumulators()
    for flags in (PROX_STATIC, PROX_STATIC | PROX_COUNT, PROX_STATIC | PROX_BRUTE_FORCE):
        assert _readings(_ask(w, rec, flags)[0])["found"].all()
    assert w.snapshot() == snap and np.array_equal(rcu.bits(w.accumulators()), rcu.bits(acc)) and np.any(acc)
    for x in (w, twin):
        x.step_internal(1.0 / 120.0, 4)
    assert np.array_equal(rcu.bits(w.transforms()), rcu.bits(twin.transforms())) and np.array_equal(rcu.bits(w.velocities()), rcu.bits(twin.velocities()))
    w.close(); twin.close()


def test_queries_follow_the_stepped_bodies(mi):
    w, rec = _carriers(mi)
    before, wp0 = _ask(w, rec, PROX_STATIC | PROX_COUNT)
    for _ in range(30):
        w.step_internal(1.0 / 120.0, 4)
    after, wp1 = _ask(w, rec, PROX_STATIC | PROX_COUNT)
    poses = w.transforms()
    for out in (before, after):
        r = _readings(out)
        assert r["found"].all() and np.array_equal(r["body"], 2 * np.arange(6) + 1) and np.all(r["numWithin"] == 1)
        assert np.abs(r["distance"] - 1.5).max() <= 64 * EPS * 8 and np.abs(r["normal"] - [-1, 0, 0]).max() <= 64 * EPS
    fell = wp0.view(np.float32)[:, 1] - wp1.view(np.float32)[:, 1]
    assert np.all(fell > 0.2) and np.abs(wp1.view(np.float32)[:, 0:3] - poses[0::2, 0:3]).max() == 0.0, fell
    w.close()


def _device_array(ptr, rows, ext):
    """A float32 torch view [rows, 4] of world-owned device memory (mi_device_state), to be used on the world's stream"""
    class _Span:
        __cuda_array_interface__ = {"shape": (rows, 4), "typestr": "<f4", "data": (int(ptr), False), "version": 2}
    with torch.cuda.stream(ext):
        return torch.as_tensor(_Span(), device="cuda")


def test_poses_written_through_the_device_state_are_seen(mi):
    w, rec = _carriers(mi, gravity=0.0)
    w.step_internal(1.0 / 120.0, 1)
    before = _readings(_ask(w, rec, PROX_STATIC)[0])
    assert before["found"].all()
    ds = w.device_state()
    dev, ext = _stream(w)
    with torch.cuda.stream(ext):
        for p in (ds.pose, ds.pose0, ds.poseLerp):          # teleport: body 0 (a carrier) 10 up, body 3 (a target) 1 m further away
            a = _device_array(p, 2 * ds.numBodies, ext)
            a[0] = torch.tensor([0.0, 13.0, 0.0, 0.0], device=dev)
            a[6] = torch.tensor([3.0, 3.5, 4.0, 0.0], device=dev)
        ext.synchronize()
    out, wp = _ask(w, rec, PROX_STATIC)
    after = _readings(out)
    assert after["found"][0] == 0 and np.array_equal(wp.view(np.float32)[0, 0:3], [0.0, 13.0, 0.0]), (after[0], wp[0])
    assert after["found"][1] == 1 and abs(float(after["distance"][1]) - 2.5) <= 64 * EPS * 8
    assert after[2:].tobytes() == before[2:].tobytes()
    w.close()


def test_deleted_mounts_other_mounts_and_disabled_queries(mi):
    w, rec = _carriers(mi, gravity=0.0)
    w.delete_body(4)
    rec = rec.copy()
    rec["mount"][3] = 12                   # = numBodies: no body
    rec["mount"][4] = 0xFFFFFFFE           # no body either (only MI_STATIC_BODY means world space)
    rec["mount"][5] = STATIC_BODY          # world space: the point as it is, the origin
    rec["point"][5] = (0.25, 3.0, 0.0)
    rec["enabled"][1] = 0
    out, wp = _ask(w, rec, PROX_STATIC | PROX_COUNT)
    for i in (1, 2, 3, 4):
        assert not out[i].any() and not wp[i].any(), (i, out[i], wp[i])
    r = _readings(out)
    assert r["found"][0] == 1 and r["found"][5] == 1 and r["collider"][5] == 0 and r["distance"][5] == np.float32(-0.25)
    assert np.array_equal(wp.view(np.float32)[5], [0.25, 3.0, 0.0, 3.0])
    w.close()


def _batch(w, rays, flags):
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    dev, ext = _stream(w)
    with torch.cuda.stream(ext):
        d_rays = torch.from_numpy(rays).to(dev)
        d_out = torch.full((len(rays), 8), SENTINEL, dtype=torch.float32, device=dev)
        code = w.lib.mi_raycast_batch(w.w, ctypes.c_uint32(len(rays)), ctypes.c_void_p(d_rays.data_ptr()), ctypes.c_uint32(flags), ctypes.c_void_p(d_out.data_ptr()))
        ext.synchronize()
        out = d_out.cpu().numpy()
    assert code == MI_OK, code
    return np.ascontiguousarray(out).view(np.uint32)


def test_proximity_calls_and_ray_casts_do_not_disturb_each_other(mi, random_world):
    cw, rec = random_world
    _, rays = rcu.random_world()
    w = cw.instantiate(mi.World())
    dev, ext = _stream(w)
    a, _ = _ask(w, rec, PROX_STATIC | PROX_COUNT)
    b = _batch(w, rays[:512], 1)
    a2, _ = _ask(w, rec, PROX_STATIC | PROX_COUNT)
    b2 = _batch(w, rays[:512], 1)
    bodies_only, _ = _ask(w, rec[:3], PROX_BRUTE_FORCE)          # another candidate set, leaves only
    b3 = _batch(w, rays[:512], 1)
    a3, _ = _ask(w, rec, PROX_STATIC | PROX_COUNT)
    # back to back on the stream, no host synchronisation in between
    with torch.cuda.stream(ext):
        d_q = torch.from_numpy(rec.view(np.float32).reshape(-1, 8).copy()).to(dev)
        d_r = torch.from_numpy(rays[:512].copy()).to(dev)
        o1, o2 = torch.empty((len(rec), 12), device=dev), torch.empty((512, 8), device=dev)
        o3, o4 = torch.empty((len(rec), 12), device=dev), torch.empty((512, 8), device=dev)
        for dq, do, kind in ((d_q, o1, 0), (d_r, o2, 1), (d_q, o3, 0), (d_r, o4, 1)):
            if kind == 0:
                assert w.lib.mi_proximity(w.w, ctypes.c_uint32(len(rec)), ctypes.c_void_p(dq.data_ptr()), ctypes.c_uint32(PROX_STATIC | PROX_COUNT), ctypes.c_void_p(do.data_ptr()), None) == MI_OK
            else:
                assert w.lib.mi_raycast_batch(w.w, ctypes.c_uint32(512), ctypes.c_void_p(dq.data_ptr()), ctypes.c_uint32(1), ctypes.c_void_p(do.data_ptr())) == MI_OK
        ext.synchronize()
        o = [x.cpu().numpy().view(np.uint32) for x in (o1, o2, o3, o4)]
    _same(a, a2, "proximity after a ray cast"); _same(a, a3, "proximity after a shorter call"); _same(b, b2, "ray cast after proximity"); _same(b, b3, "ray cast after a leaves-only build")
    _same(o[0], a, "back to back"); _same(o[2], a, "back to back"); _same(o[1], b, "back to back"); _same(o[3], b, "back to back")
    w.close()


# ---- 8: the façade ---------------------------------------------------------------------------------------------------------------------------
def test_facade_proximity_example(tmp_path):
    host = os.path.join(ROOT, "directx-renderer-kurth_amd", "host")
    lib_dir = os.path.join(ROOT, "directx-renderer-kurth_amd")
    exe = str(tmp_path / "example_proximity")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(host, "example_proximity.cpp"),
                    "-L" + lib_dir, "-lmi_physics", "-Wl,-rpath," + lib_dir, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    lines = {l.split()[0]: [float(x) for x in l.split()[1:]] for l in out.strip().splitlines()}
    # pelvis sphere (radius 0.15) at (0, 1, 0); a box with its face at x = 1; an octahedron hull with its tip at (0, 1, -0.8)
    assert lines["self"][0] == pytest.approx(-0.15, abs=1e-6), "without exclusion the sensor at the pelvis centre reports the pelvis"
    d, nx, ny, nz = lines["box"]
    assert abs(d - 0.4) <= 1e-5 and np.abs(np.array([nx, ny, nz]) - [-1, 0, 0]).max() <= 1e-6, "the sensor 0.6 m to the pelvis's right"
    d, nx, ny, nz = lines["hull"]
    assert abs(d - 0.8) <= 1e-5 and np.abs(np.array([nx, ny, nz]) - [0, 0, 1]).max() <= 1e-5
    assert lines["count"] == [2.0] and lines["count_near"] == [0.0] and lines["count_all"] == [3.0]
