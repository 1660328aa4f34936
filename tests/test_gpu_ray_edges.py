"""The batched push kernel (k_interaction_batch), the host entry point mi_test_physics_interaction and the CPU oracle on the ray battery
of tests/ray64.py, all six collider types: the three must agree bit for bit, and the kernel must agree with the float64 reading
within the bounds measured for the oracle (ray64.MEASURED).  Then the kernel's launch shapes and the life of a push until the step."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch  # before libmi_physics.so is loaded: the process then uses torch's HIP runtime for both

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray64 as r64  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = r64.ray_battery()
FIRST, PER_RAY, SENTINEL, EXTRA = 5, r64.MAX_BODIES_PER_CASE, -7, 64
MI_ERR_INVALID_ARGUMENT = 2
S1 = (0, 0, 0, 0.5)


def _kernel_world(mi):
    """Every case as its own body range of one world: 5 leading bodies no range covers (spheres where many rays pass), then per case
    its scene padded to 3 bodies with collider-less ones; a static collider after every third case keeps the collider indices of
    the bodies from being contiguous."""
    w = mi.World()
    for k in range(FIRST):
        w.add_collider(w.add_body((0.2 * k, 0.1, 0.0)), r64.SPHERE, (0, 0, 0, 0.6), r64.MATERIAL)
    geometry = {}
    for i, c in enumerate(CASES):
        for h in c.scene.hulls:
            if id(h) not in geometry:
                geometry[id(h)] = w.add_hull_geometry(*h)
        ids = [geometry[id(h)] for h in c.scene.hulls]
        got = c.scene.instantiate(w, ids)
        assert got == list(range(FIRST + PER_RAY * i, FIRST + PER_RAY * i + len(got)))
        for _ in range(PER_RAY - len(got)):
            w.add_body((0, 0, 0), gravity_factor=0.0)
        if i % 3 == 0:
            w.add_static_collider(r64.AABB, (-1, -1, -1, 1, 1, 1), r64.MATERIAL, pos=(0.0, -500.0 - i, 0.0))
    return w


@pytest.fixture(scope="module")
def battery(mi, oracle):
    """Per case: what the oracle, the host entry point and the kernel pushed (body, accumulators [6]) and what ray64 expects."""
    orc = r64.run_whole_world(CASES, oracle.OracleWorld, lambda w: w.accumulators())
    host = r64.run_whole_world(CASES, mi.World, lambda w: w.accumulators())
    w = _kernel_world(mi)
    out = w.test_physics_interaction_batch(np.stack([c.ray for c in CASES]), FIRST, PER_RAY, fill=SENTINEL, extra=EXTRA)
    acc, cogs = w.accumulators(), w.mass_properties()[:, 0:3]
    assert np.all(out[len(CASES):] == SENTINEL), "the kernel wrote results past its rays"
    kernel, pushed_bodies = [], set()
    for i, c in enumerate(CASES):
        base = FIRST + PER_RAY * i
        assert out[i] == 0 or base < out[i] <= base + PER_RAY, (c.id, int(out[i]), "a lane that wrote nothing, or a body outside the ray's range")
        pushed = int(out[i]) - 1 - base if out[i] else None
        kernel.append((pushed, acc[out[i] - 1].copy() if out[i] else np.zeros(6, np.float32), cogs[base:base + len(c.scene.bodies)]))
        pushed_bodies.add(int(out[i]) - 1)
    untouched = [b for b in range(len(acc)) if b not in pushed_bodies]
    assert not np.any(acc[untouched]), "a body nobody pushed has a force"
    w.close()
    return [dict(case=c, oracle=o, host=h, kernel=k, expect=c.scene.expect(c.ray, o[2])) for c, o, h, k in zip(CASES, orc, host, kernel)]


def test_kernel_host_and_oracle_push_the_same_body(battery):
    """Every case, the undecided ones too: the three run the same float32 formulas with contraction off."""
    wrong = [(r["case"].id, r["kernel"][0], r["host"][0], r["oracle"][0]) for r in battery if not (r["kernel"][0] == r["host"][0] == r["oracle"][0])]
    assert not wrong, wrong


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_kernel_host_and_oracle_accumulators_are_bit_equal(battery):
    """Force and torque of every case: the same bits on all three.  Only the antiparallel-axis family goes through libm (sinf, cosf of
    rotateFromTo): there the bound measured for the oracle against float64 holds between any two, and nothing else needs the excuse."""
    differ, same_centres = {}, []
    for r in battery:
        same_centres.append(np.array_equal(_bits(r["oracle"][2]), _bits(r["host"][2])) and np.array_equal(_bits(r["oracle"][2]), _bits(r["kernel"][2])))
        k, h, o = r["kernel"][1], r["host"][1], r["oracle"][1]
        if not (np.array_equal(_bits(k), _bits(h)) and np.array_equal(_bits(k), _bits(o))):
            differ.setdefault(r["case"].family, []).append(r)
    assert all(same_centres), "the centres of gravity differ between the worlds: the torques cannot be compared"
    assert set(differ) <= {r64.ANTIPARALLEL}, {f: [(r["case"].id, r["kernel"][1], r["host"][1], r["oracle"][1]) for r in rs] for f, rs in differ.items() if f != r64.ANTIPARALLEL}
    for r in differ.get(r64.ANTIPARALLEL, []):
        e, strength = r["expect"], abs(float(r["case"].ray[3]))
        for a, b in ((r["kernel"][1], r["host"][1]), (r["kernel"][1], r["oracle"][1])):
            assert np.array_equal(_bits(a[0:3]), _bits(b[0:3]))
            err = float(np.abs(a[3:6].astype(np.float64) - b[3:6].astype(np.float64)).max()) / (strength * (1 + e.arm))
            assert err <= r64.bound(r64.ANTIPARALLEL)[1], (r["case"].id, err)


def test_kernel_against_float64(battery):
    """The decided cases: the body ray64 names, the force one rounding from direction * strength, the torque within the family's bound."""
    worst = {}
    for r in battery:
        c, e, (pushed, acc, _) = r["case"], r["expect"], r["kernel"]
        if not e.decided:
            continue
        assert pushed == e.body, (c.id, pushed, e.body)
        if e.body is None:
            continue
        _, ef, eq = r64.errors(c, e, acc)
        worst[c.family] = max(worst.get(c.family, 0.0), eq)
        print("%-60s force %.3g torque %.3g (bound %.3g)" % (c.id, ef, eq, r64.bound(c.family)[1]))
        assert ef <= 2.0 ** -24 and eq <= r64.bound(c.family)[1], (c.id, ef, eq, r64.bound(c.family))
    print({f: "%.3g" % v for f, v in sorted(worst.items())})


# ---- launch shapes ----------------------------------------------------------------------------------------------------------------------
def _row_world(mi, num_bodies):
    """Bodies in a row along x, 3 apart, the six types in turn (two hull geometries); every 7th deleted, every 11th without a collider,
    a static collider after every 4th."""
    w = mi.World()
    hulls = [r64.TETRA, r64.BRICK]
    geometry = [w.add_hull_geometry(*h) for h in hulls]
    bodies, colliders, alive = [], [], []
    for j in range(num_bodies):
        pos = np.array([3.0 * j, 0.0, 0.0], np.float32)
        b = w.add_body(pos, gravity_factor=0.0, linear_damping=0.0, angular_damping=0.0)
        bodies.append((b, pos, r64.IDENT))
        if j % 11 != 10:
            kind = j % 6
            s = np.zeros(10, np.float32)
            shape = r64._local_shape(kind, offset=(0, 0, 0), hull=(j // 6) % 2)
            s[:len(shape)] = shape
            colliders.append((w.add_collider(b, kind, s, r64.MATERIAL), b, kind, s))
        if j % 4 == 3:
            w.add_static_collider(r64.AABB, (-1, -1, -1, 1, 1, 1), r64.MATERIAL, pos=(3.0 * j, -50.0, 0.0))
        alive.append(j % 7 != 6)
    for j in range(num_bodies):
        if not alive[j]:
            w.delete_body(j)
    return w, bodies, colliders, hulls, alive


@pytest.mark.parametrize("first_body", [0, 5])
@pytest.mark.parametrize("per_ray", [1, 3])
@pytest.mark.parametrize("num_rays", [1, 63, 64, 65, 130])
def test_launch_shapes(mi, num_rays, per_ray, first_body):
    """Ray i sees the bodies first_body + i * per_ray ... and no other: vertical rays at one body of the range, rays along the row
    through the whole range and every body after it, disabled rays in between; dead and collider-less bodies inside the ranges."""
    nb = first_body + num_rays * per_ray + 2
    w, bodies, colliders, hulls, alive = _row_world(mi, nb)
    rays = []
    for i in range(num_rays):
        b0 = first_body + i * per_ray
        if i % 2 == 0:
            rays.append(r64.ray((3.0 * (b0 + i % per_ray) + 0.05, 5.0, 0.02), (0, -1, 0), 500.0 + i, enabled=float(i % 5 != 3), unit=False))
        else:
            rays.append(r64.ray((3.0 * b0 - 2.0, 0.03, 0.02), (1, 0, 0), 500.0 + i, enabled=float(i % 5 != 3), unit=False))
    rays = np.stack(rays)
    out = w.test_physics_interaction_batch(rays, first_body, per_ray, fill=SENTINEL, extra=EXTRA)
    acc, cogs = w.accumulators(), w.mass_properties()[:, 0:3]
    assert np.all(out[num_rays:] == SENTINEL)
    want_acc = np.zeros((nb, 6))
    hits = 0
    for i in range(num_rays):
        b0 = first_body + i * per_ray
        e = r64.expect(rays[i], bodies[b0:b0 + per_ray], colliders, hulls, cogs, alive)
        assert e.decided, i
        assert out[i] == (0 if e.body is None else 1 + e.body), (i, int(out[i]), e.body)
        if e.body is not None:
            hits += 1
            kind = [c for c in colliders if c[0] == e.collider][0][2]
            assert np.array_equal(_bits(acc[e.body, 0:3]), _bits(rays[i, 4:7] * rays[i, 3]))
            err = float(np.abs(acc[e.body, 3:6] - e.torque).max()) / (float(rays[i, 3]) * (1 + e.arm))
            assert err <= r64.bound("posed-" + r64.TYPE_NAMES[kind])[1], (i, kind, err)
            want_acc[e.body] = 1
    assert hits >= num_rays // 2
    assert not np.any(acc[want_acc[:, 0] == 0]), "a body outside every hit has a force"
    w.close()


def test_a_range_past_the_last_body_is_rejected(mi):
    w, *_ = _row_world(mi, 10)
    rays = np.stack([r64.ray((3.0 * k + 0.05, 5.0, 0.02), (0, -1, 0), unit=False) for k in range(4)])
    code, out = w._interaction_batch(rays, 5, 2, SENTINEL, EXTRA)       # 5 + 4 * 2 = 13 > 10
    assert code == MI_ERR_INVALID_ARGUMENT
    assert np.all(out == SENTINEL), "the rejected call launched"
    acc = np.ones((10, 6), np.float32)
    # the world keeps its first error, and World.accumulators() would raise it again: the C call fills the buffer all the same
    assert w.lib.mi_debug_read_accumulators(w.w, acc.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(10)) == MI_ERR_INVALID_ARGUMENT
    assert not np.any(acc)
    w.close()


# ---- lifecycle ------------------------------------------------------------------------------------------------------------------------
def _free_spheres(mi, n):
    w = mi.World()
    for k in range(n):
        w.add_collider(w.add_body((3.0 * k, 0, 0), gravity_factor=0.0, linear_damping=0.0, angular_damping=0.0), r64.SPHERE, S1, r64.MATERIAL)
    return w


def _down(k, strength):
    return r64.ray((3.0 * k, 5.0, 0.0), (0, -1, 0), strength, unit=False)    # through the centre of gravity: no torque


VELOCITY_TOL = 4 * 2.0 ** -24     # F * invMass * dt: three float32 roundings


def test_two_batch_calls_before_a_step_accumulate(mi):
    w = _free_spheres(mi, 2)
    assert list(w.test_physics_interaction_batch(np.stack([_down(0, 300.0), _down(1, 700.0)]), 0, 1)) == [1, 2]
    assert list(w.test_physics_interaction_batch(np.stack([_down(0, 150.0), _down(1, 0.0)]), 0, 1)) == [1, 2]
    acc = w.accumulators()
    assert np.array_equal(acc[:, 1], np.array([-450.0, -700.0], np.float32)) and not np.any(acc[:, [0, 2, 3, 4, 5]])
    inv_mass, dt = w.mass_properties()[:, 3].astype(np.float64), 1.0 / 120.0
    w.step_internal(dt, 1)
    v = w.velocities().astype(np.float64)
    want = np.array([-450.0, -700.0]) * inv_mass * float(np.float32(dt))
    assert np.all(np.abs(v[:, 1] - want) <= VELOCITY_TOL * np.abs(want)), (v[:, 1], want)
    assert not np.any(w.accumulators()), "the step did not clear the accumulators"
    w.close()


def test_tables_are_rebuilt_after_a_new_hull_geometry(mi):
    w = _free_spheres(mi, 2)
    w.add_collider(0, r64.HULL, (0, 0, 0, 1, 0, 0, 0, w.add_hull_geometry(*r64.TETRA)), r64.MATERIAL)
    assert list(w.test_physics_interaction_batch(np.stack([_down(0, 300.0), _down(1, 700.0)]), 0, 1)) == [1, 2]
    before = w.accumulators()
    b = w.add_body((6.0, 0, 0), gravity_factor=0.0, linear_damping=0.0, angular_damping=0.0)
    w.add_collider(b, r64.HULL, (0, 0, 0, 1, 0, 0, 0, w.add_hull_geometry(*r64.BRICK)), r64.MATERIAL)
    hit = r64.ray((6.6, 5.0, 0.1), (0, -1, 0), 900.0, unit=False)          # the brick's top face at y = 0.5, outside the tetrahedron's reach
    assert list(w.test_physics_interaction_batch(hit[None], b, 1)) == [1 + b]
    acc, cog = w.accumulators(), w.mass_properties()[:, 0:3]
    assert np.array_equal(acc[:2], before), "the pushes of before the add were lost"
    e = r64.expect(hit, [(b, (6.0, 0, 0), r64.IDENT)], [(3, b, r64.HULL, np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0], np.float32))], [r64.BRICK], cog)
    assert e.body == b and abs(e.t - 4.5) <= 1e-9
    assert np.array_equal(acc[b, 0:3], np.array([0, -900.0, 0], np.float32))
    assert float(np.abs(acc[b, 3:6] - e.torque).max()) / (900.0 * (1 + e.arm)) <= r64.bound("hull")[1] + r64.bound("posed-hull")[1]
    w.close()


@pytest.mark.parametrize("stepped_before", [False, True], ids=["fresh", "state-on-device"])
def test_batch_and_host_pushes_of_one_frame_both_reach_the_step(mi, stepped_before):
    w = _free_spheres(mi, 3)
    dt = 1.0 / 120.0
    if stepped_before:
        w.step_internal(dt, 1)      # nothing moves (no gravity, no force): the state now lives on the device
    assert list(w.test_physics_interaction_batch(_down(0, 300.0)[None], 0, 1)) == [1]
    assert w.test_physics_interaction((6.0, 5.0, 0.0), (0, -1, 0), 700.0) == 2
    inv_mass = w.mass_properties()[:, 3].astype(np.float64)
    w.step_internal(dt, 1)
    v = w.velocities().astype(np.float64)
    want = np.array([-300.0, 0.0, -700.0]) * inv_mass * float(np.float32(dt))
    assert np.all(np.abs(v[:, 1] - want) <= VELOCITY_TOL * np.abs(want)), (v[:, 1], want)
    assert not np.any(v[:, [0, 2, 3, 4, 5]])
    w.close()
