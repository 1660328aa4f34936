"""The learned controller on the device (host/locomotion_batch.hip: k_loco_policy, rolloutPhysicsBatchDevice) and on the single
environment (updatePhysicsPolicy).  The kernel is pinned to the numpy restatement of applyLayer (policy_util.py): the tanh vectors
within K_DEVICE ulp of float64 tanh, the linear layer bit for bit; the fused update, the rollout and the device-side reset are pinned
bit for bit to the paths that existed before them.  The reference ships no trained network, so what is checked is the arithmetic and
the plumbing, not that a ragdoll walks.

K_DEVICE: test_device_tanhf_sweep samples the device tanhf (OCML) at 2^20 points of [-10, 10] through an identity first layer; the
measured maximum distance to float64 tanh is TANHF_DEVICE_MEASURED ulp.  K_DEVICE is that plus 1 ulp: the sweep is a sample."""
import ctypes as C

import numpy as np
import pytest
import torch  # before libmi_physics.so is loaded: the process then uses torch's HIP runtime for both

import policy_util as pu
from test_gpu_locomotion_batch import motor_words, quiet_seed, smooth

TANHF_DEVICE_MEASURED = 1
K_DEVICE = TANHF_DEVICE_MEASURED + 1
# The rollout case, picked on the GPU: with this seed and last-layer scale 7 of the 16 environments fall within ROLLOUT_STEPS updates (the
# first at update 113, so it runs on for 67 updates after its reset) and 9 never do.  The test asserts at least 2 of each.
ROLLOUT_STEPS, ROLLOUT_SEED, ROLLOUT_ACTION_GAIN = 180, 11, 0.3


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def all_motor_words(batch, mi):
    w = batch.world
    return [motor_words(w, mi, e) for e in range(batch.n)]


def same_motors(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


@pytest.mark.gpu
def test_policy_exports(mi):
    from test_locomotion_policy_cpu import NEW_SYMBOLS
    lib = C.CDLL(mi.LOCOMOTION_LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in mi.LOCOMOTION_SYMBOLS and hasattr(lib, name), name


@pytest.mark.gpu
def test_device_tanhf_sweep(mi):
    batch = mi.LocomotionBatch(1, seed=1)
    batch.set_policy(*pu.identity_policy())
    points = pu.tanh_sweep_points()
    states = np.zeros((len(points), pu.STATE), np.float32); states[:, :64] = points
    _, a, _ = batch.act(states, hidden=True)
    worst = int(pu.ulps(a, pu.tanh32(points)).max())
    print("device tanhf against float64 over 2^20 points of [-10, 10]: max %d ulp" % worst)
    assert worst <= TANHF_DEVICE_MEASURED


@pytest.mark.gpu
@pytest.mark.parametrize("hidden", [128, 40, 256])
def test_kernel_against_formula(mi, hidden):
    batch = mi.LocomotionBatch(2, seed=1)
    policy = pu.make_policy(hidden, seed=1)
    batch.set_policy(*policy)
    rng = np.random.default_rng(7)
    for count in (1, 63, 64, 65, 257, 1000):
        states = rng.normal(0.0, 1.0, (count, pu.STATE)).astype(np.float32)
        if count >= 63:
            states[5] = 0.0; states[17] = 50.0; states[40] = -50.0; states[count - 1, ::2] = 50.0
        actions, a, b = batch.act(states, hidden=True)
        assert actions.shape == (count, 27) and a.shape == b.shape == (count, hidden)
        print("rows %d, H %d:" % (count, hidden), end=" ")
        pu.check_against_formula(policy, states, actions, np.ascontiguousarray(a), np.ascontiguousarray(b), K_DEVICE)
        # tensors in, tensors out, the same bits; without the hidden output too
        t = batch.act(torch.from_numpy(states).cuda())
        assert t.is_cuda and same(t, actions)


@pytest.mark.gpu
def test_fused_update_equals_two_calls(mi):
    n, steps = 8, 30
    seed = quiet_seed(n, steps)
    policy = pu.make_policy(128, seed=2)

    def run(fused):
        batch = mi.LocomotionBatch(n, seed=seed)
        batch.set_policy(*policy)
        batch.reset()
        out = []
        for _ in range(steps):
            if fused == "device":
                st, rw, fl, ac = batch.step_policy(device=True)
                torch.cuda.synchronize()
                st, rw, fl, ac = (t.cpu().numpy() for t in (st, rw, fl, ac))
            elif fused == "host":
                st, rw, fl = batch.step_policy()
                ac = None
            else:
                ac = batch.act(batch.observe()[0])
                st, rw, fl = batch.step(ac)
            out.append((st, rw, fl, ac, all_motor_words(batch, mi)))
        return out

    two, dev, host = run("two calls"), run("device"), run("host")
    for k in range(steps):
        for other in (dev, host):
            assert same(other[k][0], two[k][0]) and same(other[k][1], two[k][1]) and same(other[k][2], two[k][2]), k
            assert same_motors(other[k][4], two[k][4]), k
        assert same(dev[k][3], two[k][3]), k
    assert np.isfinite(two[-1][0]).all() and np.abs(two[-1][0][:, 39:]).max() > 0.0


@pytest.mark.gpu
def test_single_env_and_env_zero(mi):
    seed = quiet_seed(1, 4)
    policy = pu.make_policy(128, seed=3)
    batch = mi.LocomotionBatch(4, seed=seed)
    batch.set_policy(*policy)
    states0 = batch.reset()
    lib = batch.lib
    state0 = np.zeros(66, np.float32); out = np.zeros(66, np.float32); reward = C.c_float(0.0)
    lib.resetPhysics(_fp(state0))
    assert lib.updatePhysicsPolicy(_fp(out), C.byref(reward)) in (0, 1)
    single = smooth(np.zeros(27, np.float32), mi.infer_policy(state0))
    assert same(out[39:66], single)
    st, _, _ = batch.step_policy()
    first = smooth(np.zeros(27, np.float32), batch.act(states0[:1])[0])
    assert same(st[0, 39:66], first)
    print("smoothed action after one update, single environment against env 0 of the batch: max |difference| %.3g (the two tanhf, and the "
          "reset states, which agree to 2e-6)" % np.abs(single - first).max())
    # the Python wrapper of the single environment
    lib.resetPhysics(_fp(state0))
    s, r, fallen = mi.update_policy()
    assert same(s, out) and r == reward.value


def _host_rollout(batch, steps, reset):
    rows = []
    for _ in range(steps):
        st, rw, fl, ac = batch.step_policy(device=True)
        torch.cuda.synchronize()
        rows.append([t.cpu().numpy() for t in (st, ac, rw, fl)])
        ids = np.nonzero(rows[-1][3])[0]
        if reset and len(ids):
            batch.reset_envs(ids)
    return [np.stack([r[i] for r in rows]) for i in range(4)]


@pytest.mark.gpu
def test_rollout_equals_single_updates(mi):
    n, steps = 16, ROLLOUT_STEPS
    policy = pu.make_policy(128, seed=4, action_gain=ROLLOUT_ACTION_GAIN)
    for auto_reset in (True, False):
        batch = mi.LocomotionBatch(n, seed=ROLLOUT_SEED)
        batch.set_policy(*policy)
        batch.reset()
        got = batch.rollout(steps, auto_reset=auto_reset)
        torch.cuda.synchronize()
        got = [t.cpu().numpy() for t in got]
        final = batch.observe()
        batch = mi.LocomotionBatch(n, seed=ROLLOUT_SEED)
        batch.reset()                                  # the library keeps the policy
        expected = _host_rollout(batch, steps, auto_reset)
        for name, g, e in zip(("states", "actions", "rewards", "fallen"), got, expected):
            assert g.shape == e.shape and same(g, e), (auto_reset, name, np.argwhere(bits(g) != bits(e))[:4])
        for g, e in zip(final, batch.observe()):
            assert same(g, e), auto_reset
        falls = got[3].sum(0)
        print("auto_reset %s: falls per environment %s" % (auto_reset, falls.tolist()))
        if auto_reset:
            # the run resets, and not everything: at least 2 environments fall and are reset, at least 2 never fall
            assert (falls > 0).sum() >= 2 and (falls == 0).sum() >= 2, falls
            # a reset environment stands again: after the update that follows its first fall its head is above 1 m
            e = int(np.argmax(falls > 0)); t = int(np.argmax(got[3][:, e]))
            assert t + 1 < steps and got[0][t + 1, e, 22] > 1.0 and not got[3][t + 1, e]


@pytest.mark.gpu
def test_existing_updates_unchanged_and_current_state_tracked(mi):
    n = 8
    seed = quiet_seed(n, 10)
    rng = np.random.default_rng(5)
    acts = [rng.uniform(-0.6, 0.6, (n, 27)).astype(np.float32) for _ in range(10)]
    policy = pu.make_policy(128, seed=6)
    batch = mi.LocomotionBatch(n, seed=seed)
    batch.set_policy(*policy)
    batch.reset()
    ref = [batch.step(a) for a in acts]
    # the policy's input follows the host update ...
    st, rw, fl, ac = batch.step_policy(device=True)
    assert same(ac, batch.act(ref[-1][0]))
    # ... a reset of some environments ...
    rows = batch.reset_envs([1, 6])
    current = st.cpu().numpy(); current[[1, 6]] = rows[[1, 6]]
    st, rw, fl, ac = batch.step_policy(device=True)
    assert same(ac, batch.act(current))
    # the device variant, a policy loaded, reproduces the host variant bit for bit
    batch = mi.LocomotionBatch(n, seed=seed)
    batch.reset()
    for k, a in enumerate(acts):
        st, rw, fl = batch.step(torch.from_numpy(a).cuda())
        torch.cuda.synchronize()
        assert same(st, ref[k][0]) and same(rw, ref[k][1]) and same(fl, ref[k][2]), k
    # ... and the update into the caller's buffers
    st2, rw2, fl2, ac = batch.step_policy(device=True)
    assert same(ac, batch.act(st))
