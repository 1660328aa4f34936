"""Collecting PPO training data on the device (host/locomotion_batch.hip: k_loco_sample, k_loco_policy<1, false>, k_loco_noise, k_loco_gae) and
the trainer over it (training.py).  Everything the device adds is pinned to something that existed before or to a restatement
(training_util.py): the critic to applyLayer's sums like the policy; the noise to the integer hash bit for bit and to float64 Box-Muller
at a measured tolerance; GAE to its float32 order bit for bit; collect() with std = 0 to rollout() bit for bit; collect() with noise to
step() driven from the host with the same clamped actions, bit for bit.

NOISE_DEVICE_MEASURED: the largest |eps - eps64| over noise(0, 607) with 64 environments (about 2^20 samples; OCML's logf, cosf, sqrtf).
RATIO_DEV_MEASURED: the largest |ratio - 1| of the device's log-probabilities against the float64 statement of the network over the two
iterations of test_trainer_plumbing, before the first optimiser step of each.  Both are allowed 4 x: the runs are samples."""
import ctypes as C

import numpy as np
import pytest
import torch  # before libmi_physics.so is loaded: the process then uses torch's HIP runtime for both

import policy_util as pu
import training_util as tu
from test_locomotion_training_cpu import NOISE_HOST_MEASURED
from test_gpu_locomotion_policy import K_DEVICE, ROLLOUT_ACTION_GAIN, ROLLOUT_SEED, ROLLOUT_STEPS, bits, same

NOISE_DEVICE_MEASURED = 1.535e-6
RATIO_DEV_MEASURED = 6.083e-6
CLIP_RANGE = 0.1


def cpu(t):
    return t.detach().cpu().numpy()


def action_ranges(lib):
    smin = np.zeros(66, np.float32); smax = np.zeros(66, np.float32); amin = np.zeros(27, np.float32); amax = np.zeros(27, np.float32)
    lib.getPhysicsRanges(*[a.ctypes.data_as(C.c_void_p) for a in (smin, smax, amin, amax)])
    assert (amin <= amax).all() and (amax > amin).any()
    return amin, amax


@pytest.mark.gpu
@pytest.mark.parametrize("hidden,value_hidden", [(128, 128), (40, 256), (256, 40)])
def test_critic_kernel_against_formula(mi, hidden, value_hidden):
    batch = mi.LocomotionBatch(2, seed=1)
    batch.set_policy(*pu.make_policy(hidden, seed=1))
    net = tu.make_value_network(value_hidden, seed=2)
    batch.set_value_network(*net)
    assert batch.hidden == hidden and batch.value_hidden == value_hidden
    rng = np.random.default_rng(7)
    for count in (1, 63, 65, 257):
        states = rng.normal(0.0, 1.0, (count, pu.STATE)).astype(np.float32)
        if count >= 63:
            states[5] = 0.0; states[17] = 50.0; states[40] = -50.0; states[count - 1, ::2] = 50.0
        values, a, b = batch.values(states, hidden=True)
        assert values.shape == (count,) and a.shape == b.shape == (count, value_hidden)
        print("rows %d, Hv %d:" % (count, value_hidden), end=" ")
        tu.check_value_against_formula(net, states, values, a, b, K_DEVICE)
        t = batch.values(torch.from_numpy(states).cuda())
        assert t.is_cuda and same(t, values)
    # the critic survives a reset, as the policy does
    batch.reset()
    assert same(batch.values(states), values)


@pytest.mark.gpu
def test_noise(mi):
    seed, updates = 77, 607
    batch = mi.LocomotionBatch(64, seed=seed)
    eps = cpu(batch.noise(0, updates))
    assert eps.shape == (updates, 64, 27) and batch.noise_counter == 0
    _, _, u1, u2 = tu.noise_uniforms(seed, np.arange(64), np.arange(updates))
    worst = float(np.abs(eps.astype(np.float64) - tu.noise64(u1, u2)).max())
    count = eps.size
    mean, var = float(eps.astype(np.float64).mean()), float(eps.astype(np.float64).var())
    print("device noise against float64 Box-Muller over %d samples: max |difference| %.3e (recorded %.3e); mean %.2e, variance - 1 %.2e"
          % (count, worst, NOISE_DEVICE_MEASURED, mean, var - 1.0))
    assert worst <= 4.0 * NOISE_DEVICE_MEASURED
    assert abs(mean) <= 5.0 / np.sqrt(count) and abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / count)
    # different environments and different updates differ
    assert len({eps[0, e].tobytes() for e in range(64)}) == 64 and len({eps[u, 0].tobytes() for u in range(updates)}) == updates
    # a window that starts later is the same function
    assert same(batch.noise(600, 7), eps[600:])
    # the rows of environment e do not depend on the number of environments
    rows = {}
    for n in (4, 16):
        batch = mi.LocomotionBatch(n, seed=seed)
        rows[n] = cpu(batch.noise(3, 9))
    assert same(rows[4], rows[16][:, :4]) and same(rows[16], eps[3:12, :16])
    # the host twin draws from the same integers: equal up to the two libms
    host = np.stack([mi.sample_noise(seed, e, 5) for e in range(16)])
    assert np.abs(host.astype(np.float64) - rows[16][2].astype(np.float64)).max() <= 4.0 * NOISE_DEVICE_MEASURED + 4.0 * NOISE_HOST_MEASURED


@pytest.mark.gpu
@pytest.mark.parametrize("steps,n", [(1, 1), (2, 65), (33, 64), (128, 7)])
def test_gae_bit_equal(mi, steps, n):
    batch = mi.LocomotionBatch(1, seed=1)
    rng = np.random.default_rng(steps * 1000 + n)
    r = rng.uniform(0.0, 1.0, (steps, n)).astype(np.float32); v = rng.normal(0.0, 2.0, (steps, n)).astype(np.float32); last = rng.normal(0.0, 2.0, n).astype(np.float32)
    random = (rng.uniform(size=(steps, n)) < 0.1).astype(np.int32)
    last_row = random.copy(); last_row[-1, 0] = 1; last_row[-1, n // 2] = 1
    for name, d in (("none", np.zeros((steps, n), np.int32)), ("all", np.ones((steps, n), np.int32)), ("random", random), ("last row", last_row)):
        for gamma, lam in ((0.99, 0.95), (0.9, 1.0)):
            adv, ret = batch.gae(*[torch.from_numpy(x).cuda() for x in (r, v, d, last)], gamma=gamma, lam=lam)
            e_adv, e_ret = tu.gae32(r, v, d, last, gamma, lam)
            assert same(adv, e_adv) and same(ret, e_ret), (name, gamma, lam, np.abs(cpu(adv) - e_adv).max())
    # all done: the advantage is r - V, nothing bootstraps
    adv, ret = batch.gae(*[torch.from_numpy(x).cuda() for x in (r, v, np.ones((steps, n), np.int32), last)])
    assert same(adv, r - v) and same(ret, (r - v) + v)


def _networks(batch, hidden, value_hidden, log_std, policy_seed=4, action_gain=ROLLOUT_ACTION_GAIN):
    policy = pu.make_policy(hidden, seed=policy_seed, action_gain=action_gain)
    net = tu.make_value_network(value_hidden, seed=5)
    batch.set_policy(*policy); batch.set_value_network(*net); batch.set_log_std(log_std)
    return policy, net


@pytest.mark.gpu
def test_collect_refuses_without_networks(mi):
    batch = mi.LocomotionBatch(2, seed=1)
    lib = batch.lib
    # the library may hold networks from earlier tests of this process: only the argument checks are unconditional
    assert lib.collectPhysicsBatchDevice(1, 1, None, None, None, None, None, None, None, None) != 0
    assert lib.gaePhysicsBatchDevice(1, 1, C.c_float(0.99), C.c_float(0.95), None, None, None, None, None, None) != 0
    assert lib.samplePhysicsBatchNoiseDevice(0, 1, None) != 0
    assert lib.inferPhysicsBatchValueDevice(1, None, None, None) != 0
    assert batch.noise_counter == 0


@pytest.mark.gpu
def test_collect_with_zero_std_equals_rollout(mi):
    n, steps = 16, ROLLOUT_STEPS
    batch = mi.LocomotionBatch(n, seed=ROLLOUT_SEED)
    _networks(batch, 128, 256, np.full(27, -np.inf, np.float32))   # std = exp(-inf) = 0: the sample is the mean
    batch.reset()
    data = {k: cpu(v) for k, v in batch.collect(steps, clip=False).items()}
    assert batch.noise_counter == steps
    eps = cpu(batch.noise(0, steps))
    batch = mi.LocomotionBatch(n, seed=ROLLOUT_SEED)
    first = batch.reset()
    states, actions, rewards, fallen = [cpu(t) for t in batch.rollout(steps)]
    assert same(data["actions"], actions) and same(data["rewards"], rewards) and same(data["dones"], fallen)
    assert same(data["eps"], eps)
    assert same(data["obs"][0], first)
    stand = fallen[:-1] == 0
    assert same(data["obs"][1:][stand], states[:-1][stand])
    # after a fall the networks see the reset state: the head is back above 1 m
    assert (data["obs"][1:][~stand][:, 22] > 1.0).all()
    falls = fallen.sum(0)
    print("falls per environment %s" % falls.tolist())
    assert (falls > 0).sum() >= 2 and (falls == 0).sum() >= 2, falls
    assert same(data["values"], batch.values(data["obs"].reshape(-1, 66)).reshape(steps, n))


@pytest.mark.gpu
def test_collect_equals_host_driven_steps(mi):
    n, steps, seed = 8, 40, 21
    log_std = np.full(27, -1.0, np.float32)
    std = np.exp(log_std.astype(np.float64)).astype(np.float32)
    batch = mi.LocomotionBatch(n, seed=seed)
    policy, net = _networks(batch, 128, 40, log_std)
    batch.reset()
    data = {k: cpu(v) for k, v in batch.collect(steps, clip=True).items()}
    final = batch.observe()[0]
    assert batch.noise_counter == steps
    eps = cpu(batch.noise(0, steps))
    assert same(data["eps"], eps)
    # per row: the sample, the value, the log-probability
    obs = data["obs"].reshape(-1, 66)
    mu = batch.act(obs).reshape(steps, n, 27)
    expected = mu + std[None, None, :] * eps
    assert expected.dtype == np.float32 and same(data["actions"], expected)
    assert same(data["values"], batch.values(obs).reshape(steps, n))
    assert same(data["last_values"], batch.values(final))
    logp64, bound = tu.log_prob_bound(eps, log_std)
    err = np.abs(data["log_probs"].astype(np.float64) - logp64)
    print("log-probability against float64: max |difference| %.3e, smallest bound %.3e" % (err.max(), bound.min()))
    assert (err <= bound).all()
    # ... and bit for bit in the stated float32 order
    total = np.zeros((steps, n), np.float32)
    for j in range(27):
        total = total + ((np.float32(-0.5) * (eps[..., j] * eps[..., j])) - log_std[j])
    assert same(data["log_probs"], total - tu.LOG_PROB_CONSTANT)
    # the environments: a fresh batch stepped from the host with the clamped actions
    lo, hi = action_ranges(batch.lib)
    clamped = np.clip(data["actions"], lo, hi)
    assert (clamped != data["actions"]).any()   # the clamp is at work in this run
    second = batch.collect(steps)
    assert batch.noise_counter == 2 * steps == int(batch.lib.getPhysicsBatchNoiseCounter())
    assert same(second["eps"], batch.noise(steps, steps)) and same(second["obs"][0], final)
    batch = mi.LocomotionBatch(n, seed=seed)
    current = batch.reset()                        # the library keeps the networks
    assert batch.noise_counter == 0
    for t in range(steps):
        assert same(data["obs"][t], current), t
        st, rw, fl = batch.step(clamped[t])
        assert same(data["rewards"][t], rw) and same(data["dones"][t], fl), t
        current = st.copy()
        ids = np.nonzero(fl)[0]
        if len(ids):
            current[ids] = batch.reset_envs(ids)[ids]
    assert same(final, current)
    print("falls per environment %s" % data["dones"].sum(0).tolist())


@pytest.mark.gpu
def test_trainer_plumbing(mi):
    from directx_renderer_kurth_amd import training
    n, hidden = 8, 40
    batch = mi.LocomotionBatch(n, seed=31)
    trainer = training.PPOTrainer(batch, hidden=hidden, value_hidden=hidden, n_epochs=2, batch_size=32, seed=3)
    assert (trainer.clip_range, trainer.gamma, trainer.gae_lambda, trainer.vf_coef, trainer.ent_coef, trainer.max_grad_norm) == (CLIP_RANGE, 0.99, 0.95, 0.5, 0.0, 0.5)
    before = {k: v.clone() for k, v in trainer.model.state_dict().items()}
    worst = 0.0
    for it in range(2):
        stats = trainer.iterate(16)
        print("iteration %d: %s" % (it, stats))
        assert all(np.isfinite(v) for v in stats.values()), stats
        assert stats["rows"] == 16 * n
        worst = max(worst, stats["ratio_dev_first_f64"])
        assert stats["ratio_dev_first"] < CLIP_RANGE / 10
    assert batch.noise_counter == 32
    after = trainer.model.state_dict()
    assert all(torch.isfinite(v).all() for v in after.values())
    changed = [k for k in after if not torch.equal(after[k], before[k])]
    assert set(pu.NAMES) <= set(changed) and set(tu.VALUE_NAMES) <= set(changed) and "log_std" in changed, changed
    print("max |ratio - 1| of the device's log-probabilities against the float64 network: %.3e (recorded %.3e)" % (worst, RATIO_DEV_MEASURED))
    assert 4.0 * RATIO_DEV_MEASURED < CLIP_RANGE / 10      # a condition, not a measurement: the first epoch is not clipped by rounding
    assert worst <= 4.0 * RATIO_DEV_MEASURED
    # after the sync the device networks are the module's
    trainer.sync()
    policy = [cpu(after[k]) for k in pu.NAMES]; net = [cpu(after[k]) for k in tu.VALUE_NAMES]
    states = np.random.default_rng(9).normal(0.0, 1.0, (65, pu.STATE)).astype(np.float32)
    actions, a, b = batch.act(states, hidden=True)
    pu.check_against_formula(policy, states, actions, np.ascontiguousarray(a), np.ascontiguousarray(b), K_DEVICE)
    values, a, b = batch.values(states, hidden=True)
    tu.check_value_against_formula(net, states, values, a, b, K_DEVICE)
