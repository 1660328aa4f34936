"""The training additions of libmi_locomotion.so on the host, without a GPU: the critic (setPhysicsValueNetwork / inferPhysicsValue), the
exploration noise (samplePhysicsNoise) and the PPO loss of training.py.  The critic is pinned like the policy (test_locomotion_policy_cpu):
tanh vectors within K_HOST ulp of float64 tanh, the linear layer bit for bit.  The noise is pinned in two stages: the integer hash and
the two uniforms bit for bit (training_util.noise_uniforms), the float32 Box-Muller against float64 at a measured tolerance.

NOISE_HOST_MEASURED: the largest |eps - eps64| over the sweep of test_host_noise (64 environments x 607 updates x 27 actions, about
2^20 samples; glibc's logf, cosf and sqrtf).  The test allows 4 x that, because the sweep is a sample."""
import ctypes as C

import numpy as np
import pytest

import policy_util as pu
import training_util as tu
from test_locomotion_policy_cpu import K_HOST

NOISE_HOST_MEASURED = 1.534e-6
TRAINING_SYMBOLS = ["setPhysicsValueNetwork", "inferPhysicsValue", "inferPhysicsBatchValueDevice", "setPhysicsActionStd", "samplePhysicsBatchNoiseDevice",
                    "samplePhysicsNoise", "samplePhysicsNoiseUniforms", "getPhysicsBatchNoiseCounter", "collectPhysicsBatchDevice", "gaePhysicsBatchDevice"]
INVALID_ARGUMENT = 2


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def lib(mi):
    mi.build()
    lib = C.CDLL(mi.LOCOMOTION_LIB_PATH)
    lib.samplePhysicsNoise.argtypes = [C.c_ulonglong, C.c_uint32, C.c_ulonglong, C.c_void_p]
    lib.samplePhysicsNoiseUniforms.argtypes = [C.c_ulonglong, C.c_uint32, C.c_ulonglong, C.c_void_p, C.c_void_p]
    lib.samplePhysicsBatchNoiseDevice.argtypes = [C.c_ulonglong, C.c_uint32, C.c_void_p]
    lib.gaePhysicsBatchDevice.argtypes = [C.c_uint32, C.c_uint32, C.c_float, C.c_float] + [C.c_void_p] * 6
    lib.getPhysicsBatchNoiseCounter.restype = C.c_ulonglong
    return lib


def set_value_network(lib, net, hidden=None):
    return lib.setPhysicsValueNetwork(C.c_uint32(net[1].size if hidden is None else hidden), *[_p(a) if a is not None else None for a in net])


def test_training_exports_resolve_and_refuse_without_a_batch(mi, lib):
    for name in TRAINING_SYMBOLS:
        assert name in mi.LOCOMOTION_SYMBOLS, name
        assert hasattr(lib, name), name
    # a policy, a critic and a std are set, and there is still no batch: the device entry points refuse without touching memory
    policy = pu.make_policy(40, seed=1)
    assert lib.setPhysicsPolicy(C.c_uint32(40), *[_p(a) for a in policy]) == 0
    assert set_value_network(lib, tu.make_value_network(40, seed=1)) == 0
    scales = np.zeros(27, np.float32)
    assert lib.setPhysicsActionStd(_p(scales), _p(scales)) == 0
    assert lib.inferPhysicsBatchValueDevice(1, None, None, None) != 0
    assert lib.samplePhysicsBatchNoiseDevice(0, 1, None) != 0
    assert lib.collectPhysicsBatchDevice(1, 1, None, None, None, None, None, None, None, None) != 0
    assert lib.gaePhysicsBatchDevice(1, 1, 0.99, 0.95, None, None, None, None, None, None) != 0
    assert lib.getPhysicsBatchNoiseCounter() == 0
    assert lib.setPhysicsActionStd(None, _p(scales)) == INVALID_ARGUMENT and lib.setPhysicsActionStd(_p(scales), None) == INVALID_ARGUMENT
    assert lib.samplePhysicsNoise(1, 0, 0, None) == INVALID_ARGUMENT


@pytest.mark.parametrize("hidden", [128, 40])
def test_host_critic_matches_apply_layer(lib, hidden):
    net = tu.make_value_network(hidden, seed=11)
    assert set_value_network(lib, net) == 0
    states = np.random.default_rng(2).normal(0.0, 1.0, (256, pu.STATE)).astype(np.float32)
    states = np.concatenate([states, np.zeros((1, pu.STATE), np.float32), np.full((1, pu.STATE), 50.0, np.float32), np.full((1, pu.STATE), -50.0, np.float32)])
    values = np.zeros(len(states), np.float32); ab = np.zeros((len(states), 2 * hidden), np.float32)
    for i, s in enumerate(states):
        assert lib.inferPhysicsValue(_p(s), _p(values[i:i + 1]), _p(ab[i])) == 0
    tu.check_value_against_formula(net, states, values, ab[:, :hidden], ab[:, hidden:], K_HOST)
    alone = np.zeros(1, np.float32)
    assert lib.inferPhysicsValue(_p(states[3]), _p(alone), None) == 0           # hidden may be NULL
    assert alone.view(np.uint32)[0] == values.view(np.uint32)[3]
    # argument errors leave the critic as it is
    assert set_value_network(lib, net, hidden=0) == INVALID_ARGUMENT and set_value_network(lib, tu.make_value_network(257, seed=1)) == INVALID_ARGUMENT
    for missing in range(6):
        broken = list(net); broken[missing] = None
        assert set_value_network(lib, broken, hidden=hidden) == INVALID_ARGUMENT, missing
    assert lib.inferPhysicsValue(None, _p(alone), None) == INVALID_ARGUMENT and lib.inferPhysicsValue(_p(states[3]), None, None) == INVALID_ARGUMENT
    assert lib.inferPhysicsValue(_p(states[3]), _p(alone), None) == 0 and alone.view(np.uint32)[0] == values.view(np.uint32)[3]


def test_python_value_mapping(mi, lib):
    net = tu.make_value_network(40, seed=12)
    mi.set_value_network(dict(zip(tu.VALUE_NAMES, net)))
    state = np.random.default_rng(3).normal(0.0, 1.0, pu.STATE).astype(np.float32)
    value, a, b = mi.infer_value(state, hidden=True)
    expected = np.zeros(1, np.float32)
    assert set_value_network(lib, net) == 0 and lib.inferPhysicsValue(_p(state), _p(expected), None) == 0
    assert np.float32(value).view(np.uint32) == expected.view(np.uint32)[0] and a.shape == b.shape == (40,)
    assert tuple(mi.VALUE_NAMES) == tuple(tu.VALUE_NAMES)
    with pytest.raises(ValueError):
        mi.set_value_network(*net[:5])
    with pytest.raises(ValueError):
        mi.set_value_network(*pu.make_policy(40, seed=1))   # a policy's last layer is not a critic's


def test_host_noise(mi, lib):
    seed, envs, updates = 0x1234567887654321, np.arange(64), np.arange(607)
    k1, k2, u1, u2 = tu.noise_uniforms(seed, envs, updates)
    assert k1.max() < 1 << 24 and k2.max() < 1 << 24 and u1.min() > 0.0 and u1.max() <= 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
    eps = np.zeros(k1.shape, np.float32); g1 = np.zeros(k1.shape, np.float32); g2 = np.zeros(k1.shape, np.float32)
    for u in updates:
        for e in envs:
            assert lib.samplePhysicsNoise(seed, int(e), int(u), _p(eps[u, e])) == 0
            assert lib.samplePhysicsNoiseUniforms(seed, int(e), int(u), _p(g1[u, e]), _p(g2[u, e])) == 0
    # the integer stage: the uniforms are exact, so they carry k1 and k2
    assert np.array_equal(g1.view(np.uint32), u1.view(np.uint32)) and np.array_equal(g2.view(np.uint32), u2.view(np.uint32))
    assert np.array_equal((g1.astype(np.float64) * 2.0 ** 24 - 1).astype(np.uint32), k1) and np.array_equal((g2.astype(np.float64) * 2.0 ** 24).astype(np.uint32), k2)
    worst = float(np.abs(eps.astype(np.float64) - tu.noise64(u1, u2)).max())
    print("host noise against float64 Box-Muller over %d samples: max |difference| %.3e (recorded %.3e)" % (eps.size, worst, NOISE_HOST_MEASURED))
    assert worst <= 4.0 * NOISE_HOST_MEASURED
    # the Python wrapper, another seed, large counters
    assert np.array_equal(mi.sample_noise(seed, 5, 17).view(np.uint32), eps[17, 5].view(np.uint32))
    big = mi.sample_noise(2 ** 64 - 1, 2 ** 32 - 1, 2 ** 63 + 5)
    _, _, b1, b2 = tu.noise_uniforms(2 ** 64 - 1, [2 ** 32 - 1], [2 ** 63 + 5])
    assert np.abs(big.astype(np.float64) - tu.noise64(b1, b2)[0, 0]).max() <= 4.0 * NOISE_HOST_MEASURED
    assert not np.array_equal(mi.sample_noise(seed + 1, 5, 17), eps[17, 5])


def test_gae_restatement_against_float64():
    """The float32 restatement the GPU test pins the kernel to is itself GAE: against a plain float64 recursion on a seeded buffer."""
    rng = np.random.default_rng(4)
    steps, n, gamma, lam = 33, 7, 0.99, 0.95
    r = rng.uniform(0.0, 1.0, (steps, n)).astype(np.float32); v = rng.normal(0.0, 1.0, (steps, n)).astype(np.float32)
    d = (rng.uniform(size=(steps, n)) < 0.1).astype(np.int32); last = rng.normal(0.0, 1.0, n).astype(np.float32)
    d[-1, 0] = 1
    adv, ret = tu.gae32(r, v, d, last, gamma, lam)
    a = np.zeros(n); expected = np.zeros((steps, n))
    for t in range(steps - 1, -1, -1):
        nxt = last if t == steps - 1 else v[t + 1]
        a = r[t] + gamma * nxt * (1 - d[t]) - v[t] + gamma * lam * (1 - d[t]) * a
        expected[t] = a
    assert np.abs(adv - expected).max() <= 1e-4 and np.abs(ret - (expected + v)).max() <= 1e-4


def test_ppo_loss_float64():
    import torch
    from directx_renderer_kurth_amd import training
    rng = np.random.default_rng(5)
    rows, clip = 128, 0.1
    old = rng.normal(-30.0, 3.0, rows); new = old + rng.uniform(-0.3, 0.3, rows)
    adv = rng.normal(0.0, 1.0, rows); values = rng.normal(0.0, 1.0, rows); returns = values + rng.normal(0.0, 0.5, rows); entropy = rng.normal(38.0, 0.1, rows)
    ratio = np.exp(new - old)
    for sign in (1, -1):   # ratios on both sides of the clip range and inside it, with advantages of both signs
        assert ((ratio > 1 + clip) & (sign * adv > 0)).any() and ((ratio < 1 - clip) & (sign * adv > 0)).any() and ((np.abs(ratio - 1) < clip) & (sign * adv > 0)).any()
    for vf_coef, ent_coef in ((0.5, 0.0), (0.25, 0.01)):
        got = training.ppo_loss(*[torch.from_numpy(x) for x in (new, old, adv, values, returns, entropy)], clip_range=clip, vf_coef=vf_coef, ent_coef=ent_coef)
        assert all(t.dtype == torch.float64 for t in got)
        expected = tu.ppo_loss64(new, old, adv, values, returns, entropy, clip, vf_coef, ent_coef)
        for g, e in zip(got[:3], expected):
            assert abs(float(g) - e) <= 1e-12 * abs(e), (float(g), e)
        assert np.allclose(got[3].numpy(), ratio, rtol=1e-12, atol=0.0)
    # the unclipped surrogate differs: the clip is active on this buffer
    assert abs(-(adv * ratio).mean() - expected[1]) > 1e-3
    # the module's names feed set_policy / set_value_network, its action layer starts small, log_std at 0
    model = training.ActorCritic(40, 24)
    state = model.state_dict()
    assert all(k in state for k in pu.NAMES) and all(k in state for k in tu.VALUE_NAMES)
    assert state["action_net.weight"].abs().max() <= 0.01 and not state["action_net.bias"].any() and not state["log_std"].any()
    assert state["value_net.weight"].shape == (1, 24) and state["mlp_extractor.policy_net.2.weight"].shape == (40, 40)
    # Gaussian log-probability and entropy against scipy-free float64 statements
    mean = torch.from_numpy(rng.normal(0, 1, (5, 27))); log_std = torch.from_numpy(rng.normal(-1, 0.3, 27)); act = torch.from_numpy(rng.normal(0, 1, (5, 27)))
    lp = training.gaussian_log_prob(mean, log_std, act).numpy()
    s = np.exp(log_std.numpy())
    e = (-0.5 * ((act.numpy() - mean.numpy()) / s) ** 2 - np.log(s) - 0.5 * np.log(2 * np.pi)).sum(-1)
    assert np.allclose(lp, e, rtol=1e-12)
    assert np.isclose(float(training.gaussian_entropy(log_std)), (0.5 * np.log(2 * np.pi * np.e * s * s)).sum(), rtol=1e-12)
