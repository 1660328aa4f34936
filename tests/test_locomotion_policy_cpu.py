"""The learned controller's network on the host (libmi_locomotion.so: setPhysicsPolicy / inferPhysicsPolicy, host/locomotion_policy.h),
without a GPU: the library is loaded with ctypes as test_abi.py loads libmi_physics.so.  inferPhysicsPolicy is pinned to a numpy
restatement of applyLayer (policy_util.py) layer by layer: the two tanh vectors within K_HOST ulp of float64 tanh, the last, linear
layer bit for bit.

K_HOST: test_host_tanhf_sweep samples the library's tanhf (glibc's) at 2^20 points of [-10, 10] through an identity first layer; the
measured maximum distance to float64 tanh is 2 ulp.  K_HOST is that plus 1 ulp, because the sweep is a sample, not a proof."""
import ctypes as C

import numpy as np
import pytest

import policy_util as pu

TANHF_HOST_MEASURED = 2
K_HOST = TANHF_HOST_MEASURED + 1
NEW_SYMBOLS = ["setPhysicsPolicy", "inferPhysicsPolicy", "updatePhysicsPolicy", "inferPhysicsBatchDevice", "updatePhysicsBatchPolicy",
               "updatePhysicsBatchPolicyDevice", "rolloutPhysicsBatchDevice"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def lib(mi):
    mi.build()
    return C.CDLL(mi.LOCOMOTION_LIB_PATH)


def set_policy(lib, policy, hidden=None):
    return lib.setPhysicsPolicy(C.c_uint32(policy[1].size if hidden is None else hidden), *[_p(a) if a is not None else None for a in policy])


def infer(lib, states, hidden):
    actions = np.zeros((len(states), pu.ACTION), np.float32); ab = np.zeros((len(states), 2 * hidden), np.float32)
    for i, s in enumerate(np.ascontiguousarray(states, np.float32)):
        assert lib.inferPhysicsPolicy(_p(s), _p(actions[i]), _p(ab[i])) == 0
    return actions, np.ascontiguousarray(ab[:, :hidden]), np.ascontiguousarray(ab[:, hidden:])


def seeded_states(count, seed=2):
    return np.random.default_rng(seed).normal(0.0, 1.0, (count, pu.STATE)).astype(np.float32)


def test_policy_exports_resolve(mi, lib):
    for name in NEW_SYMBOLS:
        assert name in mi.LOCOMOTION_SYMBOLS, name
        assert hasattr(lib, name), name
    # without a batch the device entry points refuse instead of touching a world
    assert lib.inferPhysicsBatchDevice(1, None, None, None) != 0
    assert lib.updatePhysicsBatchPolicy(None, None, None) < 0
    assert lib.updatePhysicsBatchPolicyDevice(None, None, None, None) != 0
    assert lib.rolloutPhysicsBatchDevice(1, 1, None, None, None, None) != 0


def test_host_tanhf_sweep(lib):
    assert set_policy(lib, pu.identity_policy()) == 0
    points = pu.tanh_sweep_points()
    states = np.zeros((len(points), pu.STATE), np.float32); states[:, :64] = points
    _, a, _ = infer(lib, states, 64)
    worst = int(pu.ulps(a, pu.tanh32(points)).max())
    print("host tanhf against float64 over 2^20 points of [-10, 10]: max %d ulp" % worst)
    assert worst <= TANHF_HOST_MEASURED


@pytest.mark.parametrize("hidden", [128, 40])
def test_infer_matches_apply_layer(lib, hidden):
    policy = pu.make_policy(hidden, seed=1)
    states = seeded_states(256)
    # the weight scale exercises tanh: pre-activations roughly within |z| <= 3, neither all linear nor all saturated
    z1 = pu.layer_sums(policy[0], policy[1], states)
    z2 = pu.layer_sums(policy[2], policy[3], pu.tanh32(z1))
    for z in (z1, z2):
        m = np.abs(z)
        assert np.quantile(m, 0.99) <= 3.5 and 0.3 <= np.median(m) <= 1.5, (np.quantile(m, 0.99), np.median(m))
        assert (m < 0.5).mean() >= 0.15 and (m > 2.0).mean() >= 0.01, ((m < 0.5).mean(), (m > 2.0).mean())
    assert set_policy(lib, policy) == 0
    states = np.concatenate([states, np.zeros((1, pu.STATE), np.float32), np.full((1, pu.STATE), 50.0, np.float32), np.full((1, pu.STATE), -50.0, np.float32)])
    actions, a, b = infer(lib, states, hidden)
    pu.check_against_formula(policy, states, actions, a, b, K_HOST)
    # hidden may be NULL
    alone = np.zeros(pu.ACTION, np.float32)
    assert lib.inferPhysicsPolicy(_p(states[3]), _p(alone), None) == 0
    assert np.array_equal(alone.view(np.uint32), actions[3].view(np.uint32))


def test_argument_errors_leave_the_previous_policy(lib):
    INVALID_ARGUMENT = 2
    policy = pu.make_policy(40, seed=3)
    assert set_policy(lib, policy) == 0
    state = seeded_states(1)[0]
    before = np.zeros(pu.ACTION, np.float32)
    assert lib.inferPhysicsPolicy(_p(state), _p(before), None) == 0
    other = pu.make_policy(40, seed=4)
    assert set_policy(lib, other, hidden=0) == INVALID_ARGUMENT
    assert set_policy(lib, pu.make_policy(257, seed=4)) == INVALID_ARGUMENT
    for missing in range(6):
        broken = list(other); broken[missing] = None
        assert set_policy(lib, broken, hidden=40) == INVALID_ARGUMENT, missing
    after = np.zeros(pu.ACTION, np.float32)
    assert lib.inferPhysicsPolicy(_p(state), _p(after), None) == 0
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert lib.inferPhysicsPolicy(None, _p(after), None) == INVALID_ARGUMENT
    assert lib.inferPhysicsPolicy(_p(state), None, None) == INVALID_ARGUMENT
    # a valid set replaces it
    assert set_policy(lib, other) == 0
    assert lib.inferPhysicsPolicy(_p(state), _p(after), None) == 0
    assert not np.array_equal(before, after)


def test_python_policy_mapping(mi, lib):
    policy = pu.make_policy(128, seed=5)
    mi.set_policy(dict(zip(pu.NAMES, policy)))
    state = seeded_states(1)[0]
    action, a, b = mi.infer_policy(state, hidden=True)
    expected = np.zeros(pu.ACTION, np.float32)
    assert set_policy(lib, policy) == 0 and lib.inferPhysicsPolicy(_p(state), _p(expected), None) == 0
    assert np.array_equal(action.view(np.uint32), expected.view(np.uint32)) and a.shape == b.shape == (128,)
    with pytest.raises(ValueError):
        mi.set_policy(*policy[:5])
    with pytest.raises(ValueError):
        mi.set_policy(policy[0][:, :60], *policy[1:])
