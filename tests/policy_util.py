"""Shared by the learned-controller tests: seeded policies, the numpy restatement of applyLayer (host/locomotion_policy.h) and ulp
distances.  The restatement keeps applyLayer's order: per output unit the float32 products are added one by one in ascending input
order, each product and each sum rounded to float32, then the bias; tanh is taken in float64 and rounded."""
import numpy as np

STATE, ACTION = 66, 27
NAMES = ("mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias", "mlp_extractor.policy_net.2.weight",
         "mlp_extractor.policy_net.2.bias", "action_net.weight", "action_net.bias")


def make_policy(hidden, seed, gain=2.2, action_gain=None):
    """W ~ U(-s, s) with s = gain / sqrt(fan-in) per layer (action_gain for the last one), biases ~ U(-0.1, 0.1).  With unit-scale inputs
    gain 2.2 puts the hidden pre-activations at a spread of about 1: part of the units in tanh's linear range, part saturated."""
    rng = np.random.default_rng(seed)
    out = []
    for (rows, cols), g in zip(((hidden, STATE), (hidden, hidden), (ACTION, hidden)), (gain, gain, gain if action_gain is None else action_gain)):
        s = g / np.sqrt(cols)
        out += [rng.uniform(-s, s, (rows, cols)).astype(np.float32), rng.uniform(-0.1, 0.1, rows).astype(np.float32)]
    return out


def layer_sums(weights, bias, rows):
    """z [count, out] of applyLayer before the activation, for rows [count, in]."""
    weights = np.asarray(weights, np.float32); rows = np.asarray(rows, np.float32)
    total = np.zeros((rows.shape[0], weights.shape[0]), np.float32)
    for x in range(weights.shape[1]):
        total = total + rows[:, x:x + 1] * weights[None, :, x]   # float32 product, then float32 sum
    assert total.dtype == np.float32
    return total + np.asarray(bias, np.float32)[None, :]


def tanh32(z):
    return np.tanh(z.astype(np.float64)).astype(np.float32)


def ordered(a):
    """float32 -> int64 that orders like the floats, so that a difference is a distance in ulps."""
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulps(a, b):
    return np.abs(ordered(a) - ordered(b))


def tanh_sweep_points():
    """2^20 float32 points spanning [-10, 10], as [16384, 64]."""
    return np.linspace(-10.0, 10.0, 1 << 20).astype(np.float32).reshape(-1, 64)


def identity_policy():
    """H = 64 with W1 = [I | 0] and b1 = 0: unit j of the first layer is tanhf(x[j]) of exactly x[j] (1 * x is exact, every other product is
    a zero), so the first hidden vector samples the library's tanhf at the inputs."""
    h = 64
    w1 = np.zeros((h, STATE), np.float32); w1[np.arange(h), np.arange(h)] = 1.0
    return [w1, np.zeros(h, np.float32), np.zeros((h, h), np.float32), np.zeros(h, np.float32), np.zeros((ACTION, h), np.float32), np.zeros(ACTION, np.float32)]


def check_against_formula(policy, states, actions, a, b, k):
    """The three checks of one inference: a within k ulp of tanh(z1 restated from the inputs), b within k ulp of tanh(z2 restated from the
    given a), actions bit-equal to layer 3 restated from the given b.  Returns the two maxima in ulp."""
    w1, b1, w2, b2, w3, b3 = policy
    da = ulps(a, tanh32(layer_sums(w1, b1, states)))
    db = ulps(b, tanh32(layer_sums(w2, b2, a)))
    print("tanh distance to float64, ulp: layer 1 max %d, layer 2 max %d (allowed %d)" % (da.max(), db.max(), k))
    assert da.max() <= k, int(da.max())
    assert db.max() <= k, int(db.max())
    expected = layer_sums(w3, b3, b)
    assert np.array_equal(actions.view(np.uint32), expected.view(np.uint32)), np.abs(actions - expected).max()
    return int(da.max()), int(db.max())
