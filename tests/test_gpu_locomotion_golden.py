"""The learned controller's kernels (host/locomotion_layers.h, locomotion_batch.hip, locomotion_update.hip) against bits recorded on the
device: tests/golden/locomotion_networks.npz, written by tests/golden/make_locomotion_golden.py from record() below.  The other tests
pin the linear layers bit for bit but allow tanh K_DEVICE ulp and hold the gradient step to a float64 oracle at a tolerance; a change
that reorders a sum of the backward pass passes them.  Here every array is equal, uint32 for uint32: a condition, not a tolerance.

Every input comes from fixed seeds (policy_util.make_policy, training_util.make_value_network, numpy.random.default_rng); the fixture
holds outputs only, and only of entry points whose recorded values depend on no physics step.  Two shapes: (H, Hv) = (12, 68) is a
two-wave block with the critic's last layer on lane 64 and hidden sizes that are no multiples of 4 or 64 and unequal; (12, 20) is a
one-wave block with the critic on lane 32.  Per shape:
  act, values   5 rows with the hidden vectors: a tile of 4 and a remainder of 1
  collect       row 0 of collect(1) on 5 fresh environments at log_std -1: what k_loco_sample writes before the first step
  gradients     ppo_gradients on 517 of 520 rows through a permutation: 130 tiles for 128 groups, so two groups add a second tile into
                their slab row, and the last tile holds one row
  update        parameters() and the statistics after 2 epochs of minibatches of 128 (the last of 8) over the 520 rows, ent_coef 0.01
A tensor is stored in full, or, where the file would pass the size of the largest fixture, as its SHA-256 under "sha256/<name>"."""
import hashlib
import os

import numpy as np
import pytest
import torch  # before libmi_physics.so is loaded: the process then uses torch's HIP runtime for both

import policy_util as pu
import ppo_util as ppo
import training_util as tu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "locomotion_networks.npz")
SHAPES = [(12, 68), (12, 20)]
ROWS, GATHERED, BATCH, EPOCHS, ENVS, LOG_STD = 520, 517, 128, 2, 5, -1.0


def _forward64(net, x):
    """The network in float64 with every sum in one written-out order (ascending input), so that the inputs below do not depend on a
    matrix product's blocking: (tanh(z2), output)."""
    def layer(w, b, rows):
        total = np.zeros((rows.shape[0], w.shape[0]), np.float64)
        for i in range(w.shape[1]):
            total = total + rows[:, i:i + 1] * w[None, :, i].astype(np.float64)
        return total + b.astype(np.float64)[None, :]
    w1, b1, w2, b2, w3, b3 = net
    hidden = np.tanh(layer(w2, b2, np.tanh(layer(w1, b1, x.astype(np.float64)))))
    return layer(w3, b3, hidden)


def make_inputs(hidden, value_hidden):
    """Networks, 520 rows in ppo_util.make_case's recipe (old log-probabilities around the networks' own, so that ratios fall on both
    sides of the clip range; advantages of both signs), the gathered minibatch and the epochs' permutations."""
    rng = np.random.default_rng(100 * hidden + value_hidden)
    policy, critic = pu.make_policy(hidden, seed=hidden + 1, action_gain=0.5), tu.make_value_network(value_hidden, seed=value_hidden + 2)
    log_std = np.full(pu.ACTION, LOG_STD, np.float32)
    states = rng.normal(0.0, 1.0, (ENVS, pu.STATE)).astype(np.float32)
    obs = rng.normal(0.0, 1.0, (ROWS, pu.STATE)).astype(np.float32)
    std = np.exp(log_std.astype(np.float64))
    mu = _forward64(policy, obs)
    actions = (mu + std * rng.normal(0.0, 1.0, (ROWS, pu.ACTION))).astype(np.float32)
    z = (actions.astype(np.float64) - mu) / std
    lp64 = (-0.5 * z * z - log_std.astype(np.float64)).sum(-1) - tu.LOG_PROB_CONSTANT64
    old = (lp64 + ppo.DELTAS[rng.integers(0, len(ppo.DELTAS), ROWS)]).astype(np.float32)
    advantages = (rng.choice([-1.0, 1.0], ROWS) * (0.05 + np.abs(rng.normal(0.0, 1.0, ROWS)))).astype(np.float32)
    returns = (_forward64(critic, obs)[:, 0] + rng.normal(0.0, 0.5, ROWS)).astype(np.float32)
    gathered = rng.permutation(ROWS)[:GATHERED]
    order = np.stack([rng.permutation(ROWS) for _ in range(EPOCHS)])
    return dict(policy=policy, critic=critic, log_std=log_std, states=states, rows=(obs, actions, old, advantages, returns), gathered=gathered, order=order)


def record(mi, hidden, value_hidden):
    """name -> float32 numpy array: everything the fixture holds for one shape, from the library as it is."""
    x = make_inputs(hidden, value_hidden)
    batch = mi.LocomotionBatch(ENVS, seed=77)

    def load():
        batch.set_policy(*x["policy"]); batch.set_value_network(*x["critic"]); batch.set_log_std(x["log_std"])
    load()
    out = {}
    for name, result in (("act", batch.act(x["states"], hidden=True)), ("values", batch.values(x["states"], hidden=True))):
        out.update(zip((name, name + "/a", name + "/b"), result))
    data = batch.collect(1, clip=True)   # the batch is fresh: k_loco_sample sees the spawn states and noise counter 0
    for name in ("obs", "actions", "eps", "log_probs", "values"):
        out["collect/" + name] = data[name][0]
    rows = [torch.from_numpy(r).cuda() for r in x["rows"]]
    gradients, ratios, stats = batch.ppo_gradients(*rows, indices=x["gathered"], ent_coef=0.01)
    out.update(("gradients/" + k, v) for k, v in gradients.items())
    out["gradients/ratios"], out["gradients/stats"] = ratios, stats
    load()
    batch.begin_training(lr=1e-3)
    out["update/stats"] = batch.ppo_update(*rows, x["order"], BATCH, ent_coef=0.01)
    out.update(("update/" + k, v) for k, v in batch.parameters().items())
    batch.end_training()
    return {k: np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, np.float32) for k, v in out.items()}


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).digest(), np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("hidden,value_hidden", SHAPES)
def test_bits_against_the_recording(mi, hidden, value_hidden):
    golden = np.load(FIXTURE, allow_pickle=False)
    prefix = "h%d_v%d/" % (hidden, value_hidden)
    got = record(mi, hidden, value_hidden)
    stored = {k[len(prefix):] for k in golden.files if k.startswith(prefix)}
    assert stored == {k if k in stored else "sha256/" + k for k in got}, sorted(stored)
    wrong = []
    for name, value in sorted(got.items()):
        assert np.isfinite(value).all(), name
        if name in stored:
            expected = golden[prefix + name]
            assert expected.dtype == np.uint32 and expected.shape == value.shape, name
            if not np.array_equal(value.view(np.uint32), expected):
                wrong.append((name, np.argwhere(value.view(np.uint32) != expected)[:4].tolist()))
        elif not np.array_equal(digest(value), golden[prefix + "sha256/" + name]):
            wrong.append((name, "sha256"))
    assert not wrong, wrong
