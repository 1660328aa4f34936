"""The PPO gradient step on the device (host/locomotion_update.hip: k_loco_ppo_backward, k_loco_ppo_reduce, k_loco_ppo_adam) against the
float64 oracle of ppo_util.py (the numpy statement that test_locomotion_update_cpu.py pins to training.py's loop in float64), over the
shapes and configurations listed there.  The device is allowed 4 x what training.py's own float32 path measures against the same oracle
on the CPU (GRAD_DEV_MEASURED, ADAM_DEV_MEASURED, and STATS_DEV_MEASURED for the statistics rows): the same float32 arithmetic in another
summation order."""
import ctypes as C

import numpy as np
import pytest
import torch  # before libmi_physics.so is loaded: the process then uses torch's HIP runtime for both

import policy_util as pu
import ppo_util as ppo
import training_util as tu
from test_gpu_locomotion_policy import K_DEVICE
from test_gpu_locomotion_training import RATIO_DEV_MEASURED
from test_locomotion_update_cpu import ADAM_DEV_MEASURED, GRAD_DEV_MEASURED, STATS_DEV_MEASURED

CASES = ppo.all_cases()


def load(mi, case):
    batch = mi.LocomotionBatch(1, seed=1)
    batch.set_policy(case["state"]); batch.set_value_network(case["state"]); batch.set_log_std(case["state"]["log_std"])
    data = [torch.from_numpy(case[k]).cuda() for k in ("obs", "actions", "old_log_probs", "advantages", "returns")]
    return batch, data


def settings(case):
    return dict(clip_range=ppo.CLIP_RANGE, vf_coef=ppo.VF_COEF, ent_coef=case["ent_coef"])


def check_stats(got, expected, what):
    """Statistics rows against the oracle's, within 4 x what training.py's float32 loop measures on the same runs (ppo_util.stats_deviation)."""
    worst = ppo.stats_deviation(got, expected)
    print("%s: statistics against the oracle %.3e (allowed %.3e)" % (what, worst, 4.0 * STATS_DEV_MEASURED))
    assert worst <= 4.0 * STATS_DEV_MEASURED, what


@pytest.mark.gpu
@pytest.mark.parametrize("hidden,value_hidden,config", CASES)
def test_gradients_against_the_oracle(mi, hidden, value_hidden, config):
    case = ppo.make_case(hidden, value_hidden, config)
    batch, data = load(mi, case)
    before = batch.parameters()
    for idx in ppo.gradient_minibatches(case):
        expected, ratio64, stats64, margins = ppo.gradients64(case["state"], case, idx)
        assert min(margins) > ppo.MARGIN, margins
        grads, ratios, stats = batch.ppo_gradients(*data, indices=idx, **settings(case))
        got = {k: v.cpu().numpy() for k, v in grads.items()}
        host = ppo.torch_loop(case, [idx], 1e-3, torch.float32, step=False)[1]
        device, loop = ppo.gradient_deviation(got, expected), ppo.gradient_deviation(host, expected)
        print("%s, %d rows: gradients against the oracle: device %.3e (%s), training.py in float32 %.3e (%s), allowed %.3e"
              % (config, len(idx), device[0], device[1], loop[0], loop[1], 4.0 * GRAD_DEV_MEASURED))
        assert device[0] <= 4.0 * GRAD_DEV_MEASURED
        assert np.abs(ratios.cpu().numpy() - ratio64).max() <= 4.0 * RATIO_DEV_MEASURED * 1.3   # 1.3: the largest ratio of a case, exp(0.2) + rounding
        check_stats(stats.cpu().numpy(), [stats64], "%s, %d rows" % (config, len(idx)))
    # all rows in order, without indices and without normalisation
    expected = ppo.gradients64(case["state"], case, np.arange(case["rows"]), normalize=False)[0]
    grads = batch.ppo_gradients(*data, normalize_advantage=False, **settings(case))[0]
    assert ppo.gradient_deviation({k: v.cpu().numpy() for k, v in grads.items()}, expected)[0] <= 4.0 * GRAD_DEV_MEASURED
    # the parity facility moves nothing
    after = batch.parameters()
    assert all(np.array_equal(before[k], after[k]) for k in ppo.NAMES) and all(np.array_equal(before[k], case["state"][k]) for k in ppo.NAMES)


@pytest.mark.gpu
@pytest.mark.parametrize("hidden,value_hidden,config", CASES)
def test_parameters_after_steps(mi, hidden, value_hidden, config):
    case = ppo.make_case(hidden, value_hidden, config)
    batch, data = load(mi, case)
    size = case["batch_size"]
    per_epoch = (case["rows"] + size - 1) // size
    runs = [(lr, ppo.minibatches(case, 2)[:3]) for lr in ppo.LEARNING_RATES] + [(ppo.LEARNING_RATES[0], ppo.minibatches(case, 2))]
    for lr, batches in runs:
        batch.set_policy(case["state"]); batch.set_value_network(case["state"]); batch.set_log_std(case["state"]["log_std"])
        batch.begin_training(lr=lr, betas=ppo.BETAS, eps=ppo.ADAM_EPS)
        expected, rows64, margins = ppo.steps64(case, batches, lr)
        assert min(margins) > ppo.MARGIN, margins
        if len(batches) == 2 * per_epoch:
            stats = batch.ppo_update(*data, case["order"], size, max_grad_norm=case["max_grad_norm"], **settings(case))
        else:   # three steps: each minibatch's rows gathered here and given as one epoch of one minibatch; the session carries Adam's state
            steps = []
            for idx in batches:
                rows_of = [t[torch.from_numpy(idx).cuda()] for t in data]
                steps.append(batch.ppo_update(*rows_of, np.arange(len(idx))[None], len(idx), max_grad_norm=case["max_grad_norm"], **settings(case)))
            stats = torch.cat(steps)
        got = batch.parameters()
        device = ppo.parameter_deviation(got, expected, case["state"])
        print("%s, lr %g, %d steps: parameters against the oracle %.3e of the movement (%s), allowed %.3e" % (config, lr, len(batches), device[0], device[1], 4.0 * ADAM_DEV_MEASURED))
        assert device[0] <= 4.0 * ADAM_DEV_MEASURED
        check_stats(stats.cpu().numpy(), rows64, "%s, lr %g" % (config, lr))
        # std follows logStd: set_log_std's statement
        std = np.zeros(27, np.float32); log_std = np.zeros(27, np.float32)
        assert batch.lib.readPhysicsBatchLogStd(C.c_void_p(std.ctypes.data), C.c_void_p(log_std.ctypes.data)) == 0
        assert np.array_equal(log_std, got["log_std"]) and np.array_equal(std, np.exp(log_std.astype(np.float64)).astype(np.float32))
        batch.end_training()


@pytest.mark.gpu
def test_ratio_on_collected_data(mi):
    """RATIO_DEV_MEASURED was taken on test_trainer_plumbing's rows: a fresh ActorCritic (action layer U(-0.01, 0.01), log_std 0), n = 8,
    16 steps.  The same kind of networks and rows here."""
    n, steps = 8, 16
    batch = mi.LocomotionBatch(n, seed=31)
    batch.set_policy(*pu.make_policy(40, seed=4, action_gain=0.01 * np.sqrt(40))); batch.set_value_network(*tu.make_value_network(40, seed=5))
    batch.set_log_std(np.zeros(27, np.float32))
    batch.reset()
    data = batch.collect(steps)
    advantages, returns = batch.gae(data["rewards"], data["values"], data["dones"], data["last_values"])
    _, ratios, stats = batch.ppo_gradients(data["obs"], data["actions"], data["log_probs"], advantages, returns)
    worst = float((ratios - 1.0).abs().max())
    print("max |ratio - 1| of the update's log-probabilities on collected rows, weights unmoved: %.3e (allowed %.3e)" % (worst, 4.0 * RATIO_DEV_MEASURED))
    assert ratios.shape == (steps * n,) and worst <= 4.0 * RATIO_DEV_MEASURED
    assert float(stats[3]) == 0.0


def _update_from(mi, batch, case, data, epochs=2):
    batch.set_policy(case["state"]); batch.set_value_network(case["state"]); batch.set_log_std(case["state"]["log_std"])
    batch.begin_training(lr=1e-3)
    stats = batch.ppo_update(*data, case["order"][:epochs], case["batch_size"], max_grad_norm=case["max_grad_norm"], **settings(case))
    return batch.parameters(), stats.cpu().numpy()


@pytest.mark.gpu
def test_master_copy_moves_in_place(mi):
    case = ppo.make_case(40, 256, "entropy")
    batch, data = load(mi, case)
    after, _ = _update_from(mi, batch, case, data)
    assert all(np.isfinite(after[k]).all() and (after[k] != case["state"][k]).any() for k in ppo.NAMES)
    # no sync(): the inference kernels read what Adam wrote
    states = np.random.default_rng(9).normal(0.0, 1.0, (65, pu.STATE)).astype(np.float32)
    actions, a, b = batch.act(states, hidden=True)
    pu.check_against_formula([after[k] for k in pu.NAMES], states, actions, np.ascontiguousarray(a), np.ascontiguousarray(b), K_DEVICE)
    values, a, b = batch.values(states, hidden=True)
    tu.check_value_against_formula([after[k] for k in tu.VALUE_NAMES], states, values, a, b, K_DEVICE)


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["short", "entropy"])
def test_update_is_bit_reproducible(mi, config):
    case = ppo.make_case(128, 128, config)
    batch, data = load(mi, case)
    # more tiles than groups: a group adds several tiles into its slab row, in the same order every time
    idx = np.random.default_rng(3).integers(0, case["rows"], 4 * 128 * 2 + 3)
    expected, _, _, margins = ppo.gradients64(case["state"], case, idx)
    assert min(margins) > ppo.MARGIN, margins
    g1, r1, _ = batch.ppo_gradients(*data, indices=idx, **settings(case))
    g2, r2, _ = batch.ppo_gradients(*data, indices=idx, **settings(case))
    assert all(torch.equal(g1[k], g2[k]) for k in ppo.NAMES) and torch.equal(r1, r2)
    assert ppo.gradient_deviation({k: v.cpu().numpy() for k, v in g1.items()}, expected)[0] <= 4.0 * GRAD_DEV_MEASURED
    first, first_stats = _update_from(mi, batch, case, data)
    second, second_stats = _update_from(mi, batch, case, data)
    assert all(np.array_equal(first[k].view(np.uint32), second[k].view(np.uint32)) for k in ppo.NAMES)
    assert np.array_equal(first_stats.view(np.uint32), second_stats.view(np.uint32)) and np.isfinite(first_stats).all()


@pytest.mark.gpu
def test_trainer_with_the_device_update(mi):
    from directx_renderer_kurth_amd import training
    n, hidden = 8, 40
    batch = mi.LocomotionBatch(n, seed=31)
    trainer = training.PPOTrainer(batch, hidden=hidden, value_hidden=hidden, n_epochs=2, batch_size=32, seed=3, device_update=True)
    before = {k: v.clone() for k, v in trainer.model.state_dict().items()}
    for it in range(2):
        stats = trainer.iterate(16)
        print("iteration %d: %s" % (it, stats))
        assert all(np.isfinite(v) for v in stats.values()), stats
        assert stats["rows"] == 16 * n
        assert {"loss", "policy_loss", "value_loss", "clip_fraction", "first_loss", "mean_reward", "falls"} <= set(stats)
    assert batch.noise_counter == 32
    # the module is refreshed on request only
    assert all(torch.equal(v, before[k]) for k, v in trainer.model.state_dict().items())
    trainer.pull()
    after = trainer.model.state_dict()
    assert all(torch.isfinite(v).all() for v in after.values())
    assert all(not torch.equal(after[k].cpu(), before[k].cpu()) for k in ppo.NAMES)
    assert all(np.array_equal(after[k].cpu().numpy(), v) for k, v in batch.parameters().items())


@pytest.mark.gpu
def test_refusals(mi):
    case = ppo.make_case(40, 256, "entropy")
    batch, data = load(mi, case)
    with pytest.raises(mi.PhysicsError):
        batch.ppo_update(*data, case["order"], 32)              # before begin_training
    batch.begin_training()
    batch.ppo_update(*data, case["order"][:1], 32)
    with pytest.raises(ValueError):
        batch.ppo_update(*data, case["order"] + 1, 32)          # an index past the rows
    batch.set_policy(case["state"])                              # a new network from the host ends the session
    with pytest.raises(mi.PhysicsError):
        batch.ppo_update(*data, case["order"], 32)
    assert all(np.array_equal(batch.parameters()[k], case["state"][k]) for k in pu.NAMES)
    for setter, value in ((batch.set_value_network, case["state"]), (batch.set_log_std, case["state"]["log_std"])):
        batch.begin_training()
        setter(value)
        with pytest.raises(mi.PhysicsError):
            batch.ppo_update(*data, case["order"], 32)
    batch.begin_training(); batch.end_training()
    with pytest.raises(mi.PhysicsError):
        batch.ppo_update(*data, case["order"], 32)
    batch.ppo_gradients(*data)                                   # the parity facility needs no session
