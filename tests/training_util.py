"""Shared by the training tests: numpy restatements of what the library computes for PPO (host/locomotion_policy.h: noiseUniforms,
noiseSample, noiseLogProb; host/locomotion_batch.hip: k_loco_gae), in the style of policy_util.py, which this file extends: integer and
float32 stages restated bit for bit, transcendental stages in float64."""
import numpy as np

import policy_util as pu

GOLDEN, MIX1, MIX2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
LOG_PROB_CONSTANT64 = 13.5 * np.log(2.0 * np.pi)
LOG_PROB_CONSTANT = np.float32(LOG_PROB_CONSTANT64)
VALUE_NAMES = ("mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias", "mlp_extractor.value_net.2.weight",
               "mlp_extractor.value_net.2.bias", "value_net.weight", "value_net.bias")


def make_value_network(hidden, seed, gain=2.2):
    """pu.make_policy's recipe for the critic 66 -> Hv -> Hv -> 1."""
    rng = np.random.default_rng(seed)
    out = []
    for rows, cols in ((hidden, pu.STATE), (hidden, hidden), (1, hidden)):
        s = gain / np.sqrt(cols)
        out += [rng.uniform(-s, s, (rows, cols)).astype(np.float32), rng.uniform(-0.1, 0.1, rows).astype(np.float32)]
    return out


def check_value_against_formula(net, states, values, a, b, k):
    """pu.check_against_formula for the critic: tanh vectors within k ulp, the value bit-equal to layer 3 restated from the given b."""
    return pu.check_against_formula(net, states, np.ascontiguousarray(values, np.float32).reshape(-1, 1), np.ascontiguousarray(a), np.ascontiguousarray(b), k)


def _mix(z):
    z = z ^ (z >> np.uint64(30)); z = z * MIX1
    z = z ^ (z >> np.uint64(27)); z = z * MIX2
    return z ^ (z >> np.uint64(31))


def noise_uniforms(seed, envs, updates):
    """(k1, k2, u1, u2), each [len(updates), len(envs), 27]: the integer stage of noiseUniforms and its two float32 uniforms."""
    with np.errstate(over="ignore"):
        e = np.asarray(envs, np.uint64)[None, :, None]; u = np.asarray(updates, np.uint64)[:, None, None]; j = np.arange(pu.ACTION, dtype=np.uint64)[None, None, :]
        h = _mix(np.uint64(seed) + GOLDEN * (e + np.uint64(1)))
        h = _mix(h ^ u)
        h = _mix(h + GOLDEN * (j + np.uint64(1)))
    k1 = (h >> np.uint64(40)).astype(np.uint32); k2 = ((h >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.uint32)
    scale = np.float32(2.0 ** -24)
    u1 = (k1 + np.uint32(1)).astype(np.float32) * scale; u2 = k2.astype(np.float32) * scale
    return k1, k2, u1, u2


def noise64(u1, u2):
    """Box-Muller in float64 on the exact uniforms."""
    return np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(2.0 * np.pi * u2.astype(np.float64))


def log_prob_terms64(eps, log_std):
    """The 27 terms -eps^2 / 2 - logStd per row in float64, from the float32 eps and logStd."""
    eps = np.asarray(eps, np.float32).astype(np.float64); log_std = np.asarray(log_std, np.float32).astype(np.float64)
    return -0.5 * eps * eps - log_std


def log_prob_bound(eps, log_std):
    """(log-probability in float64, allowed |error| of the float32 one): 64 u (sum |term| + |c|), u = 2^-24."""
    terms = log_prob_terms64(eps, log_std)
    return terms.sum(-1) - LOG_PROB_CONSTANT64, 64.0 * 2.0 ** -24 * (np.abs(terms).sum(-1) + LOG_PROB_CONSTANT64)


def gae32(rewards, values, dones, last_values, gamma, lam):
    """k_loco_gae's order in float32: (advantages, returns) [steps, n]."""
    r = np.asarray(rewards, np.float32); v = np.asarray(values, np.float32); last = np.asarray(last_values, np.float32)
    gamma, lam = np.float32(gamma), np.float32(lam)
    gl = gamma * lam
    steps = r.shape[0]
    adv = np.zeros_like(r); ret = np.zeros_like(r)
    nxt = last.copy(); a = np.zeros_like(last)
    for t in range(steps - 1, -1, -1):
        nd = np.where(np.asarray(dones[t]) != 0, np.float32(0.0), np.float32(1.0))
        delta = (r[t] + (gamma * nxt) * nd) - v[t]
        a = delta + (gl * nd) * a
        adv[t] = a; ret[t] = a + v[t]
        nxt = v[t]
    assert adv.dtype == np.float32 and ret.dtype == np.float32
    return adv, ret


def ppo_loss64(log_probs, old_log_probs, advantages, values, returns, entropy, clip_range, vf_coef, ent_coef):
    """training.ppo_loss stated in numpy float64: (loss, policy, value)."""
    lp, old, adv, v, ret, ent = (np.asarray(x, np.float64) for x in (log_probs, old_log_probs, advantages, values, returns, entropy))
    ratio = np.exp(lp - old)
    policy = -np.minimum(adv * ratio, adv * np.clip(ratio, 1.0 - clip_range, 1.0 + clip_range)).mean()
    value = ((ret - v) ** 2).mean()
    return policy + vf_coef * value - ent_coef * ent.mean(), policy, value
