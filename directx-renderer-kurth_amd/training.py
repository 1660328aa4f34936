"""PPO for the ragdoll locomotion controller, as the reference trains it (learning/learn_locomotion.py:71-107: stable-baselines PPO,
pi=[128,128], vf=[128,128], tanh, clip_range 0.1, n_epochs 10, batch_size 128, lr 2.5e-5, action layer initialised U(-0.01, 0.01)),
split where the work is: the rollouts, the sampled actions, their log-probabilities, the values and the advantages come from the device
kernels of LocomotionBatch.collect() and .gae(); the gradient step is PyTorch's by default, and with device_update=True the device's
(LocomotionBatch.ppo_update: the same loss, clipping and Adam in three launches per minibatch, the parameters staying on the device).
stable-baselines is not needed.

The torch modules carry stable-baselines' parameter names, so ActorCritic.state_dict() is what LocomotionBatch.set_policy() and
.set_value_network() take."""
import math

import torch
from torch import nn

STATE_SIZE, ACTION_SIZE = 66, 27


class _Extractor(nn.Module):
    def __init__(self, hidden, value_hidden):
        super().__init__()
        self.policy_net = nn.Sequential(nn.Linear(STATE_SIZE, hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.Tanh())
        self.value_net = nn.Sequential(nn.Linear(STATE_SIZE, value_hidden), nn.Tanh(), nn.Linear(value_hidden, value_hidden), nn.Tanh())


class ActorCritic(nn.Module):
    """Diagonal-Gaussian actor 66 -> H -> H -> 27 and a separate critic 66 -> Hv -> Hv -> 1, tanh, with a state-independent log_std."""

    def __init__(self, hidden=128, value_hidden=128):
        super().__init__()
        self.mlp_extractor = _Extractor(hidden, value_hidden)
        self.action_net = nn.Linear(hidden, ACTION_SIZE)
        self.value_net = nn.Linear(value_hidden, 1)
        self.log_std = nn.Parameter(torch.zeros(ACTION_SIZE))
        with torch.no_grad():  # learn_locomotion.py:97-102
            self.action_net.weight.uniform_(-0.01, 0.01)
            self.action_net.bias.zero_()

    def mean(self, obs):
        return self.action_net(self.mlp_extractor.policy_net(obs))

    def value(self, obs):
        return self.value_net(self.mlp_extractor.value_net(obs)).squeeze(-1)

    def evaluate(self, obs, actions):
        """(log N(actions; mean(obs), exp(log_std)) [rows], value(obs) [rows], entropy [rows]) in the dtype of the module."""
        return gaussian_log_prob(self.mean(obs), self.log_std, actions), self.value(obs), gaussian_entropy(self.log_std).expand(obs.shape[0])


def gaussian_log_prob(mean, log_std, actions):
    z = (actions - mean) * torch.exp(-log_std)
    return (-0.5 * z * z - log_std).sum(-1) - 0.5 * ACTION_SIZE * math.log(2.0 * math.pi)


def gaussian_entropy(log_std):
    return (0.5 + 0.5 * math.log(2.0 * math.pi) + log_std).sum(-1)


def normalize_advantages(advantages):
    """stable-baselines' per-minibatch normalisation: (A - mean) / (std + 1e-8), std with Bessel's correction."""
    return (advantages - advantages.mean()) / (advantages.std() + 1e-8)


def ppo_loss(log_probs, old_log_probs, advantages, values, returns, entropy, clip_range=0.1, vf_coef=0.5, ent_coef=0.0):
    """PPO's loss on one minibatch, a pure function of tensors [rows], computed in their dtype:
        ratio = exp(log_probs - old_log_probs)
        policy = -mean(min(A * ratio, A * clamp(ratio, 1 - clip, 1 + clip)))
        value = mean((returns - values)^2)
        loss = policy + vf_coef * value - ent_coef * mean(entropy)
    Returns (loss, policy, value, ratio)."""
    ratio = torch.exp(log_probs - old_log_probs)
    policy = -torch.minimum(advantages * ratio, advantages * torch.clamp(ratio, 1.0 - clip_range, 1.0 + clip_range)).mean()
    value = ((returns - values) ** 2).mean()
    return policy + vf_coef * value - ent_coef * entropy.mean(), policy, value, ratio


class PPOTrainer:
    """PPO over a LocomotionBatch.  iterate(steps) collects steps x n transitions on the device and runs the epochs of minibatches.
    With device_update the epochs run on the device too: the module's parameters go to the device once, before the first iteration, the
    device's copy is the one that learns, and pull() brings it back into trainer.model when it is wanted."""

    def __init__(self, batch, hidden=128, value_hidden=128, clip_range=0.1, n_epochs=10, batch_size=128, lr=2.5e-5, gamma=0.99, gae_lambda=0.95,
                 vf_coef=0.5, ent_coef=0.0, max_grad_norm=0.5, normalize_advantage=True, clip_actions=True, seed=0, device_update=False):
        self.batch = batch
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.generator = torch.Generator(device="cpu").manual_seed(seed)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            self.model = ActorCritic(hidden, value_hidden)
        self.model.to(self.device)
        self.optimizer = torch.optim.Adam(self.model.parameters(), lr=lr, eps=1e-5)
        self.clip_range, self.n_epochs, self.batch_size = clip_range, n_epochs, batch_size
        self.gamma, self.gae_lambda, self.vf_coef, self.ent_coef, self.max_grad_norm = gamma, gae_lambda, vf_coef, ent_coef, max_grad_norm
        self.normalize_advantage, self.clip_actions = normalize_advantage, clip_actions
        self.lr, self.adam_eps, self.device_update, self._session = lr, 1e-5, device_update, False

    def sync(self):
        """The module's weights and log_std to the library (and so to the batch's device copies)."""
        state = self.model.state_dict()
        self.batch.set_policy(state)
        self.batch.set_value_network(state)
        self.batch.set_log_std(state["log_std"])

    def iterate(self, steps):
        """One PPO iteration: sync, collect, gae, epochs.  Returns statistics as a dict of floats."""
        if self.device_update:
            return self._iterate_device(steps)
        self.sync()
        data = self.batch.collect(steps, clip=self.clip_actions)
        advantages, returns = self.batch.gae(data["rewards"], data["values"], data["dones"], data["last_values"], self.gamma, self.gae_lambda)
        rows = steps * self.batch.n
        obs = data["obs"].reshape(rows, STATE_SIZE); actions = data["actions"].reshape(rows, ACTION_SIZE)
        old_log_probs = data["log_probs"].reshape(rows); advantages = advantages.reshape(rows); returns = returns.reshape(rows)
        stats = dict(mean_reward=float(data["rewards"].mean()), falls=int(data["dones"].sum()), rows=rows)
        with torch.no_grad():
            # how far the device's log-probabilities are from the module's own, before any weight moves: in the module's float32 graph, and
            # against the float64 statement of the same network
            lp32, _, _ = self.model.evaluate(obs, actions)
            double = ActorCritic(self.model.action_net.in_features, self.model.value_net.in_features).to(self.device, torch.float64)
            double.load_state_dict({k: v.double() for k, v in self.model.state_dict().items()})
            lp64 = gaussian_log_prob(double.mean(obs.double()), double.log_std, actions.double())
            stats["ratio_dev_first"] = float((torch.exp(lp32 - old_log_probs) - 1.0).abs().max())
            stats["ratio_dev_first_f64"] = float((torch.exp(lp64 - old_log_probs.double()) - 1.0).abs().max())
        losses = []
        for _ in range(self.n_epochs):
            order = torch.randperm(rows, generator=self.generator).to(self.device)
            for start in range(0, rows, self.batch_size):
                idx = order[start:start + self.batch_size]
                log_probs, values, entropy = self.model.evaluate(obs[idx], actions[idx])
                adv = advantages[idx]
                if self.normalize_advantage and len(idx) > 1:
                    adv = normalize_advantages(adv)
                loss, policy, value, ratio = ppo_loss(log_probs, old_log_probs[idx], adv, values, returns[idx], entropy, self.clip_range, self.vf_coef, self.ent_coef)
                self.optimizer.zero_grad()
                loss.backward()
                nn.utils.clip_grad_norm_(self.model.parameters(), self.max_grad_norm)
                self.optimizer.step()
                losses.append((loss.item(), policy.item(), value.item(), ((ratio.detach() - 1.0).abs() > self.clip_range).float().mean().item()))
        stats.update(loss=losses[-1][0], policy_loss=sum(l[1] for l in losses) / len(losses), value_loss=sum(l[2] for l in losses) / len(losses),
                     clip_fraction=sum(l[3] for l in losses) / len(losses), first_loss=losses[0][0])
        return stats

    def _iterate_device(self, steps):
        """iterate() with the epochs on the device: the same permutations from the same generator, one ppo_update, one read of its statistics."""
        if not self._session:
            self.sync()
            self.batch.begin_training(lr=self.lr, eps=self.adam_eps)
            self._session = True
        data = self.batch.collect(steps, clip=self.clip_actions)
        advantages, returns = self.batch.gae(data["rewards"], data["values"], data["dones"], data["last_values"], self.gamma, self.gae_lambda)
        rows = steps * self.batch.n
        order = torch.stack([torch.randperm(rows, generator=self.generator) for _ in range(self.n_epochs)])
        steps_stats = self.batch.ppo_update(data["obs"], data["actions"], data["log_probs"], advantages, returns, order, self.batch_size, self.clip_range,
                                            self.vf_coef, self.ent_coef, self.max_grad_norm, self.normalize_advantage)
        s = steps_stats.cpu().double()   # the one read of the update
        stats = dict(mean_reward=float(data["rewards"].mean()), falls=int(data["dones"].sum()), rows=rows)
        stats.update(loss=float(s[-1, 0]), policy_loss=float(s[:, 1].mean()), value_loss=float(s[:, 2].mean()), clip_fraction=float(s[:, 3].mean()),
                     first_loss=float(s[0, 0]), grad_norm=float(s[:, 4].mean()))
        return stats

    def pull(self):
        """The device's parameters into trainer.model (device_update: the module is not refreshed per step)."""
        self.model.load_state_dict({k: torch.from_numpy(v) for k, v in self.batch.parameters().items()})
