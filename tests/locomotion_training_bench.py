"""Developer tool (not a test, not part of bench.py): what collecting training data costs per update of the batched ragdoll environments,
next to the deterministic rollout it extends, in one process on one GPU.  Host clock around a synchronised block of --steps updates
after a warm-up, every run from a fresh reset with the same seed, the two paths alternating --repeats times:
    rollout  rollout(steps, auto_reset=True): k_loco_policy, push, step, gather, reset, gather per update
    collect  collect(steps, clip=False) with std = 0: k_loco_sample in place of k_loco_policy (adds the critic, the noise, the sample and
             its log-probability to that launch) and one critic launch at the end; with std = 0 it steps the rollout's trajectory, resets
             included, so only the launch differs
and once each: collect(steps, clip=True) at log_std = -1 (another trajectory: reported beside the others) and gae() on its rows.
Prints one JSON line (--out FILE also writes it): ms per update (all runs and the median), environment steps per second from the median.
    python tests/locomotion_training_bench.py [--steps 200] [--warmup 50] [--sizes 64,256,1024] [--hidden 128] [--repeats 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--sizes", default="64,256,1024")
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import directx_renderer_kurth_amd as mi
    import policy_util as pu
    import training_util as tu
    policy = pu.make_policy(args.hidden, seed=4, action_gain=0.3)
    net = tu.make_value_network(args.hidden, seed=5)
    out = {"steps": args.steps, "warmup": args.warmup, "hidden": args.hidden}
    for n in [int(s) for s in args.sizes.split(",")]:
        b = mi.LocomotionBatch(n, seed=1)
        b.set_policy(*policy); b.set_value_network(*net)

        def timed(path):
            b.reset()
            path(args.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = path(args.steps)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps * 1e3, last

        b.set_log_std(np.full(27, -np.inf, np.float32))
        runs = {"rollout": [], "collect": []}
        for _ in range(args.repeats):
            ms, r = timed(lambda count: b.rollout(count, auto_reset=True))
            runs["rollout"].append(ms)
            ms, c = timed(lambda count: b.collect(count, clip=False))
            runs["collect"].append(ms)
        res = {"same_trajectory": bool(torch.equal(r[2], c["rewards"]) and torch.equal(r[3], c["dones"])), "falls": int(r[3].sum())}
        for key, ms in runs.items():
            med = float(np.median(ms))
            res[key + "_ms"] = ms; res[key + "_median_ms"] = med; res[key + "_env_steps_per_s"] = n / med * 1e3
        res["collect_over_rollout"] = res["collect_median_ms"] / res["rollout_median_ms"]
        b.set_log_std(np.full(27, -1.0, np.float32))
        ms, c = timed(lambda count: b.collect(count, clip=True))
        res["collect_noisy_ms"] = ms; res["collect_noisy_falls"] = int(c["dones"].sum())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            b.gae(c["rewards"], c["values"], c["dones"], c["last_values"])
        torch.cuda.synchronize()
        res["gae_ms_per_call"] = (time.perf_counter() - t0) / 20 * 1e3
        out["n_%d" % n] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
