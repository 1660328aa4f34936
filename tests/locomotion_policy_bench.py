"""Developer tool (not a test, not part of bench.py): what the learned controller costs per update of the batched ragdoll environments,
at N = 256 and N = 1024, in one process on one GPU.  Host clock around a synchronised block of --steps updates after a warm-up, every
path from a fresh reset with the same seed.  The policy has a zero last weight matrix and the constant action as its last bias, so
every path without resets steps the same trajectory and only the plumbing differs:
    a  step(tensor) with a constant action tensor: updatePhysicsBatchDevice, one Python call and stream hand-over per update
       (timed three times first: the spread of the three is the noise margin)
    b  step(act(states)): the two-call path, network on the device, no torch GEMMs
    c  rollout(steps, auto_reset=False): the same launches with k_loco_policy in place of k_loco_actions, enqueued by one call
    d  rollout(steps, auto_reset=True): adds the reset and gather launches, reported beside the others
Prints one JSON line (--out FILE also writes it).
    python tests/locomotion_policy_bench.py [--steps 200] [--warmup 50] [--sizes 256,1024] [--profile-steps 0]
--profile-steps K only runs rollout(K, auto_reset=False) at the first size (for a rocprofv3 --kernel-trace --stats run)."""
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
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--profile-steps", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import directx_renderer_kurth_amd as mi
    import policy_util as pu
    sizes = [int(s) for s in args.sizes.split(",")]
    constant = np.random.default_rng(0).uniform(-0.5, 0.5, 27).astype(np.float32)
    policy = pu.make_policy(128, seed=1)
    policy[4][:] = 0.0; policy[5][:] = constant
    if args.profile_steps:
        b = mi.LocomotionBatch(sizes[0], seed=1)
        b.set_policy(*policy)
        b.rollout(args.profile_steps, auto_reset=False)
        torch.cuda.synchronize()
        print(json.dumps({"profiled_updates": args.profile_steps, "n": sizes[0]}))
        return
    out = {"steps": args.steps, "warmup": args.warmup}
    for n in sizes:
        b = mi.LocomotionBatch(n, seed=1)
        b.set_policy(*policy)
        actions = torch.from_numpy(np.broadcast_to(constant, (n, 27)).copy()).cuda()

        def path_a(count):
            for _ in range(count):
                last = b.step(actions)
            return last[0]

        def path_b(count):
            states = torch.from_numpy(b.observe()[0]).cuda()
            for _ in range(count):
                states = b.step(b.act(states))[0]
            return states

        def path_c(count):
            return b.rollout(count, auto_reset=False)[0][-1]

        def path_d(count):
            return b.rollout(count, auto_reset=True)[0][-1]

        def timed(path):
            b.reset()
            path(args.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = path(args.steps)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps * 1e3, last.cpu().numpy()

        a_runs = [timed(path_a) for _ in range(3)]
        a_ms = [r[0] for r in a_runs]
        res = {"a_step_tensor_ms": a_ms, "a_median_ms": float(np.median(a_ms)), "a_spread_ms": max(a_ms) - min(a_ms)}
        for key, path in (("b_step_act_ms", path_b), ("c_rollout_ms", path_c), ("d_rollout_auto_reset_ms", path_d)):
            ms, last = timed(path)
            res[key] = ms
            if key != "d_rollout_auto_reset_ms":
                res[key.replace("_ms", "_same_states_as_a")] = bool(np.array_equal(last, a_runs[0][1]))
        res["c_not_slower_than_a"] = bool(res["c_rollout_ms"] <= res["a_median_ms"] + res["a_spread_ms"])
        out["n_%d" % n] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
