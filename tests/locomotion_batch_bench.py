"""Developer tool (not a test, not part of bench.py): batched ragdoll env-steps/s (updatePhysicsBatch at N = 256 and 1024) against the
single environment's updatePhysics loop, in one process on one GPU.  Host clock around synchronised calls (updatePhysicsBatch
returns after its copy out), warm-up first.  Prints one JSON line.
    python tests/locomotion_batch_bench.py [--steps 50] [--warmup 10] [--sizes 256,1024] [--single 256] [--profile-steps 0]
--profile-steps K only runs K batched updates at the first size (for a rocprofv3 --kernel-trace --stats run)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--single", type=int, default=256)
    ap.add_argument("--profile-steps", type=int, default=0)
    args = ap.parse_args()
    import directx_renderer_kurth_amd as mi
    sizes = [int(s) for s in args.sizes.split(",")]
    rng = np.random.default_rng(0)
    out = {}
    if args.profile_steps:
        b = mi.LocomotionBatch(sizes[0], seed=1)
        a = rng.uniform(-0.5, 0.5, (sizes[0], 27)).astype(np.float32)
        for _ in range(args.profile_steps):
            b.step(a)
        print(json.dumps({"profiled_updates": args.profile_steps, "n": sizes[0]}))
        return
    for n in sizes:
        b = mi.LocomotionBatch(n, seed=1)
        a = rng.uniform(-0.5, 0.5, (n, 27)).astype(np.float32)
        for _ in range(args.warmup):
            b.step(a)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            b.step(a)
        dt = (time.perf_counter() - t0) / args.steps
        out["batch_%d" % n] = {"ms_per_update": dt * 1e3, "env_steps_per_s": n / dt}
    lib = C.CDLL(mi.LOCOMOTION_LIB_PATH)
    state = np.zeros(66, np.float32); reward = C.c_float(0.0)
    a = np.zeros(27, np.float32)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    lib.resetPhysics(fp(state))
    for _ in range(args.warmup):
        lib.updatePhysics(fp(a), fp(state), C.byref(reward))
    t0 = time.perf_counter()
    for _ in range(args.single):
        if lib.updatePhysics(fp(a), fp(state), C.byref(reward)):
            lib.resetPhysics(fp(state))
    dt = (time.perf_counter() - t0) / args.single
    out["single"] = {"ms_per_update": dt * 1e3, "env_steps_per_s": 1.0 / dt}
    out["speedup_256"] = out.get("batch_256", {}).get("env_steps_per_s", 0.0) / out["single"]["env_steps_per_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
