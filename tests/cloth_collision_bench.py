"""Developer tool (not part of bench.py, no assertion on the timings): what cloth collision costs per internal step.

    python tests/cloth_collision_bench.py [--settle STEPS] [--repeats N] [--cloths 16] [--grid 64] [--colliders 1000]

16 cloths of 64 x 64 particles laid over a field of 1 000 colliders (a third static, the rest on resting bodies).  Time of one
mi_step_internal (HIP events around the call on the world's stream, median of repeated calls after a warm-up) with collision off on
every cloth and with it on, the difference per step and per particle, and how many particles were pushed off something in the last step."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import directx_renderer_kurth_amd as mi  # noqa: E402
from bench_util import time_calls  # noqa: E402

MATERIAL = (0.1, 0.5, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settle", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--cloths", type=int, default=16)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--colliders", type=int, default=1000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cloth_collision_bench: no GPU; there is nothing to measure on a CPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(5)
    w = mi.World()
    side = int(np.ceil(np.sqrt(args.cloths)))
    span = 6.0 * side
    w.add_static_collider(3, (-span, -1.0, -span, span, 0.0, span), MATERIAL)
    for i in range(args.colliders):
        x, z = rng.uniform(-0.5 * span, 0.5 * span, 2)
        r = float(rng.uniform(0.3, 0.8))
        if i % 3 == 0:
            w.add_static_collider(0, (0, 0, 0, r), MATERIAL, (x, r, z))
        else:
            w.add_collider(w.add_body((x, r + 0.01, z)), 0 if i % 3 == 1 else 4, (0, 0, 0, r) if i % 3 == 1 else (0, 0, 0, 1, 0, 0, 0, r, r, r), MATERIAL)
    cloths = []
    for k in range(args.cloths):
        c = w.add_cloth(5.0, 5.0, args.grid, args.grid, 4.0)
        w.cloth_set_fixed_vertices(c, ((k % side - 0.5 * (side - 1)) * 6.0, 2.0, (k // side - 0.5 * (side - 1)) * 6.0 + 2.5), (0, 0, 0, 1), True)
        cloths.append(c)
    particles = args.cloths * args.grid * args.grid
    stream = torch.cuda.ExternalStream(w.device_state().stream or 0, device=dev)

    def step():
        return w.lib.mi_step_internal(w.w, ctypes.c_float(1.0 / 120.0), ctypes.c_uint32(8))
    results = {}
    for on in (False, True, False, True):
        for c in cloths:
            if on:
                w.cloth_set_collision(c, 0.05, friction=0.3)
            else:
                w.cloth_clear_collision(c)
        for _ in range(args.settle):
            w.step_internal(1.0 / 120.0, 8)
        w.synchronize()
        results.setdefault(on, []).append(time_calls(step, stream, args.repeats))
        touched = sum(int(np.count_nonzero(w.cloth_contacts(c) != mi.CLOTH_NO_CONTACT)) for c in cloths)
        print("collision %-3s: step %.3f ms [%.3f, %.3f], %d of %d particles touching" % (("on" if on else "off",) + results[on][-1] + (touched, particles)), flush=True)
    off, on = min(r[0] for r in results[False]), min(r[0] for r in results[True])
    print("%d bodies, %d colliders, %d cloths of %d x %d: the pass costs %.3f ms per step = %.2f ns per particle" % (
        w.num_bodies, w.num_colliders, args.cloths, args.grid, args.grid, on - off, (on - off) * 1e6 / particles))
    w.close()


if __name__ == "__main__":
    main()
