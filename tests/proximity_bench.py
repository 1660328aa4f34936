"""Developer tool (not part of bench.py, no assertion on the timings): what a proximity call costs on the settled C3 generator at 100 k.

    python tests/proximity_bench.py [--settle STEPS] [--repeats N] [--queries 4096]

Query points are spread over the settled pile (x/z uniformly over its extent, y between the ground and its top).  Per radius (0.5 m, 5 m,
+inf) and with / without MI_PROX_COUNT: time of one mi_proximity call through the tree and with MI_PROX_BRUTE_FORCE (HIP events around
the call on the world's stream, median of repeated calls after a warm-up), the part of the tree call that is the build (a call with one
query), how many queries found something, and whether the two paths returned the same bytes.  tests/raycast_bench.py times the ray cast
over the same world and count."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import directx_renderer_kurth_amd as mi  # noqa: E402
from directx_renderer_kurth_amd import scenes  # noqa: E402
from bench_util import time_calls  # noqa: E402


def time_queries(w, stream, d_in, d_out, n, flags, repeats, warmup=3):
    return time_calls(lambda: w.lib.mi_proximity(w.w, ctypes.c_uint32(n), ctypes.c_void_p(d_in.data_ptr()), ctypes.c_uint32(flags), ctypes.c_void_p(d_out.data_ptr()), None), stream, repeats, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settle", type=int, default=120)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--brute-repeats", type=int, default=3)
    ap.add_argument("--queries", type=int, default=4096)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("proximity_bench: no GPU; there is nothing to measure on a CPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    s = scenes.c3_mixed(100000)
    w = s.instantiate(mi.World())
    for _ in range(args.settle):
        w.step_internal(s.dt)
    w.synchronize()
    tr = w.transforms()
    lo, hi = tr[:, 0:3].min(axis=0), tr[:, 0:3].max(axis=0)
    stream = torch.cuda.ExternalStream(w.device_state().stream or 0, device=dev)
    print("c3: %d bodies, %d colliders, pile [%.1f, %.1f] x [%.1f, %.1f] x [%.1f, %.1f]" % (w.num_bodies, w.num_colliders, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]), flush=True)
    n = args.queries
    rng = np.random.default_rng(99)
    rec = np.zeros(n, mi.PROXIMITY_QUERY_DTYPE)
    rec["point"], rec["mount"], rec["enabled"] = rng.uniform(lo, hi, (n, 3)), mi.STATIC_BODY, 1
    for radius in (0.5, 5.0, np.inf):
        rec["radius"] = radius
        for count in (0, mi.PROX_COUNT):
            with torch.cuda.stream(stream):
                d_in = torch.from_numpy(rec.view(np.float32).reshape(n, 8).copy()).to(dev)
                d_tree, d_brute = torch.zeros((n, 12), dtype=torch.float32, device=dev), torch.zeros((n, 12), dtype=torch.float32, device=dev)
                stream.synchronize()
                build = time_queries(w, stream, d_in, d_tree, 1, mi.PROX_STATIC | count, args.repeats)
                tree = time_queries(w, stream, d_in, d_tree, n, mi.PROX_STATIC | count, args.repeats)
                brute = time_queries(w, stream, d_in, d_brute, n, mi.PROX_STATIC | count | mi.PROX_BRUTE_FORCE, args.brute_repeats, warmup=1)
                stream.synchronize()
                same = bool(torch.equal(d_tree.view(torch.int32), d_brute.view(torch.int32)))
                found = int(d_tree.view(torch.int32)[:, 3].sum().item())
                within = float(d_tree.view(torch.int32)[:, 7].float().mean().item())
            print("  radius %4s, count %d: tree %.3f ms/call [%.3f, %.3f] (build alone %.3f ms, walk %.3f ms) = %.3g queries/s; brute force %.3f ms/call [%.3f, %.3f]; "
                  "%d found, mean numWithin %.1f, records identical: %s" % (radius, 1 if count else 0, tree[0], tree[1], tree[2], build[0], tree[0] - build[0], n / (tree[0] * 1e-3),
                                                                            brute[0], brute[1], brute[2], found, within, same), flush=True)
    w.close()


if __name__ == "__main__":
    main()
