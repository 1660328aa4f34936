"""Developer tool (not a test, not part of bench.py): what one PPO optimiser step costs on the device (LocomotionBatch.ppo_update: three
launches per minibatch) next to training.py's PyTorch loop, in one process on one GPU.  Host clock around a synchronised block after a
warm-up, the two paths alternating --repeats times, medians reported.
    step     milliseconds per optimiser step over one epoch of --rows rows in minibatches of --batch (H = Hv = --hidden).  The PyTorch
             figure is PPOTrainer.iterate itself, its source unchanged, over a stand-in batch whose collect() and gae() hand back rows made
             beforehand: it includes iterate's one sync() and its two evaluations of the log-probabilities before the first step.  The
             device figure is ppo_update on the same rows, with the upload of the permutation.
    iterate  one PPOTrainer.iterate(--steps) at --envs environments with the reference's 10 epochs, split into collect (collect + gae,
             synchronised) and update (the rest), for device_update=False and True.
Prints one JSON line (--out FILE also writes it).
    python tests/locomotion_update_bench.py [--rows 16384] [--batch 128] [--hidden 128] [--envs 256] [--steps 64] [--repeats 3]"""
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


class Timed:
    """A LocomotionBatch whose collect() + gae() are timed (synchronised after gae), or, with `rows`, replaced by rows made beforehand."""

    def __init__(self, batch, rows=None):
        self._batch, self._rows, self.collect_s = batch, rows, 0.0

    def __getattr__(self, name):
        return getattr(self._batch, name)

    def collect(self, steps, clip=True):
        if self._rows is not None:
            return self._rows[0]
        torch.cuda.synchronize()
        self._t0 = time.perf_counter()
        return self._batch.collect(steps, clip=clip)

    def gae(self, *args):
        if self._rows is not None:
            return self._rows[1]
        out = self._batch.gae(*args)
        torch.cuda.synchronize()
        self.collect_s += time.perf_counter() - self._t0
        return out


def clock(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import directx_renderer_kurth_amd as mi
    from directx_renderer_kurth_amd import training
    out = {"rows": args.rows, "batch": args.batch, "hidden": args.hidden, "envs": args.envs, "steps": args.steps}

    # ---- ms per optimiser step on rows made beforehand
    n = 64
    batch = mi.LocomotionBatch(n, seed=1)
    make = lambda rows, device_update, b: training.PPOTrainer(Timed(b, rows) if rows else b, hidden=args.hidden, value_hidden=args.hidden, n_epochs=1,
                                                              batch_size=args.batch, seed=3, device_update=device_update)
    seed_trainer = make(None, False, batch)
    seed_trainer.sync()
    data = batch.collect(args.rows // n)
    rows = (data, batch.gae(data["rewards"], data["values"], data["dones"], data["last_values"]))
    steps_per_epoch = (args.rows + args.batch - 1) // args.batch
    host, device = make(rows, False, batch), make(rows, True, batch)
    runs = {"torch": [], "device": []}
    host.iterate(args.rows // n); device.iterate(args.rows // n)   # warm-up of both paths at the timed shapes
    for _ in range(args.repeats):
        runs["torch"].append(clock(lambda: host.iterate(args.rows // n))[0] / steps_per_epoch * 1e3)
        device._session = False                                      # the host path's sync() ended the session: a new one, from the module
        runs["device"].append(clock(lambda: device.iterate(args.rows // n))[0] / steps_per_epoch * 1e3)
    out["step"] = {"steps_per_epoch": steps_per_epoch, "torch_ms": runs["torch"], "device_ms": runs["device"],
                   "torch_median_ms": float(np.median(runs["torch"])), "device_median_ms": float(np.median(runs["device"]))}
    out["step"]["torch_over_device"] = out["step"]["torch_median_ms"] / out["step"]["device_median_ms"]

    # ---- one iterate() split into collect and update
    split = {}
    for name, device_update in (("torch", False), ("device", True)):
        split[name] = {"collect_ms": [], "update_ms": []}
    for r in range(args.repeats + 1):                               # the first round is the warm-up
        for name, device_update in (("torch", False), ("device", True)):
            b = Timed(mi.LocomotionBatch(args.envs, seed=1))
            trainer = training.PPOTrainer(b, hidden=args.hidden, value_hidden=args.hidden, batch_size=args.batch, seed=3, device_update=device_update)
            total, stats = clock(lambda: trainer.iterate(args.steps))
            if r:
                split[name]["collect_ms"].append(b.collect_s * 1e3); split[name]["update_ms"].append((total - b.collect_s) * 1e3)
            split[name]["optimiser_steps"] = trainer.n_epochs * ((stats["rows"] + args.batch - 1) // args.batch)
    for name in split:
        for key in ("collect_ms", "update_ms"):
            split[name][key.replace("_ms", "_median_ms")] = float(np.median(split[name][key]))
    out["iterate"] = split
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
