#!/usr/bin/env python3
"""Step time of the lifter's train step per criterion (pl.PoseCriterion):

    python tools/time_pose_criterion.py [--kinds none,mse,l1,smooth_l1,mpjpe] [--rounds 5] [--steps 300] [--configs ...]

configs: b4096 (the bench's f16x3 step, eager), b64-eager and b64-graph (the reference's own batch: AdamW rides in the
backward launches; replayed from a hipGraph).  One line per (config, kind): the median over `rounds` windows of `steps`
steps each (host clock around work that ends in a device synchronise), and the windows' min .. max.  kind none =
criterion=None; a checkout without pl.PoseCriterion runs that kind alone, so the same script times the parent commit.
The non-MSE kinds carry per-joint weights (root joint 0), as a user of them would."""
import argparse
import importlib
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("3d_poseestimation_amd")
DEV = torch.device("cuda", 0)


def criterion(kind):
    if kind == "none":
        return None
    w = None
    if kind != "mse":
        w = torch.ones(17)
        w[0] = 0.0
    return pkg.PoseCriterion(kind, joint_weights=w, coords=3).to(DEV)


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def make(config, kind):
    B = 4096 if config == "b4096" else 64
    torch.manual_seed(0)
    m = pkg.LinearModel(34, 51, compute_dtype="f16x3").to(DEV).train()
    opt = pkg.FlatAdamW(m, lr=1e-4)
    x, y = pkg.synth.synthetic_batch(B, 1, DEV)
    kw = {} if kind == "none" else {"criterion": criterion(kind)}
    if config == "b64-graph":
        g = pkg.GraphedTrainStep(m, opt, x, y, **kw)
        gx, gy = g.inputs
        return lambda: g(gx, gy)
    return lambda: pkg.train_step(m, opt, x, y, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="none,mse,l1,smooth_l1,mpjpe")
    ap.add_argument("--configs", default="b4096,b64-eager,b64-graph")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    kinds = a.kinds.split(",") if hasattr(pkg, "PoseCriterion") else ["none"]
    for config in a.configs.split(","):
        fns = {k: make(config, k) for k in kinds}
        for fn in fns.values():
            window(fn, a.warmup)
        times = {k: [] for k in kinds}
        for _ in range(a.rounds):                   # the kinds alternate inside a round: drift hits them alike
            for k, fn in fns.items():
                times[k].append(window(fn, a.steps))
        for k in kinds:
            t = times[k]
            print(f"{a.label:8s} {config:10s} {k:10s} median {statistics.median(t):.4f} ms/step  (min {min(t):.4f} .. max {max(t):.4f}, "
                  f"{a.rounds} x {a.steps} steps)", flush=True)


if __name__ == "__main__":
    main()
