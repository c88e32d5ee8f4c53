#!/usr/bin/env python3
"""Step time of the lifter's train step with the criterion's skeleton terms (pl.PoseCriterion(skeleton=)):

    python tools/time_skeleton_terms.py [--cases none,mpjpe,terms,terms-denorm] [--rounds 5] [--steps 300] [--configs ...]

configs: b4096 (the bench's f16x3 step, H = 1024, eager), b64-eager and b64-graph (AdamW rides in the backward launches;
replayed from a hipGraph).  cases: none = criterion=None; mpjpe = PoseCriterion("mpjpe") weighted per joint (root joint 0);
terms = the same with H36M_SKELETON and both lambdas nonzero; terms-denorm = the same with a PoseTransform.  One line per
(config, case): device events around `steps` back-to-back steps, the median over `rounds` such windows and their min .. max;
the cases alternate inside a round.  A checkout without pl.Skeleton runs none and mpjpe alone, so the same script times the
parent commit (copy it there)."""
import argparse
import importlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("3d_poseestimation_amd")
DEV = torch.device("cuda", 0)


def criterion(case):
    if case == "none":
        return None
    w = torch.ones(17)
    w[0] = 0.0
    if case == "mpjpe":
        return pkg.PoseCriterion("mpjpe", joint_weights=w, coords=3).to(DEV)
    denorm = None
    if case == "terms-denorm":
        st = pkg.synth.h36m_stats()
        denorm = pkg.PoseTransform(torch.zeros(17, 3), torch.from_numpy(st["std_train_3d"]).reshape(17, 3))
    return pkg.PoseCriterion("mpjpe", joint_weights=w, coords=3, skeleton=pkg.H36M_SKELETON, bone_weight=0.1, symmetry_weight=0.05,
                             denorm=denorm).to(DEV)


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def make(config, case):
    B = 4096 if config == "b4096" else 64
    torch.manual_seed(0)
    m = pkg.LinearModel(34, 51, compute_dtype="f16x3").to(DEV).train()
    opt = pkg.FlatAdamW(m, lr=1e-4)
    x, y = pkg.synth.synthetic_batch(B, 1, DEV)
    kw = {} if case == "none" else {"criterion": criterion(case)}
    if config == "b64-graph":
        g = pkg.GraphedTrainStep(m, opt, x, y, **kw)
        gx, gy = g.inputs
        return lambda: g(gx, gy)
    return lambda: pkg.train_step(m, opt, x, y, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="none,mpjpe,terms,terms-denorm")
    ap.add_argument("--configs", default="b4096,b64-eager,b64-graph")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    cases = [c for c in a.cases.split(",") if hasattr(pkg, "Skeleton") or not c.startswith("terms")]
    for config in a.configs.split(","):
        fns = {c: make(config, c) for c in cases}
        for fn in fns.values():
            window(fn, a.warmup)
        times = {c: [] for c in cases}
        for _ in range(a.rounds):                   # the cases alternate inside a round: drift hits them alike
            for c, fn in fns.items():
                times[c].append(window(fn, a.steps))
        for c in cases:
            t = times[c]
            print(f"{a.label:8s} {config:10s} {c:13s} median {statistics.median(t):.4f} ms/step  (min {min(t):.4f} .. max {max(t):.4f}, "
                  f"{a.rounds} x {a.steps} steps)", flush=True)


if __name__ == "__main__":
    main()
