"""Time of the heat-map supervision in the 3-D head: the plain and the _hm forward and backward kernels on NHWC logits at
the head's shapes (J = 17, 64 x 64 x 64), alternating in one run, device events, median of several rounds with the spread.

    python tools/bench_heatmap_loss.py [--batches 64,256] [--rounds 9] [--sigma 0.5] [--parent-lib PATH] [--out FILE]

--parent-lib: another build of libposelift.so (the parent commit's) whose plain kernels are timed in the same alternation.
The bytes moved are identical (4 B read per voxel forward, 4 B read + 4 B written backward), so the times should be close.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.build()
    L = pkg.lib()
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        for name in ("pl_softargmax3d_nhwc_fwd", "pl_softargmax3d_nhwc_bwd"):
            fn = getattr(parent, name)
            fn.restype, fn.argtypes = pkg._lib.SIGNATURES[name]
    dev = torch.device("cuda", 0)
    J, H, W = 17, 64, 64
    law = (ctypes.c_float * 6)(*pkg.heatmap_law(W, H, 64, True, "head"))
    rows = []
    for B in [int(b) for b in args.batches.split(",")]:
        g = torch.Generator(device=dev).manual_seed(B)
        x = torch.randn(B, H, W, J * 64, device=dev, generator=g) * 2
        t = torch.rand(B * J, 3, device=dev, generator=g) * 1.8 - 0.9
        gc = torch.randn(B * J, 3, device=dev, generator=g) * 1e-2
        gsq = torch.full((B * J,), 1e-3, device=dev)
        dl = torch.empty_like(x)
        coords = torch.empty(B * J, 3, device=dev)
        sq = torch.empty(B * J, device=dev)
        st5 = torch.empty(B * J, 5, device=dev)
        st8 = torch.empty(B * J, 8, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        p = lambda v: v.data_ptr()
        calls = {
            "fwd plain": lambda: L.pl_softargmax3d_nhwc_fwd(p(x), B, J, H, W, p(coords), p(st5), s),
            "fwd hm": lambda: L.pl_softargmax3d_nhwc_hm_fwd(p(x), p(t), B, J, H, W, args.sigma, law, p(coords), p(sq), p(st8), s),
            "bwd plain": lambda: L.pl_softargmax3d_nhwc_bwd(p(x), p(st5), p(gc), B, J, H, W, p(dl), s),
            "bwd hm": lambda: L.pl_softargmax3d_nhwc_hm_bwd_ex(p(x), p(t), p(st8), p(gc), p(gsq), B, J, H, W, args.sigma, law, p(dl),
                                                               None, 0, None, s),
        }
        if parent is not None:
            calls["fwd parent"] = lambda: parent.pl_softargmax3d_nhwc_fwd(p(x), B, J, H, W, p(coords), p(st5), s)
            calls["bwd parent"] = lambda: parent.pl_softargmax3d_nhwc_bwd(p(x), p(st5), p(gc), B, J, H, W, p(dl), s)
        for fn in calls.values():                                   # warm-up, and the stats both backward passes read
            assert fn() == 0, L.pl_last_error()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, fn in calls.items():                             # alternating: every kernel once per round
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / args.iters)
        gb = x.numel() * 4 / 1e9
        for k, v in times.items():
            med = statistics.median(v)
            traffic = gb * (2 if k.startswith("bwd") else 1)
            rows.append({"B": B, "kernel": k, "median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                         "GB_per_s": round(traffic / (med * 1e-3), 1)})
        del x, dl
        torch.cuda.empty_cache()
    print(f"{'B':>4} {'kernel':<11} {'median ms':>10} {'min':>9} {'max':>9} {'GB/s':>8}")
    for r in rows:
        print(f"{r['B']:>4} {r['kernel']:<11} {r['median_ms']:>10.4f} {r['min_ms']:>9.4f} {r['max_ms']:>9.4f} {r['GB_per_s']:>8.1f}")
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"sigma": args.sigma, "rounds": args.rounds, "iters": args.iters, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
