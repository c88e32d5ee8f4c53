"""Host cost of the soft-argmax heads: a forward plus backward of soft_argmax_3d_nhwc and soft_argmax_3d_nhwc_hm through
the package, with and without a PlaneLink, on logits so small ((B, H, W, J) = (1, 8, 8, 17): 278 KB) that the kernels
take a few microseconds and the Python and host side of the calls is what the clock sees.  Wall clock around a
synchronised loop of --iters calls, the median of --blocks such loops per case (single loops of 0.1 s were seen at twice
the usual time now and then); one JSON line.

    python tools/bench_heads_host.py [--iters 1000] [--blocks 9] [--warmup 500]

For a comparison of two commits run it in each checkout, in alternating fresh processes.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=500)
    args = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.build()
    conv = importlib.import_module("3d_poseestimation_amd.conv")
    dev = torch.device("cuda", 0)
    B, H, W, J = 1, 8, 8, 17
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(B, H, W, J * 64, generator=g) * 2).to(dev).requires_grad_()
    y = (torch.rand(B, J * 3, generator=g) * 1.6 - 0.8).to(dev)
    gc, gs = torch.randn(B, J * 3, generator=g).to(dev), torch.randn(B, J, generator=g).to(dev)

    def plain(link):
        pkg.soft_argmax_3d_nhwc(x, J, link).backward(gc)

    def hm(link):
        coords, sq = pkg.soft_argmax_3d_nhwc_hm(x, y, num_joints=J, link=link)
        torch.autograd.backward((coords, sq), (gc, gs))

    out = {}
    for name, fn in (("plain", plain), ("hm", hm)):
        for linked in (False, True):
            link = conv.PlaneLink(pkg._lib.PL_F16X3) if linked else None
            times = []
            for n in [args.warmup] + [args.iters] * args.blocks:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    x.grad = None
                    fn(link)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) / n * 1e6)
            out[f"{name}{' link' if linked else ''}"] = round(statistics.median(times[1:]), 3)
    print(json.dumps({"bench": "heads_host", "shape_BHWJ": [B, H, W, J], "iters": args.iters, "blocks": args.blocks, "us_per_fwd_bwd": out}))


if __name__ == "__main__":
    main()
