#!/usr/bin/env python3
"""MyViT training step on one MI355X: ms/step and poses/s of pl.MyViT (f16x3, fp32, bf16p) and of an equivalent stock-torch
module (eager fp32, eager bf16 autocast), timed the same way (HIP events around `steps` steps after `warmup`; MSE + AdamW
step included).  Prints one JSON line.

    python tools/bench_vit.py [--batches 4096,64] [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
PEAK_FP32_MFMA_TFLOPS = 157.3      # MI355X fp32 matrix peak (the f16x3 planes GEMM issues 3 fp16 MFMAs per product)


class EagerViT(nn.Module):
    """The same network in stock torch ops (what torch.compile-free PyTorch-ROCm runs for the reference module)."""

    def __init__(self, vit):
        super().__init__()
        self.v = vit

    def forward(self, x):
        v = self.v
        H, nh = v.hidden_d, v.n_heads
        B, n, _ = x.shape
        h = v.linear_mapper(x) + v.pos_embed
        for b in v.blocks:
            a = b.mhsa.norm(b.norm1(h))
            q, k, w = b.mhsa.to_qkv(a).chunk(3, dim=-1)
            q, k, w = (z.reshape(B, n, nh, H // nh).transpose(1, 2) for z in (q, k, w))
            att = torch.softmax((q @ k.transpose(-1, -2)) * (H // nh) ** -0.5, dim=-1)
            h = h + b.mhsa.to_out((att @ w).transpose(1, 2).reshape(B, n, H))
            h = h + b.mlp[2](F.gelu(b.mlp[0](b.norm2(h))))
        return v.mlp[2](torch.relu(v.mlp[0](h)))


def flops(B, seq=17, H=256, n_blocks=2, out_d=3, in_d=2):
    T = B * seq
    lin = 2 * T * (H * 3 * H + H * H + H * 4 * H + 4 * H * H) * n_blocks + 2 * T * (H * H // 2 + H // 2 * out_d + in_d * H)
    att = 2 * 2 * B * (H // 64) * seq * seq * 64 * n_blocks
    return lin + att, 3 * lin + 2.5 * att       # forward; training step (backward = 2x forward GEMMs)


def time_steps(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4096,64")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import __graft_entry__ as ge
    pl = ge.build()
    res = {"metric": "vit_train_step", "steps": a.steps, "warmup": a.warmup, "runs": {}}
    for B in [int(b) for b in a.batches.split(",")]:
        g = torch.Generator().manual_seed(B)
        x = torch.rand(B, 17, 2, generator=g).to(DEV)
        t = (0.2 * torch.randn(B, 17, 3, generator=g)).to(DEV)
        fwd, step_flops = flops(B)
        row = {"gflop_forward": fwd / 1e9, "gflop_step": step_flops / 1e9}
        for mode in ("f16x3", "fp32", "bf16p"):
            torch.manual_seed(0)
            m = pl.MyViT(compute_dtype=mode).to(DEV).train()
            opt = pl.FlatAdam(m, lr=1e-4, weight_decay=0.01, decoupled_weight_decay=True)
            ms = time_steps(lambda: pl.train_step(m, opt, x, t), a.steps, a.warmup)
            row[mode] = {"ms": ms, "poses_per_s": B / ms * 1e3, "tflops": step_flops / ms / 1e9,
                         "share_of_fp32_mfma_peak": step_flops / ms / 1e9 / PEAK_FP32_MFMA_TFLOPS}
        for name, ac in (("eager_fp32", False), ("eager_bf16_autocast", True)):
            torch.manual_seed(0)
            ref = EagerViT(pl.MyViT(compute_dtype="fp32")).to(DEV).train()
            opt = torch.optim.AdamW([p for p in ref.parameters() if p.requires_grad], lr=1e-4)

            def step():
                opt.zero_grad()
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=ac):
                    loss = F.mse_loss(ref(x).float(), t)
                loss.backward()
                opt.step()
            ms = time_steps(step, a.steps, a.warmup)
            row[name] = {"ms": ms, "poses_per_s": B / ms * 1e3}
        row["f16x3_over_eager_fp32"] = row["f16x3"]["ms"] / row["eager_fp32"]["ms"]
        row["fp32_over_eager_fp32"] = row["fp32"]["ms"] / row["eager_fp32"]["ms"]
        row["bf16p_over_eager_bf16_autocast"] = row["bf16p"]["ms"] / row["eager_bf16_autocast"]["ms"]
        row["bf16p_over_f16x3"] = row["bf16p"]["ms"] / row["f16x3"]["ms"]
        res["runs"][str(B)] = row
    res["bound"] = ("GEMM share of peak against the fp32 MFMA peak; the non-GEMM kernels are HBM-bound "
                    "(per-kernel times: rocprofv3 --kernel-trace --stats, profiles/vit_*)")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
