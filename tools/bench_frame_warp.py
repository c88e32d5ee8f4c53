"""pl_frame_warp_gather against what a user can do today with stock torch on the same device: B = 256 frames into 256 x 256
from a resident uint8 table of 1000 x 1002 frames and from one of 256 x 256 frames; plain resize, flip, and every stage on.

The torch composition arrives at the same [B,256,256,3] fp32 NHWC tensor: frames[idx], .float() / 256, F.affine_grid +
F.grid_sample(bilinear, align_corners=False) on the NCHW view, permuted back and made contiguous (its per-sample matrices
are built on the device beforehand and not timed; for the plain resize F.interpolate is timed too).  Device event pairs
around single calls after warm-up, variants alternated, a different batch of the permutation each call; median [min .. p90].
The output store's rate is the output's bytes (B * 256 * 256 * 3 * 4) over the median time, against the HBM rate the
microarchitecture notes call achievable (6.3 TB/s).

    python tools/bench_frame_warp.py [--out profiles/frame_warp_time.txt]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the table to this file")
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--reps", type=int, default=40)
args = ap.parse_args()
pkg = ge.build()
dev = torch.device("cuda", 0)
B, HO, WO, HBM = args.batch, 256, 256, 6.3e12
OUT_BYTES = B * HO * WO * 3 * 4
g = torch.Generator(device=dev).manual_seed(0)
NB = 4                                                 # different batches of the permutation, cycled


def matrices(aug, rows):
    """[B,2,3] affine_grid matrices of about the same transforms (normalised [-1, 1] coordinates); built once, not timed."""
    n = rows.numel()
    r = torch.rand(n, 5, generator=g, device=dev)
    flip = torch.where(r[:, 0] < aug.p_flip, -1.0, 1.0)
    th = (2 * r[:, 1] - 1) * aug.max_rot
    s = 1 / (1 + (2 * r[:, 2] - 1) * aug.scale_range)
    t = -2 * (2 * r[:, 3:5] - 1) * aug.max_shift
    c, sn = torch.cos(th) * s, torch.sin(th) * s
    return torch.stack([torch.stack([flip * c, flip * sn, flip * t[:, 0]], 1), torch.stack([-sn, c, t[:, 1]], 1)], 1).contiguous()


def torch_warp(table, idx, theta):
    x = table[idx].float() / 256
    grid = F.affine_grid(theta, (idx.numel(), 3, HO, WO), align_corners=False)
    y = F.grid_sample(x.permute(0, 3, 1, 2), grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    return y.permute(0, 2, 3, 1).contiguous()


def torch_resize(table, idx):
    x = table[idx].float() / 256
    y = F.interpolate(x.permute(0, 3, 1, 2), size=(HO, WO), mode="bilinear", align_corners=False)
    return y.permute(0, 2, 3, 1).contiguous()


def _ours(table, idx, aug, x2d=None):
    """One launch: the gather is the kernel's src_idx (data.py _frame_launch, what FrameFeeder's resident mode calls).
    x2d: the table's source 2-D poses -> the launch with crop=PersonCrop() (pl_frame_warp_gather_crop)."""
    out = torch.empty((idx.numel(), HO, WO, 3), dtype=torch.float32, device=dev)
    st = pkg.data._frame_augment_struct(aug)
    crop = pkg.PersonCrop().struct(table.shape[1:3]) if x2d is not None else None
    pkg.data._frame_launch(table, pkg._lib.FRAME_U8, idx, idx, idx.numel(), out, 1.0 / 256.0, 0.0, st, 3, crop, x2d)
    return out


AUGS = [("plain", None), ("flip (p = 0.5)", pkg.PoseAugment(p_flip=0.5, seed=1)),
        ("every stage on", pkg.PoseAugment(p_flip=0.5, max_rot=0.5, scale_range=0.25, max_shift=0.1, jitter_sigma=0.05, seed=1))]
lines = [f"B = {B} frames into {HO} x {WO} x 3 fp32 ({OUT_BYTES / 1e6:.0f} MB written per call), resident uint8 tables, "
         f"{torch.cuda.get_device_name(0)}",
         f"us per call: median [min .. p90] of {args.reps} single calls between a device event pair, variants alternated | "
         f"output bytes / median time, and its share of {HBM / 1e12:.1f} TB/s"]
slower = []
for hs, ws in ((1000, 1002), (256, 256)):
    n_frames = B * NB
    table = torch.randint(0, 256, (n_frames, hs, ws, 3), dtype=torch.uint8, device=dev, generator=g)
    perm = torch.randperm(n_frames, generator=g, device=dev)
    batches = [perm[k * B:(k + 1) * B].contiguous() for k in range(NB)]
    # crop rows: 17 joints spread over 0.32 of the frame about a centre in [0.3, 0.7)^2 -- boxes of about 400 px on the large table
    x2d = (0.3 + 0.4 * torch.rand(n_frames, 1, 2, generator=g, device=dev)
           + 0.32 * (torch.rand(n_frames, 17, 2, generator=g, device=dev) - 0.5)).contiguous()
    variants = []
    for name, aug in AUGS:
        ours = lambda k, aug=aug: _ours(table, batches[k % NB], aug)
        thetas = [matrices(aug if aug is not None else pkg.PoseAugment(), b) for b in batches]
        variants.append((f"pl_frame_warp_gather, {name}", ours, True))
        variants.append((f"torch index + float/256 + affine_grid + grid_sample, {name}",
                         lambda k, thetas=thetas: torch_warp(table, batches[k % NB], thetas[k % NB]), False))
        if name != "flip (p = 0.5)":
            variants.append((f"pl_frame_warp_gather_crop, {name} + crop", lambda k, aug=aug: _ours(table, batches[k % NB], aug, x2d), True))
        if aug is None:
            variants.append(("torch index + float/256 + F.interpolate, plain", lambda k: torch_resize(table, batches[k % NB]), False))

    for _, fn, _ in variants:
        for k in range(3):
            fn(k)
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    for k in range(args.reps):
        for name, fn, _ in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(k)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
            del out
    lines.append(f"-- table {n_frames} x {hs} x {ws} x 3 uint8 ({n_frames * hs * ws * 3 / 2 ** 30:.2f} GiB)")
    med = {}
    for name, _, mine in variants:
        s = sorted(times[name])
        med[name] = statistics.median(s)
        rate = OUT_BYTES / (med[name] * 1e-6)
        lines.append(f"{name:66s} {med[name]:9.1f} [{s[0]:9.1f} .. {s[int(0.9 * len(s))]:9.1f}] | {rate / 1e12:5.2f} TB/s "
                     f"{100 * rate / HBM:5.1f} %")
    for name, aug in AUGS:
        mine = med[f"pl_frame_warp_gather, {name}"]
        base = med[f"torch index + float/256 + affine_grid + grid_sample, {name}"]
        lines.append(f"   {name}: kernel {mine:.1f} us, torch composition {base:.1f} us: {base / mine:.1f} x")
        if not mine < base:
            slower.append((hs, ws, name))
    del table
    torch.cuda.empty_cache()
lines.append("the kernel is faster than the torch composition in every row" if not slower
             else f"the kernel is NOT faster than the torch composition in: {slower}")
print("\n".join(lines))
if args.out:
    with open(args.out, "w") as f:
        f.write(f"python tools/bench_frame_warp.py --out {args.out}\n\n" + "\n".join(lines) + "\n")
