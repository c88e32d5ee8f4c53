"""What the person-centred crop costs: the frame warp and the pose gather with and without `crop=`, and -- with --parent-lib,
a build of the parent commit's library -- the launches without a crop against the parent's in the same session.

Protocol of tools/bench_frame_warp.py: B = 256 frames into 256 x 256 from resident uint8 tables of 1000 x 1002 and 256 x 256
frames, device event pairs around single launches after warm-up, variants alternated, a different batch of the permutation
each call (order reversed on odd repetitions); median [min .. p90] of --reps.  The whole loop runs twice: the two medians of one variant are the session's
run-to-run spread, which a difference between two variants has to exceed to mean anything.  Poses are synthetic, 17 joints
spread over 0.32 of the frame about a centre in [0.3, 0.7)^2: with margin 1.25 the boxes are about 400 px on the large table.
The pose launch: B = 4096 from a 1048576-row table, the protocol of tools/bench_pose_table.py part 1 (--pose-reps launches).

    python tools/bench_frame_crop.py [--parent-lib PATH] [--out profiles/frame_crop_time.txt]"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the table to this file")
ap.add_argument("--parent-lib", default=None, help="libposelift.so built from the parent commit")
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--pose-reps", type=int, default=400)
args = ap.parse_args()
pkg = ge.build()
L = pkg._lib
dev = torch.device("cuda", 0)
B, HO, WO, HBM, NB = args.batch, 256, 256, 6.3e12, 4
OUT_BYTES = B * HO * WO * 3 * 4
g = torch.Generator(device=dev).manual_seed(0)
libs = {"this tree": pkg.lib()}
if args.parent_lib:
    parent = ctypes.CDLL(args.parent_lib)
    for name in ("pl_frame_warp_gather", "pl_pose_augment_gather", "pl_version"):
        getattr(parent, name).restype, getattr(parent, name).argtypes = L.SIGNATURES[name]
    libs = {"parent": parent, "this tree": pkg.lib()}
ALL_ON = pkg.PoseAugment(p_flip=0.5, max_rot=0.5, scale_range=0.25, max_shift=0.1, jitter_sigma=0.05, seed=1)
CROP = pkg.PersonCrop()


def poses(n):
    c = 0.3 + 0.4 * torch.rand(n, 1, 2, generator=g, device=dev)
    return (c + 0.32 * (torch.rand(n, 17, 2, generator=g, device=dev) - 0.5)).contiguous()


def timed(variants, reps):
    """{name: (median, min, p90)} in us, single calls between an event pair, variants alternated: in list order on even
    repetitions and in reverse on odd ones, and neighbours in the list on different batches, so that no variant always
    runs behind the same other one or finds its own batch in the caches."""
    for _, fn in variants:
        for k in range(3):
            fn(k)
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    order = list(enumerate(variants))
    for k in range(reps):
        for vi, (name, fn) in (order if k % 2 == 0 else reversed(order)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(k + vi)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    out = {}
    for name, t in times.items():
        s = sorted(t)
        out[name] = (statistics.median(s), s[0], s[int(0.9 * len(s))])
    return out


def report(lines, variants, reps, rate_bytes=None):
    first, second = timed(variants, reps), timed(variants, reps)
    for name, _ in variants:
        (m1, lo1, p1), (m2, lo2, p2) = first[name], second[name]
        rate = "" if rate_bytes is None else f" | {rate_bytes / (min(m1, m2) * 1e-6) / 1e12:5.2f} TB/s {100 * rate_bytes / (min(m1, m2) * 1e-6) / HBM:5.1f} %"
        lines.append(f"{name:44s} {m1:8.1f} [{lo1:8.1f} .. {p1:8.1f}]   {m2:8.1f} [{lo2:8.1f} .. {p2:8.1f}]   spread {abs(m1 - m2):6.1f}{rate}")
    return first, second


lines = [f"{torch.cuda.get_device_name(0)}; libraries: " + ", ".join(f"{k} version {v.pl_version()}" for k, v in libs.items()),
         f"1. + 2.  B = {B} frames into {HO} x {WO} x 3 fp32 ({OUT_BYTES / 1e6:.0f} MB written per launch), resident uint8 tables",
         f"us per launch: median [min .. p90] of {args.reps} single launches between a device event pair, variants alternated; the "
         f"whole loop twice (first pass, second pass), spread = |difference of the two medians| | output bytes / the lower median, "
         f"and its share of {HBM / 1e12:.1f} TB/s"]
for hs, ws in ((1000, 1002), (256, 256)):
    n_frames = B * NB
    table = torch.randint(0, 256, (n_frames, hs, ws, 3), dtype=torch.uint8, device=dev, generator=g)
    x2d = poses(n_frames)
    perm = torch.randperm(n_frames, generator=g, device=dev)
    batches = [perm[k * B:(k + 1) * B].contiguous() for k in range(NB)]
    out = torch.empty((B, HO, WO, 3), dtype=torch.float32, device=dev)
    crop_s = CROP.struct((hs, ws))
    boxes = pkg.crop_boxes(x2d, CROP, (hs, ws))
    side = boxes[:, 2]

    def launch(lib, k, aug, crop):
        idx = batches[k % NB]
        st = pkg.data._frame_augment_struct(aug)
        a = L.PLFrameWarp(table.data_ptr(), L.FRAME_U8, 3, n_frames, hs, ws, idx.data_ptr(), idx.data_ptr(), B, out.data_ptr(), HO,
                          WO, 1.0 / 256.0, 0.0, ctypes.pointer(st) if st is not None else None, 3)
        if crop:
            rc = lib.pl_frame_warp_gather_crop(ctypes.byref(a), ctypes.byref(crop_s), x2d.data_ptr(), L.current_stream_ptr())
        else:
            rc = lib.pl_frame_warp_gather(ctypes.byref(a), L.current_stream_ptr())
        assert rc == 0

    variants = []
    for cname, aug in (("plain", None), ("every stage on", ALL_ON)):
        for lname, lib in libs.items():
            variants.append((f"{cname}, {lname}", lambda k, lib=lib, aug=aug: launch(lib, k, aug, False)))
        variants.append((f"{cname} + crop, this tree", lambda k, aug=aug: launch(libs["this tree"], k, aug, True)))
    lines.append(f"-- table {n_frames} x {hs} x {ws} x 3 uint8 ({n_frames * hs * ws * 3 / 2 ** 30:.2f} GiB); boxes: side median "
                 f"{side.median().item():.0f} px [{side.min().item():.0f} .. {side.max().item():.0f}]")
    report(lines, variants, args.reps, OUT_BYTES)
    if args.parent_lib:                                      # finite results of the launches without a crop are bitwise equal
        same = []
        for aug in (None, ALL_ON):
            launch(libs["parent"], 0, aug, False)
            ref = out.clone()
            launch(libs["this tree"], 0, aug, False)
            same.append(torch.equal(out, ref))
        lines.append(f"   without a crop, parent and this tree write the same bits on batch 0: plain {same[0]}, every stage on {same[1]}")
    del table
    torch.cuda.empty_cache()

N, PB = 1 << 20, 4096
a, b = poses(N).reshape(N, 34), torch.randn(N, 51, device=dev, generator=g)
perm = torch.randperm(N, generator=g, device=dev)
pb = [perm[k * PB:(k + 1) * PB].contiguous() for k in range(NB)]
oa, ob, bx = torch.empty(PB, 34, device=dev), torch.empty(PB, 51, device=dev), torch.empty(PB, 4, device=dev)
crop_s = CROP.struct((1000, 1002))


def pose_launch(lib, k, aug, crop):
    idx, st = pb[k % NB], aug.struct()
    head = (a.data_ptr(), b.data_ptr(), idx.data_ptr(), idx.data_ptr(), PB, N, oa.data_ptr(), ob.data_ptr(), ctypes.byref(st), 3)
    if crop:
        rc = lib.pl_pose_augment_gather_crop(*head, ctypes.byref(crop_s), bx.data_ptr(), L.current_stream_ptr())
    else:
        rc = lib.pl_pose_augment_gather(*head, L.current_stream_ptr())
    assert rc == 0


variants = []
for cname, aug in (("augment identity", pkg.PoseAugment()), ("augment all on", ALL_ON)):
    for lname, lib in libs.items():
        variants.append((f"{cname}, {lname}", lambda k, lib=lib, aug=aug: pose_launch(lib, k, aug, False)))
    variants.append((f"{cname} + crop, this tree", lambda k, aug=aug: pose_launch(libs["this tree"], k, aug, True)))
lines.append(f"3.  the pose launch: B = {PB} poses from a {N}-row resident table; us per launch, median [min .. p90] of {args.pose_reps} "
             f"single launches between an event pair, variants alternated, the loop twice")
report(lines, variants, args.pose_reps)
print("\n".join(lines))
if args.out:
    with open(args.out, "w") as f:
        f.write("python tools/bench_frame_crop.py" + (" --parent-lib <the parent commit's libposelift.so>" if args.parent_lib else "")
                + f" --out {args.out}\n\n" + "\n".join(lines) + "\n")
