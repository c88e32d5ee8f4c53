"""pl_gather_rows2 against pl_pose_augment_gather at B = 4096 from a 1M-row resident table: hipEvent pairs around single
launches (median of 400 after warm-up, variants alternated) and back-to-back launches (2000 between one event pair).
The back-to-back column is bounded by the host's launch rate when the kernel is shorter than a launch.

    python tools/bench_pose_augment.py [--out profiles/pose_augment_time.txt]"""
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
args = ap.parse_args()
pkg = ge.build()
L = pkg.lib()
dev = torch.device("cuda", 0)
ROWS, B = 1 << 20, 4096
g = torch.Generator().manual_seed(0)
a = torch.rand(ROWS, 17, 2, generator=g).to(dev)
b = torch.randn(ROWS, 17, 3, generator=g).to(dev)
perm = torch.randperm(ROWS, generator=g).to(dev)
NB = 64                                               # 64 different batches of the permutation, cycled
oa, ob = torch.empty(B, 17, 2, device=dev), torch.empty(B, 17, 3, device=dev)
stream = pkg._lib.current_stream_ptr()


def plain(k):
    idx = perm[(k % NB) * B:(k % NB + 1) * B]
    assert L.pl_gather_rows2(a.data_ptr(), 34, b.data_ptr(), 51, idx.data_ptr(), B, ROWS, oa.data_ptr(), ob.data_ptr(), stream) == 0


def augmented(aug):
    st = aug.struct()

    def run(k):
        idx = perm[(k % NB) * B:(k % NB + 1) * B]
        assert L.pl_pose_augment_gather(a.data_ptr(), b.data_ptr(), idx.data_ptr(), idx.data_ptr(), B, ROWS, oa.data_ptr(),
                                        ob.data_ptr(), ctypes.byref(st), 3, stream) == 0
    return run


variants = [("pl_gather_rows2", plain),
            ("augment identity", augmented(pkg.PoseAugment())),
            ("augment flip only (p=0.5)", augmented(pkg.PoseAugment(p_flip=0.5, seed=1))),
            ("augment all on", augmented(pkg.PoseAugment(p_flip=0.5, max_rot=0.5, scale_range=0.25, max_shift=0.1,
                                                          jitter_sigma=0.05, seed=1)))]
for _, fn in variants:
    for k in range(50):
        fn(k)
torch.cuda.synchronize()

single = {name: [] for name, _ in variants}
for k in range(400):
    for name, fn in variants:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(k)
        e1.record()
        e1.synchronize()
        single[name].append(e0.elapsed_time(e1) * 1e3)
stream_us = {name: [] for name, _ in variants}
for rep in range(5):
    for name, fn in variants:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for k in range(2000):
            fn(k)
        e1.record()
        e1.synchronize()
        stream_us[name].append(e0.elapsed_time(e1) * 1e3 / 2000)

lines = [f"B = {B} poses from a {ROWS}-row resident table ({ROWS * 340 / 2 ** 20:.0f} MiB), {torch.cuda.get_device_name(0)}",
         "us per launch: median [min .. p90] of 400 single launches between an event pair | median of 5 x 2000 back-to-back launches"]
for name, _ in variants:
    s = sorted(single[name])
    lines.append(f"{name:28s} {statistics.median(s):7.2f} [{s[0]:6.2f} .. {s[int(0.9 * len(s))]:6.2f}] | "
                 f"{statistics.median(stream_us[name]):7.2f}")
print("\n".join(lines))
if args.out:
    with open(args.out, "w") as f:
        f.write(f"python tools/bench_pose_augment.py --out {args.out}\n\n" + "\n".join(lines) + "\n")
