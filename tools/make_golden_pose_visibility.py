"""Writes tests/golden/g16_pose_visibility.npz: the weights of the g13 skeletons (tests/golden/g13_pose_metrics.npz; seed 0 of
row_weights_oracle.weights: about a quarter zeros, row 64 and joint 5 all zero) and the fp64 answers of
tests/pose_visibility_oracle.py on them -- a drift guard for that oracle, produced by this repository alone.

    python tools/make_golden_pose_visibility.py

The fixture is data only: w (128, 17) fp32, err (3, 128, 17), aligned (128, 17, 3) and gap (128,) fp64."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_visibility_oracle as orc  # noqa: E402


def main():
    pred, tgt = orc.golden_poses()
    w = orc.weights(128, 17, 0)
    err, aligned, gap = orc.pose_errors(pred, tgt, w)
    np.savez_compressed(orc.GOLDEN, w=w, err=err, aligned=aligned, gap=gap)
    v = orc.visible(w)
    print(f"{orc.GOLDEN}: {os.path.getsize(orc.GOLDEN)} bytes; masked MPJPE {err[0][v].mean():.4f} N-MPJPE {err[1][v].mean():.4f} "
          f"P-MPJPE {err[2][v].mean():.4f}, smallest eigenvalue gap {gap.min():.3f}")


if __name__ == "__main__":
    main()
