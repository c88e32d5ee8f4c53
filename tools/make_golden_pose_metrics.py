"""Writes tests/golden/g13_pose_metrics.npz: 128 real skeletons as evaluation inputs and the fp64 oracle's answers.

    python tools/make_golden_pose_metrics.py /path/to/reference

Targets are frames 0:640:5 of the reference's phase2_opp_mb/MB_npy/"Walking 1.mp4.npy" ((frames, 17, 3) fp32), root-centred;
the "predictions" are frames 3:643:5, root-centred: the same walk 3 frames later, a few centimetres off in every joint.
The fixture is data only: pred, tgt (128, 17, 3) fp32, err (3, 128, 17) and aligned (128, 17, 3) fp64 from
tests/pose_metrics_oracle.py, and gap (128,)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_metrics_oracle as orc  # noqa: E402


def main(reference_root):
    seq = np.load(os.path.join(reference_root, "phase2_opp_mb", "MB_npy", "Walking 1.mp4.npy")).astype(np.float32)
    assert seq.ndim == 3 and seq.shape[1:] == (17, 3) and seq.shape[0] >= 643, seq.shape
    seq = seq - seq[:, :1]
    tgt = np.ascontiguousarray(seq[0:640:5])
    pred = np.ascontiguousarray(seq[3:643:5])
    err, aligned, gap = orc.pose_errors(pred, tgt)
    np.savez_compressed(orc.GOLDEN, pred=pred, tgt=tgt, err=err, aligned=aligned, gap=gap)
    print(f"{orc.GOLDEN}: {os.path.getsize(orc.GOLDEN)} bytes; MPJPE {err[0].mean():.4f} N-MPJPE {err[1].mean():.4f} "
          f"P-MPJPE {err[2].mean():.4f} (the sequence's own units), smallest eigenvalue gap {gap.min():.2f}")


if __name__ == "__main__":
    main(sys.argv[1])
