#!/usr/bin/env python3
"""Generate tests/golden/g17_cameras.npz: the four Human3.6M intrinsic rows the reference carries, data only.

Build-container only: reads the literal `h36m_cameras_intrinsic_params` out of the reference's
phase3_direct/my_HybrIK/utils.py (lines 131-172: id, centre, focal length, three radial and two tangential coefficients,
resolution per camera) without importing or copying the file, and records

    cameras  (4, 9) float64   fx, fy, cx, cy, k1, k2, k3, p1, p2 per row (the layout of csrc/camera.h)
    ids      (4,)   int64     the camera serial numbers, row by row
    res      (4, 2) int64     (width, height)

    python tools/make_camera_golden.py [--reference /root/reference]
"""
import argparse
import ast
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reference", default="/root/reference")
args = ap.parse_args()

path = os.path.join(args.reference, "phase3_direct", "my_HybrIK", "utils.py")
with open(path) as f:
    tree = ast.parse(f.read())
rows = None
for node in tree.body:
    if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "h36m_cameras_intrinsic_params" for t in node.targets):
        rows = ast.literal_eval(node.value)
assert rows is not None and len(rows) == 4, "h36m_cameras_intrinsic_params not found"
cameras = np.array([r["focal_length"] + r["center"] + r["radial_distortion"] + r["tangential_distortion"] for r in rows],
                   dtype=np.float64)
ids = np.array([int(r["id"]) for r in rows], dtype=np.int64)
res = np.array([[r["res_w"], r["res_h"]] for r in rows], dtype=np.int64)
assert cameras.shape == (4, 9) and np.isfinite(cameras).all() and 58860488 in ids
out = os.path.join(ROOT, "tests", "golden", "g17_cameras.npz")
np.savez(out, cameras=cameras, ids=ids, res=res)
print(out, os.path.getsize(out))
