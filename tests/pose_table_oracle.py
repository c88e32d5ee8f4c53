"""numpy restatement of csrc/pose_table.h, written from the text of the reference (phase3_direct/my_HybrIK/H36_dataset.py
:205-300, :303-379; utils.py:324-340): fp64 for the statistics, fp64 with the reference's term order for the camera view,
float32 for root-centring and the transform."""
import numpy as np


def q_mult(q1, q2):
    """utils.py:328-335, term by term (numpy float64 arrays or scalars; no fused operations in numpy)."""
    w1, x1, y1, z1 = q1
    w2, x2, y2, z2 = q2
    w = w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2
    x = w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2
    y = w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2
    z = w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2
    return w, x, y, z


def camera_view(p, cams, cam_id):
    """p (N, J, 3) float32, cams (C, 7) float64 = (t, w, x, y, z), cam_id (N,) -> float32: q (0, (double)p - t) q*, rounded
    once.  Rows whose cam_id is outside [0, C) are NaN."""
    p = np.asarray(p, np.float32)
    cam_id = np.asarray(cam_id, np.int64)
    ok = (cam_id >= 0) & (cam_id < len(cams))
    cam = np.asarray(cams, np.float64)[np.where(ok, cam_id, 0)]                  # (N, 7)
    v = p.astype(np.float64) - cam[:, None, 0:3]
    q = tuple(cam[:, None, 3 + k] for k in range(4))
    qc = (q[0], -q[1], -q[2], -q[3])
    zero = np.zeros_like(v[..., 0])
    r = q_mult(q_mult(q, (zero, v[..., 0], v[..., 1], v[..., 2])), qc)
    out = np.stack(r[1:], axis=-1).astype(np.float32)
    out[~ok] = np.nan
    return out


def root_centre(p):
    """H36_dataset.py:209-211, :288-289 in float32: joints 1.. minus joint 0, joint 0 = +0."""
    p = np.asarray(p, np.float32)
    out = p - p[:, :1]
    out[:, 0] = 0.0
    return out


def prepare(raw, joints=None, cams=None, cam_id=None, zero_centre=False):
    out = np.asarray(raw, np.float32)
    if joints is not None:
        out = out[:, list(joints)]
    bad = None
    if cams is not None:
        out = camera_view(out, cams, cam_id)
        bad = np.isnan(out).all(axis=(1, 2))
    if zero_centre:
        out = root_centre(out)
        if bad is not None:
            out[bad] = np.nan
    return np.ascontiguousarray(out)


def stats(x):
    """x (N, W) float32 -> (4, W) float64: mean, population std about the mean (H36_dataset.py:215-222), min, max.  A
    constant column has mean = its value and std = 0 (the library's rule)."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    n = x64.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        mean = x64.sum(axis=0) / n
        lo, hi = x64.min(axis=0), x64.max(axis=0)
        mean = np.where(lo == hi, lo, mean)
        std = np.sqrt(((x64 - mean) ** 2).sum(axis=0) / n)
    return np.stack([mean, std, lo, hi])


def apply(x, sub, div):
    """numpy's (x - sub) / div on float32; a column with div == 0 gives 0."""
    x, sub, div = np.asarray(x, np.float32), np.asarray(sub, np.float32), np.asarray(div, np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        y = (x - sub) / div
    return np.where(np.broadcast_to(div == 0, y.shape), np.float32(0), y).astype(np.float32)


def invert(y, sub, div):
    """y * div + sub on float32 (two roundings); a column with div == 0 gives sub."""
    y, sub, div = np.asarray(y, np.float32), np.asarray(sub, np.float32), np.asarray(div, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        x = y * div + sub
    return np.where(np.broadcast_to(div == 0, x.shape), np.broadcast_to(sub, x.shape), x).astype(np.float32)
