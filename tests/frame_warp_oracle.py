"""Restatement of the frame-warp definition (csrc/frame_warp.h, include/poselift.h PLFrameWarp) in numpy, written from the
definition: in fp64 (the oracle) and, same formulas, in fp32 (the twin, whose own error against fp64 is the yardstick for the
code under test).  The decisions of a row are pose_augment_oracle.decisions: nothing about the draws is restated.  Shared by
test_frame_warp_host.py and test_gpu_frame_warp.py.

Definition.  src [N][Hs][Ws][3] uint8 or fp32 -> out [n][Ho][Wo][3] fp32.  Output pixel (i, j) of a sample whose row drew
flip, theta, s, tx, ty (c = cos theta, sn = sin theta); a stage whose parameter is 0 is skipped:
  u = (j + 0.5) / Wo, v = (i + 0.5) / Ho
  u -= tx, v -= ty;   u = (u - cx) / s + cx, v = (v - cy) / s + cy
  du = u - cx, dv = v - cy: u = (c du + sn dv) + cx, v = (-sn du + c dv) + cy;   flipped: u = 1 - u
  xs = u Ws - 0.5, ys = v Hs - 0.5   (evaluated as frame_warp.h says: the flip as xs = (Ws - 1) - xs, and with shift, scale
  and rotation off xs = (j + 0.5) (Ws / Wo) - 0.5, ys likewise);  outside [-0.5, Ws - 0.5] x [-0.5, Hs - 0.5]: fill
  else clamp xs to [0, Ws - 1], ys to [0, Hs - 1]; x0 = floor xs, x1 = min(x0 + 1, Ws - 1), fx = xs - x0, y likewise;
  value = scale ((1 - fy) ((1 - fx) p00 + fx p01) + fy ((1 - fx) p10 + fx p11))
"""
import numpy as np

import pose_augment_oracle as pao


def source_positions(cfg, epoch, rows, src_hw, out_hw, dtype):
    """(xs, ys, decisions): the source position (n, Ho, Wo) of every output pixel, arithmetic in dtype."""
    T = dtype
    (Hs, Ws), (Ho, Wo) = src_hw, out_hw
    rows = np.asarray(rows, dtype=np.uint64)
    n = len(rows)
    d = pao.decisions(cfg, epoch, rows, T)
    cx, cy = T(cfg["cx"]), T(cfg["cy"])
    per = lambda x: np.asarray(x, dtype=T)[:, None, None]
    jc, ic = np.arange(Wo).astype(T) + T(0.5), np.arange(Ho).astype(T) + T(0.5)
    if cfg["max_shift"] == 0.0 and cfg["scale_range"] == 0.0 and cfg["max_rot"] == 0.0:
        xs = np.broadcast_to((jc * (T(Ws) / T(Wo)) - T(0.5))[None, None, :], (n, Ho, Wo)).copy()
        ys = np.broadcast_to((ic * (T(Hs) / T(Ho)) - T(0.5))[None, :, None], (n, Ho, Wo)).copy()
    else:
        u = np.broadcast_to((jc / T(Wo))[None, None, :], (n, Ho, Wo)).copy()
        v = np.broadcast_to((ic / T(Ho))[None, :, None], (n, Ho, Wo)).copy()
        if cfg["max_shift"] != 0.0:
            u, v = u - per(d["tx"]), v - per(d["ty"])
        if cfg["scale_range"] != 0.0:
            u, v = (u - cx) / per(d["s"]) + cx, (v - cy) / per(d["s"]) + cy
        if cfg["max_rot"] != 0.0:
            c, s = per(np.cos(d["theta"])), per(np.sin(d["theta"]))
            du, dv = u - cx, v - cy
            u, v = (c * du + s * dv) + cx, ((-s) * du + c * dv) + cy
        xs, ys = u * T(Ws) - T(0.5), v * T(Hs) - T(0.5)
    if cfg["p_flip"] > 0.0:
        xs = np.where(d["flip"][:, None, None], T(Ws - 1) - xs, xs)
    assert xs.dtype == T and ys.dtype == T
    return xs, ys, d


def sample(frames, xs, ys, scale, fill, dtype):
    """Steps 4-6 on already gathered frames (n, Hs, Ws, 3): (out (n, Ho, Wo, 3) in dtype, inside mask (n, Ho, Wo))."""
    T = dtype
    n, Hs, Ws, C = frames.shape
    assert C == 3 and xs.shape[0] == n
    inside = (xs >= T(-0.5)) & (xs <= T(Ws) - T(0.5)) & (ys >= T(-0.5)) & (ys <= T(Hs) - T(0.5))
    xc, yc = np.clip(xs, T(0), T(Ws - 1)), np.clip(ys, T(0), T(Hs - 1))
    xf, yf = np.floor(xc), np.floor(yc)
    fx, fy = (xc - xf)[..., None], (yc - yf)[..., None]
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, Ws - 1), np.minimum(y0 + 1, Hs - 1)
    k = np.arange(n)[:, None, None]
    p00, p01 = frames[k, y0, x0].astype(T), frames[k, y0, x1].astype(T)
    p10, p11 = frames[k, y1, x0].astype(T), frames[k, y1, x1].astype(T)
    gx, gy = T(1) - fx, T(1) - fy
    val = T(scale) * (gy * (gx * p00 + fx * p01) + fy * (gx * p10 + fx * p11))
    out = np.where(inside[..., None], val, T(fill))
    assert out.dtype == T
    return out, inside


def warp(cfg, epoch, rows, frames, out_hw, scale, fill=0.0, dtype=np.float64):
    """frames (n, Hs, Ws, 3) uint8 / fp32: the SOURCE frames of the rows (already gathered) -> dict(out, inside, xs, ys,
    decisions), arithmetic in dtype."""
    frames = np.asarray(frames)
    xs, ys, d = source_positions(cfg, epoch, rows, frames.shape[1:3], out_hw, dtype)
    out, inside = sample(frames, xs, ys, scale, fill, dtype)
    return dict(out=out, inside=inside, xs=xs, ys=ys, decisions=d)
