"""Restatement of the person-centred crop (csrc/frame_crop.h, include/poselift.h PLPoseCrop) in numpy, written from the
definition: in fp64 (the oracle) and, same formulas, in fp32 (the twin, whose own error against fp64 is the yardstick for the
code under test).  The augmentation behind the crop is pose_augment_oracle's, the sampling of a source position
frame_warp_oracle's: nothing of either is restated.  Shared by test_frame_crop_host.py and test_gpu_frame_crop.py.

Definition.  Box of a row from its source 2-D pose a (17,2), image-normalised, and the source frame (Hs, Ws):
  ex = (xmax - xmin) Ws, ey = (ymax - ymin) Hs;  side = max(ceil(margin max(ex, ey)), min_side)
  bbox: ccx = (0.5 (xmin + xmax)) Ws, ccy = (0.5 (ymin + ymax)) Hs;   root: ccx = a[0][0] Ws, ccy = a[0][1] Hs
  x0 = rint(ccx - 0.5 side), y0 = rint(ccy - 0.5 side)     (ties to even)
  a non-finite coordinate, or side > 2^20: the box is NaN
Pose: a'x = (ax Ws - x0) / side, a'y = (ay Hs - y0) / side, then pose_augment_oracle.augment on a'.
Back: ax = (a'x side + x0) / Ws, ay = (a'y side + y0) / Hs.
Frame: u, v of frame_warp_oracle through the inverse pose transform (crop-normalised), then
  xl = u side - 0.5 (shift, scale and rotation all off: xl = (j + 0.5) (side / Wo) - 0.5), flipped: xl = (side - 1) - xl,
  xs = xl + x0;  yl, ys likewise with Ho and y0 and no flip;  then frame_warp_oracle.sample against the frame.
  A NaN box: a NaN frame.
"""
import numpy as np

import frame_warp_oracle as fwo
import pose_augment_oracle as pao

MAX_SIDE = 2.0 ** 20


def spec(margin=1.25, centre="bbox", min_side=8):
    """A full crop spec; margin is rounded to fp32, which is what the library is handed."""
    assert centre in ("bbox", "root")
    return dict(margin=float(np.float32(margin)), centre=centre, min_side=int(min_side))


def boxes(sp, a, src_hw, dtype):
    """a (n,17,2) -> (n,4) = (x0, y0, side, side) in dtype; NaN rows where the definition says so."""
    T = dtype
    Hs, Ws = src_hw
    A = np.asarray(a).reshape(-1, 17, 2).astype(T)
    with np.errstate(invalid="ignore", over="ignore"):
        finite = np.isfinite(A).all(axis=(1, 2))
        x, y = np.where(np.isfinite(A[:, :, 0]), A[:, :, 0], T(0)), np.where(np.isfinite(A[:, :, 1]), A[:, :, 1], T(0))
        xmin, xmax, ymin, ymax = x.min(axis=1), x.max(axis=1), y.min(axis=1), y.max(axis=1)
        ex, ey = (xmax - xmin) * T(Ws), (ymax - ymin) * T(Hs)
        side = np.maximum(np.ceil(T(sp["margin"]) * np.maximum(ex, ey)), T(sp["min_side"]))
        if sp["centre"] == "root":
            ccx, ccy = x[:, 0] * T(Ws), y[:, 0] * T(Hs)
        else:
            ccx, ccy = (T(0.5) * (xmin + xmax)) * T(Ws), (T(0.5) * (ymin + ymax)) * T(Hs)
        h = T(0.5) * side
        x0, y0 = np.rint(ccx - h), np.rint(ccy - h)
        bad = ~finite | ~(side <= T(MAX_SIDE))
    out = np.stack([x0, y0, side, side], axis=1)
    out[bad] = np.nan
    assert out.dtype == T
    return out


def crop_poses(p, bx, src_hw, dtype, offset=True):
    """Image-normalised (n,17,2) -> crop-normalised; offset=False leaves x0, y0 out (the map's factor alone)."""
    T = dtype
    P, B = np.asarray(p).reshape(-1, 17, 2).astype(T), np.asarray(bx).astype(T)
    W = np.array([src_hw[1], src_hw[0]], T)
    t = P * W
    if offset:
        t = t - B[:, None, 0:2]
    out = t / B[:, None, 2:3]
    assert out.dtype == T
    return out


def uncrop_poses(p, bx, src_hw, dtype, offset=True):
    T = dtype
    P, B = np.asarray(p).reshape(-1, 17, 2).astype(T), np.asarray(bx).astype(T)
    W = np.array([src_hw[1], src_hw[0]], T)
    t = P * B[:, None, 2:3]
    if offset:
        t = t + B[:, None, 0:2]
    out = t / W
    assert out.dtype == T
    return out


def augment(cfg, epoch, rows, a, b, sp, src_hw, dtype=np.float64, bx=None):
    """The source poses of the rows -> (oa, ob, boxes, decisions) in dtype: crop, then pose_augment_oracle.augment.
    bx: boxes to use in place of the ones dtype gives (the fp64 oracle on the library's integer boxes)."""
    if bx is None:
        bx = boxes(sp, a, src_hw, dtype)
    with np.errstate(invalid="ignore"):
        oa, ob, d = pao.augment(cfg, epoch, rows, crop_poses(a, bx, src_hw, dtype), b, dtype)
    return oa, ob, bx, d


def source_positions(cfg, epoch, rows, bx, out_hw, dtype):
    """(xs, ys, decisions): the source position (n, Ho, Wo), in the frame, of every output pixel; bx (n,4) finite."""
    T = dtype
    Ho, Wo = out_hw
    rows = np.asarray(rows, dtype=np.uint64)
    n = len(rows)
    d = pao.decisions(cfg, epoch, rows, T)
    cx, cy = T(cfg["cx"]), T(cfg["cy"])
    per = lambda x: np.asarray(x, dtype=T)[:, None, None]
    B = np.asarray(bx).astype(T)
    x0, y0, side = per(B[:, 0]), per(B[:, 1]), per(B[:, 2])
    jc, ic = np.arange(Wo).astype(T) + T(0.5), np.arange(Ho).astype(T) + T(0.5)
    if cfg["max_shift"] == 0.0 and cfg["scale_range"] == 0.0 and cfg["max_rot"] == 0.0:
        xl = jc[None, None, :] * (side / T(Wo)) - T(0.5) + np.zeros((n, Ho, Wo), T)
        yl = ic[None, :, None] * (side / T(Ho)) - T(0.5) + np.zeros((n, Ho, Wo), T)
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
        xl, yl = u * side - T(0.5), v * side - T(0.5)
    if cfg["p_flip"] > 0.0:
        xl = np.where(d["flip"][:, None, None], (side - T(1)) - xl, xl)
    xs, ys = xl + x0, yl + y0
    assert xs.dtype == T and ys.dtype == T
    return xs, ys, d


def warp(cfg, epoch, rows, frames, a, sp, out_hw, scale, fill=0.0, dtype=np.float64, bx=None):
    """frames (n, Hs, Ws, 3) and a (n,17,2): the SOURCE frames and poses of the rows (already gathered) ->
    dict(out, inside, xs, ys, boxes, decisions), arithmetic in dtype.  bx as in augment."""
    frames = np.asarray(frames)
    if bx is None:
        bx = boxes(sp, a, frames.shape[1:3], dtype)
    nan = np.isnan(np.asarray(bx)[:, 2])
    safe = np.where(nan[:, None], np.array([0, 0, 1, 1], dtype), np.asarray(bx).astype(dtype))
    xs, ys, d = source_positions(cfg, epoch, rows, safe, out_hw, dtype)
    out, inside = fwo.sample(frames, xs, ys, scale, fill, dtype)
    out[nan] = np.nan
    inside[nan] = False
    return dict(out=out, inside=inside, xs=xs, ys=ys, boxes=bx, decisions=d)
