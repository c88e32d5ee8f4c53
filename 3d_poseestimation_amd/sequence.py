"""Video tracks on the device: from a detector's per-frame keypoints to filtered 3-D poses (csrc/track.h has the
definitions).

  coco_to_h36m      COCO-17 rows in the H36M-17 layout                              pl_track_remap
                    (phase1_lifting/video2keypoints.py:14-57)
  prepare_tracks    remap, scale, validity and gap fill -> (xy, w, state)           pl_track_prepare
  TemporalFilter    odd, non-negative FIR taps (gaussian, box)
  filter_tracks     the confidence-weighted FIR along time                          pl_track_filter
  velocity_errors   MPJVE (order 1) and acceleration error (order 2)                pl_track_velocity_errors
  SequenceLifter    prepare -> 2-D filter -> transform -> model -> denorm -> 3-D filter; locate(): + the root trajectory
  load_keypoints_json   the reference's recorded tracks (host only)

Rows are frames: row t + 1 follows row t unless `seq_ids` (T,) int32 says otherwise -- the frames of one video carry one id
and are contiguous; nothing reads across a change of id.  Every function here only enqueues work on the current stream.
The `w` of prepare_tracks is shaped for `row_weights=` and `normalize_row_weights`.
"""
import json
import math

import numpy as np
import torch

from . import _lib
from .pose_table import PoseTransform, transform_pair

LAYOUTS = {"coco17": 0, "h36m17": 1}
STATE_VALID, STATE_INTERPOLATED, STATE_HELD, STATE_LOST = 0, 1, 2, 3
MAX_GAP, MAX_TAPS, MAX_JOINTS = 64, 65, 32


def _layout(layout):
    try:
        return LAYOUTS[str(layout).lower()]
    except KeyError:
        raise ValueError(f"layout is one of {sorted(LAYOUTS)}, got {layout!r}") from None


def _det(det):
    if not isinstance(det, torch.Tensor):
        raise TypeError("det must be a device tensor")
    _lib.require_device_tensor(det, "det")
    if det.dim() != 3 or det.shape[0] == 0 or tuple(det.shape[1:]) != (17, 3):
        raise ValueError(f"det is (T, 17, 3): x, y, confidence per joint, got {tuple(det.shape)}")
    return det


def _seq(seq_ids, T, device):
    """The (T,) int32 device tensor of sequence ids, or None."""
    if seq_ids is None:
        return None
    if not isinstance(seq_ids, torch.Tensor):
        raise TypeError("seq_ids must be a device tensor or None")
    _lib.require_device_tensor(seq_ids, "seq_ids", torch.int32)
    if tuple(seq_ids.shape) != (T,) or seq_ids.device != device:
        raise ValueError(f"seq_ids holds one int32 id per frame on the frames' device, got {tuple(seq_ids.shape)} on {seq_ids.device}")
    return seq_ids


def _ptr(t):
    return None if t is None else t.data_ptr()


def coco_to_h36m(det):
    """det (T, 17, 3) COCO-17 rows (x, y, confidence) -> a new (T, 17, 3) tensor in the H36M-17 layout: coco2h36m's
    arithmetic in fp32; the confidence of a derived joint is the minimum of its sources'."""
    det = _det(det)
    out = torch.empty_like(det)
    with _lib.on_device(det.device):
        rc = _lib.lib().pl_track_remap(det.data_ptr(), det.shape[0], LAYOUTS["coco17"], out.data_ptr(), _lib.current_stream_ptr())
    _lib.check(rc, "pl_track_remap")
    return out


def prepare_tracks(det, layout="coco17", div=(1.0, 1.0), conf_thr=0.1, max_gap=8, fill_conf=0.5, seq_ids=None):
    """det (T, 17, 3) detector rows -> (xy (T, 17, 2), w (T, 17), state (T, 17) uint8), one launch.  xy = the joints in the
    H36M-17 layout divided by div = (width, height); a joint is valid when its confidence is >= conf_thr and its
    coordinates are finite (a missing frame is all zeros: invalid for conf_thr > 0).  An invalid joint is interpolated
    between the nearest valid samples of that joint when the gap is at most max_gap frames (state 1, w = fill_conf *
    the smaller confidence), held from one side when the other side is the end of the sequence (state 2), and otherwise
    keeps its own value with w = 0 (state 3).  state 0 = valid, w = the confidence."""
    det = _det(det)
    T = det.shape[0]
    seq = _seq(seq_ids, T, det.device)
    xy = torch.empty((T, 17, 2), dtype=torch.float32, device=det.device)
    w = torch.empty((T, 17), dtype=torch.float32, device=det.device)
    state = torch.empty((T, 17), dtype=torch.uint8, device=det.device)
    with _lib.on_device(det.device):
        rc = _lib.lib().pl_track_prepare(det.data_ptr(), T, _layout(layout), float(div[0]), float(div[1]), float(conf_thr),
                                         int(max_gap), float(fill_conf), _ptr(seq), xy.data_ptr(), w.data_ptr(),
                                         state.data_ptr(), _lib.current_stream_ptr())
    _lib.check(rc, "pl_track_prepare")
    return xy, w, state


class TemporalFilter:
    """An FIR along time: K taps, K odd and at most 65, each non-negative and finite, stored as fp32.  The filter divides by
    the sum of the taps (times the weights) it used, so the taps need not sum to one."""

    def __init__(self, taps):
        taps = np.asarray(taps, dtype=np.float64).reshape(-1)
        if taps.size < 1 or taps.size > MAX_TAPS or taps.size % 2 == 0:
            raise ValueError(f"a TemporalFilter has an odd number of taps, at most {MAX_TAPS}; got {taps.size}")
        self.taps = np.ascontiguousarray(taps.astype(np.float32))
        if not (np.isfinite(self.taps).all() and (self.taps >= 0).all()):
            raise ValueError("the taps must be non-negative and finite (in fp32)")

    @classmethod
    def gaussian(cls, sigma, radius=None):
        """exp(-k^2 / (2 sigma^2)) for |k| <= radius (default int(3 sigma + 0.5)), normalised in fp64."""
        sigma = float(sigma)
        if not sigma > 0 or not math.isfinite(sigma):
            raise ValueError("sigma must be positive and finite")
        radius = int(3 * sigma + 0.5) if radius is None else int(radius)
        k = np.arange(-radius, radius + 1, dtype=np.float64)
        t = np.exp(-(k * k) / (2.0 * sigma * sigma))
        return cls(t / t.sum())

    @classmethod
    def box(cls, n):
        """n equal taps (n odd)."""
        return cls(np.full(int(n), 1.0 / int(n), dtype=np.float64))

    def __len__(self):
        return int(self.taps.size)


def filter_tracks(x, filt, weights=None, seq_ids=None):
    """x (T, J, D), D in {2, 3}, J <= 32 -> a new tensor y, y[t, j] = sum_k taps[k] w[s, j] x[s, j] / sum_k taps[k] w[s, j]
    over the frames s = t + k - K // 2 of t's sequence; weights (T, J) or None (weight 1).  A frame whose window holds no
    positive weight keeps x[t].  One launch."""
    if not isinstance(filt, TemporalFilter):
        raise TypeError("filt must be a TemporalFilter")
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a device tensor")
    _lib.require_device_tensor(x, "x")
    if x.dim() != 3 or x.shape[0] == 0 or x.shape[2] not in (2, 3) or not 1 <= x.shape[1] <= MAX_JOINTS:
        raise ValueError(f"x is (T, J, 2) or (T, J, 3), J <= {MAX_JOINTS}, got {tuple(x.shape)}")
    T, J, D = x.shape
    if weights is not None:
        _lib.require_device_tensor(weights, "weights")
        if tuple(weights.shape) != (T, J) or weights.device != x.device:
            raise ValueError(f"weights is (T, J) = {(T, J)} on x's device, got {tuple(weights.shape)}")
    seq = _seq(seq_ids, T, x.device)
    y = torch.empty_like(x)
    with _lib.on_device(x.device):
        rc = _lib.lib().pl_track_filter(x.data_ptr(), T, J, D, _ptr(weights), _ptr(seq), filt.taps.ctypes.data, len(filt),
                                        y.data_ptr(), _lib.current_stream_ptr())
    _lib.check(rc, "pl_track_filter")
    return y


def velocity_errors(pred, target, seq_ids=None, order=1, denorm=None):
    """pred, target (T, J, 3) -> (err (T, J), count (T,) uint8).  order 1: the norm of the difference of the two tracks'
    frame-to-frame velocities (MPJVE once averaged); order 2: of their second differences (acceleration error).  count is 1
    where frame t has its stencil inside its sequence and err is 0 elsewhere, so the mean over real differences is
    err.sum(0) / count.sum().  denorm: the PoseTransform whose space both tracks are in."""
    if not isinstance(pred, torch.Tensor) or not isinstance(target, torch.Tensor):
        raise TypeError("pred and target must be device tensors")
    _lib.require_device_tensor(pred, "pred")
    _lib.require_device_tensor(target, "target")
    if pred.dim() != 3 or pred.shape != target.shape or pred.shape[0] == 0 or pred.shape[2] != 3 or not 1 <= pred.shape[1] <= MAX_JOINTS:
        raise ValueError(f"pred and target are (T, J, 3), J <= {MAX_JOINTS}, got {tuple(pred.shape)} and {tuple(target.shape)}")
    if order not in (1, 2):
        raise ValueError("order is 1 (velocity) or 2 (acceleration)")
    T, J, _ = pred.shape
    seq = _seq(seq_ids, T, pred.device)
    sub, div, _keep = transform_pair(denorm, (J, 3), pred.device, "denorm")
    err = torch.empty((T, J), dtype=torch.float32, device=pred.device)
    count = torch.empty((T,), dtype=torch.uint8, device=pred.device)
    with _lib.on_device(pred.device):
        rc = _lib.lib().pl_track_velocity_errors(pred.data_ptr(), target.data_ptr(), T, J, _ptr(seq), int(order), sub, div,
                                                 err.data_ptr(), count.data_ptr(), _lib.current_stream_ptr())
    _lib.check(rc, "pl_track_velocity_errors")
    return err, count


def load_keypoints_json(path):
    """The reference's recorded track (phase1_lifting/video2keypoints.py:100-109): a list of {"image_id", "category_id",
    "keypoints": 51 numbers or 17 rows of 3, "score"}, one per frame -> (T, 17, 3) float32 on the host."""
    with open(path) as f:
        frames = json.load(f)
    if not isinstance(frames, list) or not frames:
        raise ValueError(f"{path}: expected a non-empty list of frames")
    out = np.zeros((len(frames), 17, 3), dtype=np.float32)
    for t, fr in enumerate(frames):
        kp = np.asarray(fr["keypoints"], dtype=np.float64)
        if kp.size != 51:
            raise ValueError(f"{path}: frame {t} has {kp.size} keypoint numbers, expected 51")
        out[t] = kp.reshape(17, 3)
    return out


class SequenceLifter:
    """Detector rows of a video to 3-D poses: prepare_tracks, the optional 2-D filter (weighted by w), transform_2d, the
    model's eval forward in chunks of `chunk` rows (through predict_flip_tta when flip_tta), denorm.invert, the optional 3-D
    filter (weighted by w).  Nothing in lift() reads the device."""

    def __init__(self, model, layout="coco17", div=(1.0, 1.0), transform_2d=None, denorm=None, conf_thr=0.1, max_gap=8,
                 fill_conf=0.5, filter_2d=None, filter_3d=None, flip_tta=False, chunk=4096):
        for name, t in (("transform_2d", transform_2d), ("denorm", denorm)):
            if t is not None and not isinstance(t, PoseTransform):
                raise TypeError(f"{name} must be a PoseTransform or None")
        for name, f in (("filter_2d", filter_2d), ("filter_3d", filter_3d)):
            if f is not None and not isinstance(f, TemporalFilter):
                raise TypeError(f"{name} must be a TemporalFilter or None")
        if int(chunk) < 1:
            raise ValueError("chunk must be at least 1")
        _layout(layout)
        self.model, self.layout, self.div = model, layout, (float(div[0]), float(div[1]))
        self.transform_2d, self.denorm = transform_2d, denorm
        self.conf_thr, self.max_gap, self.fill_conf = float(conf_thr), int(max_gap), float(fill_conf)
        self.filter_2d, self.filter_3d, self.flip_tta, self.chunk = filter_2d, filter_3d, bool(flip_tta), int(chunk)
        self._div_dev = {}

    @torch.no_grad()
    def lift(self, det, seq_ids=None):
        """det (T, 17, 3) -> (poses (T, 17, 3), w (T, 17), state (T, 17) uint8)."""
        return self._lift(det, seq_ids, False)[:3]

    def _pixels(self, xy):
        """The prepared track back in pixels, xy * div: a new tensor (the transform below works in place on xy)."""
        div = self._div_dev.get(xy.device)
        if div is None:
            div = self._div_dev[xy.device] = torch.tensor(self.div, dtype=torch.float32, device=xy.device)
        return xy * div

    def _lift(self, det, seq_ids, want_pixels):
        """lift(), and the prepared 2-D track in pixels when asked for."""
        from .train import predict_flip_tta
        if self.model.training:
            raise ValueError("SequenceLifter.lift runs the model's eval forward: call model.eval() first")
        xy, w, state = prepare_tracks(det, self.layout, self.div, self.conf_thr, self.max_gap, self.fill_conf, seq_ids)
        px = self._pixels(xy) if want_pixels else None
        if self.filter_2d is not None:
            xy = filter_tracks(xy, self.filter_2d, w, seq_ids)
        if self.transform_2d is not None:
            xy = self.transform_2d.apply_(xy)
        T = xy.shape[0]
        poses = torch.empty((T, 17, 3), dtype=torch.float32, device=xy.device)
        for r0 in range(0, T, self.chunk):
            rows = xy[r0:r0 + self.chunk]
            out = predict_flip_tta(self.model, rows) if self.flip_tta else self.model(rows)
            poses[r0:r0 + self.chunk].copy_(out.reshape(-1, 17, 3))
        if self.denorm is not None:
            self.denorm.invert_(poses)
        if self.filter_3d is not None:
            poses = filter_tracks(poses, self.filter_3d, w, seq_ids)
        return poses, w, state, px

    @torch.no_grad()
    def locate(self, det, cams, cam_ids=None, seq_ids=None, iters=3, filter_t=None):
        """det (T, 17, 3) -> (poses (T, 17, 3), t (T, 3), rms (T,), w (T, 17), state (T, 17) uint8): lift(), then the root
        translation of every frame in its camera's frame (camera.fit_translation: cams a CameraTable, cam_ids (T,) int32 or
        None) fitted against the prepared 2-D track in pixels, xy * div, the joints weighted by the track's w (a lost joint
        does not take part), then -- filter_t, a TemporalFilter -- the trajectory filtered along time inside its sequence,
        frames whose fit is degenerate (rms NaN) weighing 0.  poses + t[:, None] are the camera-frame joints."""
        from .camera import fit_translation
        if filter_t is not None and not isinstance(filter_t, TemporalFilter):
            raise TypeError("filter_t must be a TemporalFilter or None")
        poses, w, state, px = self._lift(det, seq_ids, True)
        t, rms = fit_translation(poses, px, cams, cam_ids=cam_ids, weights=w, iters=iters)
        if filter_t is not None:
            ok = torch.isfinite(rms).to(torch.float32).reshape(-1, 1)
            t = filter_tracks(t.reshape(-1, 1, 3), filter_t, ok, seq_ids).reshape(-1, 3)
        return poses, t, rms, w, state
