"""Cameras on the device: projection with distortion, reprojection error and loss, and the root translation that places a
root-relative pose in front of its camera (csrc/camera.h has the definitions).

  CameraTable           fp32 (C, 9) rows fx, fy, cx, cy, k1, k2, k3, p1, p2
  project_poses         (B, J, 3) -> (B, J, 2); autograd, the backward is a kernel        pl_camera_project / _bwd
  reprojection_errors   per-joint pixel distance to a 2-D target                           pl_camera_reproj_errors
  reprojection_loss     l1 / mse / l2 mean with its gradient; autograd                      pl_camera_reproj_loss_fwd_bwd
  fit_translation       per pose: linear initialisation + a fixed number of Gauss-Newton steps   pl_camera_fit_translation

The reference carries the Human3.6M intrinsics (phase3_direct/my_HybrIK/utils.py:131-172) but never projects with them
(PARITY UNPINNED).  Shared arguments: `cam_ids` (B,) int32 picks a pose's camera row (None: row 0; an id outside the table
makes the pose's values NaN: no row is read); `translation` (B, 3) is added to every joint of its pose; `denorm`, a PoseTransform of shape
(J, 3), takes X to raw units first (x div + sub) and gradients are chained through it.  Every function only enqueues work on
the current stream and reads nothing back.
"""
import numpy as np
import torch

from . import _lib
from .pose_table import PoseTransform, transform_pair

MAX_JOINTS, MAX_ITERS = 32, 8
KINDS = {"l1": 0, "mse": 1, "l2": 2}


def _host_array(v, cols, name, C=None):
    if isinstance(v, torch.Tensor):
        if v.requires_grad:
            raise ValueError(f"CameraTable: {name} requires grad, and nothing here has a gradient with respect to the cameras")
        v = v.detach().cpu().numpy()
    a = np.asarray(v, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != cols or a.shape[0] < 1 or (C is not None and a.shape[0] != C):
        raise ValueError(f"CameraTable: {name} is (C, {cols}), got {a.shape}")
    return a


class CameraTable:
    """cams = CameraTable(focal (C, 2), centre (C, 2), radial=None (C, 3), tangential=None (C, 2)): the intrinsics of C cameras
    as one fp32 (C, 9) table, fx, fy, cx, cy, k1, k2, k3, p1, p2 per row; missing distortion is zero.  .table is the host
    copy; .to(device) copies it there once (do it before a graph capture); .save(path) / CameraTable.load(path) keep it as
    an .npz."""

    def __init__(self, focal, centre, radial=None, tangential=None):
        focal = _host_array(focal, 2, "focal")
        C = focal.shape[0]
        centre = _host_array(centre, 2, "centre", C)
        radial = np.zeros((C, 3)) if radial is None else _host_array(radial, 3, "radial", C)
        tangential = np.zeros((C, 2)) if tangential is None else _host_array(tangential, 2, "tangential", C)
        table = np.concatenate([focal, centre, radial, tangential], axis=1).astype(np.float32)
        if not np.isfinite(table).all():
            raise ValueError("CameraTable: every value must be finite (in fp32)")
        self.table = torch.from_numpy(np.ascontiguousarray(table))
        self._dev = {}

    @classmethod
    def from_table(cls, table):
        """From (C, 9) rows fx, fy, cx, cy, k1, k2, k3, p1, p2."""
        t = _host_array(table, 9, "table")
        return cls(t[:, 0:2], t[:, 2:4], t[:, 4:7], t[:, 7:9])

    def __len__(self):
        return int(self.table.shape[0])

    def on(self, device):
        """The table on `device`, copied there once."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._dev.get(device)
        if t is None:
            t = self._dev[device] = self.table.to(device)
        return t

    def to(self, device):
        self.on(device)
        return self

    def save(self, path):
        np.savez(path, cameras=self.table.numpy())

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls.from_table(z["cameras"])


def _tensor(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a device tensor")
    return t


def _no_grad(t, name, who):
    if t.requires_grad:
        raise ValueError(f"{who}: {name} requires grad, and {who} has no gradient with respect to it")


def _scene(who, X, cams, cam_ids, translation, denorm, target=None, weights=None):
    """Checks in the order type, shape, device, then dtype / contiguity; returns (X, B, J, table, ids, t, sub, div, keep, target,
    weights) with every tensor contiguous."""
    _tensor(X, "X")
    if not isinstance(cams, CameraTable):
        raise TypeError(f"{who}: cams must be a CameraTable")
    if denorm is not None and not isinstance(denorm, PoseTransform):
        raise TypeError(f"{who}: denorm must be a PoseTransform or None")
    if X.dim() != 3 or X.shape[0] == 0 or X.shape[2] != 3 or not 1 <= X.shape[1] <= MAX_JOINTS:
        raise ValueError(f"{who}: X is (B, J, 3), J <= {MAX_JOINTS}, got {tuple(X.shape)}")
    B, J = X.shape[0], X.shape[1]
    dev = X.device
    others = []
    if cam_ids is not None:
        _tensor(cam_ids, "cam_ids")
        if tuple(cam_ids.shape) != (B,):
            raise ValueError(f"{who}: cam_ids holds one int32 id per pose, got {tuple(cam_ids.shape)}")
        others.append(("cam_ids", cam_ids, torch.int32))
    if translation is not None:
        _tensor(translation, "translation")
        if tuple(translation.shape) != (B, 3):
            raise ValueError(f"{who}: translation is (B, 3) = {(B, 3)}, got {tuple(translation.shape)}")
        others.append(("translation", translation, torch.float32))
    if target is not None:
        _tensor(target, "target")
        _no_grad(target, "the 2-D target", who)
        if tuple(target.shape) != (B, J, 2):
            raise ValueError(f"{who}: the 2-D target is (B, J, 2) = {(B, J, 2)}, got {tuple(target.shape)}")
        others.append(("target", target, torch.float32))
    if weights is not None:
        _tensor(weights, "weights")
        _no_grad(weights, "weights", who)
        if tuple(weights.shape) != (B, J):
            raise ValueError(f"{who}: weights is (B, J) = {(B, J)}, got {tuple(weights.shape)}")
        others.append(("weights", weights, torch.float32))
    for name, t, _ in others:
        if t.device != dev:
            raise ValueError(f"{who}: {name} on {t.device}, X on {dev}")
    out = {}
    for name, t, dtype in [("X", X, torch.float32)] + others:
        t = (t.float() if name == "weights" else t).contiguous()        # (a bool mask is converted, as check_row_weights does)
        _lib.require_device_tensor(t, name, dtype)
        out[name] = t
    sub, div, keep = transform_pair(denorm, (J, 3), dev, "denorm")
    return (out["X"], B, J, cams.on(dev), out.get("cam_ids"), out.get("translation"), sub, div, keep, out.get("target"),
            out.get("weights"))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _div(div, who):
    w, h = float(div[0]), float(div[1])
    if not (w > 0 and h > 0 and np.isfinite(w) and np.isfinite(h)):
        raise ValueError(f"{who}: div = (width, height) must be positive and finite, got {div!r}")
    return w, h


class _ProjectFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, t, table, ids, sub, div, keep):
        B, J = X.shape[0], X.shape[1]
        uv = torch.empty((B, J, 2), dtype=torch.float32, device=X.device)
        with _lib.on_device(X.device):
            rc = _lib.lib().pl_camera_project(X.data_ptr(), B, J, table.data_ptr(), table.shape[0], _ptr(ids), _ptr(t), sub, div,
                                              uv.data_ptr(), _lib.current_stream_ptr())
        _lib.check(rc, "pl_camera_project")
        ctx.save_for_backward(X, t if t is not None else X)
        ctx.has_t, ctx.args = t is not None, (table, ids, sub, div, keep)
        return uv

    @staticmethod
    def backward(ctx, g):
        X, t = ctx.saved_tensors
        t = t if ctx.has_t else None
        table, ids, sub, div, _keep = ctx.args
        B, J = X.shape[0], X.shape[1]
        g = g.contiguous()
        dX = torch.empty_like(X)
        dT = torch.empty((B, 3), dtype=torch.float32, device=X.device) if t is not None and ctx.needs_input_grad[1] else None
        with _lib.on_device(X.device):
            rc = _lib.lib().pl_camera_project_bwd(X.data_ptr(), g.data_ptr(), B, J, table.data_ptr(), table.shape[0], _ptr(ids),
                                                  _ptr(t), sub, div, dX.data_ptr(), _ptr(dT), _lib.current_stream_ptr())
        _lib.check(rc, "pl_camera_project_bwd")
        return dX, dT, None, None, None, None, None


def project_poses(X, cams, cam_ids=None, translation=None, denorm=None):
    """X (B, J, 3), J <= 32 -> uv (B, J, 2) in pixels: x = X/Z, y = Y/Z, the radial and tangential distortion of the camera
    row, then focal length and centre (csrc/camera.h; no clamp and no special case for Z <= 0).  Differentiable in X and
    translation: the backward is one launch of the analytic Jacobian."""
    X, B, J, table, ids, t, sub, div, keep, _, _ = _scene("project_poses", X, cams, cam_ids, translation, denorm)
    return _ProjectFn.apply(X, t, table, ids, sub, div, keep)


def reprojection_errors(X, uv, cams, cam_ids=None, translation=None, denorm=None, div=(1.0, 1.0)):
    """err (B, J): the distance between the projection of X and the 2-D target uv (B, J, 2), each residual divided by
    div = (width, height) -- (1, 1) for pixels, the convention of prepare_tracks.  One launch, no gradient."""
    w, h = _div(div, "reprojection_errors")
    X, B, J, table, ids, t, sub, dv, _keep, uv, _ = _scene("reprojection_errors", X, cams, cam_ids, translation, denorm, target=uv)
    err = torch.empty((B, J), dtype=torch.float32, device=X.device)
    with _lib.on_device(X.device):
        rc = _lib.lib().pl_camera_reproj_errors(X.data_ptr(), uv.data_ptr(), B, J, table.data_ptr(), table.shape[0], _ptr(ids),
                                                _ptr(t), sub, dv, w, h, err.data_ptr(), _lib.current_stream_ptr())
    _lib.check(rc, "pl_camera_reproj_errors")
    return err


class _ReprojLossFn(torch.autograd.Function):
    """value and gradient in the same launch pair (pl_camera_reproj_loss_fwd_bwd), like criterion._PoseLossFn"""

    @staticmethod
    def forward(ctx, X, t, uv, table, ids, sub, div, keep, weights, kind, dw, dh):
        B, J = X.shape[0], X.shape[1]
        need_t = t is not None and t.requires_grad
        need = X.requires_grad or need_t
        dX = torch.empty_like(X) if need else None
        dT = torch.empty((B, 3), dtype=torch.float32, device=X.device) if need_t else None
        loss = torch.empty((), dtype=torch.float32, device=X.device)
        L = _lib.lib()
        with _lib.on_device(X.device):
            scratch = torch.empty(L.pl_camera_reproj_loss_scratch_bytes(B, J), dtype=torch.uint8, device=X.device)
            rc = L.pl_camera_reproj_loss_fwd_bwd(X.data_ptr(), uv.data_ptr(), B, J, table.data_ptr(), table.shape[0], _ptr(ids),
                                                 _ptr(t), sub, div, _ptr(weights), kind, dw, dh, 1.0, _ptr(dX), _ptr(dT),
                                                 loss.data_ptr(), scratch.data_ptr(), _lib.current_stream_ptr())
        _lib.check(rc, "pl_camera_reproj_loss_fwd_bwd")
        ctx.grads = (dX, dT)
        return loss

    @staticmethod
    def backward(ctx, g):
        dX, dT = ctx.grads
        ctx.grads = None
        return ((dX.mul_(g) if dX is not None and ctx.needs_input_grad[0] else None), (dT.mul_(g) if dT is not None else None),
                None, None, None, None, None, None, None, None, None, None)


def reprojection_loss(X, uv, cams, cam_ids=None, translation=None, weights=None, kind="l1", denorm=None, div=(1.0, 1.0)):
    """The mean reprojection residual of X (B, J, 3) against the 2-D target uv (B, J, 2), a scalar with gradients for X and
    translation (none for the target, the weights or the cameras: requires_grad on those raises ValueError).
    kind "l1": mean of |du| + |dv| over B J 2 elements; "mse": of du^2 + dv^2 over B J 2; "l2": of the pixel distance over
    B J; (du, dv) = (projection - uv) / div.  weights (B, J) multiply a joint's value (a zero weight does not hide a NaN, as
    in PoseCriterion); the normaliser stays the element count.  Two launches; the sums have a fixed order."""
    if kind not in KINDS:
        raise ValueError(f"reprojection_loss: kind {kind!r} is not one of {sorted(KINDS)}")
    w, h = _div(div, "reprojection_loss")
    X, B, J, table, ids, t, sub, dv, keep, uv, weights = _scene("reprojection_loss", X, cams, cam_ids, translation, denorm,
                                                                target=uv, weights=weights)
    return _ReprojLossFn.apply(X, t, uv, table, ids, sub, dv, keep, weights, KINDS[kind], w, h)


def fit_translation(X_rel, uv, cams, cam_ids=None, weights=None, denorm=None, iters=3):
    """(t (B, 3), rms (B,)): per pose the translation that places the root-relative X_rel (B, J, 3) in front of its camera so
    that it reprojects onto uv (B, J, 2), in pixels.  A joint takes part iff its weight is > 0 (weights (B, J) select here,
    as in the metrics).  A linear initialisation without distortion, then `iters` (0..8) Gauss-Newton steps on the distorted
    model: a fixed count.  rms is the weighted RMS reprojection error after the last step.  A pose with fewer than two
    joints taking part, or whose 3 x 3 system is singular, gets t = rms = NaN.  One launch."""
    if int(iters) != iters or not 0 <= iters <= MAX_ITERS:
        raise ValueError(f"fit_translation: iters is 0..{MAX_ITERS}, got {iters!r}")
    X, B, J, table, ids, _, sub, dv, _keep, uv, weights = _scene("fit_translation", X_rel, cams, cam_ids, None, denorm, target=uv,
                                                                 weights=weights)
    t = torch.empty((B, 3), dtype=torch.float32, device=X.device)
    rms = torch.empty((B,), dtype=torch.float32, device=X.device)
    with _lib.on_device(X.device):
        rc = _lib.lib().pl_camera_fit_translation(X.data_ptr(), uv.data_ptr(), B, J, table.data_ptr(), table.shape[0], _ptr(ids),
                                                  _ptr(weights), sub, dv, int(iters), t.data_ptr(), rms.data_ptr(),
                                                  _lib.current_stream_ptr())
    _lib.check(rc, "pl_camera_fit_translation")
    return t, rms
