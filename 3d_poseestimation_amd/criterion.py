"""The criterion of the lifter's train step (include/poselift.h PLCriterion).

  mse, l1      nn.MSELoss / nn.L1Loss(reduction="mean"): the two the reference toggles between
               (phase1_lifting/train_1.py:36-37, main.py:404-405, two2three.py:416-417; phase5_loop/losses.py:21;
               train_project.py:39 trains the 3-D -> 2-D projector with L1)
  smooth_l1    nn.SmoothL1Loss(beta)                                             PARITY UNPINNED (the reference has none)
  mpjpe        torch.norm(pred - target, dim=-1).mean() over (B, J, coords)      PARITY UNPINNED
each optionally weighted per joint (a zero weight on the zero-centred root joint takes the dead target out, instead of the
reference's 17/16 factors).  All arithmetic is in libposelift.so.
"""
import ctypes

import torch

from . import _lib

KINDS = {"mse": _lib.CRIT_MSE, "l1": _lib.CRIT_L1, "smooth_l1": _lib.CRIT_SMOOTH_L1, "mpjpe": _lib.CRIT_MPJPE}
MAX_MPJPE_COORDS = 4


class _PoseLossFn(torch.autograd.Function):
    """value and gradient in the same launch pair (pl_pose_loss_fwd_bwd), like train._MSEFn"""

    @staticmethod
    def forward(ctx, pred, tgt, crit):
        _lib.require_device_tensor(pred, "pred")
        _lib.require_device_tensor(tgt, "target")
        B = pred.shape[0]
        O = pred.numel() // B
        need = pred.requires_grad
        dpred = torch.empty_like(pred) if need else None
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        L = _lib.lib()
        with _lib.on_device(pred.device):
            st = crit.struct(O, pred.device)
            scratch = torch.empty(L.pl_pose_loss_scratch_bytes(B, O, ctypes.byref(st)), dtype=torch.uint8, device=pred.device)
            rc = L.pl_pose_loss_fwd_bwd(pred.data_ptr(), tgt.data_ptr(), B, O, ctypes.byref(st), 1.0,
                                        dpred.data_ptr() if need else None, loss.data_ptr(), scratch.data_ptr(),
                                        _lib.current_stream_ptr())
        _lib.check(rc, "pl_pose_loss_fwd_bwd")
        ctx.dpred = dpred
        return loss

    @staticmethod
    def backward(ctx, g):
        d = ctx.dpred
        ctx.dpred = None
        return (d.mul_(g) if d is not None else None), None, None


class PoseCriterion(torch.nn.Module):
    """crit = PoseCriterion(kind="mse", beta=1.0, joint_weights=None, coords=3); loss = crit(pred, target).

    kind           "mse" | "l1" | "smooth_l1" | "mpjpe"
    beta           smooth_l1's threshold, > 0 (beta = 0 is "l1"; Huber(delta) = delta * smooth_l1(beta=delta))
    joint_weights  J floats or None (all ones); a registered buffer: it follows .to() / .cuda(), and in-place edits are
                   seen by the next call -- and by the next replay of a GraphedTrainStep that captured this criterion
    coords         coordinates per joint: 3 for the lifter, 2 for the projector, 1 = no grouping

    pred, target: (B, J * coords) or (B, J, coords) fp32 on the device.  The mean is over B * J * coords elements, for
    "mpjpe" over B * J joints; the weights need not sum to anything.  Pass it as train_step(..., criterion=crit),
    GraphedTrainStep(..., criterion=crit), eval_step(..., criterion=crit) or as a GraphedModuleStep's loss_fn."""

    def __init__(self, kind="mse", beta=1.0, joint_weights=None, coords=3):
        super().__init__()
        if kind not in KINDS:
            raise ValueError(f"PoseCriterion: kind {kind!r} is not one of {sorted(KINDS)}")
        if int(coords) != coords or coords < 1:
            raise ValueError(f"PoseCriterion: coords = {coords!r}")
        if kind == "mpjpe" and coords > MAX_MPJPE_COORDS:
            raise ValueError(f"PoseCriterion: mpjpe takes joints of at most {MAX_MPJPE_COORDS} coordinates")
        beta = float(beta)
        if kind == "smooth_l1" and not (0.0 < beta < float("inf")):
            raise ValueError("PoseCriterion: smooth_l1 needs a finite beta > 0 (beta = 0 is kind='l1')")
        self.kind, self.beta, self.coords = kind, beta, int(coords)
        if joint_weights is not None:
            joint_weights = torch.as_tensor(joint_weights, dtype=torch.float32).detach().clone().contiguous()
            if joint_weights.dim() != 1 or joint_weights.numel() < 1:
                raise ValueError("PoseCriterion: joint_weights is a vector of J floats")
        self.register_buffer("joint_weights", joint_weights)

    def extra_repr(self):
        w = "None" if self.joint_weights is None else f"[{self.joint_weights.numel()}]"
        return f"kind={self.kind!r}, beta={self.beta}, joint_weights={w}, coords={self.coords}"

    def check_outputs(self, O):
        """ValueError unless O outputs are whole joints and the weights count them."""
        if O < 1 or O % self.coords != 0:
            raise ValueError(f"PoseCriterion: {O} outputs are not whole joints of {self.coords} coordinates")
        if self.joint_weights is not None and self.joint_weights.numel() != O // self.coords:
            raise ValueError(f"PoseCriterion: {self.joint_weights.numel()} joint weights for {O // self.coords} joints")

    def struct(self, O, device):
        """The _lib.PLCriterion of a call on [B][O] tensors of `device` (it points into joint_weights: keep self alive)."""
        self.check_outputs(O)
        w = self.joint_weights
        if w is not None:
            if w.device != device or w.dtype != torch.float32 or not w.is_contiguous():
                raise _lib.PoseliftError(f"PoseCriterion: joint_weights on {w.device} ({w.dtype}), the tensors on {device}: "
                                         "move the criterion with .to(device)")
        return _lib.PLCriterion(KINDS[self.kind], self.coords, self.beta, w.data_ptr() if w is not None else None)

    def forward(self, pred, target):
        if pred.shape != target.shape:
            raise ValueError(f"PoseCriterion: shapes differ: {tuple(pred.shape)} vs {tuple(target.shape)}")
        if pred.dim() == 3 and pred.shape[2] != self.coords:
            raise ValueError(f"PoseCriterion: (B, J, {pred.shape[2]}) tensors, coords = {self.coords}")
        if pred.dim() not in (2, 3) or pred.shape[0] < 1:
            raise ValueError("PoseCriterion expects (B, J * coords) or (B, J, coords) tensors, B >= 1")
        self.check_outputs(pred.numel() // pred.shape[0])
        return _PoseLossFn.apply(pred.contiguous(), target.contiguous(), self)
