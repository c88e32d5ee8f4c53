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
BONE_RHOS = {"l1": _lib.RHO_L1, "mse": _lib.RHO_MSE}
# the skeleton's registered buffers, None without one: they follow .to(); term_weights = {bone_weight, symmetry_weight}
SKELETON_BUFFERS = ("bone_child", "bone_parent", "pair_a", "pair_b", "term_weights", "denorm_sub", "denorm_div")


class Skeleton:
    """Skeleton(parents, left=None, right=None): which joints a bone connects, and which bones are each other's mirror image.

    parents[j]   the parent joint of joint j, -1 for the root: exactly one root, every index in range, no cycle.  The bones
                 are the non-root joints in joint order: bone k = (child, parent) = (bones[k], parents[bones[k]])
    left, right  child joints whose bones pair up, left[i] with right[i]: equal length, no repeats, never the root
    At most 32 joints and 16 pairs (include/poselift.h PLSkeleton).  Immutable; the device tables are PoseCriterion's."""

    def __init__(self, parents, left=None, right=None):
        parents = [int(p) for p in parents]
        J = len(parents)
        if not 2 <= J <= _lib.SKELETON_MAX_JOINTS:
            raise ValueError(f"Skeleton: {J} joints (2 .. {_lib.SKELETON_MAX_JOINTS})")
        roots = [j for j, p in enumerate(parents) if p == -1]
        if len(roots) != 1:
            raise ValueError(f"Skeleton: exactly one joint has parent -1 (the root), got {len(roots)}")
        for j, p in enumerate(parents):
            if p != -1 and not 0 <= p < J:
                raise ValueError(f"Skeleton: parent {p} of joint {j} is outside 0 .. {J - 1}")
        for j in range(J):
            a, steps = j, 0
            while parents[a] != -1:
                a, steps = parents[a], steps + 1
                if steps > J:
                    raise ValueError(f"Skeleton: joint {j} never reaches the root (a cycle)")
        self.parents, self.root = tuple(parents), roots[0]
        self.bones = tuple(j for j in range(J) if j != self.root)
        self.bone_parents = tuple(parents[j] for j in self.bones)
        left, right = tuple(int(j) for j in (left or ())), tuple(int(j) for j in (right or ()))
        if len(left) != len(right):
            raise ValueError(f"Skeleton: {len(left)} left joints for {len(right)} right joints")
        if len(left) > _lib.SKELETON_MAX_PAIRS:
            raise ValueError(f"Skeleton: {len(left)} pairs (at most {_lib.SKELETON_MAX_PAIRS})")
        for j in left + right:
            if not 0 <= j < J:
                raise ValueError(f"Skeleton: paired joint {j} is outside 0 .. {J - 1}")
            if j == self.root:
                raise ValueError(f"Skeleton: the root (joint {j}) has no bone to pair")
        if len(set(left + right)) != len(left + right):
            raise ValueError("Skeleton: a joint is named twice in left / right")
        self.left, self.right = left, right
        bone_of = {j: k for k, j in enumerate(self.bones)}
        self.pairs = tuple((bone_of[a], bone_of[b]) for a, b in zip(left, right))

    @property
    def joints(self):
        return len(self.parents)

    def __repr__(self):
        return f"Skeleton(parents={self.parents}, left={self.left}, right={self.right})"

    def tables(self, device):
        """(bone_child, bone_parent, pair_a or None, pair_b or None): int32 tensors on `device`"""
        def i32(v):
            return torch.tensor(v, dtype=torch.int32, device=device)
        pa, pb = ([p[0] for p in self.pairs], [p[1] for p in self.pairs]) if self.pairs else (None, None)
        return i32(self.bones), i32(self.bone_parents), i32(pa) if pa else None, i32(pb) if pb else None


# Human3.6M's 17 joints in the order of pose_table.H36M_17_OF_32; left / right are flip_pose's lists
H36M_SKELETON = Skeleton((-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15), left=(4, 5, 6, 11, 12, 13),
                         right=(1, 2, 3, 14, 15, 16))


def _denorm_pair(denorm, J, coords, what):
    """(sub, div) of an optional PoseTransform as flat fp32 host tensors, (None, None) without one"""
    from .pose_table import PoseTransform
    if denorm is None:
        return None, None
    if not isinstance(denorm, PoseTransform):
        raise TypeError(f"{what}: denorm must be a PoseTransform or None")
    if denorm.shape != (J, coords):
        raise ValueError(f"{what}: denorm has shape {denorm.shape}, the poses ({J}, {coords})")
    return denorm.sub.reshape(-1).clone(), denorm.div.reshape(-1).clone()


def bone_lengths(poses, skeleton, denorm=None):
    """(B, K) bone lengths of (B, J, 2|3) device poses, bone k as in skeleton.bones; with denorm (a PoseTransform of shape
    (J, coords)) the poses are first taken to raw units, x div + sub.  One launch (pl_bone_lengths)."""
    if not isinstance(skeleton, Skeleton):
        raise TypeError("bone_lengths: skeleton must be a Skeleton")
    _lib.require_device_tensor(poses, "poses")
    if poses.dim() != 3 or poses.shape[0] < 1 or poses.shape[1] != skeleton.joints or poses.shape[2] not in (2, 3):
        raise ValueError(f"bone_lengths expects (B, {skeleton.joints}, 2|3) poses, B >= 1, got {tuple(poses.shape)}")
    B, J, G = poses.shape
    sub, div = _denorm_pair(denorm, J, G, "bone_lengths")
    child, parent, _, _ = skeleton.tables(poses.device)
    if sub is not None:
        sub, div = sub.to(poses.device), div.to(poses.device)
    st = _lib.PLSkeleton(J, len(skeleton.bones), 0, 0, child.data_ptr(), parent.data_ptr(), None, None, None,
                         sub.data_ptr() if sub is not None else None, div.data_ptr() if div is not None else None)
    out = torch.empty((B, len(skeleton.bones)), dtype=torch.float32, device=poses.device)
    with _lib.on_device(poses.device):
        rc = _lib.lib().pl_bone_lengths(poses.data_ptr(), B, G, ctypes.byref(st), out.data_ptr(), _lib.current_stream_ptr())
    _lib.check(rc, "pl_bone_lengths")
    return out


def normalize_row_weights(row_weights):
    """rw * (B J / sum rw), zeros where sum rw == 0: with these weights the criterion's fixed 1 / (B O) (mpjpe: 1 / (B J))
    normaliser gives the masked / weighted MEAN -- the loss divided by the total weight instead of the element count.
    Plain torch ops on the tensor's device; nothing synchronises.  (Under data parallelism each rank normalises by its own
    rows' sum.)"""
    rw = row_weights.float()
    total = rw.sum()
    scale = torch.where(total == 0, torch.zeros_like(total), rw.numel() / total)
    return rw * scale


def check_row_weights(row_weights, B, J, device, who="PoseCriterion"):
    """The (B, J) fp32 contiguous device tensor the library reads, from what a caller passed: ValueError on a wrong shape or
    requires_grad (there is no gradient with respect to the weights); a non-fp32 tensor (a bool mask) is converted with
    .float() and a non-contiguous one with .contiguous() -- either is a copy, so later in-place edits of the caller's tensor
    are not seen."""
    if not torch.is_tensor(row_weights):
        raise TypeError(f"{who}: row_weights must be a tensor")
    if row_weights.requires_grad:
        raise ValueError(f"{who}: row_weights requires grad, and the criterion has no gradient with respect to its weights")
    if tuple(row_weights.shape) != (B, J):
        raise ValueError(f"{who}: row_weights has shape {tuple(row_weights.shape)}, the batch ({B}, {J}) = (poses, joints)")
    if row_weights.device != device:
        raise ValueError(f"{who}: row_weights on {row_weights.device}, the tensors on {device}")
    return row_weights.float().contiguous()


class _PoseLossFn(torch.autograd.Function):
    """value and gradient in the same launch pair (pl_pose_loss_fwd_bwd), like train._MSEFn"""

    @staticmethod
    def forward(ctx, pred, tgt, crit, rw=None):
        _lib.require_device_tensor(pred, "pred")
        _lib.require_device_tensor(tgt, "target")
        B = pred.shape[0]
        O = pred.numel() // B
        need = pred.requires_grad
        dpred = torch.empty_like(pred) if need else None
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        L = _lib.lib()
        with _lib.on_device(pred.device):
            st = crit.struct(O, pred.device, rw)
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
        return (d.mul_(g) if d is not None else None), None, None, None


class PoseCriterion(torch.nn.Module):
    """crit = PoseCriterion(kind="mse", beta=1.0, joint_weights=None, coords=3, skeleton=None, bone_weight=0.0,
    symmetry_weight=0.0, bone_rho="l1", denorm=None); loss = crit(pred, target, row_weights=None).

    kind           "mse" | "l1" | "smooth_l1" | "mpjpe"
    beta           smooth_l1's threshold, > 0 (beta = 0 is "l1"; Huber(delta) = delta * smooth_l1(beta=delta))
    joint_weights  J floats or None (all ones); a registered buffer: it follows .to() / .cuda(), and in-place edits are
                   seen by the next call -- and by the next replay of a GraphedTrainStep that captured this criterion
    coords         coordinates per joint: 3 for the lifter, 2 for the projector, 1 = no grouping
    skeleton       a Skeleton (H36M_SKELETON), or None: adds  bone_weight * L_bone + symmetry_weight * L_sym  to the loss,
                   L_bone = mean rho(predicted - target bone length), L_sym = mean rho(predicted left - right bone length)
                   (include/poselift.h PLSkeleton; PARITY UNPINNED), in one launch more; coords 2 or 3
    bone_weight, symmetry_weight   the two lambdas, kept in the registered buffer term_weights (two floats, read by the
                   kernel from device memory: in-place edits are seen by the next call and the next replay)
    bone_rho       "l1" (|e|) or "mse" (e^2)
    denorm         a PoseTransform of shape (J, coords): the bone terms measure lengths in raw units, x div + sub; the base
                   loss stays in the model's space

    pred, target: (B, J * coords) or (B, J, coords) fp32 on the device.  The mean is over B * J * coords elements, for
    "mpjpe" over B * J joints; the weights need not sum to anything.  Pass it as train_step(..., criterion=crit),
    GraphedTrainStep(..., criterion=crit), eval_step(..., criterion=crit) or as a GraphedModuleStep's loss_fn.

    row_weights    (B, J) on the tensors' device, or None: the weight of joint j of POSE b -- a visibility mask, a detector's
                   or a pseudo-label's confidence, a per-row weight broadcast over the joints, zeros on padding rows.  The
                   effective weight is row_weights[b, j], times joint_weights[j] when there are both (one fp32 product);
                   it stands where the joint weight stands, on every route of the fused step, in the same launches.  The
                   normaliser stays 1 / (B * J * coords) (mpjpe: 1 / (B * J)): normalize_row_weights(rw) rescales the
                   weights so that the loss is the weighted mean.  Not differentiable (requires_grad raises ValueError).
                   fp32 contiguous tensors are read in place; any other dtype (a bool mask) is converted with .float(),
                   which is a copy.  Not with a skeleton (ValueError): the bone terms have no per-pose weights yet.
                   Weights MULTIPLY, as joint_weights do and as torch's (w * elementwise).mean() does: 0 * NaN = NaN, so a
                   zero weight does not hide a non-finite prediction or target.  Targets that code "missing" as NaN need
                   target = torch.nan_to_num(target) next to the mask that zeroes those joints."""

    def __init__(self, kind="mse", beta=1.0, joint_weights=None, coords=3, skeleton=None, bone_weight=0.0, symmetry_weight=0.0,
                 bone_rho="l1", denorm=None):
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
        bone_weight, symmetry_weight = float(bone_weight), float(symmetry_weight)
        if bone_rho not in BONE_RHOS:
            raise ValueError(f"PoseCriterion: bone_rho {bone_rho!r} is not one of {sorted(BONE_RHOS)}")
        if skeleton is None:
            if bone_weight != 0.0 or symmetry_weight != 0.0:
                raise ValueError("PoseCriterion: bone_weight / symmetry_weight need a skeleton")
            if denorm is not None:
                raise ValueError("PoseCriterion: denorm is the skeleton terms' transform and needs a skeleton")
        else:
            if not isinstance(skeleton, Skeleton):
                raise TypeError("PoseCriterion: skeleton must be a Skeleton or None")
            if self.coords not in (2, 3):
                raise ValueError(f"PoseCriterion: a skeleton takes joints of 2 or 3 coordinates, coords = {self.coords}")
            if symmetry_weight != 0.0 and not skeleton.pairs:
                raise ValueError("PoseCriterion: symmetry_weight on a skeleton without left / right pairs")
        self.skeleton, self.bone_rho = skeleton, bone_rho
        tabs = skeleton.tables("cpu") if skeleton is not None else (None,) * 4
        sub, div = _denorm_pair(denorm, skeleton.joints, self.coords, "PoseCriterion") if skeleton is not None else (None, None)
        for name, t in zip(SKELETON_BUFFERS, tabs + (torch.tensor([bone_weight, symmetry_weight], dtype=torch.float32)
                                                     if skeleton is not None else None, sub, div)):
            self.register_buffer(name, t)

    def extra_repr(self):
        w = "None" if self.joint_weights is None else f"[{self.joint_weights.numel()}]"
        s = f"kind={self.kind!r}, beta={self.beta}, joint_weights={w}, coords={self.coords}"
        if self.skeleton is not None:
            s += (f", skeleton=[{self.skeleton.joints} joints, {len(self.skeleton.pairs)} pairs], bone_rho={self.bone_rho!r}, "
                  f"denorm={self.denorm_sub is not None}")
        return s

    def check_outputs(self, O):
        """ValueError unless O outputs are whole joints and the weights and the skeleton count them."""
        if O < 1 or O % self.coords != 0:
            raise ValueError(f"PoseCriterion: {O} outputs are not whole joints of {self.coords} coordinates")
        if self.joint_weights is not None and self.joint_weights.numel() != O // self.coords:
            raise ValueError(f"PoseCriterion: {self.joint_weights.numel()} joint weights for {O // self.coords} joints")
        if self.skeleton is not None and self.skeleton.joints != O // self.coords:
            raise ValueError(f"PoseCriterion: a skeleton of {self.skeleton.joints} joints for {O // self.coords} joints")

    def device_ptrs(self):
        """data_ptr() of every buffer a launch reads (0 where there is none): what a captured graph has baked in"""
        return tuple(t.data_ptr() if t is not None else 0
                     for t in [self.joint_weights] + [getattr(self, n) for n in SKELETON_BUFFERS])

    def _on(self, t, name, device, dtype):
        if t is not None and (t.device != device or t.dtype != dtype or not t.is_contiguous()):
            raise _lib.PoseliftError(f"PoseCriterion: {name} on {t.device} ({t.dtype}), the tensors on {device}: "
                                     "move the criterion with .to(device)")
        return t.data_ptr() if t is not None else None

    def struct(self, O, device, row_weights=None):
        """The _lib.PLCriterion of a call on [B][O] tensors of `device` (it points into the buffers: keep self alive); with a
        skeleton the _lib.PLSkeletonCriterion that extends it; with row_weights (what check_row_weights returned: keep it
        alive as well) the _lib.PLRowWeightsCriterion."""
        self.check_outputs(O)
        if row_weights is not None and self.skeleton is not None:
            raise ValueError("PoseCriterion: row_weights with a skeleton are not built (the bone terms have no per-pose weights)")
        w = self._on(self.joint_weights, "joint_weights", device, torch.float32)
        if row_weights is not None:
            if row_weights.dim() != 2 or row_weights.shape[1] != O // self.coords:
                raise ValueError(f"PoseCriterion: row_weights {tuple(row_weights.shape)} for {O // self.coords} joints")
            st = _lib.PLRowWeightsCriterion(KINDS[self.kind] | _lib.CRIT_HAS_ROW_WEIGHTS, self.coords, self.beta, w)
            st.row_weights = self._on(row_weights, "row_weights", device, torch.float32)
            return st
        if self.skeleton is None:
            return _lib.PLCriterion(KINDS[self.kind], self.coords, self.beta, w)
        if self.term_weights is None or self.term_weights.numel() != 2:
            raise _lib.PoseliftError("PoseCriterion: term_weights is {bone_weight, symmetry_weight}: two floats")
        ptr = {n: self._on(getattr(self, n), n, device, torch.float32 if n in ("term_weights", "denorm_sub", "denorm_div")
                           else torch.int32) for n in SKELETON_BUFFERS}
        sk = _lib.PLSkeleton(self.skeleton.joints, len(self.skeleton.bones), len(self.skeleton.pairs), BONE_RHOS[self.bone_rho],
                             ptr["bone_child"], ptr["bone_parent"], ptr["pair_a"], ptr["pair_b"], ptr["term_weights"],
                             ptr["denorm_sub"], ptr["denorm_div"])
        st = _lib.PLSkeletonCriterion(KINDS[self.kind] | _lib.CRIT_HAS_SKELETON, self.coords, self.beta, w)
        st.skeleton = ctypes.pointer(sk)          # (the struct keeps sk alive)
        return st

    def row_weights_for(self, row_weights, B, O, device):
        """check_row_weights against a (B, O) batch of this criterion (None stays None); ValueError with a skeleton"""
        if row_weights is None:
            return None
        if self.skeleton is not None:
            raise ValueError("PoseCriterion: row_weights with a skeleton are not built (the bone terms have no per-pose weights)")
        self.check_outputs(O)
        return check_row_weights(row_weights, B, O // self.coords, device)

    def forward(self, pred, target, row_weights=None):
        if pred.shape != target.shape:
            raise ValueError(f"PoseCriterion: shapes differ: {tuple(pred.shape)} vs {tuple(target.shape)}")
        if pred.dim() == 3 and pred.shape[2] != self.coords:
            raise ValueError(f"PoseCriterion: (B, J, {pred.shape[2]}) tensors, coords = {self.coords}")
        if pred.dim() not in (2, 3) or pred.shape[0] < 1:
            raise ValueError("PoseCriterion expects (B, J * coords) or (B, J, coords) tensors, B >= 1")
        self.check_outputs(pred.numel() // pred.shape[0])
        rw = self.row_weights_for(row_weights, pred.shape[0], pred.numel() // pred.shape[0], pred.device)
        return _PoseLossFn.apply(pred.contiguous(), target.contiguous(), self, rw)
