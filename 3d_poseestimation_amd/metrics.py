"""Evaluation on the device: the usual Human3.6M table -- MPJPE (protocol 1), P-MPJPE (protocol 2: after a per-pose rigid
and scale alignment), N-MPJPE (after a per-pose scale), PCK / AUC, each per action -- without copying a prediction to
the host.

  pose_errors        (3, B, J) per-pose, per-joint errors: [0] MPJPE, [1] N-MPJPE, [2] P-MPJPE      pl_pose_errors
  procrustes_align   the aligned prediction (B, J, 3)                                               pl_pose_errors
  PoseMetrics        per-group sums, PCK counts and pose counts, accumulated on the device           pl_pose_metrics_accum
  summarise          the arithmetic of PoseMetrics.compute() on CPU tensors

The reference reports protocol 1 only (train_1.py:19-23,100-104: loss_MPJPE / epoch_mpjpe_mm here).  Definitions and
degenerate rules: include/poselift.h and DESIGN.md ("Evaluation metrics").  All arithmetic is in libposelift.so; tensors
that are computed on must live on the ROCm device.

denorm= (a pose_table.PoseTransform): prediction and target are in a model's standardised space and are taken back to the
raw units as the launch loads them (pl_pose_errors_t), so errors and the P-MPJPE alignment are those of the poses.

weights= (a (B, J) tensor, e.g. what SequenceLifter.lift / prepare_tracks return, or a dataset's annotation mask): joint j of
pose b is visible iff weights[b, j] > 0 (zero, negative and NaN: not visible).  The N-MPJPE scale and the P-MPJPE alignment
are fitted on the visible joints with these weights, every joint is then scored, and a visibility meter
(PoseMetrics(visibility=True)) reports masked means over the visible entries.  The sums over visible joints are selects, not
products -- a NaN-coded missing target touches only its own joint -- which differs on purpose from the criterion's
row_weights, where weights multiply.  Nothing validates weights on the host: nothing synchronises.
"""
import torch

from . import _lib
from .pose_table import transform_pair

METRICS = ("mpjpe", "n_mpjpe", "p_mpjpe")
AUC_THRESHOLDS = tuple(round(0.005 * i, 3) for i in range(31))          # 0 ... 0.150 m
MAX_GROUPS = MAX_THRESHOLDS = 32


def _pose_pair(pred, target):
    pred, target = pred.detach().float().contiguous(), target.detach().float().contiguous()
    pred, target = _lib.aligned16(pred), _lib.aligned16(target)     # (pose_errors_kernel loads both 16 bytes at a time)
    _lib.require_device_tensor(pred, "pred")
    _lib.require_device_tensor(target, "target")
    if target.dim() != 3 or target.shape[2] != 3 or pred.shape != target.shape:
        raise ValueError(f"expected two (B, J, 3) tensors, got {tuple(pred.shape)} and {tuple(target.shape)}")
    return pred, target


def _weights(weights, B, J):
    """(B, J) fp32, contiguous, on the device; only 4-byte alignment is asked of it."""
    weights = weights.detach().float().contiguous()
    _lib.require_device_tensor(weights, "weights")
    if tuple(weights.shape) != (B, J):
        raise ValueError(f"weights: expected ({B}, {J}), one weight per pose and joint, got {tuple(weights.shape)}")
    return weights


def _errors(pred, target, want_aligned, denorm=None, weights=None):
    pred, target = _pose_pair(pred, target)
    B, J, _ = target.shape
    if weights is not None:
        weights = _weights(weights, B, J)
    err = torch.empty((3, B, J), dtype=torch.float32, device=target.device)
    aligned = torch.empty_like(pred) if want_aligned else None
    with _lib.on_device(target.device):
        if weights is not None:
            sub, div, _keep = transform_pair(denorm, (J, 3), target.device, "denorm") if denorm is not None else (None, None, None)
            rc = _lib.lib().pl_pose_errors_w(pred.data_ptr(), target.data_ptr(), B, J, weights.data_ptr(), sub, div,
                                             err.data_ptr(), aligned.data_ptr() if want_aligned else None,
                                             _lib.current_stream_ptr())
        elif denorm is None:
            rc = _lib.lib().pl_pose_errors(pred.data_ptr(), target.data_ptr(), B, J, err.data_ptr(),
                                           aligned.data_ptr() if want_aligned else None, _lib.current_stream_ptr())
        else:
            sub, div, _keep = transform_pair(denorm, (J, 3), target.device, "denorm")
            rc = _lib.lib().pl_pose_errors_t(pred.data_ptr(), target.data_ptr(), B, J, sub, div, err.data_ptr(),
                                             aligned.data_ptr() if want_aligned else None, _lib.current_stream_ptr())
    _lib.check(rc, "pl_pose_errors")
    return err, aligned


def pose_errors(pred, target, denorm=None, weights=None):
    """(B, J, 3), (B, J, 3) -> (3, B, J): per pose and joint, [0] ||P - T||, [1] ||s P - T|| with the best scale s,
    [2] ||a R (P - muP) + muT - T|| with the best proper rotation R and scale a (3 <= J <= 32).
    denorm: the PoseTransform whose space both tensors are in; they are inverted as they are loaded.
    weights: (B, J); s, R, a and the centroids are fitted on the joints with weight > 0, weighted; every joint is scored."""
    return _errors(pred, target, False, denorm, weights)[0]


def procrustes_align(pred, target, denorm=None, weights=None):
    """The prediction after the P-MPJPE alignment, a R (P - muP) + muT, (B, J, 3); with denorm, in the raw units.
    weights: (B, J); the alignment is fitted on the joints with weight > 0 and carries the others along."""
    return _errors(pred, target, True, denorm, weights)[1]


def summarise(sums, counts, n_poses, thresholds, group_names=None, n_valid=None):
    """The arithmetic of PoseMetrics.compute() on CPU tensors: sums (G, 3, J), counts (G, 3, T, J), n_poses (G + 1,).
    A group (or a whole meter) without poses reports NaN, not a division error.
    n_valid (G, J): the state of a visibility meter, the visible entries per group and joint.  Every mean is then a masked
    one: per joint sums / n_valid[j] (NaN for a joint that was never visible), `{metric}_mm` the mean over all visible
    entries (sum_j sums / sum_j n_valid), PCK and AUC over sum_j n_valid; `n_joints` and `n_valid_per_joint` are added."""
    sums, counts, n_poses = sums.double().cpu(), counts.double().cpu(), n_poses.cpu()
    G, _, J = sums.shape
    T = counts.shape[2]
    if tuple(counts.shape) != (G, 3, T, J) or n_poses.numel() != G + 1 or len(thresholds) != T:
        raise ValueError("summarise: accumulator shapes disagree")
    if n_valid is not None:
        n_valid = n_valid.cpu()
        if tuple(n_valid.shape) != (G, J):
            raise ValueError("summarise: accumulator shapes disagree")
    names = list(group_names) if group_names is not None else [str(g) for g in range(G)]

    def table(s, c, n, nv=None):
        nan = float("nan")
        out = {"n_poses": int(n)}
        k = max(range(T), key=lambda t: thresholds[t]) if T else None
        if nv is None:
            per_joint = s / n if n > 0 else torch.full_like(s, nan)          # (3, J), metres
            pck_t = c.sum(dim=2) / (n * J) if n > 0 else torch.full((3, T), nan, dtype=torch.float64)      # (3, T)
            mean = [per_joint[m].mean() for m in range(3)]
        else:
            total = float(nv.sum())
            seen = nv > 0
            per_joint = torch.where(seen, s / nv.double().clamp(min=1), torch.full_like(s, nan))          # (3, J)
            pck_t = c.sum(dim=2) / total if total > 0 else torch.full((3, T), nan, dtype=torch.float64)
            mean = s.sum(dim=1) / total if total > 0 else torch.full((3,), nan, dtype=torch.float64)
            out["n_joints"] = int(total)
            out["n_valid_per_joint"] = [int(v) for v in nv.tolist()]
        for m, name in enumerate(METRICS):
            out[f"{name}_mm"] = float(mean[m] * 1000.0)
            out[f"{name}_per_joint_mm"] = (per_joint[m] * 1000.0).tolist()
            out[f"pck_{name}"] = float(pck_t[m, k]) if T else nan
            out[f"auc_{name}"] = float(pck_t[m].mean()) if T else nan
        return out

    n = n_poses[:G].double()
    out = table(sums.sum(dim=0), counts.sum(dim=0), float(n.sum()), n_valid.sum(dim=0) if n_valid is not None else None)
    out["pck_threshold_m"] = float(max(thresholds)) if T else float("nan")
    out["n_out_of_range"] = int(n_poses[G])
    if G > 1:
        out["groups"] = {names[g]: table(sums[g], counts[g], float(n[g]), n_valid[g] if n_valid is not None else None)
                         for g in range(G)}
    return out


class PoseMetrics:
    """Accumulates the evaluation table on the device.

        meter = pl.PoseMetrics(groups=15, group_names=ACTIONS)
        for y1, y2, action_id in loader:
            pl.eval_step(model, y1, y2, meter=meter, group_ids=action_id)      # or meter.update(y2_hat, y2, action_id)
        table = meter.compute()                                                # the one host read

    compute() reports, overall and per group, `mpjpe_mm`, `n_mpjpe_mm`, `p_mpjpe_mm` -- the mean over poses and ALL J
    joints, times 1000 -- their per-joint vectors, PCK at the largest threshold and AUC (the mean PCK over the threshold
    list) of each metric, and the pose counts.  This all-joint mean is the usual convention; `epoch_mpjpe_mm` is the
    reference's literal one (train_1.py:100-104: joints 1..16, times 17/16), so the two differ when joint 0 is not exact.

    State is three tensors: sums (G, 3, J) fp32, counts (G, 3, T, J) int64, n_poses (G + 1,) int64 (the last cell counts
    poses whose group id was outside [0, G): compute() raises when it is not 0).  A meter on device="cpu" can hold, load,
    all-reduce and summarise state; update() needs the GPU.

    visibility=True: a meter for data with missing joints.  update() then NEEDS weights= (B, J) -- joint j of pose b is
    visible iff its weight is > 0 -- and the table is a masked mean: only visible entries enter sums and counts, a fourth
    state tensor n_valid (G, J) int64 counts them, per-joint values divide by n_valid[j] (NaN for a joint never seen),
    `{metric}_mm` is the mean over all visible entries, PCK / AUC are fractions of them, and compute() adds `n_joints` and
    `n_valid_per_joint`.  The weights' magnitudes matter to the N-MPJPE scale and the P-MPJPE alignment only (fitted on
    the visible joints).  n_poses stays the pose count, fully invisible poses included.  A meter without visibility=True
    is unchanged and refuses weights=.

        poses, w, state = lifter.lift(det)                     # sequence.SequenceLifter: w (T, 17), 0 for a lost joint
        meter = pl.PoseMetrics(visibility=True)
        meter.update(poses, gt, weights=w)"""

    def __init__(self, joints=17, groups=1, group_names=None, pck_thresholds_m=AUC_THRESHOLDS, device="cuda",
                 visibility=False):
        thr = [float(t) for t in pck_thresholds_m]
        if not 3 <= joints <= 32 or not 1 <= groups <= MAX_GROUPS or len(thr) > MAX_THRESHOLDS:
            raise ValueError(f"PoseMetrics: joints in 3..32, groups in 1..{MAX_GROUPS}, at most {MAX_THRESHOLDS} thresholds")
        if group_names is not None and len(group_names) != groups:
            raise ValueError(f"PoseMetrics: {len(group_names)} group names for {groups} groups")
        self.joints, self.groups, self.thresholds = joints, groups, thr
        self.group_names = list(group_names) if group_names is not None else None
        self.device = torch.device(device)
        self._thr = torch.tensor(thr, dtype=torch.float32, device=self.device)
        self.sums = torch.zeros((groups, 3, joints), dtype=torch.float32, device=self.device)
        self.counts = torch.zeros((groups, 3, len(thr), joints), dtype=torch.int64, device=self.device)
        self.n_poses = torch.zeros(groups + 1, dtype=torch.int64, device=self.device)
        self.visibility = bool(visibility)
        self.n_valid = torch.zeros((groups, joints), dtype=torch.int64, device=self.device) if self.visibility else None

    def reset(self):
        for t in self.state().values():
            t.zero_()

    def update(self, pred, target, group_ids=None, denorm=None, weights=None):
        """Adds B poses: two library calls, three launches, no synchronisation.  group_ids: (B,) integer tensor on the
        device (None: group 0).  denorm: as in pose_errors (no further launch).  weights: (B, J), for a visibility meter
        only, which needs them (see the class docstring); still three launches."""
        if weights is not None and not self.visibility:
            raise ValueError("PoseMetrics.update: weights= needs a meter built with visibility=True (its state carries n_valid)")
        if weights is None and self.visibility:
            raise ValueError("PoseMetrics.update: a visibility meter needs weights= (B, J); torch.ones scores every joint")
        err = pose_errors(pred, target, denorm, weights)
        _, B, J = err.shape
        if J != self.joints:
            raise ValueError(f"PoseMetrics was built for {self.joints} joints, got {J}")
        if err.device != self.sums.device:
            raise _lib.PoseliftError(f"PoseMetrics lives on {self.sums.device}, the poses on {err.device}")
        if group_ids is not None:
            if group_ids.numel() != B:
                raise ValueError(f"group_ids has {group_ids.numel()} entries for {B} poses")
            group_ids = group_ids.reshape(B).to(torch.int32).contiguous()
            _lib.require_device_tensor(group_ids, "group_ids", torch.int32)
        T, L = len(self.thresholds), _lib.lib()
        if weights is not None:
            weights = _weights(weights, B, J)
            scratch = torch.empty(L.pl_pose_metrics_w_scratch_bytes(B, J, self.groups, T), dtype=torch.uint8, device=err.device)
            with _lib.on_device(err.device):
                rc = L.pl_pose_metrics_accum_w(err.data_ptr(), weights.data_ptr(), B, J,
                                               group_ids.data_ptr() if group_ids is not None else None, self.groups,
                                               self._thr.data_ptr() if T else None, T, self.sums.data_ptr(),
                                               self.counts.data_ptr() if T else None, self.n_poses.data_ptr(),
                                               self.n_valid.data_ptr(), scratch.data_ptr(), _lib.current_stream_ptr())
            _lib.check(rc, "pl_pose_metrics_accum_w")
            return
        scratch = torch.empty(L.pl_pose_metrics_scratch_bytes(B, J, self.groups, T), dtype=torch.uint8, device=err.device)
        with _lib.on_device(err.device):
            rc = L.pl_pose_metrics_accum(err.data_ptr(), B, J, group_ids.data_ptr() if group_ids is not None else None,
                                         self.groups, self._thr.data_ptr() if T else None, T, self.sums.data_ptr(),
                                         self.counts.data_ptr() if T else None, self.n_poses.data_ptr(),
                                         scratch.data_ptr(), _lib.current_stream_ptr())
        _lib.check(rc, "pl_pose_metrics_accum")

    def state(self):
        st = {"sums": self.sums, "counts": self.counts, "n_poses": self.n_poses}
        if self.visibility:
            st["n_valid"] = self.n_valid
        return st

    def load_state(self, state):
        for name, dst in self.state().items():
            src = state[name]
            if tuple(src.shape) != tuple(dst.shape):
                raise ValueError(f"PoseMetrics.load_state: {name} has shape {tuple(src.shape)}, expected {tuple(dst.shape)}")
            dst.copy_(src)

    def all_reduce(self, group=None):
        """Sums the accumulators (three; four of a visibility meter) over the process group (each rank evaluated its own
        shard)."""
        import torch.distributed as dist
        for t in self.state().values():
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)

    def compute(self):
        """The table as a dict (see the class docstring); one host read."""
        ns, nc = self.sums.numel(), self.counts.numel()
        parts = [self.sums.double().reshape(-1), self.counts.double().reshape(-1), self.n_poses.double().reshape(-1)]
        if self.visibility:
            parts.append(self.n_valid.double().reshape(-1))
        flat = torch.cat(parts).cpu()
        n_poses = flat[ns + nc:ns + nc + self.groups + 1].round().long()
        if int(n_poses[self.groups]) > 0:
            raise _lib.PoseliftError(f"PoseMetrics: {int(n_poses[self.groups])} poses had a group id outside "
                                     f"[0, {self.groups}); they are in no total")
        n_valid = flat[ns + nc + self.groups + 1:].round().long().reshape(self.n_valid.shape) if self.visibility else None
        return summarise(flat[:ns].reshape(self.sums.shape), flat[ns:ns + nc].reshape(self.counts.shape), n_poses,
                         self.thresholds, self.group_names, n_valid)
