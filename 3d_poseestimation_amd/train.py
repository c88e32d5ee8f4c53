"""Train / eval step and metrics of the lifter path, mirroring the reference script.

  train_step        /root/reference/phase1_lifting/train_1.py:75-100
  eval_step         /root/reference/phase1_lifting/train_1.py:112-145
  loss_MPJPE        /root/reference/phase1_lifting/train_1.py:19-23
  epoch_mpjpe_mm    /root/reference/phase1_lifting/train_1.py:100-104
  cycle_step        /root/reference/phase5_loop/train_5 copy.py:147-236 (the Triangle branch; Flip=True: :174-199)
All arithmetic is in libposelift.so; tensors must live on the ROCm device.
"""
import torch
from torch.autograd.graph import increment_version

from . import _lib, gradclip
from .pose_table import transform_pair


class _MSEFn(torch.autograd.Function):
    """nn.MSELoss(reduction='mean') with the gradient produced in the same pass."""

    @staticmethod
    def forward(ctx, pred, tgt):
        _lib.require_device_tensor(pred, "pred")
        _lib.require_device_tensor(tgt, "target")
        if pred.shape != tgt.shape:
            raise ValueError(f"MSE shapes differ: {tuple(pred.shape)} vs {tuple(tgt.shape)}")
        n = pred.numel()
        need = pred.requires_grad
        dpred = torch.empty_like(pred) if need else None
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        scratch = torch.empty(_lib.lib().pl_mse_scratch_bytes(n), dtype=torch.uint8, device=pred.device)
        with _lib.on_device(pred.device):
            rc = _lib.lib().pl_mse_fwd_bwd(pred.data_ptr(), tgt.data_ptr(), n, 1.0,
                                           dpred.data_ptr() if need else None, loss.data_ptr(),
                                           scratch.data_ptr(), _lib.current_stream_ptr())
        _lib.check(rc, "pl_mse_fwd_bwd")
        ctx.dpred = dpred
        return loss

    @staticmethod
    def backward(ctx, g):
        d = ctx.dpred
        ctx.dpred = None
        return (d.mul_(g) if d is not None else None), None


def mse_loss(pred, tgt):
    """torch.nn.MSELoss(reduction="mean")(pred, tgt)  (train_1.py:37,94)."""
    return _MSEFn.apply(pred.contiguous(), tgt.contiguous())


def loss_MPJPE(prediction, target, out=None, denorm=None):
    """train_1.py:19-23: (B,J,3),(B,J,3) -> (J,) sum over the batch of per-joint L2 errors.
    With `out`, accumulates into it (the reference's `train_metric_3d +=`).
    denorm: the pose_table.PoseTransform whose space both tensors are in; they are inverted as they are loaded
    (pl_mpjpe_accum_t; the reference's `* std + mean`, main.py:473-474), so the errors are in the raw units."""
    prediction, target = prediction.detach().contiguous(), target.detach().contiguous()
    _lib.require_device_tensor(prediction, "prediction")
    _lib.require_device_tensor(target, "target")
    B, J, d = target.shape
    if d != 3 or prediction.shape != target.shape:
        raise ValueError("loss_MPJPE expects two (B, J, 3) tensors")
    metric = out if out is not None else torch.zeros(J, dtype=torch.float32, device=target.device)
    scratch = torch.empty(_lib.lib().pl_mpjpe_scratch_bytes(B, J), dtype=torch.uint8, device=target.device)
    with _lib.on_device(target.device):
        if denorm is None:
            rc = _lib.lib().pl_mpjpe_accum(prediction.data_ptr(), target.data_ptr(), B, J, metric.data_ptr(),
                                           scratch.data_ptr(), _lib.current_stream_ptr())
        else:
            sub, div, _keep = transform_pair(denorm, (J, 3), target.device, "denorm")
            rc = _lib.lib().pl_mpjpe_accum_t(prediction.data_ptr(), target.data_ptr(), B, J, sub, div, metric.data_ptr(),
                                             scratch.data_ptr(), _lib.current_stream_ptr())
    _lib.check(rc, "pl_mpjpe_accum")
    return metric


def _check_pose(data, what):
    _lib.require_device_tensor(data, what)
    if data.dim() != 3 or data.shape[1] != 17 or data.shape[2] not in (2, 3):
        raise ValueError(f"{what}: expects (N, 17, 2) or (N, 17, 3)")


def _flip_ex(src, addend, x_offset, scale):
    out = torch.empty_like(src)
    with _lib.on_device(src.device):
        rc = _lib.lib().pl_flip_pose_ex(src.data_ptr(), addend.data_ptr() if addend is not None else None, out.data_ptr(),
                                        src.shape[0], 17, src.shape[2], float(x_offset), float(scale),
                                        _lib.current_stream_ptr())
    _lib.check(rc, "pl_flip_pose_ex")
    return out


class _FlipAvgFn(torch.autograd.Function):
    """y = (flip_pose(a) + b) * scale [b optional] with its backward (flip_pose is an affine involution: the gradient is
    the joint swap with x negated -- no `1 - x` offset)."""

    @staticmethod
    def forward(ctx, a, b, scale):
        a = a.contiguous()
        _check_pose(a, "flip_pose input")
        if b is not None:
            b = b.contiguous()
            _check_pose(b, "flip_pose addend")
            if b.shape != a.shape:
                raise ValueError(f"flip average: shapes differ: {tuple(a.shape)} vs {tuple(b.shape)}")
        ctx.scale, ctx.has_b = scale, b is not None
        return _flip_ex(a, b, 1.0 if a.shape[2] == 2 else 0.0, scale)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        da = _flip_ex(g, None, 0.0, ctx.scale) if ctx.needs_input_grad[0] else None
        db = g * ctx.scale if (ctx.has_b and ctx.needs_input_grad[1]) else None
        return da, db, None


def flip_pose(data):
    """utils.py:372-396: horizontal flip of (N, 17, 2|3) poses (x -> 1-x or -x, left/right joints
    swapped); differentiable.  The flip-TTA of train_1.py:128-134 is `(flip_pose(model(flip_pose(x))) + model(x)) / 2`."""
    return _FlipAvgFn.apply(data, None, 1.0)


def flip_average(a, b):
    """(flip_pose(a) + b) / 2 in one pass, differentiable in both: the combination every line of the training-mode Flip
    branch forms (train_5 copy.py:180-196)."""
    return _FlipAvgFn.apply(a, b, 0.5)


def _crop_map(p, boxes, frame_hw, invert, offset):
    out = torch.empty_like(p)
    with _lib.on_device(p.device):
        rc = _lib.lib().pl_crop_poses(p.data_ptr(), boxes.data_ptr(), p.shape[0], int(frame_hw[0]), int(frame_hw[1]), invert,
                                      offset, out.data_ptr(), _lib.current_stream_ptr())
    _lib.check(rc, "pl_crop_poses")
    return out


class _CropPosesFn(torch.autograd.Function):
    """(B,17,2) poses between image and crop coordinates (csrc/frame_crop.h crop1 / uncrop1).  Both maps are affine per
    element, so the backward pass is the same kernel on the gradient without the offset."""

    @staticmethod
    def forward(ctx, p, boxes, frame_hw, invert):
        p, boxes = p.contiguous(), boxes.detach().contiguous()
        _lib.require_device_tensor(p, "p")
        _lib.require_device_tensor(boxes, "boxes")
        if p.dim() != 3 or tuple(p.shape[1:]) != (17, 2) or p.shape[0] == 0 or tuple(boxes.shape) != (p.shape[0], 4) \
                or boxes.device != p.device:
            raise ValueError("crop_poses / uncrop_poses expect p (B,17,2) and boxes (B,4) on one device, B >= 1")
        ctx.boxes, ctx.frame_hw, ctx.invert = boxes, frame_hw, invert
        return _crop_map(p, boxes, frame_hw, invert, 1)

    @staticmethod
    def backward(ctx, g):
        dp = _crop_map(g.contiguous(), ctx.boxes, ctx.frame_hw, ctx.invert, 0) if ctx.needs_input_grad[0] else None
        return dp, None, None, None


def crop_poses(p, boxes, frame_hw):
    """Image-normalised 2-D poses p (B,17,2) -> the crop coordinates of boxes (B,4) = (x0, y0, side, side) (FrameFeeder(crop=),
    augment_poses(crop=), crop_boxes) in frames of frame_hw = (Hs, Ws): x' = (x Ws - x0) / side, y' = (y Hs - y0) / side.
    Differentiable in p; one launch.  What a projector's output goes through before it meets Model_2D's."""
    return _CropPosesFn.apply(p, boxes, tuple(frame_hw), 0)


def uncrop_poses(p, boxes, frame_hw):
    """The way back: crop coordinates -> image-normalised, x = (x' side + x0) / Ws, y = (y' side + y0) / Hs.  Differentiable
    in p; one launch.  Model_2D's output on cropped frames goes through this before the lifter, the metrics or TriangleLoss."""
    return _CropPosesFn.apply(p, boxes, tuple(frame_hw), 1)


def flip_frames_nhwc(frame_nhwc):
    """torch.flip(frame, (3,)) of train_5 copy.py:176 (width of the NCHW frame) on the NHWC frames this path keeps."""
    f = frame_nhwc.contiguous()
    _lib.require_device_tensor(f, "frames")
    if f.dim() != 4:
        raise ValueError("flip_frames_nhwc expects [B, H, W, C]")
    out = torch.empty_like(f)
    with _lib.on_device(f.device):
        rc = _lib.lib().pl_flip_w_nhwc(f.data_ptr(), out.data_ptr(), f.shape[0], f.shape[1], f.shape[2], f.shape[3],
                                       _lib.current_stream_ptr())
    _lib.check(rc, "pl_flip_w_nhwc")
    return out


def epoch_mpjpe_mm(metric_sum, n_samples, num_of_joints=17, zero_centre=True):
    """train_1.py:100-104 reproduced literally: /len(dataset), mean over joints 1..16,
    then *(17/16)*1000 (mm) when the 17-joint root-centred layout is used."""
    m = torch.mean((metric_sum / n_samples)[1:17])
    if num_of_joints == 17 and zero_centre:
        m = m * (17 / 16) * 1000
    return m


def _fusable(model, optimizer, y1, y2, criterion=None):
    from .criterion import PoseCriterion
    from .model import LinearModel
    from .optim import FlatAdamW
    return ((criterion is None or isinstance(criterion, PoseCriterion)) and isinstance(model, LinearModel) and isinstance(optimizer, FlatAdamW) and optimizer._model is model
            and model.training and torch.is_grad_enabled() and not y1.requires_grad and y1.is_cuda and y2.is_cuda
            and model._inject_keep is None and model._arenas_intact()
            and y2.numel() == y2.shape[0] * model.output_size
            and y1.numel() == y1.shape[0] * model.input_size)


def _criterion_loss(criterion, y2_hat, y2, row_weights=None):
    if row_weights is not None:
        return criterion(y2_hat, y2, row_weights=row_weights)
    return mse_loss(y2_hat, y2) if criterion is None else criterion(y2_hat, y2)


def _need_criterion(row_weights, criterion, who):
    if row_weights is not None and criterion is None:
        raise ValueError(f"{who}: row_weights need criterion= (a PoseCriterion: its coords say what a joint is)")


def train_step(model, optimizer, y1, y2, grad_sync=None, criterion=None, row_weights=None):
    """One train_1.py:75-100 step: zero_grad, forward, reshape (B,J,3), MSE(mean), backward,
    [gradient all-reduce], optimizer.step.  Returns (loss, y2_hat) as device tensors -- the
    caller decides when to pay the host sync the reference pays every step (train_1.py:98).
    grad_sync: optional callable(model) -> grad_scale, e.g. dp.GradSync; attach it with
    model.set_grad_sync(grad_sync) to have its all-reduce overlapped with the backward pass.
    criterion: a criterion.PoseCriterion in MSE's place (the reference's `# loss_function = torch.nn.L1Loss()` toggle,
    train_1.py:36-37; smooth-L1, MPJPE, per-joint weights).  LinearModel + FlatAdamW keep the fused step -- the same
    launches, AdamW riding at B <= 64, the data-parallel ranges; every other model runs criterion(y2_hat, y2) under autograd.
    row_weights: (B, J) per-pose joint weights for the criterion (PoseCriterion's row_weights; ValueError without a
    criterion), carried on every one of those routes; under a GradSync they are the weights of this rank's own rows."""
    _need_criterion(row_weights, criterion, "train_step")
    y1, y2 = y1.float(), y2.float()
    if getattr(optimizer, "_swapped", False):
        optimizer._check_live("train_step")
    if _fusable(model, optimizer, y1, y2, criterion):
        # the whole step is three library calls: fwd+loss+bwd, [all-reduce], AdamW.  Same kernels,
        # same results as the autograd route below; `zero_grad` is implicit (gradients are overwritten)
        with _lib.on_device(y1.device):
            x2, t2 = y1.reshape(y1.shape[0], -1).contiguous(), y2.reshape(y2.shape[0], -1).contiguous()
            if (grad_sync is None and model._grad_sync is None and model.step_carries_adamw(x2.shape[0])
                    and not optimizer._clipping()):
                # small batches: AdamW rides in the backward launches (pl_lifter_train_step) -- one library call per step
                # (not with max_grad_norm / skip_nonfinite: the norm of the whole gradient has to exist before any update)
                adamw = optimizer._step_struct(float(optimizer.param_groups[0]["lr"]), None, optimizer._t + 1, None)
                if adamw is not None:
                    loss, y2_hat = model.fused_train_fwd_bwd(x2, t2, None, adamw=adamw, criterion=criterion,
                                                             row_weights=row_weights)
                    optimizer._advance_host(1)
                    return loss, y2_hat.reshape(y2.shape)
            loss, y2_hat = model.fused_train_fwd_bwd(x2, t2, grad_sync if model._grad_sync is grad_sync else None,
                                                     criterion=criterion, row_weights=row_weights)
        optimizer.step(grad_scale=grad_sync(model) if grad_sync is not None else 1.0)
        return loss, y2_hat.reshape(y2.shape)
    optimizer.zero_grad()
    y2_hat = model(y1).reshape(y2.shape)
    loss = _criterion_loss(criterion, y2_hat, y2, row_weights)
    loss.backward()
    if grad_sync is not None:
        optimizer.step(grad_scale=grad_sync(model))
    else:
        optimizer.step()
    return loss, y2_hat


def _check_hyper(who, optimizer, captured):
    """betas / eps / weight_decay of a flat optimizer against what a captured step baked into its launches: a replay after a
    change would use the old value in silence (the eager step follows param_groups), so it is refused -- like every
    other host-side change a graph cannot follow."""
    now = optimizer._hyper_signature()
    if now != captured:
        names = ("beta1", "beta2", "eps", "weight_decay", "decoupled_weight_decay")
        what = ", ".join(f"{n} {a!r} -> {b!r}" for n, a, b in zip(names, captured, now) if a != b)
        raise _lib.PoseliftError(f"{who}: {what} changed in param_groups after capture (betas, eps and weight_decay are baked "
                                 "into the captured launches by value; lr is not): capture a new one")


class GraphedTrainStep:
    """The train_1.py:75-100 step captured ONCE as a hipGraph (torch.cuda.graph) and replayed: the ~50 kernel launches
    of a step become one graph launch, which is what a launch-bound step wants (B = 64, BASELINE configs[0]: the
    host needs ~3.5 us per launch, the kernels far less).

        step = GraphedTrainStep(model, optimizer, x_example, y_example)
        loss, y_hat = step(x, y)            # same results, bit for bit, as train_step(model, optimizer, x, y)

    What changes from step to step lives in device memory and is advanced INSIDE the graph: the dropout stream's
    step number and AdamW's t come from one device counter (PLDesc.step_dev, the AdamW launch's t_dev), the learning rate
    from a device scalar the host refreshes when a scheduler changed it.  Single process (a captured RCCL
    all-reduce is not wired); LinearModel + FlatAdamW; fixed batch shape.
    criterion (a criterion.PoseCriterion, None = MSE): its kind, beta and coords are fixed at capture (changing them on the
    object afterwards does nothing to the graph); the address of its joint_weights is baked into the captured launches, the
    step keeps the criterion alive, and in-place edits of the weights are seen by the next replay (moving the criterion
    to another device or replacing the tensor needs a new GraphedTrainStep: __call__ refuses).
    row_weights ((B, J), with a criterion): the step captures a static (B, J) fp32 buffer, `step.row_weights`, which the
    captured launches read; step(x, y, row_weights=rw) copies rw into it (unless rw IS that buffer), and in-place edits of
    the buffer are seen by the next replay.  A step captured with row weights refuses a call without them, and one
    captured without refuses a call with them (the launches differ)."""

    def __init__(self, model, optimizer, y1, y2, criterion=None, row_weights=None):
        _need_criterion(row_weights, criterion, "GraphedTrainStep")
        y1, y2 = y1.float(), y2.float()
        self.criterion = criterion
        self.row_weights = None
        if row_weights is not None:
            self.row_weights = criterion.row_weights_for(row_weights, y1.shape[0], y2.numel() // y2.shape[0], y2.device).clone()
        row_weights = self.row_weights
        if not _fusable(model, optimizer, y1, y2, criterion) or model._grad_sync is not None:
            raise _lib.PoseliftError("GraphedTrainStep needs a training-mode LinearModel on the GPU with its FlatAdamW "
                                     "and no gradient sync attached")
        self.model, self.opt = model, optimizer
        B = y1.shape[0]
        dev = y1.device
        self._x = y1.reshape(B, -1).contiguous().clone()
        self._y = y2.reshape(B, -1).contiguous().clone()
        self._out_shape = tuple(y2.shape)
        self._tick = torch.zeros(1, dtype=torch.int64, device=dev)          # completed replays
        self._lr_dev = gradclip.DeviceScalar(dev, optimizer.param_groups[0]["lr"])
        lr_dev = self._lr_dev.tensor
        with _lib.on_device(dev):
            # one eager step on a snapshot: every kernel is loaded and the workspace sits in the model's pool before
            # anything is captured; the snapshot is then restored (the step must not count)
            state = [model.flat_params, model._bn_running, model._bn_batches] + optimizer._capture_state()
            snap = [t.clone() for t in state]
            step0, t0 = model._step, optimizer._t
            train_step(model, optimizer, self._x, self._y.reshape(self._out_shape), criterion=criterion, row_weights=row_weights)
            for dst, src in zip(state, snap):
                dst.copy_(src)
            model._step = step0
            optimizer._advance_host(t0 - optimizer._t)
            increment_version(model._arena_tensors)      # (the copies above wrote the arenas, not these views)
            model._ensure_wplanes()          # restoring the snapshot made the persistent weight planes stale
            # max_grad_norm / skip_nonfinite: the captured sequence is fwd+bwd, the norm pass, one AdamW launch; max_norm is
            # read from a device scalar the optimizer refreshes like the learning rate here, the skipped count from its record
            self._clip_mode = optimizer._replay_refresh()
            # the averaged weights: whether the step keeps them, ema_decay / ema_warmup, the update count's base and the
            # arena's address are all baked into the captured launches (the update count itself advances on the device)
            self._ema_sig = optimizer._ema_signature()
            # betas, eps and weight_decay are arguments of the captured launches (PLAdamWStep / the AdamW launch), by value
            self._hyper_sig = optimizer._hyper_signature()
            torch.cuda.synchronize(dev)
            self.graph = torch.cuda.CUDAGraph()
            adamw = (optimizer._step_struct(0.0, lr_dev, t0, self._tick)
                     if model.step_carries_adamw(B) and not optimizer._clipping() else None)
            self._in_call = adamw is not None
            with torch.cuda.graph(self.graph):
                if adamw is not None:        # small batches: the optimizer step is inside the same call's launches
                    self.loss, y_hat = model.fused_train_fwd_bwd(self._x, self._y, None, step_dev=self._tick, adamw=adamw,
                                                                 criterion=criterion, row_weights=row_weights)
                    self._refreshes_planes = False
                else:
                    self.loss, y_hat = model.fused_train_fwd_bwd(self._x, self._y, None, step_dev=self._tick, criterion=criterion,
                                                                 row_weights=row_weights)
                    self._refreshes_planes = optimizer._enqueue_dev(lr_dev, t0, self._tick)
            self.y_hat = y_hat.reshape(self._out_shape)
            model._step = step0                                              # capturing ran nothing
        # the graph owns the dropout-stream step and AdamW's t (both = the capture-time base + the device counter):
        # what __call__ checks the host-side counters against
        self._step0, self._t0, self._seed0, self.replays = step0, t0, model._seed, 0
        self._ptrs = self._baked_ptrs()

    @property
    def inputs(self):
        """The graph's own input buffers (x [B, in], y [B, out], flat): fill them in place and call step(*step.inputs) to
        replay without the two device-to-device copies of a call with other tensors."""
        return self._x, self._y

    def _baked_ptrs(self):
        # (the criterion's joint weights and, with a skeleton, its tables, term_weights and transform)
        crit = self.criterion.device_ptrs() if self.criterion is not None else ()
        return (self.model.flat_params.data_ptr(), self.opt._m.data_ptr() if self.opt._m is not None else 0,
                self.opt._v.data_ptr() if self.opt._v is not None else 0, crit,
                self.opt._e.data_ptr() if self.opt._e is not None else 0)

    def __call__(self, y1, y2, row_weights=None):
        if (row_weights is None) != (self.row_weights is None):
            raise ValueError("GraphedTrainStep: captured " + ("with" if self.row_weights is not None else "without") +
                             " row_weights and called " + ("without" if row_weights is None else "with") +
                             " them: the captured launches differ -- capture a new one")
        if row_weights is not None and (tuple(row_weights.shape) != tuple(self.row_weights.shape) or row_weights.requires_grad):
            raise ValueError(f"GraphedTrainStep: row_weights {tuple(row_weights.shape)} (requires_grad={row_weights.requires_grad}),"
                             f" captured {tuple(self.row_weights.shape)}")
        self.opt._check_live("a GraphedTrainStep replay")
        _check_hyper("GraphedTrainStep", self.opt, self._hyper_sig)
        self._lr_dev.refresh(self.opt.param_groups[0]["lr"])                     # ReduceLROnPlateau et al. (train_1.py:106)
        if self.opt._ema_signature() != self._ema_sig:
            raise _lib.PoseliftError("GraphedTrainStep: ema_decay / ema_warmup were switched on, off or changed after capture, or "
                                     "the averaged weights were re-loaded (their constants and address are baked into the "
                                     "captured launches): capture a new one")
        if self.opt._replay_refresh() != self._clip_mode:
            raise _lib.PoseliftError("GraphedTrainStep: max_grad_norm / skip_nonfinite were switched on or off after capture "
                                     "(their value may change, not whether the step has a norm pass): capture a new one")
        # an eager train_step / optimizer.step() / load_state_dict() between replays moves the host-side counters but
        # not the device counter the captured launches read: re-seed it when both moved together, refuse otherwise
        ds, dt = self.model._step - self._step0, self.opt._t - self._t0
        if self.model._seed != self._seed0 or self._baked_ptrs() != self._ptrs:
            raise _lib.PoseliftError("GraphedTrainStep: the dropout seed, an arena address or the criterion's weight tensor "
                                     "changed after capture (manual_seed, optimizer.load_state_dict, .to()): capture a new "
                                     "GraphedTrainStep")
        if ds != dt or ds < 0:
            raise _lib.PoseliftError(f"GraphedTrainStep: the model ran {ds} steps since capture but the optimizer {dt}: "
                                     "the graph advances both from one device counter -- capture a new one")
        if ds != self.replays:
            self._tick.fill_(ds)
            self.replays = ds
        # (a feeder that writes the next batch straight into `inputs` passes those tensors back: nothing to copy)
        if y1.data_ptr() != self._x.data_ptr():
            self._x.copy_(y1.reshape(self._x.shape))
        if y2.data_ptr() != self._y.data_ptr():
            self._y.copy_(y2.reshape(self._y.shape))
        if row_weights is not None and row_weights.data_ptr() != self.row_weights.data_ptr():
            self.row_weights.copy_(row_weights)
        if not self._in_call:
            self.model._ensure_wplanes()     # parameters changed behind the graph's back (load_state_dict, ...)
        self.graph.replay()
        # the replay wrote the parameters and BatchNorm buffers through raw pointers; a small-batch step (AdamW in the same
        # call) leaves the persistent weight planes stale, the separate AdamW launch refreshed them with the parameters
        increment_version(self.model._arena_tensors)
        if self._refreshes_planes:
            self.model._wplanes_ver = self.model._planes_key()
        self.model._step += 1
        self.opt._advance_host(1)
        self.replays += 1
        return self.loss, self.y_hat


class GraphedModuleStep:
    """A whole training step of the conv models -- phase4_joined/train.py:69-89: zero_grad, Model_3D forward, loss, backward,
    Adam -- captured ONCE as a hipGraph and replayed.  The step is ~1,100 launches driven from Python autograd nodes; at the
    reference's own batch (8 frames, train.py:187) the host needs 14-17 ms to issue what the GPU finishes in less, and a replay is
    one launch.  Same kernels in the same order: results are bit-identical to the eager step's.

        opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=True)
        step = GraphedModuleStep(model, opt, torch.nn.functional.mse_loss, frames_example, target_example)
        loss = step(frames, target)         # a device scalar, overwritten by the next call

    Construction runs `warmup` eager steps on the example batch (every kernel loaded, the allocator's pool sized) and then
    puts parameters, buffers and optimizer state back exactly as they were, so the first replay is the model's first step.
    Fixed shapes; single process; the optimizer must keep its step state on the device (torch: capturable=True; give lr as
    a tensor to change it between replays; arena.FlatAdam's float lr is followed as it is, and a change of its betas, eps or
    weight_decay after capture is refused).  forward(*inputs) is whatever the module's forward takes; loss_fn(output,
    target) -- a criterion.PoseCriterion is one (its launch pair is captured like any other: kind, beta and coords as they
    are at construction, joint_weights edited in place are seen by replays).  For per-pose weights loss_fn may close over a
    static (B, J) weights tensor, loss_fn = lambda out, tgt: crit(out, tgt, row_weights=rw): the captured launches read rw's
    memory, so fill it in place (rw.copy_(...)) before each replay."""

    def __init__(self, model, optimizer, loss_fn, inputs, target, warmup=2):
        inputs = tuple(inputs) if isinstance(inputs, (tuple, list)) else (inputs,)
        dev = target.device
        if dev.type != "cuda" or any(t.device != dev for t in inputs):
            raise _lib.PoseliftError("GraphedModuleStep: inputs and target must sit on one GPU")
        if not model.training:
            raise _lib.PoseliftError("GraphedModuleStep captures a TRAINING step: call model.train() first")
        for gr in optimizer.param_groups:
            if not gr.get("capturable", False):
                raise _lib.PoseliftError("GraphedModuleStep: the optimizer must be built with capturable=True "
                                         "(its step counter has to live on the device)")
        self.model, self.opt, self.loss_fn = model, optimizer, loss_fn
        self._state = list(model.parameters()) + list(model.buffers())      # what a replay writes behind autograd's back
        self._in = tuple(t.detach().clone() for t in inputs)
        self._target = target.detach().clone()
        # arena.FlatAdam with ema_decay: the averaged weights exist before the warm-up steps (which the restore below then
        # undoes like the moments); what the captured launches bake in about them is checked at every replay
        # ... so is what they bake in of the update (betas, eps, weight_decay: _check_hyper), and a float lr is refreshed into
        # the device scalar the captured launch reads (a stock torch optimizer is left to torch's own rules: lr as a tensor)
        self._ema_sig = self._hyper_sig = None
        self._lr_is_tensor = False
        if hasattr(optimizer, "_ema_signature"):
            optimizer._check_live("GraphedModuleStep")
            optimizer._ema_bind()
            self._ema_sig = optimizer._ema_signature()
            self._hyper_sig = optimizer._hyper_signature()
            lr = optimizer.param_groups[0]["lr"]
            self._lr_is_tensor = torch.is_tensor(lr)
            self._lr_ptr = lr.data_ptr() if self._lr_is_tensor else None
        with _lib.on_device(dev):
            torch.cuda.synchronize(dev)
            state = [t for t in model.state_dict().values()]
            snap = [t.detach().clone() for t in state]
            had = {p: {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in optimizer.state.get(p, {}).items()}
                   for gr in optimizer.param_groups for p in gr["params"]}
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(max(1, int(warmup))):
                    self._step()
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            with torch.no_grad():
                for dst, src in zip(state, snap):
                    dst.copy_(src)
                for p, old in had.items():                                   # optimizer state: back to what it was, IN PLACE
                    for k, v in optimizer.state.get(p, {}).items():          # (a fresh optimizer: zeros, step 0)
                        if torch.is_tensor(v):
                            v.copy_(old[k]) if k in old else v.zero_()
            optimizer.zero_grad(set_to_none=True)
            torch.cuda.synchronize(dev)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.loss = self._step()
        self.replays = 0

    def _step(self):
        self.opt.zero_grad(set_to_none=True)
        loss = self.loss_fn(self.model(*self._in), self._target)
        loss.backward()
        self.opt.step()
        return loss.detach()

    def __call__(self, inputs, target):
        inputs = tuple(inputs) if isinstance(inputs, (tuple, list)) else (inputs,)
        if hasattr(self.opt, "_ema_signature"):
            self.opt._check_live("a GraphedModuleStep replay")
            if self.opt._ema_signature() != self._ema_sig:
                raise _lib.PoseliftError("GraphedModuleStep: ema_decay / ema_warmup were switched on, off or changed after "
                                         "capture, or the averaged weights were re-loaded: capture a new one")
            _check_hyper("GraphedModuleStep", self.opt, self._hyper_sig)
            lr = self.opt.param_groups[0]["lr"]
            if torch.is_tensor(lr) != self._lr_is_tensor or (self._lr_is_tensor and lr.data_ptr() != self._lr_ptr):
                raise _lib.PoseliftError("GraphedModuleStep: param_groups[0]['lr'] was a " +
                                         ("tensor" if self._lr_is_tensor else "float") + " at capture and the captured launch "
                                         "reads that memory: change its value, not the object -- or capture a new one")
            if not self._lr_is_tensor and hasattr(self.opt, "_lr_dev"):
                self.opt._lr_dev.refresh(lr)             # a scheduler's new float lr: FlatAdam.step() does not run in a replay
        for dst, src in zip(self._in, inputs):
            dst.copy_(src)
        self._target.copy_(target)
        self.graph.replay()
        increment_version(self._state)
        self.replays += 1
        return self.loss


@torch.no_grad()
def predict_flip_tta(model, y1, out_dims=3):
    """(flip_pose(model(flip_pose(y1))) + model(y1)) / 2 for a model in eval mode, as ONE forward
    of 2B rows (eval BatchNorm is row-wise): pack [y1; flip(y1)], lift, merge.  The intent of the
    reference's `Flip` branches (train_1.py:128-134, which at HEAD never flips the input;
    phase5_loop/train_5 copy.py:160-171)."""
    if model.training:
        raise ValueError("flip TTA is an eval-mode operation (BatchNorm on running statistics)")
    y1 = y1.float().contiguous()
    _lib.require_device_tensor(y1, "y1")
    if y1.dim() != 3 or y1.shape[1] != 17 or y1.shape[2] not in (2, 3):
        raise ValueError("flip TTA expects (B, 17, 2|3) poses")
    B, L = y1.shape[0], _lib.lib()
    xx = torch.empty((2 * B,) + tuple(y1.shape[1:]), dtype=torch.float32, device=y1.device)
    with _lib.on_device(y1.device):
        _lib.check(L.pl_flip_tta_pack(y1.data_ptr(), xx.data_ptr(), B, 17, y1.shape[2], _lib.current_stream_ptr()),
                   "pl_flip_tta_pack")
        yy = model(xx).reshape(2 * B, 17, out_dims).contiguous()
        out = torch.empty(B, 17, out_dims, dtype=torch.float32, device=y1.device)
        _lib.check(L.pl_flip_tta_merge(yy.data_ptr(), out.data_ptr(), B, 17, out_dims, _lib.current_stream_ptr()),
                   "pl_flip_tta_merge")
    return out


@torch.no_grad()
def eval_step(model, y1, y2, metric_out=None, flip=False, meter=None, group_ids=None, denorm=None, criterion=None, ema=None,
              row_weights=None, meter_weights=None):
    """train_1.py:112-145 body (model must be in eval mode): forward, MSE, loss_MPJPE.
    criterion: a criterion.PoseCriterion -- `loss` is then that criterion's value, not the MSE.
    row_weights: (B, J) per-pose joint weights of that criterion's value (ValueError without a criterion); `metric` is not
    weighted, and the meter has a keyword of its own:
    meter_weights: (B, J) visibility of the targets for a meter built with PoseMetrics(visibility=True), handed to
    meter.update(weights=): joints with weight > 0 fit the alignment and enter the masked table (metrics.py).  Independent
    of row_weights (which stays the criterion's and still needs one); ValueError without a meter or with a plain meter.
    flip=True: flip test-time augmentation (predict_flip_tta).
    meter: a metrics.PoseMetrics that also takes this batch (P-MPJPE, N-MPJPE, PCK; group_ids (B,) = e.g. the action of
    each pose); like everything here it only enqueues work.
    denorm: the pose_table.PoseTransform of the 3-D targets (y2 and the model's output are in its space).  The MSE stays
    in the model's space, as the reference's loss does; `metric` and the meter are in the raw units, both tensors inverted
    inside the launches that read them (no launch more than without).  y2_hat is returned as the model gave it.
    ema: the model's flat optimizer built with ema_decay -- the step runs on the averaged weights, i.e. inside
    `with ema.averaged_weights():` (BatchNorm running statistics stay the live ones)."""
    _need_criterion(row_weights, criterion, "eval_step")
    if meter_weights is not None and (meter is None or not getattr(meter, "visibility", False)):
        raise ValueError("eval_step: meter_weights= needs meter= a PoseMetrics built with visibility=True")
    if ema is not None:
        with ema.averaged_weights():
            return eval_step(model, y1, y2, metric_out=metric_out, flip=flip, meter=meter, group_ids=group_ids, denorm=denorm,
                             criterion=criterion, row_weights=row_weights, meter_weights=meter_weights)
    if flip and denorm is not None:
        raise ValueError("eval_step: flip=True mirrors image-normalised poses and cannot run on transformed ones; compose it: "
                         "a = model(T2.apply(raw2d)), b = model(T2.apply(flip_pose(raw2d))), then "
                         "flip_average(T3.invert(b), T3.invert(a)) is the prediction in raw units")
    y1, y2 = y1.float(), y2.float()
    y2_hat = predict_flip_tta(model, y1, y2.shape[-1]).reshape(y2.shape) if flip else model(y1).reshape(y2.shape)
    loss = _criterion_loss(criterion, y2_hat, y2, row_weights)
    metric = loss_MPJPE(y2_hat, y2, out=metric_out, denorm=denorm)
    if meter is not None:
        if meter_weights is not None:
            meter.update(y2_hat, y2, group_ids, denorm=denorm, weights=meter_weights)
        else:
            meter.update(y2_hat, y2, group_ids, denorm=denorm)
    return loss, metric, y2_hat


def cycle_step(model_2d, model_3d, model_lift, optimizers, frame_nhwc, y1, y2, loss_function, model_proj=None, Flip=False):
    """One phase5 cycle step (train_5 copy.py:147-236, `Triangle` on): zero_grad on every optimizer;
    y1^ = model_2d(frame), y2^ = model_3d(frame); the lifter on the predicted AND on the ground-truth 2-D pose (two
    calls in one graph: its input gradient flows back into model_2d); optionally the projector on y2^ and y2;
    [the Flip branch]; TriangleLoss; ONE backward; every optimizer steps.
    Flip=True reproduces train_5 copy.py:174-199 literally: every network runs a SECOND training-mode forward (its
    BatchNorm statistics move twice per step, as in the reference) -- the backbones on the mirrored frames, the lifter
    on the AVERAGED 2-D prediction (:183 feeds `y1_hat` after :180 has overwritten it with the average; it is not
    flipped) and on the flipped ground truth (:184), the projector on the averaged 3-D prediction and on flip(y2) -- and
    each result becomes (flip_pose(second) + first) / 2.
    frame_nhwc [B, H, W, 3]; y1 [B, 17, 2]; y2 [B, 17, 3].
    Returns (loss, y1_hat, y2_hat) as device tensors (the reference's `.cpu().item()` per step is the caller's choice)."""
    for opt in optimizers:
        opt.zero_grad()
    B = y1.shape[0]
    y1, y2 = y1.float(), y2.float()
    frame = frame_nhwc.float()
    y1_hat = model_2d.predict_nhwc(frame).reshape(B, 17, 2)
    y2_hat = model_3d.predict_nhwc(frame).reshape(B, 17, 3)
    lift_2d_pred = model_lift(y1_hat).reshape(B, 17, 3)
    lift_2d_gt = model_lift(y1).reshape(B, 17, 3)
    proj_3d_pred = proj_3d_gt = None
    if model_proj is not None:
        proj_3d_pred = model_proj(y2_hat).reshape(B, 17, 2)
        proj_3d_gt = model_proj(y2).reshape(B, 17, 2)
    if Flip:
        frame_f = flip_frames_nhwc(frame)                                                    # :176
        y1_f = flip_pose(y1)                                                                 # :178
        y1_hat = flip_average(model_2d.predict_nhwc(frame_f).reshape(B, 17, 2), y1_hat)      # :180
        y2_hat = flip_average(model_3d.predict_nhwc(frame_f).reshape(B, 17, 3), y2_hat)      # :181
        lift_2d_pred = flip_average(model_lift(y1_hat).reshape(B, 17, 3), lift_2d_pred)      # :184
        lift_2d_gt = flip_average(model_lift(y1_f).reshape(B, 17, 3), lift_2d_gt)            # :185
        if model_proj is not None:
            y2_f = flip_pose(y2)                                                             # :189
            proj_3d_pred = flip_average(model_proj(y2_hat).reshape(B, 17, 2), proj_3d_pred)  # :191
            proj_3d_gt = flip_average(model_proj(y2_f).reshape(B, 17, 2), proj_3d_gt)        # :192
        # (:194, :197-198 flip y2, the frame and y1 back: out of place here, the originals are still y1 / y2 / frame)
    kw = {}
    if model_proj is not None:
        kw = dict(proj_3d_pred=proj_3d_pred, proj_3d_gt=proj_3d_gt)
    out = loss_function(predicted_2d=y1_hat, predicted_3d=y2_hat, lift_2d_gt=lift_2d_gt, lift_2d_pred=lift_2d_pred,
                        gt_2d=y1, gt_3d=y2, **kw)
    loss = out[0] if isinstance(out, tuple) else out
    loss.backward()
    for opt in optimizers:
        opt.step()
    return loss.detach(), y1_hat.detach(), y2_hat.detach()
