"""FlatAdamW: torch.optim.AdamW semantics over the lifter's flat arenas, one HIP launch.

Replaces `torch.optim.AdamW(model_lift.parameters(), lr=lr)` + `optimizer_lift.step()`
(/root/reference/phase1_lifting/train_1.py:39,96): decoupled weight decay 0.01 on every
parameter, betas (0.9, 0.999), eps 1e-8, bias-corrected, in torch's single-tensor update
order.  It is a torch.optim.Optimizer subclass (LR schedulers such as the reference's
ReduceLROnPlateau, train_1.py:41, work unchanged) and its state_dict() has the stock
AdamW structure (per-parameter 'step', 'exp_avg', 'exp_avg_sq'), so the reference's
checkpoint envelope {'epoch','batch_size','model','optimizer'} (train_1.py:186) round-trips.

max_grad_norm / skip_nonfinite (gradclip.py): `nn.utils.clip_grad_norm(model.parameters(), max_norm=1)` of the reference's
lifter script (phase1_lifting/main.py:465-470, MaxNormConctraint) and "do not step on a non-finite gradient", both decided
on the device: a norm pass over the active ranges of the gradient arena writes a record, the AdamW launch reads it.  The
gradient arena is not rewritten -- unlike clip_grad_norm_, `p.grad` keeps the UNCLIPPED gradient.  A non-finite gradient
without skip_nonfinite follows torch's error_if_nonfinite=False: inf norm -> coefficient 0 -> inf * 0 = NaN parameters.

ema_decay / ema_warmup: exponentially averaged weights kept INSIDE the AdamW launches (csrc/adamw.h ema_one): one more arena,
laid out like the parameters, updated from the registers that hold the new parameter -- no launch of its own on any route (the
B <= 64 step that carries AdamW in its backward launches carries the average too), inside graph replays, and untouched by a
skipped step.  state[p]["ema"] is the per-parameter view (the stock state_dict() carries it), param_groups[0]["ema_updates"]
the number of updates; `with optimizer.averaged_weights():` exchanges parameters and averages in place for evaluation.
"""
import contextlib
import ctypes
import math
from collections import OrderedDict

import torch
from torch.autograd.graph import increment_version

from . import _lib, gradclip


def check_ema_options(ema_decay, ema_warmup=False):
    """(decay as a float in [0, 1) or None, warmup as a bool); ValueError for anything else."""
    if ema_decay is None:
        return None, bool(ema_warmup)
    if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float)):
        raise ValueError(f"ema_decay must be a number in [0, 1) or None, got {ema_decay!r}")
    d = float(ema_decay)
    if math.isnan(d) or not 0.0 <= d < 1.0:
        raise ValueError(f"ema_decay must be in [0, 1), got {ema_decay!r}")
    return d, bool(ema_warmup)


class FlatOptimizer(torch.optim.Optimizer):
    """What FlatAdamW (the lifter's arenas) and arena.FlatAdam (any module's) share: the max_grad_norm / skip_nonfinite options
    and their device state, and the one place an AdamW launch is issued.  A subclass provides _arenas() -> (parameter arena,
    gradient arena) and the moment arenas self._m / self._v beside them."""

    def __init__(self, params, defaults):
        defaults["max_grad_norm"], defaults["skip_nonfinite"] = gradclip.check_options(defaults["max_grad_norm"],
                                                                                       defaults["skip_nonfinite"])
        defaults["ema_decay"], defaults["ema_warmup"] = check_ema_options(defaults.get("ema_decay"),
                                                                          defaults.get("ema_warmup", False))
        super().__init__(params, defaults)
        self._t = 0                      # ATTEMPTED steps; taken = _t - (the record's skipped count, on the device)
        self._clip = None                # gradclip.GradClip, created by the first step that clips or skips
        self._skipped_seen = 0           # the device's skipped count at the last host read
        self._e = None                   # the EMA arena (the parameter arena's layout), created by _ema_bind
        self._e_of = None                #   ... beside the parameter arena at this address
        self._ema_t0 = 0                 # TAKEN steps when the average was started or loaded: update n = taken - _ema_t0
        self._swapped = False            # inside averaged_weights(): the live weights are parked in the EMA arena

    # ---- averaged weights ------------------------------------------------------------------------------------------
    def _ema_options(self):
        """(ema_decay or None, ema_warmup) of this step: param_groups[0], like max_grad_norm."""
        g = self.param_groups[0]
        return check_ema_options(g.get("ema_decay"), g.get("ema_warmup", False))

    def _attempted_host(self):
        return self._t

    def _taken_host(self):
        """Steps taken so far, on the host (one read of the clip record when there is one)."""
        return int(self._attempted_host()) - self.skipped_steps()

    def _ema_bind(self):
        """With ema_decay set: the EMA arena beside the parameter arena -- created as a copy of the parameters (0 updates), or
        re-created from the per-parameter state (a loaded state, a moved arena) -- and state[p]["ema"] bound to its views."""
        if self._ema_options()[0] is None:
            return
        flat = self._arenas()[0]
        if self._e is not None and self._e_of == flat.data_ptr():
            return
        e = flat.detach().clone()
        fresh = True
        for p, o in self._param_offsets():
            st, n = self.state[p], p.numel()
            view = e[o:o + n].view(p.shape)
            if "ema" in st:
                view.copy_(st["ema"])
                fresh = False
            st["ema"] = view
        if fresh:
            self._ema_t0 = self._taken_host()
        self._e, self._e_of = e, flat.data_ptr()

    def _ema_struct(self, lo=0):
        """PLEma of the arena from float `lo` on for this step's launches, or None without ema_decay."""
        decay, warmup = self._ema_options()
        if decay is None:
            return None
        self._ema_bind()
        return _lib.PLEma(self._e.data_ptr() + 4 * lo, decay, int(warmup), int(self._ema_t0))

    def _ema_signature(self):
        """What a captured step bakes in about the average: on or off, its constants, where it lives."""
        decay, warmup = self._ema_options()
        if decay is None:
            return None
        return (decay, warmup, int(self._ema_t0), self._e.data_ptr() if self._e is not None else 0)

    def _hyper_signature(self):
        """What a captured step bakes into its launches BY VALUE about the update itself: betas, eps, weight_decay (and
        whether it is applied: arena.FlatAdam's decoupled_weight_decay).  lr and max_norm are read from device scalars and t
        from a device counter, so they may change between replays; these may not (train.GraphedTrainStep /
        GraphedModuleStep refuse the replay)."""
        g = self.param_groups[0]
        return (float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                bool(g.get("decoupled_weight_decay", True)))

    def _ema_after_load(self, keep):
        """load_state_dict: `keep` = this optimizer's own (ema_decay, ema_warmup), which a loaded state does not replace.
        With ema_decay: a state that carries the averages continues them (and their update count); one that does not starts
        the average from the current parameters with 0 updates.  Without: the loaded averages are ignored."""
        g = self.param_groups[0]
        updates = int(g.get("ema_updates", 0) or 0)
        g["ema_decay"], g["ema_warmup"] = keep
        self._e = self._e_of = None
        params = [p for p, _ in self._param_offsets()]
        have = all("ema" in self.state[p] for p in params)
        if keep[0] is None or not have:
            for p in params:
                self.state[p].pop("ema", None)
            g.pop("ema_updates", None)
            updates = 0
        self._ema_bind()
        if keep[0] is not None:
            self._ema_t0 = self._taken_host() - updates
            g["ema_updates"] = updates

    def state_dict(self):
        """(with ema_decay: param_groups[0]["ema_updates"] = EMA updates so far -- one host read of the step counters)"""
        if self._ema_options()[0] is not None and self._e is not None:
            self.param_groups[0]["ema_updates"] = self._taken_host() - self._ema_t0
        return super().state_dict()

    def _check_live(self, what):
        if self._swapped:
            raise _lib.PoseliftError(f"{what} inside averaged_weights(): the parameters hold the averaged weights and the live "
                                     "ones are parked in the EMA arena -- leave the context first")

    def _swap_average(self):
        flat = self._arenas()[0]
        with _lib.on_device(flat.device):
            _lib.check(_lib.lib().pl_swap_f32(flat.data_ptr(), self._e.data_ptr(), flat.numel(), _lib.current_stream_ptr()),
                       "pl_swap_f32")
        # the parameters were written through a raw pointer: whatever is derived from them (weight planes, folded-BN
        # caches) keys on their version counters
        increment_version([p for p, _ in self._param_offsets()])

    @contextlib.contextmanager
    def averaged_weights(self):
        """Inside: the module's parameters ARE their averages (one in-place exchange of the two arenas on entry, one on exit;
        buffers -- BatchNorm running statistics -- stay the live ones).  After: bitwise what they were.  Not re-entrant, and no
        optimizer step, fused train step or graph replay inside."""
        if self._swapped:
            raise _lib.PoseliftError("averaged_weights() is not re-entrant")
        if self._ema_options()[0] is None:
            raise _lib.PoseliftError("averaged_weights(): this optimizer keeps no averaged weights (ema_decay=None)")
        self._ema_ready()
        self._swap_average()
        self._swapped = True
        try:
            yield self
        finally:
            self._swap_average()
            self._swapped = False

    def _ema_ready(self):
        self._ema_bind()

    def ema_state_dict(self):
        """The module's state_dict() with every parameter replaced by (a copy of) its average.  Buffers are the live ones:
        BatchNorm running statistics are not averaged (torch's AveragedModel(use_buffers=False))."""
        if self._ema_options()[0] is None:
            raise _lib.PoseliftError("ema_state_dict(): this optimizer keeps no averaged weights (ema_decay=None)")
        self._ema_ready()
        module = self._ema_module()
        named = dict(module.named_parameters(remove_duplicate=False))
        out = OrderedDict()
        for k, v in module.state_dict().items():
            p = named.get(k)
            if p is None or p not in self.state or "ema" not in self.state[p]:
                out[k] = v
            else:                            # (inside averaged_weights() the average sits in the parameter itself)
                out[k] = (p if self._swapped else self.state[p]["ema"]).detach().clone()
        return out

    def _clip_options(self):
        """(max_grad_norm or None, skip_nonfinite) of this step: param_groups[0], changeable between steps like lr."""
        g = self.param_groups[0]
        return gradclip.check_options(g.get("max_grad_norm"), g.get("skip_nonfinite", False))

    def _clipping(self):
        m, skip = self._clip_options()
        return m is not None or skip

    def _clip_state(self):
        dev = self._arenas()[0].device
        if self._clip is None or self._clip.device != dev:
            self._clip = gradclip.GradClip(dev)
            self._skipped_seen = 0
        return self._clip

    @property
    def grad_norm(self):
        """Device scalar: |grad_scale| * ||g||_2 of the last step that clipped or skipped (no sync)."""
        return self._clip_state().norm

    @property
    def clip_coef(self):
        """Device scalar: the coefficient the last step multiplied its gradient by (no sync)."""
        return self._clip_state().coef

    def skipped_steps(self):
        """Steps not taken because their gradient norm was not finite, since construction / load_state_dict (one host read)."""
        if self._clip is None:
            return 0
        self._skipped_seen = self._clip.skipped()
        self._step_tensor_fill()
        return self._skipped_seen

    def _step_tensor_fill(self):
        """(FlatAdamW: its host step tensor reports taken steps, so it follows the skipped count)"""

    def _forget_skipped(self):
        """load_state_dict: the loaded step counts taken steps, nothing is skipped against it."""
        if self._clip is not None:
            self._clip.reset_skipped()
        self._skipped_seen = 0

    def _capture_state(self):
        """The optimizer's tensors a captured step writes: what a capture that warms up with a real step snapshots and
        restores (train.GraphedTrainStep)."""
        self._ema_bind()
        return ([self._m, self._v] + ([self._clip_state().record] if self._clipping() else [])
                + ([self._e] if self._ema_options()[0] is not None else []))

    def _replay_refresh(self):
        """Before a capture and before every replay: bring the device scalars the captured launches read (max_norm) up to date.
        Returns (clips, skips): whether the step has a norm pass is baked into a capture, the values are not."""
        g = self.param_groups[0]
        max_norm, skip = g.get("max_grad_norm"), bool(g.get("skip_nonfinite", False))
        if max_norm is not None:
            self._clip_state().refresh(gradclip.check_options(max_norm, skip)[0])
        return max_norm is not None, skip

    def _launch_adamw(self, runs, lr, lr_ptr, t, t_ptr, weight_decay, grad_scale, planes=None):
        """THE AdamW launch: one pl_adamw_flat_planes_clip_ema per [lo, hi) run of the arenas, every optional part absent = NULL
        (lr by value or *lr_ptr, t or t + *t_ptr, planes, the clip record, the averaged weights).  With max_grad_norm /
        skip_nonfinite the norm pass over the same runs goes first and every launch takes its record.  No run: nothing is
        launched."""
        self._check_live("an optimizer step")
        if not runs:
            return
        flat, grads = self._arenas()
        g = self.param_groups[0]
        b1, b2, eps = float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])
        max_norm, skip = self._clip_options()
        with _lib.on_device(flat.device):
            record = None
            if max_norm is not None or skip:
                clip = self._clip_state()
                clip.launch(grads, runs, grad_scale, max_norm, skip, from_device=lr_ptr is not None)
                record = clip.ptr
            adamw = _lib.lib().pl_adamw_flat_planes_clip_ema
            planes = _lib.ctypes.byref(planes) if planes is not None else None
            for lo, hi in runs:
                ema = self._ema_struct(lo)
                rc = adamw(flat.data_ptr() + 4 * lo, grads.data_ptr() + 4 * lo, self._m.data_ptr() + 4 * lo,
                           self._v.data_ptr() + 4 * lo, hi - lo, float(lr), lr_ptr, b1, b2, eps, float(weight_decay), int(t), t_ptr,
                           float(grad_scale), planes, record, ctypes.byref(ema) if ema is not None else None,
                           _lib.current_stream_ptr())
                _lib.check(rc, "pl_adamw_flat_planes_clip_ema")


class FlatAdamW(FlatOptimizer):
    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None,
                 skip_nonfinite=False, ema_decay=None, ema_warmup=False):
        if not hasattr(model, "flat_params"):
            raise TypeError("FlatAdamW drives a 3d_poseestimation_amd LinearModel")
        self._model = model
        super().__init__(list(model._param_list), dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                                       max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite,
                                                       ema_decay=ema_decay, ema_warmup=ema_warmup))
        self._m = self._v = None
        self._bound_arena = None

    def _arenas(self):
        return self._model.flat_params, self._model.flat_grads

    def _param_offsets(self):
        return [(p, s.offset) for s, p in zip(self._model._slots, self._model._param_list)]

    def _ema_module(self):
        return self._model

    def _ema_ready(self):
        self._bind()

    def _bind(self):
        """(Re)create flat moment arenas next to the model's parameter arena and expose them
        as per-parameter views in self.state (the stock AdamW layout)."""
        model = self._model
        flat = model.flat_params
        if self._bound_arena is not None and self._bound_arena.data_ptr() == flat.data_ptr():
            self._ema_bind()              # (ema_decay switched on between steps: the average starts here)
            return
        m, v = torch.zeros_like(flat), torch.zeros_like(flat)
        self._step_tensor = torch.tensor(0.0)            # ONE host tensor shared by all 22 state entries
        for s, p in zip(model._slots, model._param_list):
            st = self.state[p]
            mv = m[s.offset:s.offset + s.numel].view(s.shape)
            vv = v[s.offset:s.offset + s.numel].view(s.shape)
            if "exp_avg" in st:
                mv.copy_(st["exp_avg"])
                vv.copy_(st["exp_avg_sq"])
                self._t = max(self._t, int(st["step"]))
            st["exp_avg"], st["exp_avg_sq"] = mv, vv
            st["step"] = self._step_tensor
        self._step_tensor_fill()
        self._m, self._v, self._bound_arena = m, v, flat
        self._ema_bind()

    def _active_ranges(self):
        """Arena ranges [lo, hi) (floats) the step updates.  torch.optim.AdamW skips a parameter whose grad is None:
        with BN=False the reference never touches the (unused) BatchNorm weights and biases -- no moment update and,
        in particular, no weight decay -- and the same goes for requires_grad=False tensors.  Everything active (the
        normal case) is ONE launch over the whole arena; otherwise one launch per run of adjacent active tensors."""
        model = self._model
        active = [p.requires_grad and (model.BN or "batch_norm" not in s.name)
                  for s, p in zip(model._slots, model._param_list)]
        if all(active):
            return [(0, model.flat_params.numel())]
        runs = []
        for k, (s, on) in enumerate(zip(model._slots, active)):
            if not on:
                continue
            end = model._slots[k + 1].offset if k + 1 < len(model._slots) else model.flat_params.numel()
            if runs and runs[-1][1] == s.offset:
                runs[-1] = (runs[-1][0], end)
            else:
                runs.append((s.offset, end))
        return runs

    def _step_tensor_fill(self):
        if getattr(self, "_step_tensor", None) is not None:
            self._step_tensor.fill_(float(self._t - self._skipped_seen))

    def state_dict(self):
        """'step' reports TAKEN steps (attempted - skipped): one host read of the record when a step was ever clipped."""
        self.skipped_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        keep = self._ema_options()
        super().load_state_dict(state_dict)
        self._bound_arena = None          # loaded tensors are copies: re-bind into the arenas
        self._t = 0
        self._forget_skipped()
        self._e = None
        self.param_groups[0]["ema_decay"] = None      # (_bind leaves the average to _ema_after_load)
        self._bind()
        self._ema_after_load(keep)

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_live("optimizer.step()")
        self._bind()
        _lib.require_device_tensor(self._model.flat_params, "parameters")
        self._t += 1
        self._launch(float(self.param_groups[0]["lr"]), None, self._t, None, grad_scale)
        self._step_tensor_fill()
        return loss

    def _launch(self, lr, lr_dev, t, t_dev, grad_scale):
        """The step over the active ranges.  With the whole arena active (the normal case) the same launch refreshes the
        model's persistent GEMM weight planes while the new parameters are in registers.  Returns whether it did.  (A step
        skipped for a non-finite gradient still writes the planes, from the unchanged parameters: marking them current
        below stays right.)"""
        model = self._model
        ranges = self._active_ranges()
        planes = model.adamw_plane_segments() if ranges == [(0, model.flat_params.numel())] else None
        self._launch_adamw(ranges, lr, lr_dev.data_ptr() if lr_dev is not None else None, t,
                           t_dev.data_ptr() if t_dev is not None else None, self.param_groups[0]["weight_decay"], grad_scale,
                           planes)
        increment_version(model._param_list)
        if planes is not None:                # the planes are those of the parameters just written
            model._wplanes_ver = model._planes_key()
        return planes is not None

    # ---- the step inside the model's fused call (pl_lifter_train_step) ------------------------------------------
    def _step_struct(self, lr, lr_dev, t, t_dev):
        """PLAdamWStep for LinearModel.fused_train_fwd_bwd(adamw=...), or None when this optimizer does not update the
        whole arena (frozen tensors, BN=False: torch skips grad-less parameters)."""
        self._check_live("a fused train step")
        self._bind()
        n = self._model.flat_params.numel()
        if self._active_ranges() != [(0, n)]:
            return None
        g = self.param_groups[0]
        ema = self._ema_struct()
        return _lib.PLAdamWStep(self._m.data_ptr(), self._v.data_ptr(), float(lr),
                                lr_dev.data_ptr() if lr_dev is not None else None, float(g["betas"][0]), float(g["betas"][1]),
                                float(g["eps"]), float(g["weight_decay"]), int(t),
                                t_dev.data_ptr() if t_dev is not None else None,
                                ctypes.pointer(ema) if ema is not None else None)

    # ---- graph replay (train.GraphedTrainStep): the step with t and lr read from device memory ----------------
    def _enqueue_dev(self, lr_dev, t_base, t_dev, grad_scale=1.0):
        """Enqueue (or capture) one step whose t = t_base + *t_dev and lr = *lr_dev; host-side counters are the
        caller's business (a captured launch runs many times).  Returns whether the launch refreshes the weight planes."""
        self._bind()
        return self._launch(0.0, lr_dev, t_base, t_dev, grad_scale)

    def _capture_state(self):
        self._bind()
        return super()._capture_state()

    def _advance_host(self, n=1):
        self._t += n
        self._step_tensor_fill()
