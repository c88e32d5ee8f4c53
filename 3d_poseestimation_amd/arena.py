"""Flat arenas and a one-launch Adam for modules with ordinary parameters (the conv models).

Replaces `torch.optim.Adam(model_direct.parameters(), lr)` + `optimizer.step()`
(/root/reference/phase4_joined/train.py:39,87; phase5_loop/train_5 copy.py:105-109,219-224) for Model_3D / Model_2D /
ResNet, the way optim.FlatAdamW does for the lifter:

  * ModuleArena: every parameter of the module becomes a view into ONE fp32 parameter arena (64-float aligned slots, the
    module's `parameters()` order), with gradient / Adam m / Adam v arenas of the same layout beside it.  state_dict() keys
    and shapes do not change (checkpoints load as before: load_state_dict copies into the views).
  * Parameter gradients are written by the library straight into the gradient arena: the autograd nodes of conv.py hand
    their weight / BatchNorm gradient kernels the arena view as output and return None to autograd (`p._pl_grad`, conv._pgrad);
    the first backward of a step overwrites, a second one in the same step (two forward passes: the phase5 Flip branch)
    accumulates.  No `p.grad += dw` launches, no layout copies.
  * FlatAdam.step(): ONE AdamW launch over the whole arena (weight_decay 0 = torch.optim.Adam's default; Adam's
    coupled L2 decay is not implemented; decoupled_weight_decay=True is torch.optim.AdamW), in torch's single-tensor update order; the 1/world average of a data-parallel sum
    folds into it (grad_scale).  zero_grad() sets .grad to None and launches nothing.
A torch.optim.Optimizer subclass: LR schedulers and the stock Adam state_dict layout ('step', 'exp_avg', 'exp_avg_sq' per
parameter) work unchanged; capturable=True keeps the step count on the device for train.GraphedModuleStep.
Every host call that writes a parameter or buffer through a raw pointer bumps the version counters of the tensors it wrote
(torch.autograd.graph.increment_version), so caches and backward-time checks key on `_version` (and `data_ptr`) alone.
"""
import torch
from torch.autograd.graph import increment_version

from . import _lib, gradclip
from .optim import FlatOptimizer


class ModuleArena:
    def __init__(self, module):
        params = [p for p in module.parameters()]
        if not params:
            raise ValueError("ModuleArena: the module has no parameters")
        dev = params[0].device
        if any(p.device != dev or p.dtype != torch.float32 for p in params):
            raise ValueError("ModuleArena: parameters must be float32 on one device (build it after .to(device))")
        _lib.require_device_tensor(params[0].data.contiguous(), "parameters")
        self.params, self.offsets = params, []
        off = 0
        for p in params:
            self.offsets.append(off)
            off += (p.numel() + 63) // 64 * 64
        self.numel = off
        self.flat = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(off, dtype=torch.float32, device=dev)
        for p, o in zip(params, self.offsets):
            view = self.flat[o:o + p.numel()].view(p.shape)
            view.copy_(p.data)
            p.data = view
            p.grad = None
            p._pl_grad = self.grad[o:o + p.numel()].view(p.shape)
        module._pl_arena = self

    def intact(self):
        """Every parameter still is its view of the arena (no .to() / .data reassignment since)."""
        base = self.flat.data_ptr()
        return all(p.data_ptr() == base + 4 * o for p, o in zip(self.params, self.offsets))

    def gather_grads(self):
        """Before the optimizer reads the gradient arena: a gradient some autograd node handed to autograd instead of writing
        it into the arena (an op outside conv.py) is copied in.  Returns the [lo, hi) arena ranges that hold a gradient."""
        runs = []
        for p, o in zip(self.params, self.offsets):
            g = p.grad
            if g is None:
                continue
            if g.data_ptr() != p._pl_grad.data_ptr():
                p._pl_grad.copy_(g)
                p.grad = p._pl_grad
            end = o + (p.numel() + 63) // 64 * 64
            if runs and runs[-1][1] == o:
                runs[-1] = (runs[-1][0], end)
            else:
                runs.append((o, end))
        return runs


def arena_of(module):
    a = getattr(module, "_pl_arena", None)
    if a is None or not a.intact():
        a = ModuleArena(module)
    return a


class FlatAdam(FlatOptimizer):
    """torch.optim.Adam(module.parameters(), lr, betas, eps) as one library launch over the module's flat arenas."""

    def __init__(self, module, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=False,
                 decoupled_weight_decay=False, max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=False):
        if weight_decay != 0.0 and not decoupled_weight_decay:
            raise NotImplementedError("FlatAdam: Adam's coupled L2 weight decay is not implemented (the reference uses 0); "
                                      "decoupled_weight_decay=True is AdamW")
        self.arena = a = arena_of(module)
        self._module = module
        super().__init__(a.params, dict(lr=lr, betas=betas, eps=eps, weight_decay=float(weight_decay),
                                        capturable=bool(capturable), decoupled_weight_decay=bool(decoupled_weight_decay),
                                        max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite,
                                        ema_decay=ema_decay, ema_warmup=ema_warmup))
        self._m, self._v = torch.zeros_like(a.flat), torch.zeros_like(a.flat)
        dev = a.flat.device
        # _t / _t_dev: ATTEMPTED steps, as in the base; taken = attempted - the clip record's skipped count
        self._t_dev = torch.zeros(1, dtype=torch.int64, device=dev)           # completed steps (capturable)
        self._lr_dev = gradclip.DeviceScalar(dev, lr)                         # what a capturable step reads its lr from
        step = self._t_dev if capturable else torch.tensor(0.0)
        self._step_tensor = step
        for p, o in zip(a.params, a.offsets):
            n = p.numel()
            self.state[p] = {"step": step, "exp_avg": self._m[o:o + n].view(p.shape), "exp_avg_sq": self._v[o:o + n].view(p.shape)}
        self._ema_bind()                 # (ema_decay: the EMA arena beside m and v, a copy of the parameters as they are now)

    def _arenas(self):
        return self.arena.flat, self.arena.grad

    def _param_offsets(self):
        return list(zip(self.arena.params, self.arena.offsets))

    def _ema_module(self):
        return self._module

    def _attempted_host(self):
        return int(self._t_dev.item()) if self.param_groups[0].get("capturable", False) else self._t

    def load_state_dict(self, state_dict):
        keep = self._ema_options()
        super().load_state_dict(state_dict)
        a = self.arena
        t = 0
        for p, o in zip(a.params, a.offsets):               # loaded tensors are copies: back into the arenas
            st, n = self.state[p], p.numel()
            mv, vv = self._m[o:o + n].view(p.shape), self._v[o:o + n].view(p.shape)
            if "exp_avg" in st:
                mv.copy_(st["exp_avg"]); vv.copy_(st["exp_avg_sq"])
                t = max(t, int(st["step"]))
            st["exp_avg"], st["exp_avg_sq"], st["step"] = mv, vv, self._step_tensor
        self._t = t
        self._step_tensor.fill_(t)
        self._forget_skipped()
        self._ema_after_load(keep)

    def state_dict(self):
        """'step' reports TAKEN steps (attempted - skipped); the live state keeps counting attempts (capturable: on the
        device, ticking inside the graph)."""
        sd = super().state_dict()
        k = self.skipped_steps()
        if k:
            taken = self._step_tensor - k
            for st in sd["state"].values():
                st["step"] = taken
        return sd

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        """The norm pass when max_grad_norm / skip_nonfinite are on, then one AdamW launch per run of parameters that hold a
        gradient (none anywhere: no launch).  The counters tick every attempt; the kernels subtract the record's skipped
        count.  capturable: t and lr are read on the device and the counter ticks behind the update."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_live("optimizer.step()")
        a, g = self.arena, self.param_groups[0]
        if not a.intact():
            raise _lib.PoseliftError("FlatAdam: the module's parameters left their arena (.to() / .data reassigned): "
                                     "build the optimizer after moving the module")
        runs = a.gather_grads()
        lr = g["lr"]
        wd = g["weight_decay"] if g.get("decoupled_weight_decay", False) else 0.0
        if g.get("capturable", False):
            # (a tensor lr: a device scalar the caller changes between replays)
            lr_ptr = lr.data_ptr() if torch.is_tensor(lr) else self._lr_dev.refresh(lr)
            self._launch_adamw(runs, 0.0, lr_ptr, 1, self._t_dev.data_ptr(), wd, grad_scale)
            with _lib.on_device(a.flat.device):
                _lib.check(_lib.lib().pl_counter_add(self._t_dev.data_ptr(), 1, _lib.current_stream_ptr()), "pl_counter_add")
        else:
            self._t += 1
            self._launch_adamw(runs, lr, None, self._t, None, wd, grad_scale)
            self._step_tensor.fill_(float(self._t))
        increment_version(a.params)
        return loss
