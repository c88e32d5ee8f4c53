"""Gradient-norm clipping and non-finite skip for the flat optimizers, decided on the device.

`nn.utils.clip_grad_norm(model.parameters(), max_norm=1)` between `loss.backward()` and `optimizer.step()`
(phase1_lifting/main.py:465-470, `MaxNormConctraint`) as two small launches in front of the AdamW launch: pl_grad_norm_clip
sums g^2 over the active ranges of the gradient arena in fp64 and writes a 24-byte device record (norm, coefficient, finite,
skip, skipped steps); the AdamW launch multiplies the coefficient into its gradient scale, counts t without the skipped
steps and leaves p, m, v untouched on a skipped step.  Nothing synchronises, so the same sequence is captured by
train.GraphedTrainStep / GraphedModuleStep.  The gradient arena is NOT rewritten: unlike clip_grad_norm_, `p.grad` keeps the
unclipped gradient.

GradClip is the state one optimizer keeps for this (optim.FlatOptimizer: FlatAdamW, arena.FlatAdam)."""
import torch

from . import _lib


def check_options(max_grad_norm, skip_nonfinite):
    if max_grad_norm is not None and not torch.is_tensor(max_grad_norm):     # (a device scalar is read on the device)
        if not float(max_grad_norm) >= 0.0:
            raise ValueError(f"max_grad_norm must be None or >= 0, got {max_grad_norm}")
    return max_grad_norm, bool(skip_nonfinite)


class DeviceScalar:
    """A float32 device scalar that captured launches read (lr, max_norm), with the value it holds cached on the host:
    refresh(value) returns its address, refilling it only when the value changed and never while a capture is under way (the
    captured launches then read what it already held)."""

    def __init__(self, device, value=None):
        self._host = None if value is None else float(value)
        self.tensor = torch.full((1,), self._host or 0.0, dtype=torch.float32, device=device)

    def refresh(self, value):
        v = float(value)
        if self._host != v and not torch.cuda.is_current_stream_capturing():
            self.tensor.fill_(v)
            self._host = v
        return self.tensor.data_ptr()


class GradClip:
    def __init__(self, device):
        self.device = device
        self.record = torch.zeros(6, dtype=torch.int32, device=device)       # PLClipRecord
        f = self.record.view(torch.float32)
        self.norm, self.coef = f[0], f[1]
        self._skipped = self.record.view(torch.int64)[2]
        self._scratch = None
        self._max_norm_dev = DeviceScalar(device)       # what the captured norm pass reads
        self._ranges, self._ranges_key = None, None

    @property
    def ptr(self):
        return self.record.data_ptr()

    def skipped(self):
        """Steps skipped so far (one host read)."""
        return int(self._skipped.item())

    def reset_skipped(self):
        self._skipped.zero_()

    def launch(self, grads, runs, grad_scale, max_norm, skip_nonfinite, from_device=False):
        """Enqueue the norm pass over `runs` ([lo, hi) floats of `grads`) on the current stream.  from_device: the captured
        form, max_norm read from a device scalar (refreshed here when it changed and no capture is under way)."""
        runs = tuple(runs)
        if not runs:
            return
        if len(runs) > _lib.GRAD_NORM_MAX_RANGES:
            raise _lib.PoseliftError(f"gradient clipping: {len(runs)} separate runs of parameters with a gradient "
                                     f"(at most {_lib.GRAD_NORM_MAX_RANGES})")
        if runs != self._ranges_key:
            self._ranges = (_lib.PLGradRange * len(runs))(*[_lib.PLGradRange(int(lo), int(hi)) for lo, hi in runs])
            self._ranges_key = runs
        L = _lib.lib()
        need = L.pl_grad_norm_scratch_bytes(len(runs))
        if self._scratch is None or self._scratch.numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.PoseliftError("gradient clipping: the set of parameters with a gradient grew during graph capture")
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        clip = max_norm is not None
        dev_ptr = None
        if clip and from_device:
            dev_ptr = max_norm.data_ptr() if torch.is_tensor(max_norm) else self._max_norm_dev.refresh(max_norm)
        rc = L.pl_grad_norm_clip(grads.data_ptr(), grads.numel(), self._ranges, len(runs), float(grad_scale), int(clip),
                                 float(max_norm) if clip and dev_ptr is None else 0.0, dev_ptr, int(bool(skip_nonfinite)),
                                 self.ptr, self._scratch.data_ptr(), _lib.current_stream_ptr())
        _lib.check(rc, "pl_grad_norm_clip")

    def refresh(self, max_norm):
        """Before a graph replay: bring the device scalar its captured norm pass reads up to date."""
        if max_norm is not None and not torch.is_tensor(max_norm):
            self._max_norm_dev.refresh(max_norm)
