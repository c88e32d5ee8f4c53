"""Range guard of the "f16x3" arithmetic (include/poselift.h pl_range_monitor).

"f16x3" stores activations, weights and conv-path feature maps as fp16 planes at STATIC scales, so a finite fp32 value beyond
65504 / scale becomes inf in its plane and NaN in the next GEMM where "fp32" / "bf16x6" stay finite.  With the guard enabled
every kernel that writes such a plane records, on the device, the largest value it saw leave the range, per site; the stored
planes are exactly what they are without it.  Nothing here synchronises but check():

    loss, pred = pl.train_step(model, opt, x, y)
    ...
    epoch_loss = float(loss)          # the sync the loop already has
    pl.range_guard.check()            # raises PoseliftRangeError naming the site, the magnitude, the limit and the remedy

The guard is OFF by default -- enable() / disable() per device -- because it is not free: enabled, the bench step at
B = 4096 measured 0.627 ms against 0.617 and the phase5 cycle step 92.3 ms against 91.7 ("f16x3 range guard").
One 64-byte int32 record per device lives as long as the process: the pointer is part of every captured graph.  The
library keeps the pointer per calling thread, so it is handed over again, before every launching call, on whatever
thread enqueues work (_lib.current_stream_ptr does that: every library call that launches asks it for its stream).
"""
import numpy as np
import torch

from . import _lib

SITES = 16                      # PL_RANGE_SITES
SITE_LIFTER_ACT = 0             # .. 7: hidden layer min(l, 7)
SITE_LIFTER_WEIGHT = 8
SITE_CONV_ACT = 9
SITE_CONV_WEIGHT = 10
SITE_SPLIT = 11
FP16_MAX = 65504.0
REMEDY = 'compute_dtype="bf16x6" or "fp32"'


class PoseliftRangeError(_lib.PoseliftError):
    """A tensor left the range of the "f16x3" operand planes; .sites = [(site, magnitude), ...]."""

    def __init__(self, msg, sites=()):
        super().__init__(msg)
        self.sites = list(sites)


def site_name(site):
    if SITE_LIFTER_ACT <= site < SITE_LIFTER_ACT + 7:
        return f"hidden activation of layer {site - SITE_LIFTER_ACT}"
    if site == SITE_LIFTER_ACT + 7:
        return "hidden activation of layer 7 or above"
    return {SITE_LIFTER_WEIGHT: "weight planes of the lifter's hidden Linear layers",
            SITE_CONV_ACT: "conv-path feature map",
            SITE_CONV_WEIGHT: "conv-path weight planes",
            SITE_SPLIT: "operand of a planes split with a caller-chosen scale"}.get(site, f"site {site}")


def site_limit(site):
    """Largest magnitude the planes of `site` hold: 65504 / scale (None: the scale is the caller's)."""
    if SITE_LIFTER_ACT <= site <= SITE_LIFTER_ACT + 7:
        return FP16_MAX
    return {SITE_LIFTER_WEIGHT: FP16_MAX / 16.0, SITE_CONV_ACT: FP16_MAX * 64.0, SITE_CONV_WEIGHT: FP16_MAX / 16.0}.get(site)


def flagged(record):
    """[(site, magnitude)] of the non-zero slots of a record (any 16 x 32-bit integer array: fp32 bit patterns)."""
    bits = np.ascontiguousarray(np.asarray(record)).astype(np.int64).astype(np.uint32)
    if bits.shape != (SITES,):
        raise ValueError(f"a range record has {SITES} slots, got shape {bits.shape}")
    mags = bits.view(np.float32)
    return [(s, float(mags[s])) for s in range(SITES) if bits[s]]


def describe(record):
    """The message check() raises with, or None for a clean record.  Pure: no device, no library."""
    hits = flagged(record)
    if not hits:
        return None
    lines = []
    for s, mag in hits:
        lim = site_limit(s)
        lim_txt = f"limit {lim:.6g}" if lim is not None else "limit 65504 / scale"
        lines.append(f"{site_name(s)}: magnitude {mag:.6g} reached, {lim_txt}")
    return ('"f16x3" range exceeded (the value became inf in its fp16 plane; "fp32" / "bf16x6" stay finite on this model) -- '
            + "; ".join(lines) + f".  Remedy: {REMEDY}.")


_records = {}                   # device index -> int32 [16] device tensor, never freed (captured graphs hold its address)
_state = {}                     # device index -> True / False (absent: never enabled)


def _index(device):
    if device is None:
        return torch.cuda.current_device()
    d = torch.device(device) if not isinstance(device, torch.device) else device
    if d.type != "cuda":
        raise _lib.PoseliftError(f"range_guard: {d} is not a GPU")
    return torch.cuda.current_device() if d.index is None else d.index


def _bind(idx):
    """Hand the calling thread's library state the record of device idx (or NULL).  Nothing is cached on this side: a
    direct pl_range_monitor call of the user's or another thread cannot leave the two out of step."""
    _lib.check(_lib.lib().pl_range_monitor(_records[idx].data_ptr() if _state.get(idx) else None), "pl_range_monitor")


def enable(device=None):
    idx = _index(device)
    if idx not in _records:
        _records[idx] = torch.zeros(SITES, dtype=torch.int32, device=torch.device("cuda", idx))
    _state[idx] = True
    _lib._range_bind = _bind
    if idx == torch.cuda.current_device():
        _bind(idx)


def disable(device=None):
    idx = _index(device)
    _state[idx] = False
    if _lib._range_bind is not None and idx == torch.cuda.current_device():
        _bind(idx)


def enabled(device=None):
    return bool(_state.get(_index(device)))


def status(device=None):
    """The record as a device tensor (int32 [16], fp32 bit patterns; no sync): read it in the same transfer as the loss."""
    idx = _index(device)
    if idx not in _records:
        raise _lib.PoseliftError(f"range_guard: never enabled on cuda:{idx}")
    return _records[idx]


def _zero(idx):
    if idx in _records:
        _records[idx].zero_()


def clear(device=None):
    _zero(_index(device))


def check(device=None, clear=True):
    """One device-to-host read of the record; raises PoseliftRangeError if any site overflowed, and zeroes the record."""
    idx = _index(device)
    if idx not in _records:
        return
    rec = _records[idx].cpu().numpy()
    msg = describe(rec)
    if msg is None:
        return
    if clear:                      # (the argument, as the interface names it: not the module's clear())
        _zero(idx)
    raise PoseliftRangeError(msg, flagged(rec))
