"""Gradient clipping and non-finite skip, host side (no GPU): the numpy twin (tests/grad_clip_oracle.py) against
torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW / Adam on the CPU, the new C-ABI entry points' declarations, exports
and argument checks, and the optimizers' options.

EVERY library call in this file must fail in argument validation: the pointers are made-up addresses, a call with nothing
wrong would launch a kernel on them where there is a GPU (as tests/test_conv_planes_host.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import grad_clip_oracle as gco
from conftest import ROOT
from oracle.torch_twin import TwinLifter

EINVAL, ESHAPE = -1, -2
NEW = ["pl_grad_norm_scratch_bytes", "pl_grad_norm_clip", "pl_adamw_flat_clip", "pl_adamw_flat_dev_clip",
       "pl_adamw_flat_planes_clip"]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()


# ------------------------------------------------------------------------------------------------ the twin vs torch
def _arena_of(model):
    """(offsets, arena length) of a torch module's parameters laid end to end at 4-float aligned offsets."""
    offs, off = [], 0
    for p in model.parameters():
        offs.append(off)
        off += (p.numel() + 3) // 4 * 4
    return offs, off


def _flat(model, offs, n, what):
    out = np.zeros(n, np.float32)
    for p, o in zip(model.parameters(), offs):
        t = p.data if what == "p" else p.grad
        if t is not None:
            out[o:o + p.numel()] = t.detach().numpy().reshape(-1)
    return out


def _runs(model, offs):
    runs = []
    for p, o in zip(model.parameters(), offs):
        if p.grad is None:
            continue
        end = o + (p.numel() + 3) // 4 * 4
        if runs and runs[-1][1] == o:
            runs[-1] = (runs[-1][0], end)
        else:
            runs.append((o, end))
    return runs


# largest |twin norm / torch norm - 1| seen over the steps below (CPU, torch 2.x): written by hand from the printed figure
NORM_REL_MEASURED = 8.4e-8


@pytest.mark.parametrize("kind,bn", [("adamw", True), ("adamw", False), ("adam", True)])
def test_twin_matches_torch_clip_grad_norm_and_adamw_over_4_steps(kind, bn):
    """4 steps of a small LinearModel twin (linear_size 64, B = 8) with clipping binding; on step 3 the target holds one inf
    and the torch loop does not call step().  The twin is fed torch's own gradients each step, so only the norm, the
    coefficient and the update are compared.  BN=False: the BatchNorm parameters get no gradient (several runs).

    Norms: the twin accumulates in fp64, torch in fp32 per tensor and again over the stack; they differ by fp32 summation
    error.  Measured here: largest relative difference 8.4e-8 (8.39e-8, 8.02e-8 and 7.25e-8 in the three cases, 0 on the other
    steps; 3 finite steps each); gated at 4x that.
    Parameters and moments: the bound tests/test_gpu_parity.py::test_flat_adamw_matches_oracle_and_torch_state_layout uses."""
    torch.manual_seed(3)
    model = TwinLifter(34, 51, linear_size=64, num_stage=2, p_dropout=0.0, BN=bn).train()
    offs, n = _arena_of(model)
    lr, wd = 1e-3, (0.02 if kind == "adamw" else 0.0)
    opt = (torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=wd) if kind == "adamw"
           else torch.optim.Adam(model.parameters(), lr=lr))
    g = torch.Generator().manual_seed(0)
    x, y = torch.rand(8, 17, 2, generator=g), torch.randn(8, 17, 3, generator=g)
    # max_norm below the first step's norm, read once from the twin
    opt.zero_grad()
    torch.nn.functional.mse_loss(model(x).reshape(8, 17, 3), y).backward()
    first = float(gco.grad_norm(_flat(model, offs, n, "g"), _runs(model, offs)))
    max_norm = 0.25 * first
    twin = gco.ClipAdamW(_flat(model, offs, n, "p"), lr=lr, weight_decay=wd, max_grad_norm=max_norm, skip_nonfinite=True)
    worst = 0.0
    for it in range(1, 5):
        yy = y.clone()
        if it == 3:
            yy[2, 5, 1] = float("inf")
        opt.zero_grad()
        torch.nn.functional.mse_loss(model(x).reshape(8, 17, 3), yy).backward()
        gflat, runs = _flat(model, offs, n, "g"), _runs(model, offs)
        assert (len(runs) > 1) == (not bn)
        total = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
        took = twin.step(gflat, runs)
        assert took == bool(torch.isfinite(total)) == (it != 3)
        if took:
            opt.step()
            rel = abs(float(twin.norm) / float(total) - 1.0)
            print(f"{kind} bn={bn} step {it}: twin norm {float(twin.norm):.9g} torch {float(total):.9g} rel {rel:.3g} "
                  f"coef {float(twin.coef):.6g}")
            worst = max(worst, rel)
            assert twin.coef < 1.0
        np.testing.assert_allclose(twin.p, _flat(model, offs, n, "p"), rtol=1e-6, atol=1e-8)
    assert worst <= 4 * NORM_REL_MEASURED, worst
    assert twin.t == 3 and twin.skipped == 1
    st = opt.state[next(model.parameters())]
    assert float(st["step"]) == 3.0
    mflat = np.zeros(n, np.float32)
    for p, o in zip(model.parameters(), offs):
        if p in opt.state:
            mflat[o:o + p.numel()] = opt.state[p]["exp_avg"].numpy().reshape(-1)
    np.testing.assert_allclose(twin.m, mflat, rtol=1e-6, atol=1e-9)


def test_twin_norm_and_coefficient_edges():
    g = np.array([3.0, 4.0, np.nan, 1e19, 0.0, 0.0, 0.0, 0.0, 1e19], np.float32)
    assert gco.grad_norm(g, [(0, 2)]) == np.float32(5.0)
    assert gco.grad_norm(g, [(0, 2)], grad_scale=-0.5) == np.float32(2.5)
    assert np.isnan(gco.grad_norm(g, [(0, 3)]))
    big = gco.grad_norm(g, [(3, 4), (8, 9)])                          # an fp32 square would overflow
    assert np.isfinite(big) and abs(float(big) / (1e19 * 2 ** 0.5) - 1) < 1e-6
    assert gco.grad_norm(g, [(4, 8)]) == 0 and gco.clip_coef(np.float32(0), 1.0) == np.float32(1.0)
    assert gco.clip_coef(np.float32(5), None) == 1 and gco.clip_coef(np.float32(5), 1e30) == 1
    assert gco.clip_coef(np.float32(np.inf), 1.0) == 0 and np.isnan(gco.clip_coef(np.float32(np.nan), 1.0))
    want = torch.clamp(torch.tensor(1.0) / (torch.tensor(5.0) + 1e-6), max=1.0)
    assert gco.clip_coef(np.float32(5), 1.0) == want.numpy()


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_and_library_exports_the_clip_entry_points(pkg):
    header = open(os.path.join(ROOT, "include", "poselift.h")).read()
    declared = set(re.findall(r"\b(pl_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in pkg._lib.SIGNATURES and hasattr(raw, name), name
    assert "typedef struct PLClipRecord" in header
    assert ctypes.sizeof(pkg._lib.PLClipRecord) == 24 and pkg._lib.PLClipRecord.skipped.offset == 16
    L = pkg.lib()
    assert L.pl_grad_norm_scratch_bytes(1) > 0 and L.pl_grad_norm_scratch_bytes(0) == 0
    assert L.pl_grad_norm_scratch_bytes(pkg._lib.GRAD_NORM_MAX_RANGES + 1) == 0
    assert L.pl_grad_norm_scratch_bytes(65) == 2 * L.pl_grad_norm_scratch_bytes(64)


one, odd, word = ctypes.c_void_p(16), ctypes.c_void_p(24), ctypes.c_void_p(20)   # 16-, 8- and 4-byte aligned made-up addresses


def _fail(L, name, *args):
    rc, msg = getattr(L, name)(*args), L.pl_last_error()
    assert rc != 0 and msg.startswith(b"pl_adamw_flat"), (name, rc, msg)      # (the three names share adamw_launch's checks)
    return rc, msg


def test_grad_norm_entry_rejects_bad_arguments_before_any_launch(pkg):
    L, R = pkg.lib(), pkg._lib.PLGradRange

    def norm(g=one, n=1024, ranges=((0, 1024),), nranges=None, gscale=1.0, clip=1, max_norm=1.0, max_dev=None, skip=0,
             rec=one, scratch=one):
        arr = (R * max(1, len(ranges)))(*[R(lo, hi) for lo, hi in ranges]) if ranges is not None else None
        rc, msg = L.pl_grad_norm_clip(g, n, arr, len(ranges) if nranges is None else nranges, gscale, clip, max_norm, max_dev,
                                      skip, rec, scratch, None), L.pl_last_error()
        assert rc != 0 and msg.startswith(b"pl_grad_norm_clip:"), (rc, msg)
        return rc, msg

    for kw in (dict(g=None), dict(ranges=None, nranges=1), dict(rec=None), dict(scratch=None)):
        rc, msg = norm(**kw)
        assert rc == EINVAL and b"null" in msg, (kw, msg)
    for kw in (dict(g=odd), dict(rec=word), dict(scratch=word)):
        rc, msg = norm(**kw)
        assert rc == EINVAL and b"misaligned" in msg, (kw, msg)
    for kw in (dict(nranges=0), dict(nranges=-1), dict(nranges=pkg._lib.GRAD_NORM_MAX_RANGES + 1), dict(n=0)):
        rc, msg = norm(**kw)
        assert rc == ESHAPE and b"nranges" in msg, (kw, msg)
    for ranges in (((2, 1024),), ((0, 8), (9, 16)), ((0, 8), (13, 14))):
        rc, msg = norm(ranges=ranges)
        assert rc == EINVAL and b"misaligned range" in msg, (ranges, msg)
    for ranges in (((0, 1025),), ((8, 8),), ((-4, 8),), ((8, 16), (0, 4)), ((0, 10), (8, 16))):
        rc, msg = norm(ranges=ranges)
        assert rc == ESHAPE and b"range" in msg, (ranges, msg)
    for m in (-1.0, float("nan"), -0.001):
        rc, msg = norm(max_norm=m)
        assert rc == EINVAL and b"max_norm" in msg, (m, msg)


def test_adamw_clip_forms_share_the_checks_of_the_plain_ones(pkg):
    L = pkg.lib()
    P = pkg._lib.PLAdamWPlanes
    hp = (0.9, 0.999, 1e-8, 0.01)
    for p, g, m, v in ((None, one, one, one), (one, None, one, one), (one, one, None, one), (one, one, one, None)):
        assert _fail(L, "pl_adamw_flat_clip", p, g, m, v, 64, 1e-3, *hp, 1, 1.0, one, None)[0] == EINVAL
        assert _fail(L, "pl_adamw_flat_dev_clip", p, g, m, v, 64, one, *hp, 0, one, 1.0, one, None)[0] == EINVAL
        assert _fail(L, "pl_adamw_flat_planes_clip", p, g, m, v, 64, 1e-3, None, *hp, 1, None, 1.0, None, one, None)[0] == EINVAL
    assert _fail(L, "pl_adamw_flat_clip", one, one, one, one, 0, 1e-3, *hp, 1, 1.0, one, None)[0] == ESHAPE       # n
    assert _fail(L, "pl_adamw_flat_clip", one, one, one, one, 64, 1e-3, *hp, 0, 1.0, one, None)[0] == ESHAPE      # t
    rc, msg = _fail(L, "pl_adamw_flat_clip", one, one, one, one, 64, 1e-3, *hp, 1, 1.0, word, None)
    assert rc == EINVAL and b"clip record" in msg
    assert _fail(L, "pl_adamw_flat_dev_clip", one, one, one, one, 64, None, *hp, 0, one, 1.0, one, None)[0] == EINVAL
    assert _fail(L, "pl_adamw_flat_dev_clip", one, one, one, one, 64, one, *hp, 0, None, 1.0, one, None)[0] == EINVAL
    rc, msg = _fail(L, "pl_adamw_flat_planes_clip", one, one, one, one, 64, 1e-3, one, *hp, 1, None, 1.0, None, one, None)
    assert rc == EINVAL and b"go together" in msg
    bad = P(nseg=1, kind=3, scale=16.0)
    rc, msg = _fail(L, "pl_adamw_flat_planes_clip", one, one, one, one, 64, 1e-3, None, *hp, 1, None, 1.0, ctypes.byref(bad),
                    one, None)
    assert rc == EINVAL and b"plane description" in msg


# ------------------------------------------------------------------------------------------------ the optimizers' options
def test_flat_adamw_options_live_in_param_groups_and_default_to_off(pkg):
    m = pkg.LinearModel(34, 51, linear_size=64)
    opt = pkg.FlatAdamW(m)
    g = opt.param_groups[0]
    assert g["max_grad_norm"] is None and g["skip_nonfinite"] is False and not opt._clipping()
    assert opt.skipped_steps() == 0
    opt = pkg.FlatAdamW(m, max_grad_norm=1, skip_nonfinite=True)
    assert opt.param_groups[0]["max_grad_norm"] == 1 and opt._clipping()
    opt.param_groups[0]["max_grad_norm"] = None
    assert opt._clipping()                                              # skip-only
    opt.param_groups[0]["skip_nonfinite"] = False
    assert not opt._clipping()
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            pkg.FlatAdamW(m, max_grad_norm=bad)
    # a checkpoint written before these options existed (or by the stock optimizer) loads, and leaves them off
    opt = pkg.FlatAdamW(m, max_grad_norm=None)
    opt.load_state_dict(torch.optim.AdamW(m.parameters(), lr=1e-3).state_dict())
    assert not opt._clipping() and opt.skipped_steps() == 0
