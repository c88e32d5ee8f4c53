"""The chained backward pair with dX's epilogue handed to the loader waves (csrc/gemm_planes16.h HAND-OFF, gemm_planes.hip
ChainHand): the hidden layers' backward at the smallest lifter shape that takes it and at the bench's.

launch_gemm_planes_pair chains when there are as many dX tiles as dW items -- (B / 128)(H / 128) = (H / 128)^2 tn_splits, i.e.
B = H x splits, every dW K slice H long -- and hands the epilogue off from nk1 = H / 32 >= 20 k-steps per slice on
(pair_route, kChainMinNk1): H = 640 with B = 6400 (25 tiles, 10 slices, nk1 = 20: exactly the bound) is the smallest shape
the public API reaches; H = 256 x B = 256 x splits chains with the epilogue on the computing waves, as before (nk1 = 8).
Next to it H = 1024, B = 4096 (nk1 = 32), once.  Odd hidden layers carry the skip-gradient addend, even ones do not: every
model here launches both forms, and the kernel names say so."""
import re

import numpy as np
import pytest
import torch

from oracle import lifter_oracle as orc
from oracle import philox
from test_gpu_parity import _close, _gpu_decisions, _grads
from test_gpu_planes import _gpu_kernel_names

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


def _chain_forms(names):
    """(HAND, ADD, BNR) of every planes_gemm_chain_kernel<MODE, HAND, ADD, BNR> among kernel names, demangled or not"""
    forms = set()
    for n in names:
        m = re.search(r"planes_gemm_chain_kernel<\(?[\w:]*\)?\d+, (true|false), (true|false), (true|false)>", n)
        if m:
            forms.add(tuple(g == "true" for g in m.groups()))
        m = re.search(r"planes_gemm_chain_kernelILi\d+ELb([01])ELb([01])ELb([01])E", n)
        if m:
            forms.add(tuple(g == "1" for g in m.groups()))
    return forms


def _make(pkg, H, S, dtype, p):
    torch.manual_seed(1000 * S + H)
    m = pkg.LinearModel(34, 51, linear_size=H, num_stage=S, p_dropout=p, BN=True, compute_dtype=dtype).to(DEV).train()
    m.manual_seed(99, step=0)
    return m, pkg.FlatAdamW(m, lr=1e-3)


def _step_outputs(m, opt, loss, y):
    return dict(loss=loss.clone(), y=y.clone(), grads=m.flat_grads.clone(), params=m.flat_params.clone(),
                bn_running=m._bn_running.clone(), bn_batches=m._bn_batches.clone(), m=opt._m.clone(), v=opt._v.clone())


CASES = [(6400, 640, 1, dt, p) for dt in ("f16x3", "bf16") for p in (0.5, 0.0)] + [(4096, 1024, 2, "f16x3", 0.5)]


@pytest.mark.parametrize("B,H,S,dtype,p", CASES, ids=[f"{dt}-{B}x{H}-S{S}-p{p}" for B, H, S, dt, p in CASES])
def test_hand_off_train_step(pkg, B, H, S, dtype, p):
    """One train step twice from the same state and once replayed from a graph: loss, prediction, every gradient, the
    parameters after AdamW, its moments and the BatchNorm buffers identical across the three (the hand-off adds no ordering
    race); then the same backward through autograd against the fp64-checked oracle on the device's own ReLU / dropout
    decisions, at the gates of test_gpu_parity.test_ragged_shapes_vs_oracle for the mode."""
    g = torch.Generator().manual_seed(B)
    x = torch.rand(B, 34, generator=g).to(DEV)
    t = (torch.rand(B, 51, generator=g) - 0.5).to(DEV)
    runs = []
    for how in ("eager", "eager", "graph"):
        m, opt = _make(pkg, H, S, dtype, p)
        step = pkg.GraphedTrainStep(m, opt, x, t) if how == "graph" else (lambda a, b: pkg.train_step(m, opt, a, b))
        loss, y = step(x, t)
        torch.cuda.synchronize()
        runs.append(_step_outputs(m, opt, loss, y))
    for other in runs[1:]:
        for k, v in runs[0].items():
            assert torch.equal(v, other[k]), k
    assert torch.isfinite(runs[0]["grads"]).all()

    m, _ = _make(pkg, H, S, dtype, p)
    st = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
    xr = x.clone().requires_grad_(True)
    m.manual_seed(17, step=2)
    pred = m(xr)
    loss = pkg.mse_loss(pred, t)
    names = _gpu_kernel_names(loss.backward)
    # the hand-off form ran, with the skip-gradient addend (odd layers) and without (even layers), BatchNorm pass 1 in both
    assert _chain_forms(names) == {(True, True, True), (True, False, True)}, [n for n in names if "planes_gemm" in n]
    L = 1 + 2 * S
    masks = [philox.dropout_keep_mask(17, 3, l, B, H, p) for l in range(L)] if p > 0 else None
    xn = x.cpu().numpy()
    opred, cache = orc.forward(st, xn, num_stage=S, train=True, p_dropout=p, keep_masks=masks,
                               on_masks=_gpu_decisions(pkg, m, L, H))
    bf = dtype == "bf16"
    for c in cache["layers"]:
        d = c["on_disagree"]
        assert d.size <= (0.02 if bf else 1e-3) * c["z"].size + 2 and (d.size == 0 or d.max() < (0.2 if bf else 1e-3))
    oloss, dpred = orc.mse_loss(opred, t.cpu().numpy())
    ograds, odx = orc.backward(st, cache, dpred)
    tol = 8e-2 if bf else 2e-4
    scale = np.abs(opred).max()
    _close(pred.detach().cpu().numpy() / scale, opred / scale, 0, 3e-2 if bf else 2e-5)
    _close(loss.item(), oloss, 2e-2 if bf else 2e-5, 0)
    got = _grads(m)
    for k, v in ograds.items():
        if k.endswith(".bias") and "batch_norm" not in k and k != "w2.bias":
            continue                                                # zero-true-gradient biases: both sides are round-off
        rel = np.linalg.norm((got[k] - v).astype(np.float64)) / (np.linalg.norm(v.astype(np.float64)) + 1e-30)
        assert rel < tol, (k, rel)
    rel = np.linalg.norm((xr.grad.cpu().numpy() - odx).astype(np.float64)) / np.linalg.norm(odx.astype(np.float64))
    assert rel < tol, ("dx", rel)
