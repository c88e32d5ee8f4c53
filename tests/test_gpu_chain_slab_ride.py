"""The slab ride of the chained backward pair (csrc/gemm_planes16.h SLAB RIDE): the chained launch of hidden layer l sums the
four split-K slabs of layer l + 1's weight gradient on its loader waves, during dX's k-steps, instead of the backward's
closing reduce launch.

The ride exists where a layer leaves four slabs and the launch below it takes the hand-off form: H = 1024 at B = 4096
(pair_carries_slab_sum), the bench's shape and the smallest one.  num_stage = 1 (L = 3 hidden layers: chained launches for
layers 2 and 1, one ride) and the bench's num_stage = 2 (three rides).  The sums are the reduce launch's, bit for bit, so
the reference that cannot ride is the same backward cut at every layer boundary (pl_lifter_train_fwd_bwd with (hi, lo) per
layer): every range ends before the launch that would carry its slabs, and every slab sum is a reduce job."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import lifter_oracle as orc
from oracle import philox
from test_gpu_chain_handoff import _chain_forms, _make, _step_outputs
from test_gpu_parity import _close, _gpu_decisions, _grads
from test_gpu_planes import _gpu_kernel_names

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H = 4096, 1024
CASES = [(1, "f16x3"), (2, "f16x3"), (1, "bf16")]
IDS = [f"{dt}-S{S}" for S, dt in CASES]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


@pytest.fixture(scope="module")
def batch():
    g = torch.Generator().manual_seed(B + 1)
    return torch.rand(B, 34, generator=g).to(DEV), (torch.rand(B, 51, generator=g) - 0.5).to(DEV)


def _rides(pkg, m, rows, hi, lo):
    return pkg.lib().pl_lifter_bwd_slab_rides(ctypes.byref(m._desc), rows, hi, lo)


class _CutHere:
    """What fused_train_fwd_bwd needs of a gradient sync to cut the backward into its ranges; nothing is reduced."""

    def world(self):
        return 2

    def launch_bucket(self, grads):
        pass


def _fwd_bwd(pkg, S, dtype, p, x, t, cut):
    m, _ = _make(pkg, H, S, dtype, p)
    m.manual_seed(17, step=2)
    L = 1 + 2 * S
    sync = None
    if cut:
        sync = _CutHere()
        m.set_grad_sync(sync, cuts=list(range(L - 1, -1, -1)))
        assert [(hi, lo) for hi, lo, _, _ in m._bwd_ranges()] == [(L, L - 1)] + [(l, l) for l in range(L - 2, -1, -1)]
    loss, y = m.fused_train_fwd_bwd(x, t, sync=sync)
    torch.cuda.synchronize()
    return loss.clone(), y.clone(), m.flat_grads.clone()


@pytest.mark.parametrize("S,dtype", CASES, ids=IDS)
def test_the_ride_happens(pkg, S, dtype):
    m, _ = _make(pkg, H, S, dtype, 0.5)
    L = 1 + 2 * S
    assert _rides(pkg, m, B, L, 0) == L - 2                     # every hidden layer's slab sum but the lowest pair's
    assert _rides(pkg, m, B, L - 1, 0) == L - 2                 # (the output layer has no part in it)
    assert _rides(pkg, m, B, L, 1) == L - 2 and _rides(pkg, m, B, L, 2) == L - 3
    # a range cut between a layer and the one above it carries nothing across the cut
    assert _rides(pkg, m, B, L, L - 1) == 0
    for l in range(L):
        assert _rides(pkg, m, B, l, l) == 0
    # other batches: other slab counts, or no chain at all
    assert _rides(pkg, m, 2048, L, 0) == 0 and _rides(pkg, m, 8192, L, 0) == 0 and _rides(pkg, m, 64, L, 0) == 0
    # ten slabs (the hand-off form without a ride)
    m640, _ = _make(pkg, 640, S, dtype, 0.5)
    assert _rides(pkg, m640, 6400, L, 0) == 0


@pytest.mark.parametrize("p", [0.5, 0.0])
@pytest.mark.parametrize("S,dtype", CASES, ids=IDS)
def test_bitwise_against_the_cut_backward(pkg, batch, S, dtype, p):
    """One range (the sums ride) against the backward cut at every layer boundary (every sum a reduce job)."""
    x, t = batch
    L = 1 + 2 * S
    m, _ = _make(pkg, H, S, dtype, p)
    assert _rides(pkg, m, B, L, 0) == L - 2 and all(_rides(pkg, m, B, l, l) == 0 for l in range(L))
    whole, cut = _fwd_bwd(pkg, S, dtype, p, x, t, False), _fwd_bwd(pkg, S, dtype, p, x, t, True)
    for a, b, what in zip(whole, cut, ("loss", "y", "grads")):
        assert torch.equal(a, b), what
    assert torch.isfinite(whole[2]).all() and whole[2].abs().max() > 0


@pytest.mark.parametrize("S,dtype", CASES, ids=IDS)
def test_train_step_is_deterministic_and_graph_safe(pkg, batch, S, dtype):
    """One train step twice from the same state and once replayed from a graph: the ride adds no ordering race."""
    x, t = batch
    runs = []
    for how in ("eager", "eager", "graph"):
        m, opt = _make(pkg, H, S, dtype, 0.5)
        step = pkg.GraphedTrainStep(m, opt, x, t) if how == "graph" else (lambda a, b: pkg.train_step(m, opt, a, b))
        loss, y = step(x, t)
        torch.cuda.synchronize()
        runs.append(_step_outputs(m, opt, loss, y))
    for other in runs[1:]:
        for k, v in runs[0].items():
            assert torch.equal(v, other[k]), k
    assert torch.isfinite(runs[0]["grads"]).all()


def test_gradients_against_fp64(pkg, batch):
    """L = 3, f16x3: the autograd backward (one range: the ride) against the fp64-checked oracle on the device's own ReLU /
    dropout decisions, at the gates of test_gpu_chain_handoff.test_hand_off_train_step for the mode."""
    S, dtype, p = 1, "f16x3", 0.5
    x, t = batch
    L = 1 + 2 * S
    m, _ = _make(pkg, H, S, dtype, p)
    st = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
    xr = x.clone().requires_grad_(True)
    m.manual_seed(17, step=2)
    pred = m(xr)
    loss = pkg.mse_loss(pred, t)
    names = _gpu_kernel_names(loss.backward)
    assert _chain_forms(names) == {(True, True, True), (True, False, True)}, [n for n in names if "planes_gemm" in n]
    assert _rides(pkg, m, B, L, 0) == 1
    masks = [philox.dropout_keep_mask(17, 3, l, B, H, p) for l in range(L)]
    opred, cache = orc.forward(st, x.cpu().numpy(), num_stage=S, train=True, p_dropout=p, keep_masks=masks,
                               on_masks=_gpu_decisions(pkg, m, L, H))
    for c in cache["layers"]:
        d = c["on_disagree"]
        assert d.size <= 1e-3 * c["z"].size + 2 and (d.size == 0 or d.max() < 1e-3)
    oloss, dpred = orc.mse_loss(opred, t.cpu().numpy())
    ograds, odx = orc.backward(st, cache, dpred)
    tol = 2e-4
    scale = np.abs(opred).max()
    _close(pred.detach().cpu().numpy() / scale, opred / scale, 0, 2e-5)
    _close(loss.item(), oloss, 2e-5, 0)
    got = _grads(m)
    for k, v in ograds.items():
        if k.endswith(".bias") and "batch_norm" not in k and k != "w2.bias":
            continue                                                # zero-true-gradient biases: both sides are round-off
        rel = np.linalg.norm((got[k] - v).astype(np.float64)) / (np.linalg.norm(v.astype(np.float64)) + 1e-30)
        assert rel < tol, (k, rel)
    rel = np.linalg.norm((xr.grad.cpu().numpy() - odx).astype(np.float64)) / np.linalg.norm(odx.astype(np.float64))
    assert rel < tol, ("dx", rel)


@pytest.mark.parametrize("S,dtype", CASES[:1] + CASES[2:], ids=IDS[:1] + IDS[2:])
def test_non_finite_pattern(pkg, batch, S, dtype):
    """A NaN in one element of the target reaches the slab-producing operands (dz of every layer): the riding sums leave the
    same non-finite pattern, and the same finite values beside it, as the reduce jobs of the cut form."""
    x, t = batch
    t = t.clone()
    t[77, 5] = float("nan")
    whole, cut = _fwd_bwd(pkg, S, dtype, 0.5, x, t, False), _fwd_bwd(pkg, S, dtype, 0.5, x, t, True)
    gw, gc = whole[2], cut[2]
    assert not torch.isfinite(gw).all()
    assert torch.equal(torch.isnan(gw), torch.isnan(gc)) and torch.equal(torch.isinf(gw), torch.isinf(gc))
    fin = torch.isfinite(gw)
    assert torch.equal(gw[fin], gc[fin])
