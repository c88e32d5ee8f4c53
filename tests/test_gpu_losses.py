"""GPU tests of the loss and metric reductions (pl_mse_fwd_bwd, pl_l1_terms_fwd_bwd, pl_mpjpe_accum) at the edges of
their launchers -- one element, one short of / one past a workgroup, one past the grid caps (1024 workgroups for MSE, a
fixed 64 for L1, 256 row chunks for MPJPE), more joints than the 64-thread MPJPE workgroup -- against numpy in fp64 on
the same fp32 inputs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rel(got, want):
    return np.abs(np.asarray(got, np.float64) - want) / np.abs(want)


@pytest.mark.parametrize("scale", [1.0, 1e3])
@pytest.mark.parametrize("n", [1, 3, 255, 257, 1024 * 4 + 1, 1024 * 1024 + 3])
def test_mse_loss_and_gradient_vs_fp64(pkg, n, scale):
    """Loss to 1e-5 relative: positive terms, a chain of at most five fmas per thread (1024 * 1024 + 3 elements over the
    capped 1024 x 256 threads), then fixed tree sums -- a few tens of 2^-24 at worst.  dpred to 2 ulp of 2 (p - t) / n:
    three roundings (the difference, 2 / n, their product) of half an ulp each."""
    rng = np.random.default_rng(n)
    p = (rng.standard_normal(n) * scale).astype(np.float32)
    t = (rng.standard_normal(n) * scale).astype(np.float32)
    pd = _t(p).requires_grad_(True)
    loss = pkg.mse_loss(pd, _t(t))
    loss.backward()
    d = p.astype(np.float64) - t.astype(np.float64)
    want = (d * d).mean()
    err = float(_rel(loss.item(), want))
    dwant = 2.0 * d / n
    ulps = np.abs(pd.grad.cpu().numpy().astype(np.float64) - dwant) / np.spacing(np.abs(dwant).astype(np.float32)).astype(np.float64)
    print(f"n={n} scale={scale}: loss rel err {err:.2e}, dpred max {ulps.max():.2f} ulp")
    assert err <= 1e-5
    assert ulps.max() <= 2.0


@pytest.mark.parametrize("scale", [1.0, 1e3])
def test_l1_terms_values_and_gradients_vs_fp64(pkg, scale):
    """Six terms in one launch: 1 and 63 elements (most of the 64 workgroups idle), one short of and one past a full sweep of
    the grid (64 x 256), 100 003 (seven sweeps, a tail) and 2; gradients asked for a only, b only, both and neither; one
    term with a == b at some elements.  Values to 1e-5 relative, gradients exactly +-1/n (fp32) or 0."""
    sizes = [1, 63, 64 * 256 - 1, 64 * 256 + 1, 100_003, 2]
    needs = [(True, False), (False, True), (True, True), (False, False), (True, True), (False, True)]
    rng = np.random.default_rng(7)
    A = [(rng.standard_normal(n) * scale).astype(np.float32) for n in sizes]
    Bs = [(rng.standard_normal(n) * scale).astype(np.float32) for n in sizes]
    Bs[4][::3] = A[4][::3]                                   # |a - b| = 0: the gradient there is exactly 0
    Bs[1][5] = A[1][5]
    ta = [_t(a).requires_grad_(na) for a, (na, _) in zip(A, needs)]
    tb = [_t(b).requires_grad_(nb) for b, (_, nb) in zip(Bs, needs)]
    losses = pkg.losses.l1_terms(*zip(ta, tb))
    losses.sum().backward()
    got = losses.detach().cpu().numpy()
    for k, n in enumerate(sizes):
        d = A[k].astype(np.float64) - Bs[k].astype(np.float64)
        err = float(_rel(got[k], np.abs(d).mean()))
        print(f"term {k} n={n} scale={scale}: rel err {err:.2e}")
        assert err <= 1e-5, (k, n)
        g = np.sign(d).astype(np.float32) * (np.float32(1.0) / np.float32(n))
        for tensor, need, sign in ((ta[k], needs[k][0], 1.0), (tb[k], needs[k][1], -1.0)):
            if need:
                assert np.array_equal(tensor.grad.cpu().numpy(), np.float32(sign) * g + np.float32(0.0)), (k, n, sign)
            else:
                assert tensor.grad is None
    assert (ta[4].grad.cpu().numpy()[::3] == 0).all() and (tb[4].grad.cpu().numpy()[::3] == 0).all()


@pytest.mark.parametrize("scale", [1.0, 1e3])
@pytest.mark.parametrize("J", [17, 70])
@pytest.mark.parametrize("B", [1, 63, 65, 64 * 256 + 1])
def test_mpjpe_accum_vs_fp64(pkg, B, J, scale):
    """(J,) sums over the batch of per-joint L2 errors to 1e-5 relative; a second call with out= accumulates."""
    rng = np.random.default_rng(B * 100 + J)
    p = (rng.standard_normal((B, J, 3)) * scale).astype(np.float32)
    t = (rng.standard_normal((B, J, 3)) * scale).astype(np.float32)
    want = np.sqrt(((p.astype(np.float64) - t.astype(np.float64)) ** 2).sum(-1)).sum(0)
    metric = pkg.loss_MPJPE(_t(p), _t(t))
    assert metric.shape == (J,)
    e1 = _rel(metric.cpu().numpy(), want).max()
    back = pkg.loss_MPJPE(_t(p[::-1].copy()), _t(t[::-1].copy()), out=metric)
    assert back is metric
    e2 = _rel(metric.cpu().numpy(), 2 * want).max()
    print(f"B={B} J={J} scale={scale}: rel err {e1:.2e}, accumulated {e2:.2e}")
    assert e1 <= 1e-5 and e2 <= 1e-5
