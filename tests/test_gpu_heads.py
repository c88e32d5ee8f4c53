"""GPU tests of the fused softmax + soft-argmax heads against the numpy oracle
(oracle/heads_oracle.py, restated from the reference text -- parity unpinned, see its header) and
against a plain torch fp32 evaluation of the same formulas (autograd for the backward)."""
import numpy as np
import pytest
import torch

from oracle import heads_oracle as ho

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()


def _torch_ref(out, J, D, centred):
    B, C, H, W = out.shape
    hm = torch.softmax(out.reshape(B, J, -1), 2)
    hm = (hm / hm.sum(2, keepdim=True)).reshape(B, J, D, H, W)
    cx = (hm.sum((2, 3)) * torch.arange(W, dtype=out.dtype, device=out.device)).sum(2, keepdim=True)
    cy = (hm.sum((2, 4)) * torch.arange(H, dtype=out.dtype, device=out.device)).sum(2, keepdim=True)
    if centred:
        cz = (hm.sum((3, 4)) * torch.arange(D, dtype=out.dtype, device=out.device)).sum(2, keepdim=True)
        c = torch.cat(((cx / W - 0.5) * 2, (cy / H - 0.5) * 2, (cz / D - 0.5) * 2), 2)
    else:
        c = torch.cat((cx / W, cy / H), 2)
    return c.reshape(B, -1)


@pytest.mark.parametrize("B,D,H,W,scale", [(2, 64, 64, 64, 1.0), (3, 64, 64, 64, 12.0), (5, 8, 16, 32, 4.0),
                                           (1, 64, 64, 64, 60.0)])
def test_soft_argmax_3d(pkg, B, D, H, W, scale):
    torch.manual_seed(B + D)
    J = 17
    out = (torch.randn(B, J * D, H, W) * scale)
    out[0, 5 * D + 3, 7, 9] += 40.0                      # one sharp peak: online-softmax rescale path
    x = out.to(DEV).requires_grad_(True)
    c = pkg.soft_argmax_3d(x, J, D)
    want = ho.soft_argmax(out.numpy(), J, D, True)
    np.testing.assert_allclose(c.detach().cpu().numpy(), want, rtol=0, atol=2e-5)
    assert c.shape == (B, J * 3) and float(c.detach().abs().max()) <= 1.0
    g = torch.randn(B, J * 3)
    c.backward(g.to(DEV))
    xr = out.double().requires_grad_(True)
    _torch_ref(xr, J, D, True).backward(g.double())
    ref = xr.grad.numpy()
    got = x.grad.cpu().numpy()
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max() + 1e-12


@pytest.mark.parametrize("B,H,W", [(4, 64, 64), (1, 32, 48)])
def test_soft_argmax_2d(pkg, B, H, W):
    torch.manual_seed(B)
    J = 17
    out = torch.randn(B, J, H, W) * 5
    x = out.to(DEV).requires_grad_(True)
    c = pkg.soft_argmax_2d(x, J)
    np.testing.assert_allclose(c.detach().cpu().numpy(), ho.soft_argmax(out.numpy(), J, 1, False), rtol=0, atol=2e-5)
    assert float(c.detach().min()) >= 0.0 and float(c.detach().max()) <= 1.0
    g = torch.randn(B, J * 2)
    c.backward(g.to(DEV))
    xr = out.double().requires_grad_(True)
    _torch_ref(xr, J, 1, False).backward(g.double())
    assert np.abs(x.grad.cpu().numpy() - xr.grad.numpy()).max() <= 1e-5 * xr.grad.abs().max().item() + 1e-12


def test_soft_argmax_properties_and_errors(pkg):
    J, D = 17, 64
    # a delta at voxel (d, h, w) puts the expectation exactly there
    out = torch.full((1, J * D, 64, 64), -1e4)
    out[0, 2 * D + 10, 20, 30] = 0.0
    c = pkg.soft_argmax_3d(out.to(DEV), J, D).cpu().reshape(J, 3)
    assert torch.allclose(c[2], torch.tensor([(30 / 64 - 0.5) * 2, (20 / 64 - 0.5) * 2, (10 / 64 - 0.5) * 2]), atol=1e-6)
    # shift invariance of softmax; uniform logits -> centre of the index range
    u = pkg.soft_argmax_3d(torch.zeros(1, J * D, 64, 64, device=DEV) + 3.0, J, D)
    assert torch.allclose(u, torch.full_like(u, (31.5 / 64 - 0.5) * 2), atol=1e-6)
    with pytest.raises(ValueError):
        pkg.soft_argmax_3d(torch.zeros(1, 17 * 63, 64, 64, device=DEV))
    with pytest.raises(pkg.PoseliftError):
        pkg.soft_argmax_2d(torch.zeros(1, 17, 64, 64))              # CPU tensor: no fallback


def test_soft_argmax_3d_nhwc_matches_the_nchw_kernel_and_oracle(pkg):
    """The NHWC-layout forward (what the conv path's final layer writes) against the NCHW kernel and the oracle."""
    from oracle import heads_oracle
    torch.manual_seed(5)
    x = torch.randn(3, 1088, 16, 24) * 3
    want = heads_oracle.soft_argmax(x.double().numpy(), 17, 64, True)
    got = pkg.soft_argmax_3d_nhwc(x.permute(0, 2, 3, 1).contiguous().to(DEV)).cpu().numpy()
    ref = pkg.soft_argmax_3d(x.to(DEV)).cpu().numpy()
    assert np.abs(got - want).max() < 2e-5 and np.abs(got - ref).max() < 2e-5


def test_soft_argmax_3d_nhwc_backward_vs_torch_autograd(pkg):
    """dlogits of the NHWC head against torch autograd (fp64) of the stated softmax + expectation, and against the
    NCHW kernel's backward on the same logits."""
    torch.manual_seed(6)
    B, J, D, H, W = 2, 17, 64, 12, 8
    x = torch.randn(B, J * D, H, W) * 2
    g = torch.randn(B, J * 3)
    xr = x.double().requires_grad_(True)
    hm = torch.softmax(xr.reshape(B, J, -1), 2).reshape(B, J, D, H, W)
    cx = (hm.sum((2, 3)) * torch.arange(W, dtype=torch.float64)).sum(2, keepdim=True)
    cy = (hm.sum((2, 4)) * torch.arange(H, dtype=torch.float64)).sum(2, keepdim=True)
    cz = (hm.sum((3, 4)) * torch.arange(D, dtype=torch.float64)).sum(2, keepdim=True)
    pred = torch.cat(((cx / W - .5) * 2, (cy / H - .5) * 2, (cz / D - .5) * 2), 2).reshape(B, J * 3)
    (pred * g.double()).sum().backward()
    xn = x.permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
    out = pkg.soft_argmax_3d_nhwc(xn)
    assert float((out.detach().cpu().double() - pred.detach()).abs().max()) < 2e-5
    (out * g.to(DEV)).sum().backward()
    want = xr.grad.permute(0, 2, 3, 1)
    scale = float(want.abs().max())
    assert float((xn.grad.cpu().double() - want).abs().max()) < 2e-5 * scale
    xc = x.to(DEV).requires_grad_(True)
    (pkg.soft_argmax_3d(xc) * g.to(DEV)).sum().backward()
    assert float((xn.grad.permute(0, 3, 1, 2) - xc.grad).abs().max()) < 2e-6 * scale


# ---------------------------------------------------------------------------- -inf logits, maps smaller than the workgroup
NEG = float("-inf")


def _check_nchw(pkg, out, J, D, centred, seed):
    """Forward (2e-5, oracle) and backward (1e-5 of the largest gradient, torch autograd in fp64; exactly 0 where the
    logit is -inf) of the NCHW kernels on `out` (B, J*D, H, W)."""
    B = out.shape[0]
    nc = 3 if centred else 2
    x = out.to(DEV).requires_grad_(True)
    c = pkg.soft_argmax_3d(x, J, D) if centred else pkg.soft_argmax_2d(x, J)
    got_c = c.detach().cpu().numpy()
    assert np.isfinite(got_c).all()
    np.testing.assert_allclose(got_c, ho.soft_argmax(out.numpy(), J, D, centred), rtol=0, atol=2e-5)
    g = torch.randn(B, J * nc, generator=torch.Generator().manual_seed(seed))
    c.backward(g.to(DEV))
    xr = out.double().requires_grad_(True)
    cr = _torch_ref(xr, J, D, centred)
    np.testing.assert_allclose(got_c, cr.detach().numpy(), rtol=0, atol=2e-5)
    cr.backward(g.double())
    ref, got = xr.grad.numpy(), x.grad.cpu().numpy()
    assert np.isfinite(got).all()
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max() + 1e-12
    dead = np.isneginf(out.numpy())
    assert (got[dead] == 0).all() and (ref[dead] == 0).all()
    return got_c


def _check_nhwc(pkg, out, J, seed):
    """The same for the NHWC kernels (depth 64): `out` is the (B, J*64, H, W) view of the logits."""
    B = out.shape[0]
    xn = out.permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
    c = pkg.soft_argmax_3d_nhwc(xn, J)
    got_c = c.detach().cpu().numpy()
    assert np.isfinite(got_c).all()
    np.testing.assert_allclose(got_c, ho.soft_argmax(out.numpy(), J, 64, True), rtol=0, atol=2e-5)
    g = torch.randn(B, J * 3, generator=torch.Generator().manual_seed(seed))
    c.backward(g.to(DEV))
    xr = out.double().requires_grad_(True)
    cr = _torch_ref(xr, J, 64, True)
    np.testing.assert_allclose(got_c, cr.detach().numpy(), rtol=0, atol=2e-5)
    cr.backward(g.double())
    ref, got = xr.grad.numpy(), xn.grad.permute(0, 3, 1, 2).cpu().numpy()
    assert np.isfinite(got).all()
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max() + 1e-12
    dead = np.isneginf(out.numpy())
    assert (got[dead] == 0).all() and (ref[dead] == 0).all()


def test_soft_argmax_3d_with_minus_infinity_logits(pkg):
    """A true -inf logit has softmax weight exactly 0 (torch.softmax, the oracle).  Row h = 0 of depth 0 -- the first float4
    lanes 0..7 visit -- is all -inf for two joints; a third joint is -inf everywhere but one voxel, where the expectation
    then sits exactly."""
    J, D, H, W = 17, 8, 16, 32
    out = torch.randn(1, J * D, H, W, generator=torch.Generator().manual_seed(21)) * 3
    for j in (3, 9):
        out[0, j * D, 0, :] = NEG
    out[0, 12 * D:13 * D] = NEG
    out[0, 12 * D + 5, 7, 21] = 1.5
    c = _check_nchw(pkg, out, J, D, True, 22).reshape(J, 3)
    np.testing.assert_allclose(c[12], [(21 / 32 - 0.5) * 2, (7 / 16 - 0.5) * 2, (5 / 8 - 0.5) * 2], rtol=0, atol=1e-6)


def test_soft_argmax_3d_nhwc_with_minus_infinity_logits(pkg):
    """NHWC: the first 16 pixels of one joint -- what the four wavefronts read in their first pass, every depth -- are -inf."""
    J, H, W = 17, 4, 8
    out = torch.randn(1, J * 64, H, W, generator=torch.Generator().manual_seed(23)) * 3
    out[0, 6 * 64:7 * 64, 0:2, :] = NEG
    _check_nhwc(pkg, out, J, 24)


@pytest.mark.parametrize("D,H,W", [(1, 1, 4), (1, 3, 4), (1, 4, 8), (2, 2, 4)])
def test_soft_argmax_maps_smaller_than_the_workgroup(pkg, D, H, W):
    """1, 3, 4 and 8 float4 groups per map: whole wavefronts of the 256-thread workgroup see no element."""
    J = 17
    out = torch.randn(2, J * D, H, W, generator=torch.Generator().manual_seed(D * 100 + H * 10 + W)) * 4
    _check_nchw(pkg, out, J, D, D > 1, 31)


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5)])
def test_soft_argmax_3d_nhwc_small_maps(pkg, H, W):
    """1 and 15 pixels: fewer than the 16 a pass of the four wavefronts covers."""
    J = 17
    out = torch.randn(2, J * 64, H, W, generator=torch.Generator().manual_seed(H * 10 + W)) * 4
    _check_nhwc(pkg, out, J, 32)
