"""MyViT across every shape its constructor accepts, each vit.hip kernel alone at its edges, and the autograd node's
input gradient and graph structure.  Every comparison is against an independent float64 computation (plain torch on the
CPU; the model-level twin is oracle/vit_twin.py) or is an exact identity: the seq = 1 zeros, bitwise repeats, the
dynamic-scale laws, linearity in the upstream gradient.

Tolerances are the ones of tests/test_gpu_vit.py (GRAD_TOL, the 1e-3 mm output gate, the attention and LayerNorm kernel
bounds) or tighter."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vit_twin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ["fp32", "f16x3"]
GRAD_TOL = {"fp32": 1e-4, "f16x3": 5e-4}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _mpjpe_mm(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b, axis=-1).mean() * 1000.0)


def _dev(t):
    return t.float().contiguous().to(DEV)


def _err(got, want):
    return (got.detach().cpu().double() - want).abs().max().item()


# ---------------------------------------------------------------------------------------------- attention
# every (seq, heads) at the LDS limit of pl_vit_attn_bwd (seq + 1 does not fit: test_vit_host.py), and small sequences
LDS_CORNERS = [(32, 1), (32, 2), (32, 3), (31, 4), (25, 5), (21, 6), (18, 7), (15, 8)]
ATTN_SHAPES = LDS_CORNERS + [(1, 1), (1, 4), (2, 3), (17, 1)]


def _attn_inputs(B, seq, heads, regime, g):
    dh, H = 64, heads * 64
    qkv = torch.randn(B, seq, 3 * H, generator=g, dtype=torch.float64)
    if regime == "equal":                               # every key of a sample equal: P uniform
        qkv[:, :, H:2 * H] = qkv[:, :1, H:2 * H]
    elif regime == "spread":                            # logits spread ~100 below the row maximum: exp underflows
        qkv[:, :, :2 * H] *= 0.01
        a = 100.0 * torch.rand(B, seq, heads, generator=g, dtype=torch.float64)
        j = torch.randint(seq, (1,), generator=g).item()
        a[:, j] = 0.0                                   # the row maximum
        a[:, (j + 1) % seq] = 95.0 if seq > 1 else 0.0
        for h in range(heads):
            qkv[:, :, h * dh] = 1.0
            qkv[:, :, H + h * dh] = -8.0 * a[:, :, h]   # logit ~ q.k / 8 = -a
    return qkv.reshape(B * seq, 3 * H).float()


@pytest.mark.parametrize("regime", ["normal", "equal", "spread"])
@pytest.mark.parametrize("B", [1, 3, 37])
@pytest.mark.parametrize("seq,heads", ATTN_SHAPES)
def test_attention_kernels_vs_fp64(pkg, seq, heads, B, regime):
    L = pkg.lib()
    dh, H = 64, heads * 64
    g = torch.Generator().manual_seed(1000 * seq + 10 * heads + B)
    qkv = _attn_inputs(B, seq, heads, regime, g)
    dout = torch.randn(B * seq, H, generator=g).float()
    qd, dd = _dev(qkv), _dev(dout)
    o = torch.empty(B * seq, H, device=DEV)
    lse = torch.empty(B, heads, seq, device=DEV)
    dq = torch.empty(B * seq, 3 * H, device=DEV)
    assert L.pl_vit_attn_fwd(qd.data_ptr(), B, seq, heads, dh, dh ** -0.5, o.data_ptr(), lse.data_ptr(), _stream()) == 0
    assert L.pl_vit_attn_bwd(qd.data_ptr(), lse.data_ptr(), dd.data_ptr(), B, seq, heads, dh, dh ** -0.5, dq.data_ptr(),
                             _stream()) == 0
    x = qkv.double().requires_grad_(True)
    q, k, v = x.reshape(B, seq, 3 * H).chunk(3, dim=-1)
    q, k, v = (z.reshape(B, seq, heads, dh).transpose(1, 2) for z in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * dh ** -0.5
    if regime == "spread" and seq > 1:
        assert (s.amax(-1, keepdim=True) - s).max() >= 80.0
    ref = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * seq, H)
    ref.backward(dout.double())
    assert _err(o, ref.detach()) <= 2e-5 * ref.abs().max().item()
    want_lse = torch.logsumexp(s, -1).detach()
    assert torch.allclose(lse.cpu().double(), want_lse, rtol=1e-6, atol=1e-5)
    assert _err(dq, x.grad) <= 1e-4 * x.grad.abs().max().item()
    assert torch.isfinite(dq).all() and torch.isfinite(o).all()
    if seq == 1:                                        # P = 1: o is v, and no gradient reaches q or k
        assert torch.equal(o, qd[:, 2 * H:])
        assert torch.equal(dq[:, :2 * H], torch.zeros_like(dq[:, :2 * H]))
        assert torch.equal(dq[:, 2 * H:], dd)


# ---------------------------------------------------------------------------------------------- LayerNorm
def _layer_norm64(x, g, b, eps=1e-5):
    """LayerNorm in float64 by its definition.  The mean of a constant fp32 row is exact here (its partial sums fit 53
    bits), so such a row normalises to exactly 0 -- as the kernel's does; F.layer_norm leaves ~1e-14 of rounding in it."""
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    return d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps) * g + b


def _ln_rows(T, H, g):
    """Rows of N(mu, sigma) with random mu / sigma, every 7th row constant (variance 0), every 5th a large mean with a
    small spread."""
    x = torch.randn(T, H, generator=g, dtype=torch.float64) * (0.5 + 2 * torch.rand(T, 1, generator=g, dtype=torch.float64))
    x += torch.randn(T, 1, generator=g, dtype=torch.float64)
    x[4::5] = 1e3 + 1e-2 * torch.randn(len(range(4, T, 5)), H, generator=g, dtype=torch.float64)
    x[::7] = torch.randn(len(range(0, T, 7)), 1, generator=g, dtype=torch.float64)
    return x.float()


@pytest.mark.parametrize("T", [1, 3, 255, 256, 257, 1000])
@pytest.mark.parametrize("nnorm", [0, 1, 2])
@pytest.mark.parametrize("H", [64, 192, 320, 512, 1024])
def test_layernorm_kernels_vs_fp64(pkg, H, nnorm, T):
    L = pkg.lib()
    g = torch.Generator().manual_seed(T * 7 + H + nnorm)
    x = _ln_rows(T, H, g)
    add = (0.1 * torch.randn(T, H, generator=g)).float()
    add[::7] = 0.0                                      # keep the constant rows constant after the residual add
    add[4::5] = 0.0
    ps = [(1 + 0.1 * torch.randn(H, generator=g)).float() if i % 2 == 0 else (0.1 * torch.randn(H, generator=g)).float()
          for i in range(4)]
    dy = torch.randn(T, H, generator=g).float()
    dres = torch.randn(T, H, generator=g).float()
    xd, ad, dyd, drd = (_dev(z) for z in (x, add, dy, dres))
    pd = [_dev(p) for p in ps]
    for with_add in ([True] if nnorm == 0 else [True, False]):
        xo = torch.empty(T, H, device=DEV)
        y = torch.empty(T, H, device=DEV) if nnorm else None
        st = torch.empty(nnorm, 2, T, device=DEV) if nnorm else None
        pp_ = [pd[0], pd[1], pd[2], pd[3]][:2 * nnorm] + [None] * (4 - 2 * nnorm)
        assert L.pl_vit_ln_fwd(xd.data_ptr(), ad.data_ptr() if with_add else None, T, H, nnorm,
                               *[p.data_ptr() if p is not None else None for p in pp_], 1e-5,
                               xo.data_ptr() if with_add else None, y.data_ptr() if nnorm else None,
                               st.data_ptr() if nnorm else None, _stream()) == 0
        xs32 = (x + add) if with_add else x
        if with_add:
            assert torch.equal(xo.cpu(), xs32)
        if nnorm == 0:
            continue
        xin = xo if with_add else xd
        xs = xs32.double().requires_grad_(True)
        pp = [p.double().requires_grad_(True) for p in ps]
        r = _layer_norm64(xs, pp[0], pp[1])
        if nnorm == 2:
            r = _layer_norm64(r, pp[2], pp[3])
        r.backward(dy.double())
        assert _err(y, r.detach()) <= 1e-4 * max(1.0, r.abs().max().item()), (with_add, "forward")
        if nnorm == 1:                                  # a constant row normalises to exactly beta
            assert torch.equal(y[::7].cpu(), ps[1].expand(len(range(0, T, 7)), H))
        for with_dres in (True, False):
            dx, dgb = torch.empty(T, H, device=DEV), torch.empty(nnorm * 2 * H, device=DEV)
            scratch = torch.empty(L.pl_vit_ln_bwd_scratch_bytes(T, H, nnorm), dtype=torch.uint8, device=DEV)
            assert L.pl_vit_ln_bwd(dyd.data_ptr(), drd.data_ptr() if with_dres else None, xin.data_ptr(), st.data_ptr(), T, H,
                                   nnorm, pd[0].data_ptr(), pd[1].data_ptr(), pd[2].data_ptr(), dx.data_ptr(), dgb.data_ptr(),
                                   scratch.data_ptr(), _stream()) == 0
            want_dx = xs.grad + (dres.double() if with_dres else 0.0)
            assert _err(dx, want_dx) <= 2e-4 * want_dx.abs().max().item() + 1e-5, (with_add, with_dres, "dx")
            want = [pp[0].grad, pp[1].grad] + ([pp[2].grad, pp[3].grad] if nnorm == 2 else [])
            got = dgb.cpu().double().reshape(len(want), H)
            for i, (gi, w) in enumerate(zip(got, want)):
                assert (gi - w).abs().max() <= 1e-4 * w.abs().max(), (with_add, with_dres, i)


# ---------------------------------------------------------------------------------------------- token head
@pytest.mark.parametrize("T", [1, 255, 256, 257, 4097])
@pytest.mark.parametrize("K", [32, 96, 256])
@pytest.mark.parametrize("out_d", [1, 2, 3, 4])
def test_head_kernels_vs_fp64(pkg, out_d, K, T):
    L = pkg.lib()
    g = torch.Generator().manual_seed(out_d * 1000 + K + T)
    z = torch.randn(T, K, generator=g).float()
    z[torch.rand(T, K, generator=g) < 0.15] = 0.0      # exact zeros: ReLU's gradient there is 0, as in torch
    z[0, 0] = 0.0
    z[torch.rand(T, K, generator=g) < 0.05] = -0.0
    W, b = torch.randn(out_d, K, generator=g).float(), torch.randn(out_d, generator=g).float()
    dy = torch.randn(T, out_d, generator=g).float()
    zd, Wd, bd, dyd = (_dev(t) for t in (z, W, b, dy))
    y = torch.empty(T, out_d, device=DEV)
    assert L.pl_vit_head_fwd(zd.data_ptr(), T, K, Wd.data_ptr(), bd.data_ptr(), out_d, y.data_ptr(), _stream()) == 0
    dz, dwb = torch.empty(T, K, device=DEV), torch.empty(out_d * K + out_d, device=DEV)
    scratch = torch.empty(L.pl_vit_head_bwd_scratch_bytes(T, K, out_d), dtype=torch.uint8, device=DEV)
    assert L.pl_vit_head_bwd(dyd.data_ptr(), zd.data_ptr(), T, K, Wd.data_ptr(), out_d, dz.data_ptr(), dwb.data_ptr(),
                             scratch.data_ptr(), _stream()) == 0
    zz = z.double().requires_grad_(True)
    Wz, bz = W.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = F.linear(torch.relu(zz), Wz, bz)
    ref.backward(dy.double())
    r = torch.relu(z.double())
    # bounds from the magnitudes summed: fp32 sums of at most 256 terms in order, then the ordered chunk reduction
    assert ((y.cpu().double() - ref.detach()).abs() <= 1e-5 * (r @ W.double().abs().T + b.double().abs())).all()
    assert ((dz.cpu().double() - zz.grad).abs() <= 1e-5 * (dy.double().abs() @ W.double().abs())).all()
    assert torch.equal(dz.cpu()[z == 0], torch.zeros(int((z == 0).sum())))
    dW, db = dwb[:out_d * K].cpu().double().reshape(out_d, K), dwb[out_d * K:].cpu().double()
    assert ((dW - Wz.grad).abs() <= 1e-5 * (dy.double().abs().T @ r)).all()
    assert ((db - bz.grad).abs() <= 1e-5 * dy.double().abs().sum(0)).all()


# ---------------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("H", [64, 512])
@pytest.mark.parametrize("seq", [1, 17, 32])
@pytest.mark.parametrize("in_d", [1, 2, 5, 8])
def test_embedding_kernels_vs_fp64(pkg, in_d, seq, H):
    L = pkg.lib()
    B = -(-700 // seq) + 1                              # T = B seq spans three 256-row chunks and a partial one
    T = B * seq
    g = torch.Generator().manual_seed(in_d * 100 + seq + H)
    x, W, b, pos = (torch.randn(T, in_d, generator=g), torch.randn(H, in_d, generator=g), torch.randn(H, generator=g),
                    torch.randn(seq, H, generator=g))
    dx = torch.randn(T, H, generator=g)
    xd, Wd, bd, pd, dxd = (_dev(z) for z in (x, W, b, pos, dx))
    out = torch.empty(T, H, device=DEV)
    assert L.pl_vit_embed_fwd(xd.data_ptr(), T, in_d, seq, Wd.data_ptr(), bd.data_ptr(), pd.data_ptr(), H, out.data_ptr(),
                              _stream()) == 0
    x64, W64, dd = x.double(), W.double(), dx.double()
    want = x64 @ W64.T + b.double() + pos.double().repeat(B, 1)
    assert ((out.cpu().double() - want).abs() <= 1e-6 * (x64.abs() @ W64.abs().T + b.double().abs()
                                                         + pos.double().abs().repeat(B, 1))).all()
    dwb, dpos, dxin = torch.empty(H * in_d + H, device=DEV), torch.empty(seq, H, device=DEV), torch.empty(T, in_d, device=DEV)
    scratch = torch.empty(L.pl_vit_embed_bwd_scratch_bytes(T, in_d, H), dtype=torch.uint8, device=DEV)
    assert L.pl_vit_embed_bwd(dxd.data_ptr(), xd.data_ptr(), T, in_d, seq, H, Wd.data_ptr(), dwb.data_ptr(), dpos.data_ptr(),
                              dxin.data_ptr(), scratch.data_ptr(), _stream()) == 0
    dW, db = dwb[:H * in_d].cpu().double().reshape(H, in_d), dwb[H * in_d:].cpu().double()
    assert ((dW - dd.T @ x64).abs() <= 1e-5 * (dd.abs().T @ x64.abs())).all()
    assert ((db - dd.sum(0)).abs() <= 1e-5 * dd.abs().sum(0)).all()
    assert ((dpos.cpu().double() - dd.reshape(B, seq, H).sum(0)).abs() <= 1e-5 * dd.abs().reshape(B, seq, H).sum(0)).all()
    assert ((dxin.cpu().double() - dd @ W64).abs() <= 1e-5 * (dd.abs() @ W64.abs())).all()


# ---------------------------------------------------------------------------------------------- GELU
def test_gelu_kernels_vs_exact_erf(pkg):
    L = pkg.lib()
    u = torch.cat([torch.linspace(-12.0, 12.0, 240001, dtype=torch.float64),
                   torch.tensor([1e20, -1e20, 0.0, -0.0], dtype=torch.float64)]).float()
    g = torch.Generator().manual_seed(9)
    dy = torch.randn(u.numel(), generator=g).float()
    ud, dyd = _dev(u), _dev(dy)
    y, du = torch.empty_like(ud), torch.empty_like(ud)
    assert L.pl_vit_gelu_fwd(ud.data_ptr(), u.numel(), y.data_ptr(), _stream()) == 0
    assert L.pl_vit_gelu_bwd(ud.data_ptr(), dyd.data_ptr(), u.numel(), du.data_ptr(), _stream()) == 0
    v = u.double()
    cdf = 0.5 * (1.0 + torch.special.erf(v / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)
    want_y, want_d = v * cdf, cdf + v * pdf
    assert torch.isfinite(y).all() and torch.isfinite(du).all()
    # fp32 erf carries ~1 ulp of 1 into 1 + erf: absolute error ~ 2^-24 |u| in the left tail, relative elsewhere
    assert ((y.cpu().double() - want_y).abs() <= 1e-6 * want_y.abs() + 3e-7 * v.abs()).all()
    assert ((du.cpu().double() - dy.double() * want_d).abs() <= (1e-6 * want_d.abs() + 3e-7 * (1 + v.abs())) *
            dy.double().abs()).all()
    assert y.cpu()[-4] == 1e20 and y.cpu()[-3] == 0.0 and du.cpu()[-4] == dy[-4] and du.cpu()[-3] == 0.0


# ---------------------------------------------------------------------------------------------- dynamic-scale planes
def _planes(pkg, x, rows_pad, other=None):
    """pl_vit_planes_dyn on x [rows][cols]: (scale [4], hi plane, lo plane) as float64 CPU tensors [rows_pad][cols]."""
    rows, cols = x.shape
    xd = _dev(x)
    p = torch.full((rows_pad, cols), float("nan"), device=DEV)     # every element must be written
    scale = torch.full((4,), float("nan"), device=DEV)
    scratch = torch.empty(pkg.lib().pl_vit_planes_scratch_bytes(), dtype=torch.uint8, device=DEV)
    od = _dev(other) if other is not None else None
    assert pkg.lib().pl_vit_planes_dyn(xd.data_ptr(), rows, cols, rows_pad, od.data_ptr() if od is not None else None,
                                       scale.data_ptr(), p.data_ptr(), scratch.data_ptr(), _stream()) == 0
    hl = p.cpu().view(torch.float16).reshape(2, rows_pad, cols).double()
    return scale.cpu().double(), hl[0], hl[1]


def _x_with_amax(rows, cols, amax, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(rows, cols, generator=g, dtype=torch.float64) * 2 - 1
    x = (x * (amax / x.abs().max())).float()
    x[torch.randint(rows, (1,), generator=g).item(), torch.randint(cols, (1,), generator=g).item()] = -amax
    x[-1, -1] = amax                                    # the last valid element: the tail of the max pass
    assert x.abs().max().item() == amax
    return x


# out of [2^-87, 2^114) the clamp of S to 2^+-100 leaves amax S outside [2^13, 2^14): below, fewer bits are used but the
# absolute bound 2^-10 / S still holds; from 2^114 the high plane runs into fp16's range, which ends at ~2^116
AMAX = [2.0 ** -80, 1e-20, 1.0, 2.0 ** 13, 65504.0, 1e10, 2.0 ** 100]


@pytest.mark.parametrize("amax", AMAX + [2.0 ** -90, 2.0 ** 114, 2.0 ** 115])
def test_dynamic_planes_scale_laws_and_split_bound(pkg, amax):
    rows, cols, rows_pad = 1000, 260, 1024             # several blocks of the max pass, 24 pad rows
    x = _x_with_amax(rows, cols, np.float32(amax).item(), seed=int(abs(math.log2(amax))) + 1)
    amax = x.abs().max().item()
    other = torch.tensor([2.0 ** 7, 2.0 ** -7, 0.0, 0.0])
    scale, h, l = _planes(pkg, x, rows_pad, other)
    e = math.floor(math.log2(amax))
    S = 2.0 ** min(100, max(-100, 13 - e))
    assert scale[0].item() == S
    if 2.0 ** -87 <= amax < 2.0 ** 114:
        assert 2.0 ** 13 <= amax * S < 2.0 ** 14
    else:
        assert S in (2.0 ** 100, 2.0 ** -100)
    assert scale[1].item() == 1.0 / S
    assert scale[2].item() == 2.0 ** -7 / S
    assert torch.isfinite(h).all() and torch.isfinite(l).all()
    rec = (h[:rows] + l[:rows] / 2048.0) / S
    # h = fp16(S x) is within 2^-11 |S x| of S x, l = fp16(2048 (S x - h)) keeps the residual to one fp16 ulp of a value
    # below 2^13 (in range): |S x - h - l / 2048| <= 2^-10.  Above 2^14 (amax >= 2^114) fp16's ulp doubles per octave.
    bound = 2.0 ** -10 * max(1.0, 2.0 ** math.floor(math.log2(amax * S)) / 2.0 ** 13)
    assert (rec - x.double()).abs().max().item() <= bound / S
    assert torch.equal(h[rows:], torch.zeros_like(h[rows:])) and torch.equal(l[rows:], torch.zeros_like(l[rows:]))


def test_dynamic_planes_overflow_beyond_fp16_range_is_not_finite(pkg):
    """From about 2^116 the scale stays clamped at 2^-100 and S amax exceeds fp16's largest value: the element becomes
    inf in the high plane -- never a finite wrong value."""
    x = _x_with_amax(64, 64, 2.0 ** 117, seed=3)
    scale, h, l = _planes(pkg, x, 64)
    assert scale[0].item() == 2.0 ** -100
    big = x.double().abs() * 2.0 ** -100 >= 65520.0
    assert big.any()
    assert not torch.isfinite(h[big] + l[big]).any()
    rec = (h + l / 2048.0) / scale[0]
    ok = ~big
    assert ((rec[ok] - x.double()[ok]).abs() <= 2.0 ** -6 / scale[0]).all()


def test_dynamic_planes_all_zero_gives_unit_scale_and_zero_planes(pkg):
    x = torch.zeros(37, 64)
    scale, h, l = _planes(pkg, x, 64, other=torch.tensor([2.0 ** 3, 2.0 ** -3, 0.0, 0.0]))
    assert scale[0].item() == 1.0 and scale[1].item() == 1.0 and scale[2].item() == 2.0 ** -3
    assert not h.any() and not l.any()
    scale, h, l = _planes(pkg, x, 37)
    assert scale[2].item() == 1.0


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_dynamic_planes_non_finite_stays_non_finite(pkg, bad):
    x = _x_with_amax(100, 64, 3.0, seed=5)
    x[17, 5] = bad
    x[99, 60] = bad
    scale, h, l = _planes(pkg, x, 128)
    assert math.isfinite(scale[0].item()) and scale[0].item() > 0
    assert scale[1].item() == 1.0 / scale[0].item()
    for i, j in ((17, 5), (99, 60)):
        assert not math.isfinite(h[i, j].item() + l[i, j].item() / 2048.0)
    fin = torch.isfinite(x)
    rec = (h[:100] + l[:100] / 2048.0) / scale[0]
    assert torch.isfinite(rec[fin]).all()
    assert ((rec[fin] - x.double()[fin]).abs() <= 2.0 ** -10 / scale[0]).all()
    assert not h[100:].any() and not l[100:].any()


# ---------------------------------------------------------------------------------------------- the model vs the fp64 twin
# (hidden_d, heads, seq, in_d, out_d, n_blocks, B)
CONFIGS = [(64, 1, 1, 1, 1, 1, 1), (64, 1, 1, 1, 1, 1, 4097), (128, 2, 32, 8, 4, 3, 37), (192, 3, 32, 2, 3, 2, 64),
           (256, 4, 31, 3, 2, 2, 33), (320, 5, 25, 2, 3, 1, 7), (512, 8, 15, 2, 3, 2, 1), (512, 8, 15, 2, 3, 2, 300),
           (256, 4, 2, 2, 3, 2, 2049)]
_CASE = {}


def _cfg_id(c):
    return "H{}h{}_s{}_{}to{}_nb{}_B{}".format(*c)


def _perturbed_state(pkg, seed, **kw):
    torch.manual_seed(seed)
    m = pkg.MyViT(compute_dtype="fp32", **kw)
    with torch.no_grad():                               # non-trivial LayerNorm affine parameters
        for name, p in m.named_parameters():
            if "norm" in name:
                p.add_(0.1 * torch.randn_like(p))
    return {k: v.clone() for k, v in m.state_dict().items()}


def _case(pkg, cfg):
    if cfg not in _CASE:
        H, heads, seq, in_d, out_d, nb, B = cfg
        sd = _perturbed_state(pkg, 7 + sum(cfg), chw=(1, seq, in_d), n_blocks=nb, hidden_d=H, n_heads=heads, out_d=out_d)
        rng = np.random.default_rng(sum(cfg))
        x = rng.uniform(0.0, 1.0, (B, seq, in_d)).astype(np.float32)
        t = (0.2 * rng.standard_normal((B, seq, out_d))).astype(np.float32)
        y64, g64, dx64 = vit_twin.twin(sd, x, t, n_heads=heads, x_grad=True)
        _CASE[cfg] = (sd, x, t, y64, g64, dx64, float(((y64 - t.astype(np.float64)) ** 2).mean()))
    return _CASE[cfg]


def _make(pkg, cfg, sd, mode):
    H, heads, seq, in_d, out_d, nb, B = cfg
    m = pkg.MyViT(chw=(1, seq, in_d), n_blocks=nb, hidden_d=H, n_heads=heads, out_d=out_d, compute_dtype=mode).to(DEV)
    m.load_state_dict(sd)
    return m


def _run(pkg, m, x, t):
    m.zero_grad()
    xd = torch.tensor(x, device=DEV, requires_grad=True)
    y = m(xd)
    loss = pkg.mse_loss(y, torch.as_tensor(t, device=DEV))
    loss.backward()
    grads = {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}
    return y.detach().cpu().numpy(), float(loss.detach()), grads, xd.grad.cpu().numpy()


def _check_grads(got, want, tol):
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    for k, w in want.items():
        err = np.abs(got[k].astype(np.float64) - w).max()
        assert err <= tol * np.abs(w).max(), (k, err, np.abs(w).max())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cfg", CONFIGS, ids=_cfg_id)
def test_model_envelope_vs_twin(pkg, cfg, mode):
    sd, x, t, y64, g64, dx64, loss64 = _case(pkg, cfg)
    H, seq = cfg[0], cfg[2]
    m = _make(pkg, cfg, sd, mode)
    y, loss, grads, dx = _run(pkg, m, x, t)
    assert np.isfinite(y).all() and np.isfinite(dx).all()
    assert _mpjpe_mm(y, y64) <= 1e-3
    # the output gate leaves an rms error e of ~1e-6, which moves the MSE by up to 2 sqrt(loss) e (Cauchy-Schwarz)
    assert abs(loss - loss64) <= 1e-5 * loss64 + 2e-6 * math.sqrt(loss64)
    _check_grads(grads, g64, GRAD_TOL[mode])
    _check_grads({"x": dx}, {"x": dx64}, GRAD_TOL[mode])
    y2, loss2, grads2, dx2 = _run(pkg, m, x, t)         # fixed-order reductions: a repeat is bitwise equal
    assert np.array_equal(y, y2) and loss == loss2 and np.array_equal(dx, dx2)
    for k in grads:
        assert np.array_equal(grads[k], grads2[k]), k
    if seq == 1:                                        # softmax over one key: no gradient reaches q or k
        for i in range(cfg[5]):
            w = grads[f"blocks.{i}.mhsa.to_qkv.weight"]
            assert not w[:2 * H].any() and w[2 * H:].any()


# ---------------------------------------------------------------------------------------------- input gradient, graph
LIFT, PROJ = dict(chw=(1, 17, 2), out_d=3), dict(chw=(1, 17, 3), out_d=2)
_CHAIN = {}


def _chain_case(pkg):
    """loss = mse(proj(lift(x)), t2) + mse(lift(x2), t3), as phase5_loop/train_5.py builds it: lift called twice with
    different B, proj a MyViT(chw=(1,17,3), out_d=2)."""
    if not _CHAIN:
        sl, sp = _perturbed_state(pkg, 21, **LIFT), _perturbed_state(pkg, 22, **PROJ)
        rng = np.random.default_rng(23)
        x, x2 = (rng.uniform(0.0, 1.0, (b, 17, 2)).astype(np.float32) for b in (5, 3))
        t2, t3 = ((0.2 * rng.standard_normal(s)).astype(np.float32) for s in ((5, 17, 2), (3, 17, 3)))
        res = {}
        for frozen in (False, True):
            pl, pp = vit_twin.params(sl), vit_twin.params(sp, requires_grad=not frozen)
            xa, xb = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (x, x2))
            loss = vit_twin.mse(vit_twin.forward(pp, vit_twin.forward(pl, xa)), t2) + vit_twin.mse(vit_twin.forward(pl, xb), t3)
            loss.backward()
            res[frozen] = (vit_twin.grads(pl), vit_twin.grads(pp), xa.grad.numpy(), xb.grad.numpy())
        _CHAIN.update(sl=sl, sp=sp, x=x, x2=x2, t2=t2, t3=t3, res=res)
    return _CHAIN


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_two_models_chained_one_called_twice(pkg, mode, frozen):
    c = _chain_case(pkg)
    lift = pkg.MyViT(compute_dtype=mode, **LIFT).to(DEV)
    proj = pkg.MyViT(compute_dtype=mode, **PROJ).to(DEV)
    lift.load_state_dict(c["sl"])
    proj.load_state_dict(c["sp"])
    if frozen:
        for p in proj.parameters():
            p.requires_grad_(False)
    x, x2 = (torch.tensor(v, device=DEV, requires_grad=True) for v in (c["x"], c["x2"]))
    t2, t3 = (torch.as_tensor(c[k], device=DEV) for k in ("t2", "t3"))
    loss = pkg.mse_loss(proj(lift(x)), t2) + pkg.mse_loss(lift(x2), t3)
    loss.backward()
    gl, gp, gx, gx2 = c["res"][frozen]
    tol = GRAD_TOL[mode]
    _check_grads({k: p.grad.cpu().numpy() for k, p in lift.named_parameters() if p.grad is not None}, gl, tol)
    if frozen:
        assert gp == {} and all(p.grad is None for p in proj.parameters())
    else:
        _check_grads({k: p.grad.cpu().numpy() for k, p in proj.named_parameters() if p.grad is not None}, gp, tol)
    _check_grads({"x": x.grad.cpu().numpy(), "x2": x2.grad.cpu().numpy()}, {"x": gx, "x2": gx2}, tol)


def _lift_case(pkg, mode, B=6):
    sd = _perturbed_state(pkg, 31, **LIFT)
    m = pkg.MyViT(compute_dtype=mode, **LIFT).to(DEV)
    m.load_state_dict(sd)
    rng = np.random.default_rng(B)
    x = rng.uniform(0.0, 1.0, (B, 17, 2)).astype(np.float32)
    dy = (1e-2 * rng.standard_normal((B, 17, 3))).astype(np.float32)
    return sd, m, x, dy


def _grads_for(m, x, dy):
    """(param grads, x.grad) of y.backward(dy), x a fresh leaf (a tensor: its dtype and strides are kept)."""
    m.zero_grad()
    xd = x.detach().clone().requires_grad_(True) if torch.is_tensor(x) else torch.tensor(x, device=DEV, requires_grad=True)
    y = m(xd)
    y.backward(dy)
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}, xd.grad


@pytest.mark.parametrize("mode", MODES)
def test_eval_mode_input_gradient_is_bitwise_train(pkg, mode):
    _, m, x, dy = _lift_case(pkg, mode)
    dyd = torch.as_tensor(dy, device=DEV)
    gt, xt = _grads_for(m.train(), x, dyd)
    ge, xe = _grads_for(m.eval(), x, dyd)
    assert torch.equal(xt, xe)
    assert set(gt) == set(ge)
    for k in gt:
        assert torch.equal(gt[k], ge[k]), k


@pytest.mark.parametrize("mode", MODES)
def test_float64_strided_input_and_strided_upstream_gradient(pkg, mode):
    sd, m, _, _ = _lift_case(pkg, mode)
    g = torch.Generator().manual_seed(41)
    base = torch.rand(6, 2, 17, generator=g, dtype=torch.float64)
    xt = base.to(DEV).transpose(1, 2).detach().requires_grad_(True)      # a (6, 17, 2) float64 leaf, not contiguous
    assert xt.is_leaf and not xt.is_contiguous()
    dyt = (1e-2 * torch.randn(6, 3, 17, generator=g)).float()
    dyd = dyt.to(DEV).transpose(1, 2)                                     # a non-contiguous upstream gradient
    assert not dyd.is_contiguous()
    m.zero_grad()
    y = m(xt)
    y.backward(dyd)
    assert xt.grad.dtype == torch.float64 and xt.grad.shape == xt.shape
    _, g64, dx64 = vit_twin.twin(sd, base.transpose(1, 2).float(), dy=dyt.transpose(1, 2), x_grad=True)
    tol = GRAD_TOL[mode]
    _check_grads({k: p.grad.cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}, g64, tol)
    _check_grads({"x": xt.grad.cpu().numpy()}, {"x": dx64}, tol)
    # a loss on every other token: autograd hands the node a gradient with zero rows
    m.zero_grad()
    xd = base.transpose(1, 2).float().to(DEV).requires_grad_(True)
    y = m(xd)
    (y[:, ::2] * torch.as_tensor(dyt.transpose(1, 2)[:, ::2].contiguous(), device=DEV)).sum().backward()
    dym = torch.zeros(6, 17, 3)
    dym[:, ::2] = dyt.transpose(1, 2)[:, ::2]
    _, g64, dx64 = vit_twin.twin(sd, base.transpose(1, 2).float(), dy=dym, x_grad=True)
    _check_grads({k: p.grad.cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}, g64, tol)
    _check_grads({"x": xd.grad.cpu().numpy()}, {"x": dx64}, tol)


@pytest.mark.parametrize("mode", MODES)
def test_gradients_scale_with_the_upstream_gradient(pkg, mode):
    """Every step of the backward is linear in dy and the dynamic scales are powers of two: a gradient scaled by 2^+-24
    gives the same planes, so every gradient is c times the unscaled one."""
    _, m, x, dy = _lift_case(pkg, mode)
    dyd = torch.as_tensor(dy, device=DEV)
    g1, x1 = _grads_for(m, x, dyd)
    for c in (2.0 ** -24, 2.0 ** 24):
        gc, xc = _grads_for(m, x, dyd * c)
        for k in g1:
            want = g1[k] * c
            assert (gc[k] - want).abs().max().item() <= 1e-6 * want.abs().max().item(), (c, k)
        assert (xc - x1 * c).abs().max().item() <= 1e-6 * (x1 * c).abs().max().item(), c


@pytest.mark.parametrize("mode", MODES)
def test_zero_upstream_gradient_gives_zero_gradients(pkg, mode):
    _, m, x, dy = _lift_case(pkg, mode)
    gz, xz = _grads_for(m, x, torch.zeros(dy.shape, device=DEV))
    assert len(gz) == 30
    for k, v in gz.items():
        assert torch.isfinite(v).all() and not v.any(), k
    assert torch.isfinite(xz).all() and not xz.any()


@pytest.mark.parametrize("mode", MODES)
def test_parameter_changed_between_forward_and_backward_raises(pkg, mode):
    _, m, x, dy = _lift_case(pkg, mode)
    dyd = torch.as_tensor(dy, device=DEV)
    xd = torch.tensor(x, device=DEV)
    y = m(xd)
    with torch.no_grad():
        m.blocks[1].mhsa.to_qkv.weight.mul_(1.5)
    with pytest.raises(RuntimeError, match=r"blocks\.1\.mhsa\.to_qkv\.weight"):
        y.backward(dyd)
    # another optimiser's step() between forward and backward
    y = m(xd)
    opt = torch.optim.SGD([m.mlp[0].weight], lr=0.1)
    m.mlp[0].weight.grad = torch.ones_like(m.mlp[0].weight)
    opt.step()
    with pytest.raises(RuntimeError, match=r"mlp\.0\.weight"):
        y.backward(dyd)
    # a forward after the change is backpropagated as usual, with the weights as they are now (and fresh weight planes)
    fresh = pkg.MyViT(compute_dtype=mode, **LIFT).to(DEV)
    fresh.load_state_dict(m.state_dict())
    want, got = _grads_for(fresh, x, dyd), _grads_for(m, x, dyd)
    assert torch.equal(want[1], got[1])
    for k in want[0]:
        assert torch.equal(want[0][k], got[0][k]), k


@pytest.mark.parametrize("mode", MODES)
def test_parameter_changed_in_flatadam_arena_raises(pkg, mode):
    """FlatAdam's parameters are views of one arena; an in-place change of one of them is caught by its version counter,
    and a step() (raw-pointer writes: no version moves) by the arena's step count.  train_step (forward, backward, then
    step) is unaffected."""
    _, m, x, dy = _lift_case(pkg, mode)
    opt = pkg.FlatAdam(m, lr=1e-4, weight_decay=0.01, decoupled_weight_decay=True)
    xd, dyd = torch.tensor(x, device=DEV), torch.as_tensor(dy, device=DEV)
    y = m(xd)
    with torch.no_grad():
        m.mlp[2].bias.add_(1.0)                          # another parameter of the same arena
    with pytest.raises(RuntimeError, match=r"mlp\.2\.bias was modified by an inplace operation"):
        y.backward(dyd)
    y = m(xd)
    y.backward(dyd)                                     # fine: nothing changed
    y = m(xd)
    opt.step()
    with pytest.raises(RuntimeError, match="FlatAdam"):
        y.backward(dyd)
    t = torch.as_tensor(np.zeros((6, 17, 3), np.float32), device=DEV)
    for _ in range(2):
        loss, _ = pkg.train_step(m, opt, xd, t)
        assert torch.isfinite(loss)
