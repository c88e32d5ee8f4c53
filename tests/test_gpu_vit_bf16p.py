"""MyViT "bf16p" mode on the MI355X: the bf16 operand carriers its producers write (bit for bit the bf16 rounding of
what the fp32 kernels compute, padding rows zero, NaN / inf kept), the model against the fp64 twin of oracle/vit_twin.py
with a tolerance that calibrates itself on eager torch under bf16 autocast, the phase-5 chain, training, determinism,
the weight-carrier cache and the backward-time version check."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from oracle import vit_twin
from oracle.vit_twin import twin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 1e-6          # relative error counted as zero (both sides at round-off of an exactly representable result)
TRAIN_GAP = 0.01      # final-loss gap to f16x3 after 20 AdamW steps: measured 0.078 % on one MI355X (fp32's: 0.0001 %)


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pad32(n):
    return (n + 31) // 32 * 32


def _poisoned_carrier(rows_pad, cols):
    """A carrier full of NaNs: the kernel must write every element, the padding rows included."""
    return torch.full((rows_pad, cols), float("nan"), dtype=torch.bfloat16, device=DEV)


def _assert_carrier(c, ref, rows):
    """c [rows_pad][cols] bf16 == bf16(ref) bit for bit on the first `rows` rows (NaNs: NaN at the same places), zeros past."""
    torch.cuda.synchronize()
    want = ref.reshape(rows, -1).to(torch.bfloat16)
    got = c[:rows]
    gn, wn = torch.isnan(got.float()), torch.isnan(want.float())
    assert torch.equal(gn, wn)
    gi, wi = got.view(torch.int16), want.view(torch.int16)
    bad = (gi != wi) & ~gn
    assert not bad.any(), f"{int(bad.sum())} elements differ from the bf16 rounding of the fp32 kernel"
    assert not c[rows:].view(torch.int16).any(), "padding rows not zero"


# ---------------------------------------------------------------------------------------------- kernels alone, bitwise
@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("nnorm", [1, 2])
def test_layernorm_forward_carrier(pkg, nnorm, with_add):
    L = pkg.lib()
    T, H = 300, 256
    Tp = _pad32(T)
    g = torch.Generator().manual_seed(11 + nnorm)
    x = (3.0 * torch.randn(T, H, generator=g) + 0.5).to(DEV)
    add = torch.randn(T, H, generator=g).to(DEV) if with_add else None
    ps = [((1 + 0.2 * torch.randn(H, generator=g)) if i % 2 == 0 else 0.2 * torch.randn(H, generator=g)).to(DEV)
          for i in range(4)]
    xo, y, st = torch.empty(T, H, device=DEV), torch.empty(T, H, device=DEV), torch.empty(nnorm, 2, T, device=DEV)
    assert L.pl_vit_ln_fwd(x.data_ptr(), add.data_ptr() if with_add else None, T, H, nnorm, ps[0].data_ptr(),
                           ps[1].data_ptr(), ps[2].data_ptr(), ps[3].data_ptr(), 1e-5,
                           xo.data_ptr() if with_add else None, y.data_ptr(), st.data_ptr(), _stream()) == 0
    xo2, st2 = torch.empty(T, H, device=DEV), torch.empty(nnorm, 2, T, device=DEV)
    c = _poisoned_carrier(Tp, H)
    assert L.pl_vit_ln_fwd_bf16(x.data_ptr(), add.data_ptr() if with_add else None, T, H, nnorm, ps[0].data_ptr(),
                                ps[1].data_ptr(), ps[2].data_ptr(), ps[3].data_ptr(), 1e-5,
                                xo2.data_ptr() if with_add else None, None, c.data_ptr(), Tp, st2.data_ptr(), _stream()) == 0
    _assert_carrier(c, y, T)
    assert torch.equal(st2, st)
    if with_add:
        assert torch.equal(xo2, xo)
    # with the fp32 output too: the same fp32 values
    y3 = torch.empty(T, H, device=DEV)
    c3 = _poisoned_carrier(Tp, H)
    assert L.pl_vit_ln_fwd_bf16(x.data_ptr(), add.data_ptr() if with_add else None, T, H, nnorm, ps[0].data_ptr(),
                                ps[1].data_ptr(), ps[2].data_ptr(), ps[3].data_ptr(), 1e-5,
                                xo2.data_ptr() if with_add else None, y3.data_ptr(), c3.data_ptr(), Tp, st2.data_ptr(),
                                _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(y3, y) and torch.equal(c3, c)


@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("nnorm", [1, 2])
def test_layernorm_backward_carrier(pkg, nnorm, with_dres):
    L = pkg.lib()
    T, H = 555, 256                      # three 256-row chunks, the last one ragged
    Tp = _pad32(T)
    g = torch.Generator().manual_seed(21 + nnorm)
    x = (2.0 * torch.randn(T, H, generator=g)).to(DEV)
    ps = [((1 + 0.2 * torch.randn(H, generator=g)) if i % 2 == 0 else 0.2 * torch.randn(H, generator=g)).to(DEV)
          for i in range(4)]
    y, st = torch.empty(T, H, device=DEV), torch.empty(nnorm, 2, T, device=DEV)
    assert L.pl_vit_ln_fwd(x.data_ptr(), None, T, H, nnorm, ps[0].data_ptr(), ps[1].data_ptr(), ps[2].data_ptr(),
                           ps[3].data_ptr(), 1e-5, None, y.data_ptr(), st.data_ptr(), _stream()) == 0
    dy = torch.randn(T, H, generator=g).to(DEV)
    dres = torch.randn(T, H, generator=g).to(DEV) if with_dres else None
    scratch = torch.empty(L.pl_vit_ln_bwd_scratch_bytes(T, H, nnorm), dtype=torch.uint8, device=DEV)
    dx, dgb = torch.empty(T, H, device=DEV), torch.empty(nnorm * 2 * H, device=DEV)
    args = (dy.data_ptr(), dres.data_ptr() if with_dres else None, x.data_ptr(), st.data_ptr(), T, H, nnorm,
            ps[0].data_ptr(), ps[1].data_ptr(), ps[2].data_ptr())
    assert L.pl_vit_ln_bwd(*args, dx.data_ptr(), dgb.data_ptr(), scratch.data_ptr(), _stream()) == 0
    dx2, dgb2 = torch.empty(T, H, device=DEV), torch.empty(nnorm * 2 * H, device=DEV)
    c = _poisoned_carrier(Tp, H)
    assert L.pl_vit_ln_bwd_bf16(*args, dx2.data_ptr(), c.data_ptr(), Tp, dgb2.data_ptr(), scratch.data_ptr(), _stream()) == 0
    _assert_carrier(c, dx, T)
    assert torch.equal(dx2, dx) and torch.equal(dgb2, dgb)


# the model's shape, the shortest, and for 17 and 32 tokens the most heads whose backward fits the 160 KB of LDS
ATTN_SHAPES = [(17, 4), (1, 1), (17, 7), (32, 3)]


def test_attention_lds_corners_are_the_largest_supported(pkg):
    L = pkg.lib()
    for seq, heads in ATTN_SHAPES[2:]:
        assert L.pl_vit_attn_supported(seq, heads, 64) and not L.pl_vit_attn_supported(seq, heads + 1, 64)


@pytest.mark.parametrize("seq,heads", ATTN_SHAPES)
def test_attention_carriers(pkg, seq, heads):
    L = pkg.lib()
    B = 5
    T, HD = B * seq, heads * 64
    Tp = _pad32(T)
    g = torch.Generator().manual_seed(seq * 10 + heads)
    qkv = (1.5 * torch.randn(T, 3 * HD, generator=g)).to(DEV)
    dout = torch.randn(T, HD, generator=g).to(DEV)
    sc = 64 ** -0.5
    o, lse = torch.empty(T, HD, device=DEV), torch.empty(B, heads, seq, device=DEV)
    assert L.pl_vit_attn_fwd(qkv.data_ptr(), B, seq, heads, 64, sc, o.data_ptr(), lse.data_ptr(), _stream()) == 0
    c, lse2 = _poisoned_carrier(Tp, HD), torch.empty(B, heads, seq, device=DEV)
    assert L.pl_vit_attn_fwd_bf16(qkv.data_ptr(), B, seq, heads, 64, sc, None, c.data_ptr(), Tp, lse2.data_ptr(),
                                  _stream()) == 0
    _assert_carrier(c, o, T)
    assert torch.equal(lse2, lse)
    dq = torch.empty(T, 3 * HD, device=DEV)
    assert L.pl_vit_attn_bwd(qkv.data_ptr(), lse.data_ptr(), dout.data_ptr(), B, seq, heads, 64, sc, dq.data_ptr(),
                             _stream()) == 0
    cq = _poisoned_carrier(Tp, 3 * HD)
    assert L.pl_vit_attn_bwd_bf16(qkv.data_ptr(), lse.data_ptr(), dout.data_ptr(), B, seq, heads, 64, sc, None,
                                  cq.data_ptr(), Tp, _stream()) == 0
    _assert_carrier(cq, dq, T)


def test_gelu_carriers(pkg):
    L = pkg.lib()
    T, C = 300, 1024
    Tp = _pad32(T)
    g = torch.Generator().manual_seed(31)
    u = (3.0 * torch.randn(T, C, generator=g)).to(DEV)
    dy = torch.randn(T, C, generator=g).to(DEV)
    y = torch.empty(T, C, device=DEV)
    assert L.pl_vit_gelu_fwd(u.data_ptr(), T * C, y.data_ptr(), _stream()) == 0
    c = _poisoned_carrier(Tp, C)
    assert L.pl_vit_gelu_fwd_bf16(u.data_ptr(), T, C, Tp, None, c.data_ptr(), _stream()) == 0
    _assert_carrier(c, y, T)
    du = torch.empty(T, C, device=DEV)
    assert L.pl_vit_gelu_bwd(u.data_ptr(), dy.data_ptr(), T * C, du.data_ptr(), _stream()) == 0
    du2, cd = torch.empty(T, C, device=DEV), _poisoned_carrier(Tp, C)
    assert L.pl_vit_gelu_bwd_bf16(u.data_ptr(), dy.data_ptr(), T, C, Tp, du2.data_ptr(), cd.data_ptr(), _stream()) == 0
    _assert_carrier(cd, du, T)
    assert torch.equal(du2, du)


def test_pack_carrier(pkg):
    L = pkg.lib()
    T, C = 17 * 3, 256
    Tp = _pad32(T)
    g = torch.Generator().manual_seed(41)
    x = torch.randn(T, C, generator=g) * torch.logspace(-30, 30, C)
    # ties of the bf16 rounding (both parities), the largest finite values, values that round up to +-inf
    x[0, :8] = torch.tensor([1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, -(1.0 + 2 ** -8), 3.3895e38, -3.3895e38, 3.4e38, -3.4e38,
                             2.0 ** -126])
    xd = x.to(DEV)
    c = _poisoned_carrier(Tp, C)
    assert L.pl_vit_bf16_pack(xd.data_ptr(), T, C, Tp, c.data_ptr(), _stream()) == 0
    _assert_carrier(c, xd, T)


def test_nan_and_inf_stay_nan_and_inf(pkg):
    L = pkg.lib()
    T, C = 2, 256
    Tp = 32
    special = torch.tensor([float("nan"), float("inf"), float("-inf"), -float("nan")])
    x = torch.zeros(T, C)
    x[0, :4] = special
    x[1, 8:12] = special
    xd = x.to(DEV)
    c = _poisoned_carrier(Tp, C)
    assert L.pl_vit_bf16_pack(xd.data_ptr(), T, C, Tp, c.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    got = c[:T].float().cpu()
    for r, c0 in ((0, 0), (1, 8)):
        v = got[r, c0:c0 + 4]
        assert torch.isnan(v[0]) and torch.isnan(v[3]) and v[1] == float("inf") and v[2] == float("-inf")
    # GELU: NaN -> NaN, +inf -> +inf; its backward: an infinite upstream gradient stays infinite, a NaN stays NaN
    u = torch.zeros(T, C)
    u[0, :2] = torch.tensor([float("nan"), float("inf")])
    u[1, :2] = 1.0
    dy = torch.ones(T, C)
    dy[1, :2] = torch.tensor([float("inf"), float("nan")])
    ud, dyd = u.to(DEV), dy.to(DEV)
    cg, cd = _poisoned_carrier(Tp, C), _poisoned_carrier(Tp, C)
    assert L.pl_vit_gelu_fwd_bf16(ud.data_ptr(), T, C, Tp, None, cg.data_ptr(), _stream()) == 0
    assert L.pl_vit_gelu_bwd_bf16(ud.data_ptr(), dyd.data_ptr(), T, C, Tp, None, cd.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    gf, df = cg.float().cpu(), cd.float().cpu()
    assert torch.isnan(gf[0, 0]) and gf[0, 1] == float("inf")
    assert df[1, 0] == float("inf") and torch.isnan(df[1, 1])
    assert not cg[T:].view(torch.int16).any() and not cd[T:].view(torch.int16).any()


# ---------------------------------------------------------------------------------------------- model vs the fp64 twin
class _EagerViT(nn.Module):
    """The same network in stock torch ops (tools/bench_vit.py's module): the calibration run under bf16 autocast."""

    def __init__(self, vit):
        super().__init__()
        self.v = vit

    def forward(self, x):
        v = self.v
        H, nh = v.hidden_d, v.n_heads
        B, n, _ = x.shape
        h = v.linear_mapper(x) + v.pos_embed
        for b in v.blocks:
            a = b.mhsa.norm(b.norm1(h))
            q, k, w = b.mhsa.to_qkv(a).chunk(3, dim=-1)
            q, k, w = (z.reshape(B, n, nh, H // nh).transpose(1, 2) for z in (q, k, w))
            att = torch.softmax((q @ k.transpose(-1, -2)) * (H // nh) ** -0.5, dim=-1)
            h = h + b.mhsa.to_out((att @ w).transpose(1, 2).reshape(B, n, H))
            h = h + b.mlp[2](F.gelu(b.mlp[0](b.norm2(h))))
        return v.mlp[2](torch.relu(v.mlp[0](h)))


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def _check_against_autocast(got, ac, ref, what):
    """For each tensor: bf16p's max |error| against fp64 over the tensor's max |fp64| <= 2x the same ratio of autocast."""
    worst = {}
    for k, want in ref.items():
        eb, ea = _rel(got[k], want), _rel(ac[k], want)
        assert eb <= 2.0 * ea + FLOOR, (what, k, eb, ea)
        worst[k] = (eb, ea)
    return worst


def _perturbed_state(seed, **kw):
    """A seeded MyViT state with non-trivial LayerNorm affine parameters."""
    import __graft_entry__ as ge
    torch.manual_seed(seed)
    m = ge.build().MyViT(compute_dtype="fp32", **kw)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if "norm" in name:
                p.add_(0.1 * torch.randn_like(p))
    return {k: v.clone() for k, v in m.state_dict().items()}


def _run(pkg, mode, sd, x, t, autocast=False):
    """(y, {param: grad, "x": input grad}) of MSE(model(x), t) on the GPU: pl.MyViT(mode), or eager torch under autocast."""
    m = pkg.MyViT(compute_dtype="fp32" if autocast else mode).to(DEV)
    m.load_state_dict(sd)
    xd = torch.tensor(x, device=DEV, requires_grad=True)
    td = torch.as_tensor(t, device=DEV)
    if autocast:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = _EagerViT(m)(xd)
        loss = F.mse_loss(y.float(), td)
    else:
        y = m(xd)
        loss = pkg.mse_loss(y, td)
    loss.backward()
    grads = {k: p.grad.detach().float().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}
    grads["x"] = xd.grad.cpu().numpy()
    return y.detach().float().cpu().numpy(), grads


_TWIN = {}


def _twin_case(B):
    if B not in _TWIN:
        sd = _perturbed_state(100 + B)
        rng = np.random.default_rng(B)
        x = rng.uniform(0.0, 1.0, (B, 17, 2)).astype(np.float32)
        t = (0.2 * rng.standard_normal((B, 17, 3))).astype(np.float32)
        _TWIN[B] = (sd, x, t) + twin(sd, x, t, x_grad=True)
    return _TWIN[B]


@pytest.mark.parametrize("B", [1, 3, 64, 65, 4096])
def test_twin_outputs_and_gradients_against_autocast(pkg, B):
    sd, x, t, y64, g64, gx64 = _twin_case(B)
    ref = dict(g64, x=gx64, y=y64)
    y, grads = _run(pkg, "bf16p", sd, x, t)
    ya, ga = _run(pkg, "bf16p", sd, x, t, autocast=True)
    assert np.isfinite(y).all() and all(np.isfinite(v).all() for v in grads.values())
    assert set(grads) == set(g64) | {"x"}
    worst = _check_against_autocast(dict(grads, y=y), dict(ga, y=ya), ref, f"B={B}")
    k = max((k for k in worst if k not in ("x", "y")), key=lambda k: worst[k][0])
    print(f"\nbf16p vs fp64 twin, B={B}: output {worst['y'][0]:.3e} (autocast {worst['y'][1]:.3e}); "
          f"worst parameter gradient {k} {worst[k][0]:.3e} (autocast {worst[k][1]:.3e}); "
          f"input gradient {worst['x'][0]:.3e} (autocast {worst['x'][1]:.3e})")


def test_phase5_chain_against_autocast(pkg):
    """loss = mse(proj(lift(x)), t2) + mse(lift(x2), t3): lift (17x2 -> 3) called twice in one graph, proj (17x3 -> 2)."""
    lift_kw, proj_kw = dict(chw=(1, 17, 2), out_d=3), dict(chw=(1, 17, 3), out_d=2)
    sl, sp = _perturbed_state(51, **lift_kw), _perturbed_state(52, **proj_kw)
    rng = np.random.default_rng(53)
    x, x2 = (rng.uniform(0.0, 1.0, (b, 17, 2)).astype(np.float32) for b in (64, 33))
    t2, t3 = ((0.2 * rng.standard_normal(s)).astype(np.float32) for s in ((64, 17, 2), (33, 17, 3)))
    pl, pp = vit_twin.params(sl), vit_twin.params(sp)
    xa, xb = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (x, x2))
    loss = vit_twin.mse(vit_twin.forward(pp, vit_twin.forward(pl, xa)), t2) + vit_twin.mse(vit_twin.forward(pl, xb), t3)
    loss.backward()
    ref = {**{"lift." + k: v for k, v in vit_twin.grads(pl).items()}, **{"proj." + k: v for k, v in vit_twin.grads(pp).items()},
           "x": xa.grad.numpy(), "x2": xb.grad.numpy(), "loss": np.array([loss.item()])}

    def run(autocast):
        lift = pkg.MyViT(compute_dtype="fp32" if autocast else "bf16p", **lift_kw).to(DEV)
        proj = pkg.MyViT(compute_dtype="fp32" if autocast else "bf16p", **proj_kw).to(DEV)
        lift.load_state_dict(sl)
        proj.load_state_dict(sp)
        xd, x2d = (torch.tensor(v, device=DEV, requires_grad=True) for v in (x, x2))
        t2d, t3d = torch.as_tensor(t2, device=DEV), torch.as_tensor(t3, device=DEV)
        if autocast:
            el, ep = _EagerViT(lift), _EagerViT(proj)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                ya, yb = ep(el(xd)), el(x2d)
            ls = F.mse_loss(ya.float(), t2d) + F.mse_loss(yb.float(), t3d)
        else:
            ls = pkg.mse_loss(proj(lift(xd)), t2d) + pkg.mse_loss(lift(x2d), t3d)
        ls.backward()
        out = {"lift." + k: p.grad.float().cpu().numpy() for k, p in lift.named_parameters() if p.grad is not None}
        out.update({"proj." + k: p.grad.float().cpu().numpy() for k, p in proj.named_parameters() if p.grad is not None})
        out.update(x=xd.grad.cpu().numpy(), x2=x2d.grad.cpu().numpy(), loss=np.array([ls.item()]))
        return out

    got, ac = run(False), run(True)
    assert set(got) == set(ref)
    _check_against_autocast(got, ac, ref, "phase-5 chain")


# ---------------------------------------------------------------------------------------------- training, determinism, caches
def test_training_20_adamw_steps_tracks_f16x3(pkg):
    """20 FlatAdam (AdamW) steps at B = 4096 from one seed on a learnable target: the loss falls, and the last loss is
    within TRAIN_GAP of the f16x3 run's (the fp32 run's gap to f16x3 is printed beside it for scale).  A first guess was
    5 %; 1 % is about 13x the gap measured, 0.078 % (bf16p 0.004388, f16x3 0.004392)."""
    B = 4096
    g = torch.Generator().manual_seed(61)
    x = torch.rand(B, 17, 2, generator=g)
    t = torch.cat([x - 0.5, 0.5 * (x[..., :1] - x[..., 1:]) + 0.05 * torch.randn(B, 17, 1, generator=g)], -1)
    x, t = x.to(DEV), t.to(DEV)
    losses = {}
    for mode in ("bf16p", "f16x3", "fp32"):
        torch.manual_seed(62)
        m = pkg.MyViT(compute_dtype=mode).to(DEV).train()
        opt = pkg.FlatAdam(m, lr=1e-4, weight_decay=0.01, decoupled_weight_decay=True)
        losses[mode] = [pkg.train_step(m, opt, x, t)[0].item() for _ in range(20)]
    lb, lf, l32 = losses["bf16p"], losses["f16x3"], losses["fp32"]
    assert all(np.isfinite(lb))
    assert lb[-1] < lb[0] and lf[-1] < lf[0], (lb, lf)
    gap, gap32 = abs(lb[-1] - lf[-1]) / lf[-1], abs(l32[-1] - lf[-1]) / lf[-1]
    print(f"\nlosses 0 / 10 / 20: bf16p {lb[0]:.6f} {lb[10]:.6f} {lb[-1]:.6f}, f16x3 {lf[0]:.6f} {lf[10]:.6f} {lf[-1]:.6f}; "
          f"gap to f16x3 at step 20: bf16p {100 * gap:.3f} %, fp32 {100 * gap32:.4f} %")
    assert gap <= TRAIN_GAP, (lb[-1], lf[-1])


def test_repeated_step_is_bitwise_equal_and_train_eval_agree(pkg):
    sd, x, t = _twin_case(64)[:3]
    m = pkg.MyViT(compute_dtype="bf16p").to(DEV)
    m.load_state_dict(sd)
    runs = []
    for _ in range(2):
        m.zero_grad()
        y = m(torch.as_tensor(x, device=DEV))
        loss = pkg.mse_loss(y, torch.as_tensor(t, device=DEV))
        loss.backward()
        runs.append((y.detach().clone(), loss.item(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
    (y1, l1, g1), (y2, l2, g2) = runs
    assert torch.equal(y1, y2) and l1 == l2
    assert set(g1) == set(g2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    m.eval()
    with torch.no_grad():
        ye = m(torch.as_tensor(x, device=DEV))
    assert torch.equal(ye, y1)


def test_weight_carrier_caches_follow_flatadam_steps(pkg):
    sd, x, t = _twin_case(64)[:3]
    m = pkg.MyViT(compute_dtype="bf16p").to(DEV)
    m.load_state_dict(sd)
    xd, td = torch.as_tensor(x, device=DEV), torch.as_tensor(t, device=DEV)
    opt = pkg.FlatAdam(m, lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True)
    m.eval()
    with torch.no_grad():
        before = m(xd)                                          # fills the caches (parameters already in the arena)
    pos0 = m.pos_embed.detach().clone()
    m.train()
    for _ in range(2):
        pkg.train_step(m, opt, xd, td)
    assert torch.equal(m.pos_embed.detach(), pos0)
    m.eval()
    with torch.no_grad():
        after = m(xd)
        fresh = pkg.MyViT(compute_dtype="bf16p").to(DEV)
        fresh.load_state_dict(m.state_dict())
        fresh.eval()
        want = fresh(xd)
    assert torch.equal(after, want)
    assert not torch.equal(after, before)


def test_parameter_changed_between_forward_and_backward_raises(pkg):
    sd, x, t = _twin_case(3)[:3]
    m = pkg.MyViT(compute_dtype="bf16p").to(DEV)
    m.load_state_dict(sd)
    xd, dy = torch.as_tensor(x, device=DEV), torch.ones(3, 17, 3, device=DEV)
    y = m(xd)
    with torch.no_grad():
        m.blocks[1].mhsa.to_qkv.weight.mul_(1.5)
    with pytest.raises(RuntimeError, match=r"blocks\.1\.mhsa\.to_qkv\.weight"):
        y.backward(dy)
    opt = pkg.FlatAdam(m, lr=1e-4, weight_decay=0.01, decoupled_weight_decay=True)
    y = m(xd)
    y.backward(dy)                                              # fine: nothing changed
    y = m(xd)
    opt.step()
    with pytest.raises(RuntimeError, match="FlatAdam"):
        y.backward(dy)
