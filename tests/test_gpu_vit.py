"""MyViT on the MI355X: against the reference's own numbers (tests/golden/g12_vit.npz, tools/make_golden_vit.py) and
against the fp64 twin of oracle/vit_twin.py (plain torch, from the model's definition):
outputs, every gradient, AdamW steps, the kernels alone on hard inputs, determinism, the weight-plane caches, and the
generic train / eval helpers."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from oracle.vit_twin import twin

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


@pytest.fixture(scope="module")
def g12():
    return load_golden("g12_vit.npz")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _mpjpe_mm(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b, axis=-1).mean() * 1000.0)


def _gpu_fwd_bwd(pkg, m, x, t):
    m.zero_grad()
    y = m(torch.as_tensor(x, device=DEV))
    loss = pkg.mse_loss(y, torch.as_tensor(t, device=DEV))
    loss.backward()
    return y.detach().cpu().numpy(), float(loss), {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters()
                                                   if p.grad is not None}


def _check_grads(got, want, tol):
    assert set(got) == set(want), (sorted(set(got) ^ set(want)))
    for k, w in want.items():
        err = np.abs(got[k].astype(np.float64) - w).max()
        assert err <= tol * np.abs(w).max(), (k, err, np.abs(w).max())


def _model(pkg, seed, mode, chw=(1, 17, 2), out_d=3):
    torch.manual_seed(seed)
    return pkg.MyViT(chw=chw, out_d=out_d, compute_dtype=mode).to(DEV)


# ---------------------------------------------------------------------------------------------- g12: the reference's numbers
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag,chw,out_d", [("lift", (1, 17, 2), 3), ("proj", (1, 17, 3), 2)])
def test_g12_forward_and_gradients_vs_reference(pkg, g12, mode, tag, chw, out_d):
    m = _model(pkg, int(g12[f"{tag}:seed"]), mode, chw, out_d)
    y, loss, grads = _gpu_fwd_bwd(pkg, m, g12[f"{tag}:x"], g12[f"{tag}:t"])
    assert _mpjpe_mm(y, g12[f"{tag}:y_fp64"]) <= 1e-3
    assert abs(loss - float(g12[f"{tag}:loss_fp64"])) <= 1e-5 * float(g12[f"{tag}:loss_fp64"])
    trainable = [str(k) for k in g12[f"{tag}:trainable"]]
    assert sorted(grads) == sorted(trainable)
    for k in trainable:
        idx, want = g12[f"{tag}:grad64:idx:{k}"], g12[f"{tag}:grad64:val:{k}"]
        gmax = float(g12[f"{tag}:gmax64:{k}"])
        err = np.abs(grads[k].reshape(-1)[idx].astype(np.float64) - want).max()
        assert err <= GRAD_TOL[mode] * gmax, (k, err, gmax)
        assert abs(np.abs(grads[k]).max() - gmax) <= GRAD_TOL[mode] * gmax, k


@pytest.mark.parametrize("mode", MODES)
def test_g12_three_adamw_steps_vs_reference(pkg, g12, mode):
    m = _model(pkg, int(g12["lift:seed"]), mode).train()
    pos0 = m.pos_embed.detach().clone()
    lr = float(g12["lift:adam_lr"])
    opt = pkg.FlatAdam(m, lr=lr, weight_decay=0.01, decoupled_weight_decay=True)
    x, t = torch.as_tensor(g12["lift:x"], device=DEV), torch.as_tensor(g12["lift:t"], device=DEV)
    for i in range(3):
        loss, _ = pkg.train_step(m, opt, x, t)
        ref = float(g12["lift:adam_losses"][i])
        assert abs(loss.item() - ref) <= 2e-5 * ref, (i, loss.item(), ref)
    assert torch.equal(m.pos_embed.detach(), pos0)          # no gradient: AdamW's decay does not touch it either
    sd = {k: v.detach().cpu().numpy().reshape(-1) for k, v in m.state_dict().items()}
    odd = 0
    for k in (str(k) for k in g12["lift:trainable"]):
        idx, want = g12[f"lift:adam:idx:{k}"], g12[f"lift:adam:val:{k}"]
        got = sd[k][idx]
        bad = np.abs(got - want) > 1e-5 * np.abs(want) + 2e-7
        if bad.any():
            # Adam normalises the gradient: an element whose reference gradient is at round-off level moves by up to
            # lr per step in whichever direction its rounding points
            g64, gmax = g12[f"lift:grad64:val:{k}"][bad], float(g12[f"lift:gmax64:{k}"])
            assert np.all(np.abs(g64) <= GRAD_TOL[mode] * gmax), k
            assert np.all(np.abs(got[bad] - want[bad]) <= 2 * 3 * lr), k
            odd += int(bad.sum())
    assert odd <= 8, odd


# ---------------------------------------------------------------------------------------------- fp64 twin, many batch sizes
_TWIN = {}


def _twin_case(pkg, B):
    if B not in _TWIN:
        torch.manual_seed(100 + B)
        m = pkg.MyViT(compute_dtype="fp32")
        with torch.no_grad():                      # non-trivial LayerNorm affine parameters
            for name, p in m.named_parameters():
                if "norm" in name:
                    p.add_(0.1 * torch.randn_like(p))
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        rng = np.random.default_rng(B)
        x = rng.uniform(0.0, 1.0, (B, 17, 2)).astype(np.float32)
        t = (0.2 * rng.standard_normal((B, 17, 3))).astype(np.float32)
        _TWIN[B] = (sd, x, t) + twin(sd, x, t)
    return _TWIN[B]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", [1, 3, 64, 65, 4096])
def test_twin_outputs_and_gradients(pkg, mode, B):
    sd, x, t, y64, g64 = _twin_case(pkg, B)
    m = pkg.MyViT(compute_dtype=mode).to(DEV)
    m.load_state_dict(sd)
    y, _, grads = _gpu_fwd_bwd(pkg, m, x, t)
    assert np.isfinite(y).all()
    assert _mpjpe_mm(y, y64) <= 1e-3
    _check_grads(grads, g64, GRAD_TOL[mode])


def test_pixel_unit_inputs_f16x3(pkg):
    """Coordinates up to 1000: the residual stream is large, the head's first Linear reads it in fp32 and the block
    operands carry device-chosen scales: finite, gradients within the f16x3 bound of the fp64 twin, and the output as
    close to the twin as fp32 arithmetic gets (a residual stream of ~1e3 carries fp32 rounding of ~1e-4 into the head:
    the 1e-3 mm gate of metre-scale inputs is out of reach of any fp32 evaluation here, the fp32 mode included)."""
    torch.manual_seed(5)
    m = pkg.MyViT(compute_dtype="f16x3")
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    rng = np.random.default_rng(5)
    x = rng.uniform(0.0, 1000.0, (32, 17, 2)).astype(np.float32)
    t = (0.2 * rng.standard_normal((32, 17, 3))).astype(np.float32)
    y64, g64 = twin(sd, x, t)
    m = m.to(DEV)
    y, _, grads = _gpu_fwd_bwd(pkg, m, x, t)
    assert np.isfinite(y).all() and all(np.isfinite(g).all() for g in grads.values())
    m32 = pkg.MyViT(compute_dtype="fp32").to(DEV)
    m32.load_state_dict(sd)
    y32 = _gpu_fwd_bwd(pkg, m32, x, t)[0]
    assert _mpjpe_mm(y, y64) <= max(1e-3, 2.0 * _mpjpe_mm(y32, y64)), (_mpjpe_mm(y, y64), _mpjpe_mm(y32, y64))
    _check_grads(grads, g64, GRAD_TOL["f16x3"])


def test_pos_embed_gradient_when_trainable(pkg):
    sd, x, t, _, _ = _twin_case(pkg, 3)
    m = pkg.MyViT(compute_dtype="fp32").to(DEV)
    m.load_state_dict(sd)
    m.pos_embed.requires_grad_(True)
    _, g64 = twin(sd, x, t)
    grads = _gpu_fwd_bwd(pkg, m, x, t)[2]
    assert "pos_embed" in grads
    # summed over the tokens, pos_embed's gradient is linear_mapper.bias's
    want_pos_sum = g64["linear_mapper.bias"]
    assert np.abs(grads["pos_embed"].astype(np.float64).sum(0) - want_pos_sum).max() <= 1e-4 * np.abs(want_pos_sum).max()
    assert np.abs(grads["pos_embed"]).max() > 0


# ---------------------------------------------------------------------------------------------- kernels alone
def test_attention_kernels_sharp_peaks(pkg):
    L = pkg.lib()
    B, n, heads, dh = 5, 17, 4, 64
    H = heads * dh
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B * n, 3 * H, generator=g, dtype=torch.float64)
    # logits of +-40 on a few keys: q = 40 e_j-ish against unit keys
    qkv[:, :H] = 0.0
    for i in range(B * n):
        for h in range(heads):
            qkv[i, h * dh + (i + h) % dh] = 40.0 * 8.0 * (1 if (i + h) % 3 else -1)
    qkv[:, H:2 * H] = 0.0
    for j in range(B * n):
        for h in range(heads):
            qkv[j, H + h * dh + (j + h) % dh] = 1.0
    dout = torch.randn(B * n, H, generator=g, dtype=torch.float64)
    qd, dd = qkv.float().to(DEV), dout.float().to(DEV)
    o = torch.empty(B * n, H, device=DEV)
    lse = torch.empty(B, heads, n, device=DEV)
    dq = torch.empty(B * n, 3 * H, device=DEV)
    assert L.pl_vit_attn_fwd(qd.data_ptr(), B, n, heads, dh, dh ** -0.5, o.data_ptr(), lse.data_ptr(), _stream()) == 0
    assert L.pl_vit_attn_bwd(qd.data_ptr(), lse.data_ptr(), dd.data_ptr(), B, n, heads, dh, dh ** -0.5, dq.data_ptr(),
                             _stream()) == 0
    x = qkv.float().double().clone().requires_grad_(True)
    q, k, v = x.reshape(B, n, 3 * H).chunk(3, dim=-1)
    q, k, v = (z.reshape(B, n, heads, dh).transpose(1, 2) for z in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * dh ** -0.5
    assert s.abs().max() >= 39.0
    ref = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * n, H)
    ref.backward(dout.float().double())
    assert torch.allclose(o.cpu().double(), ref.detach(), rtol=0, atol=2e-5 * ref.abs().max().item())
    assert torch.allclose(lse.cpu().double(), torch.logsumexp(s, -1).detach(), rtol=1e-6, atol=1e-5)
    gw = x.grad
    assert (dq.cpu().double() - gw).abs().max() <= 1e-4 * gw.abs().max()


@pytest.mark.parametrize("nnorm", [1, 2])
def test_layernorm_kernels_large_mean_small_spread(pkg, nnorm):
    L = pkg.lib()
    T, H = 300, 256
    g = torch.Generator().manual_seed(4)
    x = (1e3 + 1e-2 * torch.randn(T, H, generator=g, dtype=torch.float64)).float()
    add = (1e-2 * torch.randn(T, H, generator=g, dtype=torch.float64)).float()
    ps = [(1 + 0.1 * torch.randn(H, generator=g)).float() if i % 2 == 0 else (0.1 * torch.randn(H, generator=g)).float()
          for i in range(4)]
    dy = torch.randn(T, H, generator=g).float()
    dres = torch.randn(T, H, generator=g).float()
    xd, ad, dyd, drd = (z.to(DEV) for z in (x, add, dy, dres))
    pd = [p.to(DEV) for p in ps]
    xo, y, st = torch.empty(T, H, device=DEV), torch.empty(T, H, device=DEV), torch.empty(nnorm, 2, T, device=DEV)
    assert L.pl_vit_ln_fwd(xd.data_ptr(), ad.data_ptr(), T, H, nnorm, pd[0].data_ptr(), pd[1].data_ptr(), pd[2].data_ptr(),
                           pd[3].data_ptr(), 1e-5, xo.data_ptr(), y.data_ptr(), st.data_ptr(), _stream()) == 0
    dx, dgb = torch.empty(T, H, device=DEV), torch.empty(nnorm * 2 * H, device=DEV)
    scratch = torch.empty(L.pl_vit_ln_bwd_scratch_bytes(T, H, nnorm), dtype=torch.uint8, device=DEV)
    assert L.pl_vit_ln_bwd(dyd.data_ptr(), drd.data_ptr(), xo.data_ptr(), st.data_ptr(), T, H, nnorm, pd[0].data_ptr(),
                           pd[1].data_ptr(), pd[2].data_ptr(), dx.data_ptr(), dgb.data_ptr(), scratch.data_ptr(), _stream()) == 0
    xs = (x + add).double().requires_grad_(True)              # the residual sum is fp32 (x_out): normalise that
    pp = [p.double().requires_grad_(True) for p in ps]
    r = F.layer_norm(xs, (H,), pp[0], pp[1], 1e-5)
    if nnorm == 2:
        r = F.layer_norm(r, (H,), pp[2], pp[3], 1e-5)
    r.backward(dy.double())
    assert torch.equal(xo.cpu(), (x + add))
    assert (y.cpu().double() - r.detach()).abs().max() <= 2e-3, "large mean / small spread: statistics lost precision"
    assert (dx.cpu().double() - (xs.grad + dres.double())).abs().max() <= 1e-3 * xs.grad.abs().max() + 1e-5
    want = [pp[0].grad, pp[1].grad] + ([pp[2].grad, pp[3].grad] if nnorm == 2 else [])
    got = dgb.cpu().double().reshape(len(want), H)
    for gi, w in zip(got, want):
        assert (gi - w).abs().max() <= 1e-4 * w.abs().max()


def test_embedding_kernels_in_d_3(pkg):
    L = pkg.lib()
    B, n, H, d = 7, 17, 256, 3
    g = torch.Generator().manual_seed(6)
    x, W, b, pos = (torch.randn(B * n, d, generator=g), torch.randn(H, d, generator=g), torch.randn(H, generator=g),
                    torch.randn(n, H, generator=g))
    dx = torch.randn(B * n, H, generator=g)
    xd, Wd, bd, pd, dxd = (z.to(DEV) for z in (x, W, b, pos, dx))
    out = torch.empty(B * n, H, device=DEV)
    assert L.pl_vit_embed_fwd(xd.data_ptr(), B * n, d, n, Wd.data_ptr(), bd.data_ptr(), pd.data_ptr(), H, out.data_ptr(),
                              _stream()) == 0
    want = x.double() @ W.double().T + b.double() + pos.double().repeat(B, 1)
    assert (out.cpu().double() - want).abs().max() <= 1e-5
    dwb, dpos, dxin = torch.empty(H * d + H, device=DEV), torch.empty(n, H, device=DEV), torch.empty(B * n, d, device=DEV)
    scratch = torch.empty(L.pl_vit_embed_bwd_scratch_bytes(B * n, d, H), dtype=torch.uint8, device=DEV)
    assert L.pl_vit_embed_bwd(dxd.data_ptr(), xd.data_ptr(), B * n, d, n, H, Wd.data_ptr(), dwb.data_ptr(), dpos.data_ptr(),
                              dxin.data_ptr(), scratch.data_ptr(), _stream()) == 0
    dd = dx.double()
    assert (dwb[:H * d].cpu().double().reshape(H, d) - dd.T @ x.double()).abs().max() <= 1e-4
    assert (dwb[H * d:].cpu().double() - dd.sum(0)).abs().max() <= 1e-4
    assert (dpos.cpu().double() - dd.reshape(B, n, H).sum(0)).abs().max() <= 1e-4
    assert (dxin.cpu().double() - dd @ W.double()).abs().max() <= 1e-4


# ---------------------------------------------------------------------------------------------- determinism, caches, helpers
@pytest.mark.parametrize("mode", MODES)
def test_repeated_step_is_bitwise_equal_and_train_eval_agree(pkg, mode):
    sd, x, t, _, _ = _twin_case(pkg, 64)
    m = pkg.MyViT(compute_dtype=mode).to(DEV)
    m.load_state_dict(sd)
    y1, l1, g1 = _gpu_fwd_bwd(pkg, m, x, t)
    y2, l2, g2 = _gpu_fwd_bwd(pkg, m, x, t)
    assert np.array_equal(y1, y2) and l1 == l2
    for k in g1:
        assert np.array_equal(g1[k], g2[k]), k
    m.eval()
    with torch.no_grad():
        ye = m(torch.as_tensor(x, device=DEV)).cpu().numpy()
    assert np.array_equal(ye, y1)


@pytest.mark.parametrize("mode", MODES)
def test_weight_plane_caches_follow_flatadam_steps(pkg, mode):
    sd, x, t, _, _ = _twin_case(pkg, 64)
    m = pkg.MyViT(compute_dtype=mode).to(DEV)
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
        fresh = pkg.MyViT(compute_dtype=mode).to(DEV)
        fresh.load_state_dict(m.state_dict())
        fresh.eval()
        want = fresh(xd)
    assert torch.equal(after, want)
    assert not torch.equal(after, before)


def test_generic_train_and_eval_helpers(pkg, g12):
    m = _model(pkg, 0, "f16x3").train()
    opt = pkg.FlatAdam(m, lr=1e-4, weight_decay=0.01, decoupled_weight_decay=True)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=0)
    x, t = torch.as_tensor(g12["lift:x"], device=DEV), torch.as_tensor(g12["lift:t"], device=DEV)
    losses = []
    for _ in range(4):
        loss, pred = pkg.train_step(m, opt, x, t)
        losses.append(loss.item())
        sched.step(losses[-1] + 1.0 * (len(losses) > 2))        # a plateau after two steps: the scheduler must act
    assert min(losses[1:]) < losses[0]
    assert opt.param_groups[0]["lr"] < 1e-4
    m.eval()
    loss, metric, y = pkg.eval_step(m, x, t, flip=True)
    assert y.shape == t.shape and torch.isfinite(y).all() and np.isfinite(loss.item())
    assert metric.shape == (17,)
    with torch.no_grad():
        plain = m(x)
    assert not torch.equal(y, plain)                            # flip TTA really averaged two predictions
