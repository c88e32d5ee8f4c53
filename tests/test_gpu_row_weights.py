"""GPU tests of the criterion's per-pose joint weights (PoseCriterion(...)(pred, target, row_weights=); include/poselift.h
PLRowWeightsCriterion): the stand-alone pass of every kind against the fp64 oracle of
tests/row_weights_oracle.py, the bits that must coincide with the per-joint-weighted and the unweighted criterion on every
loss route of plan(), zero-weight rows, the fused / AdamW-riding / ranged / graphed steps, the non-finite sets, an unaligned
weights tensor, the autograd and evaluation routes, and the feeder's weights."""
import ctypes

import numpy as np
import pytest
import torch

import row_weights_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24                     # half an ulp, relative: the most one fp32 rounding moves a result


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _weights(J, seed=3):
    w = np.random.default_rng(seed).uniform(0.25, 2.0, J).astype(np.float32)
    w[0] = 0.0                                      # the zero-centred root joint: a dead target, taken out
    return w


def _crit(pkg, kind, coords, w=None, beta=0.5):
    return pkg.PoseCriterion(kind, beta=beta, joint_weights=w, coords=coords).to(DEV)


# (B, O, G): the shapes of tests/test_gpu_pose_criterion.py (one joint; under one workgroup; one short of / one past a
# workgroup of the pointwise and of the grouped element map; one short of / one past its threads; several workgroups; more
# than 64 joints; G = 1, 2, 3)
SHAPES = [(1, 3, 3), (2, 51, 3), (64, 51, 3), (65, 34, 2), (257, 51, 3), (5, 70, 1), (20, 210, 3),
          (341, 3, 1), (205, 5, 1), (341, 9, 3), (205, 15, 3), (85, 6, 2), (257, 3, 3)]
# the project's bounds for the weighted kinds, in units of U relative; one more with both weight sets: the
# reference then multiplies w_j and rw exactly, the kernel rounds their product once
BOUNDS = {"mse": lambda G: 4, "smooth_l1": lambda G: 5, "mpjpe": lambda G: 6 + (2 + G) / 2}
# (route, in, out, H, stages, dtype, B, coords): the seven routes of tests/test_gpu_pose_criterion.py
ROUTES = [("small", 34, 51, 256, 1, "fp32", 8, 3), ("small", 34, 51, 256, 1, "fp32", 64, 3),
          ("slabs", 51, 34, 64, 2, "fp32", 100, 2), ("slabs", 34, 51, 64, 2, "fp32", 100, 3),
          ("partial", 34, 48, 64, 2, "fp32", 100, 3), ("partial", 34, 51, 40, 2, "fp32", 100, 3),
          ("slabs-f16x3", 34, 51, 1024, 2, "f16x3", 128, 3)]
ROUTE_IDS = [f"{r[0]}-{r[1]}-{r[2]}-H{r[3]}-B{r[6]}" for r in ROUTES]
# (on SmallMse the separate training forward's y differs from the fused step's in the last bits with plain MSE already)
SEPARATE_FORWARD_IS_BITWISE = {"small": False, "slabs": True, "partial": True, "slabs-f16x3": True}


def _standalone(crit, p, t, rw):
    """(loss, dpred) of the stand-alone pass, device tensors"""
    pd = p.detach().clone().requires_grad_(True)
    loss = crit(pd, t, row_weights=rw) if rw is not None else crit(pd, t)
    loss.backward()
    return loss.detach(), pd.grad


# ------------------------------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("scale", [1.0, 1e3])
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("kind", orc.KINDS)
def test_standalone_pass_vs_fp64_oracle(pkg, kind, both, scale):
    """Loss to 1e-5 relative; every gradient element within BOUNDS (+ 1 with both weight sets) x 2^-24 relative of the fp64
    gradient; l1 exactly +-coef W or 0.  dpred = NULL leaves the loss unchanged.  The measured maxima are printed (DESIGN
    3d.2b records them)."""
    worst = 0.0
    for B, O, G in SHAPES:
        J = O // G
        rng = np.random.default_rng(1000 * B + O)
        p = (rng.standard_normal((B, O)) * scale).astype(np.float32)
        t = (rng.standard_normal((B, O)) * scale).astype(np.float32)
        t[0, :G] = p[0, :G]                                             # an exactly-zero joint
        t[B - 1, O - 1] = p[B - 1, O - 1]                               # a zero coordinate
        beta = 0.5 * scale
        if O > G:
            p[0, G], t[0, G] = np.float32(1.5 * scale), np.float32(1.0 * scale)      # |d| == beta exactly
        rw = orc.weights(B, J, seed=B + O)
        w = _weights(J) if both else None
        crit = _crit(pkg, kind, G, w, beta)
        loss, got = _standalone(crit, _t(p), _t(t), _t(rw))
        got = got.cpu().numpy()
        with torch.no_grad():
            assert crit(_t(p), _t(t), row_weights=_t(rw)).item() == loss.item()             # dpred = NULL
        W32 = orc.effective_weights(rw, w)
        W64 = rw.astype(np.float64) * (w.astype(np.float64)[None, :] if both else 1.0)
        want_l, want_g = orc.criterion(kind, p, t, G, W64, beta=beta)
        rel = abs(loss.item() - want_l) / abs(want_l) if want_l != 0 else abs(loss.item())
        assert rel <= 1e-5, (B, O, G, loss.item(), want_l)
        if kind == "l1":
            assert np.array_equal(got, orc.grad_fp32(kind, p, t, G, W32, beta=beta)), (B, O, G)
        else:
            k = BOUNDS[kind](G) + (1 if both else 0)
            err = np.abs(got.astype(np.float64) - want_g)
            nz = want_g != 0
            units = (err[nz] / (np.abs(want_g[nz]) * U)).max() if nz.any() else 0.0
            worst = max(worst, units)
            assert (err <= 1.001 * k * U * np.abs(want_g)).all(), (B, O, G, units, k)
        zero = want_g == 0
        assert (got[zero] == 0).all()
        assert zero[np.repeat(W64, G, axis=1) == 0].all()
    print(f"{kind} both={both} scale={scale}: gradient max {worst:.2f} x 2^-24 relative")


# ------------------------------------------------------------------------------------------------- 2. bits that coincide
def _triples(pkg, kind, G, B, J):
    """[(criterion, row weights) ...] in pairs that must give the same bits"""
    w = _weights(J)
    rw = orc.weights(B, J, seed=7)
    ones = np.ones((B, J), np.float32)
    rw2 = (torch.from_numpy(w)[None, :] * torch.from_numpy(rw)).numpy()             # formed by torch in fp32
    return [((_crit(pkg, kind, G, w, 0.1), None), (_crit(pkg, kind, G, None, 0.1), _t(np.tile(w, (B, 1))))),
            ((_crit(pkg, kind, G, None, 0.1), None), (_crit(pkg, kind, G, None, 0.1), _t(ones))),
            ((_crit(pkg, kind, G, w, 0.1), _t(rw)), (_crit(pkg, kind, G, None, 0.1), _t(rw2)))]


@pytest.mark.parametrize("kind", orc.KINDS)
def test_standalone_bits_coincide(pkg, kind):
    """rw[b][j] = w_j is joint_weights = w; all-ones rw is the unweighted criterion; joint_weights = w with rw is rw2 = w[None] *
    rw alone: loss and dpred bit for bit, on every shape."""
    for B, O, G in SHAPES:
        rng = np.random.default_rng(B + O)
        p, t = _t(rng.standard_normal((B, O)).astype(np.float32)), _t(rng.standard_normal((B, O)).astype(np.float32))
        for (ca, ra), (cb, rb) in _triples(pkg, kind, G, B, O // G):
            la, ga = _standalone(ca, p, t, ra)
            lb, gb = _standalone(cb, p, t, rb)
            assert torch.equal(la, lb) and torch.equal(ga, gb), (B, O, G)


def _model(pkg, i_dim, o_dim, H, S, dtype="fp32", p=0.5):
    torch.manual_seed(7)
    m = pkg.LinearModel(i_dim, o_dim, linear_size=H, num_stage=S, p_dropout=p, compute_dtype=dtype).to(DEV).train()
    m.manual_seed(3)
    return m


def _batch(B, i_dim, o_dim, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, i_dim, generator=g).to(DEV), (torch.rand(B, o_dim, generator=g) - 0.5).to(DEV)


def _fused(pkg, route, crit, rw):
    _, i_dim, o_dim, H, S, dtype, B, G = route
    x, t = _batch(B, i_dim, o_dim)
    m = _model(pkg, i_dim, o_dim, H, S, dtype)
    loss, y = m.fused_train_fwd_bwd(x, t, criterion=crit, row_weights=rw)
    return loss.clone(), y.detach().clone(), m.flat_grads.clone()


@pytest.mark.parametrize("kind", orc.KINDS)
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_route_bits_coincide(pkg, route, kind):
    """The same three identities on every loss route of the fused step: loss, y and the whole gradient arena bit for bit."""
    _, i_dim, o_dim, H, S, dtype, B, G = route
    for (ca, ra), (cb, rb) in _triples(pkg, kind, G, B, o_dim // G):
        for a, b in zip(_fused(pkg, route, ca, ra), _fused(pkg, route, cb, rb)):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- 3. zero-weight rows
@pytest.mark.parametrize("kind", orc.KINDS)
def test_zero_weight_rows(pkg, kind):
    """A row of zero weights with finite d: dpred == 0 on every element of it; a batch padded with such rows gives the
    unpadded loss times B / B_padded (1e-6 relative: the padding adds exact zeros, only the order of the sums moves)."""
    B, Bp, J, G = 50, 64, 17, 3
    rng = np.random.default_rng(4)
    p, t = rng.standard_normal((Bp, J * G)).astype(np.float32), rng.standard_normal((Bp, J * G)).astype(np.float32)
    rw = rng.uniform(0.0, 2.0, (Bp, J)).astype(np.float32)
    rw[B:] = 0.0
    rw[3] = 0.0
    for w in (None, _weights(J)):
        crit = _crit(pkg, kind, G, w)
        lp, gp = _standalone(crit, _t(p), _t(t), _t(rw))
        assert (gp[B:] == 0).all() and (gp[3] == 0).all() and gp[:B].abs().max().item() > 0
        lu, gu = _standalone(crit, _t(p[:B]), _t(t[:B]), _t(rw[:B]))
        assert abs(lp.item() - lu.item() * B / Bp) <= 1e-6 * abs(lu.item() * B / Bp), (lp.item(), lu.item())
        assert (gu[3] == 0).all()


# ------------------------------------------------------------------------------------------------- 4. the fused step
def _bwd_on_saved_state(pkg, m, x, y, t, crit, rw):
    """stand-alone criterion on y -> dy -> pl_lifter_bwd on the workspace the model's last forward wrote: the gradient arena"""
    yd = y.detach().clone().requires_grad_(True)
    crit(yd, t, row_weights=rw).backward()
    ws, g = m.last_workspace, torch.zeros_like(m.flat_grads)
    rc = pkg.lib().pl_lifter_bwd(ctypes.byref(m._desc), x.data_ptr(), yd.grad.data_ptr(), x.shape[0], ws["buf"].data_ptr(),
                                 ws["bytes"], None, g.data_ptr(), pkg._lib.current_stream_ptr())
    pkg._lib.check(rc, "pl_lifter_bwd")
    return g


@pytest.mark.parametrize("kind", orc.KINDS)
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_fused_step_is_the_separate_calls(pkg, route, kind):
    """fused_train_fwd_bwd(criterion=, row_weights=): the arena is, bit for bit, the stand-alone criterion on the returned y
    followed by pl_lifter_bwd on the saved state (every route, SmallMse included); on FromSlabs (fp32 and the f16x3 whole-tile
    case) and PartialOnly y and the arena are also the training forward, the stand-alone criterion and the backward in a row.
    The loss within 1e-5 relative of the fp64 oracle on the returned y.  (l1 and mpjpe with joint weights as well.)"""
    name, i_dim, o_dim, H, S, dtype, B, G = route
    J = o_dim // G
    x, t = _batch(B, i_dim, o_dim)
    w = _weights(J) if kind in ("l1", "mpjpe") else None
    rwn = orc.weights(B, J, seed=5)
    rw = _t(rwn)
    crit = _crit(pkg, kind, G, w, beta=0.1)
    m = _model(pkg, i_dim, o_dim, H, S, dtype)
    loss, y = m.fused_train_fwd_bwd(x, t, criterion=crit, row_weights=rw)
    grads = m.flat_grads.clone()
    assert torch.equal(grads, _bwd_on_saved_state(pkg, m, x, y, t, crit, rw))
    m0 = _model(pkg, i_dim, o_dim, H, S, dtype)
    assert torch.equal(y, m0.fused_train_fwd_bwd(x, t)[1])
    if SEPARATE_FORWARD_IS_BITWISE[name]:
        m2 = _model(pkg, i_dim, o_dim, H, S, dtype)
        y2 = m2(x)
        crit(y2, t, row_weights=rw).backward()
        assert torch.equal(y, y2.detach())
        assert torch.equal(grads, m2.flat_grads)
    want, _ = orc.criterion(kind, y.cpu().numpy(), t.cpu().numpy(), G, orc.effective_weights(rwn, w), beta=0.1)
    assert abs(loss.item() - want) <= 1e-5 * abs(want), (loss.item(), want)
    assert grads.abs().max().item() > 0


def test_lifter_entry_points_refuse_and_need_a_criterion(pkg):
    m = _model(pkg, 34, 51, 256, 1)
    x, t = _batch(8, 34, 51)
    with pytest.raises(ValueError, match="criterion"):
        m.fused_train_fwd_bwd(x, t, row_weights=torch.ones(8, 17, device=DEV))
    with pytest.raises(ValueError, match="row_weights has shape"):
        m.fused_train_fwd_bwd(x, t, criterion=_crit(pkg, "l1", 3), row_weights=torch.ones(8, 16, device=DEV))
    L = pkg._lib
    ws = m._acquire_workspace(8)
    y, loss = torch.empty(8, 51, device=DEV), torch.zeros((), device=DEV)
    before = m.flat_grads.clone()
    for flags, msg in ((L.CRIT_HAS_ROW_WEIGHTS, b"null row_weights"), (L.CRIT_HAS_ROW_WEIGHTS | L.CRIT_HAS_SKELETON, b"not built")):
        st = L.PLRowWeightsCriterion(L.CRIT_L1 | flags, 3, 1.0, None)
        st.row_weights = None if flags == L.CRIT_HAS_ROW_WEIGHTS else y.data_ptr()
        rc = pkg.lib().pl_lifter_train_fwd_bwd_crit(ctypes.byref(m._desc), x.data_ptr(), t.data_ptr(), 8, ws["buf"].data_ptr(),
                                                    ws["bytes"], m._seed, 1, ctypes.byref(st), y.data_ptr(), loss.data_ptr(),
                                                    m.flat_grads.data_ptr(), 3, 0, L.current_stream_ptr())
        assert rc == -1 and msg in pkg.lib().pl_last_error()
    m._release_workspace(ws)
    assert torch.equal(before, m.flat_grads)


# ------------------------------------------------------------------------------------------------- 5. AdamW riding
@pytest.mark.parametrize("kind", ["l1", "mpjpe"])
def test_adamw_riding_step_is_fused_plus_optimizer_step(pkg, kind):
    """B = 64: the riding step (pl_lifter_train_step_crit) equals fused_train_fwd_bwd(criterion=, row_weights=) +
    optimizer.step() bit for bit on parameters, both moments and the losses of three steps with three weight tensors."""
    B, out = 64, []
    crit = _crit(pkg, kind, 3, _weights(17))
    for in_call in (True, False):
        m = _model(pkg, 34, 51, 256, 1)
        opt = pkg.FlatAdamW(m, lr=1e-3, weight_decay=0.02)
        assert m.step_carries_adamw(B)
        losses = []
        for i in range(3):
            x, t = _batch(B, 34, 51, seed=40 + i)
            rw = _t(orc.weights(B, 17, seed=i))
            if in_call:
                loss, _ = pkg.train_step(m, opt, x, t, criterion=crit, row_weights=rw)
            else:
                loss, _ = m.fused_train_fwd_bwd(x, t, criterion=crit, row_weights=rw)
                opt.step()
            losses.append(loss.clone())
        assert opt.state_dict()["state"][0]["step"] == 3
        out.append((torch.stack(losses), m.flat_params.clone(), opt._m.clone(), opt._v.clone(), m.flat_grads.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    # the weights mattered: the unweighted first step gives another loss
    m = _model(pkg, 34, 51, 256, 1)
    loss, _ = pkg.train_step(m, pkg.FlatAdamW(m, lr=1e-3, weight_decay=0.02), *_batch(B, 34, 51, seed=40), criterion=crit)
    assert loss.item() != out[0][0][0].item()


# ------------------------------------------------------------------------------------------------- 6. layer ranges
@pytest.mark.parametrize("route", [ROUTES[2], ROUTES[3]], ids=[ROUTE_IDS[2], ROUTE_IDS[3]])
def test_layer_ranges_equal_the_single_call(pkg, route):
    """pl_lifter_train_fwd_bwd_crit over (L, 2) then (1, 0) -- the data-parallel overlap -- against (L, 0), with row weights:
    bit for bit."""
    _, i_dim, o_dim, H, S, dtype, B, G = route
    x, t = _batch(B, i_dim, o_dim)
    crit = _crit(pkg, "mpjpe", G, _weights(o_dim // G))
    rw = _t(orc.weights(B, o_dim // G, seed=9))
    L, lib = 1 + 2 * S, pkg.lib()
    outs = []
    for ranges in (((L, 0),), ((L, 2), (1, 0))):
        m = _model(pkg, i_dim, o_dim, H, S, dtype)
        ws = m._acquire_workspace(B)
        y, loss = torch.empty(B, o_dim, device=DEV), torch.zeros((), device=DEV)
        st = crit.struct(o_dim, x.device, rw)
        for hi, lo in ranges:
            rc = lib.pl_lifter_train_fwd_bwd_crit(ctypes.byref(m._desc), x.data_ptr(), t.data_ptr(), B, ws["buf"].data_ptr(),
                                                  ws["bytes"], m._seed, 1, ctypes.byref(st), y.data_ptr(), loss.data_ptr(),
                                                  m.flat_grads.data_ptr(), hi, lo, pkg._lib.current_stream_ptr())
            pkg._lib.check(rc, "pl_lifter_train_fwd_bwd_crit")
        torch.cuda.synchronize()
        outs.append((y.clone(), loss.clone(), m.flat_grads.clone()))
        m._release_workspace(ws)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert outs[0][1].item() > 0
    single = _fused(pkg, route, crit, rw)
    assert torch.equal(single[0], outs[0][1]) and torch.equal(single[2], outs[0][2])


# ------------------------------------------------------------------------------------------------- 7. graph replay
def test_graphed_step_replays_the_eager_step(pkg):
    """Three replays of a GraphedTrainStep at B = 8 equal three eager steps bit for bit, with other weights each step; an
    in-place edit of step.row_weights is seen by the next replay; a call without weights on a weighted step raises, and a
    call with weights on an unweighted one."""
    B = 8
    res = []
    for graphed in (False, True):
        m = _model(pkg, 34, 51, 256, 1)
        opt = pkg.FlatAdamW(m, lr=1e-3)
        crit = _crit(pkg, "smooth_l1", 3, _weights(17), beta=0.1)
        x, t = _batch(B, 34, 51)
        step = pkg.GraphedTrainStep(m, opt, x, t, criterion=crit, row_weights=torch.ones(B, 17, device=DEV)) if graphed else None
        out = []
        for i in range(4):
            xi, ti = _batch(B, 34, 51, seed=20 + i)
            rw = _t(orc.weights(B, 17, seed=30 + min(i, 2)))
            if i == 3:                                   # the fourth step: the third's weights, edited in place
                rw[:, 5] = 3.0
                rw[2] *= 0.5
            if not graphed:
                loss, y = pkg.train_step(m, opt, xi, ti, criterion=crit, row_weights=rw)
            elif i < 3:
                loss, y = step(xi, ti, row_weights=rw)
            else:
                assert step.row_weights.shape == (B, 17) and step.row_weights.data_ptr() != rw.data_ptr()
                step.row_weights[:, 5] = 3.0
                step.row_weights[2] *= 0.5
                loss, y = step(xi, ti, row_weights=step.row_weights)
            out += [loss.clone(), y.clone()]
        res.append(out + [m.flat_params.clone(), opt._m.clone(), opt._v.clone()])
        if graphed:
            with pytest.raises(ValueError, match="row_weights"):
                step(xi, ti)
            with pytest.raises(ValueError, match="row_weights"):
                step(xi, ti, row_weights=torch.ones(B, 16, device=DEV))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert len({o.item() for o in res[0][0:8:2]}) == 4
    m = _model(pkg, 34, 51, 256, 1)
    x, t = _batch(B, 34, 51)
    plain = pkg.GraphedTrainStep(m, pkg.FlatAdamW(m, lr=1e-3), x, t, criterion=_crit(pkg, "l1", 3))
    assert plain.row_weights is None
    with pytest.raises(ValueError, match="row_weights"):
        plain(x, t, row_weights=torch.ones(B, 17, device=DEV))


# ------------------------------------------------------------------------------------------------- 8. non-finite values
@pytest.mark.parametrize("zero_weight", [False, True])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("kind", orc.KINDS)
def test_nonfinite_set_is_torch_cpus(pkg, kind, bad, zero_weight):
    """One poisoned element of pred, under a non-zero and under a zero weight: the non-finite loss and gradient entries sit
    where torch's (fp32, CPU) do, with and without joint weights."""
    for w in (None, np.linspace(0.5, 1.5, 17).astype(np.float32)):
        rng = np.random.default_rng(5)
        p, t = rng.standard_normal((6, 51)).astype(np.float32), rng.standard_normal((6, 51)).astype(np.float32)
        rw = rng.uniform(0.5, 1.5, (6, 17)).astype(np.float32)
        p[2, 7] = bad
        if zero_weight:
            rw[2, 7 // 3] = 0.0
        want_l, want_g = orc.torch_criterion(kind, p, t, 3, orc.effective_weights(rw, w), 0.5, dtype=np.float32)
        loss, got = _standalone(_crit(pkg, kind, 3, w), _t(p), _t(t), _t(rw))
        got = got.cpu().numpy()
        assert np.isnan(loss.item()) == np.isnan(want_l) and np.isinf(loss.item()) == np.isinf(want_l)
        assert np.array_equal(np.isnan(got), np.isnan(want_g)) and np.array_equal(np.isinf(got), np.isinf(want_g))
        fin = np.isfinite(want_g)
        np.testing.assert_allclose(got[fin], want_g[fin], rtol=1e-5, atol=0)


# ------------------------------------------------------------------------------------------------- 9. alignment
@pytest.mark.parametrize("kind", orc.KINDS)
def test_weights_off_16_byte_alignment(pkg, kind):
    """rw a contiguous view that starts 4 bytes off 16-byte alignment: the aligned call's bits, stand-alone and on a slabs and a
    small route."""
    def off(a):
        buf = torch.empty(a.numel() + 1, dtype=torch.float32, device=DEV)
        v = buf[1:].view(a.shape)
        v.copy_(a)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    for B, O, G in ((65, 34, 2), (257, 51, 3), (5, 70, 1)):
        rng = np.random.default_rng(B)
        p, t = _t(rng.standard_normal((B, O)).astype(np.float32)), _t(rng.standard_normal((B, O)).astype(np.float32))
        rw = _t(orc.weights(B, O // G, seed=1))
        assert rw.data_ptr() % 16 == 0
        crit = _crit(pkg, kind, G, _weights(O // G))
        for a, b in zip(_standalone(crit, p, t, rw), _standalone(crit, p, t, off(rw))):
            assert torch.equal(a, b)
    for route in (ROUTES[0], ROUTES[3]):
        B, G, J = route[6], route[7], route[2] // route[7]
        rw = _t(orc.weights(B, J, seed=1))
        crit = _crit(pkg, kind, G, None)
        for a, b in zip(_fused(pkg, route, crit, rw), _fused(pkg, route, crit, off(rw))):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- 10. other routes
def test_train_step_on_another_model_is_the_autograd_composition(pkg):
    """train_step(MyViT, FlatAdam, criterion=l1, row_weights=) = zero_grad, forward, criterion, backward, step by hand."""
    g = torch.Generator().manual_seed(2)
    x, t = torch.rand(8, 17, 2, generator=g).to(DEV), (torch.rand(8, 17, 3, generator=g) - 0.5).to(DEV)
    rwn = orc.weights(8, 17, seed=2)
    rw = _t(rwn)
    crit = _crit(pkg, "l1", 3, _weights(17))
    torch.manual_seed(1)
    sd = {k: v.clone() for k, v in pkg.MyViT(n_blocks=1, compute_dtype="fp32").state_dict().items()}
    res = []
    for by_hand in (False, True):
        m = pkg.MyViT(n_blocks=1, compute_dtype="fp32").to(DEV)
        m.load_state_dict(sd)
        m.train()
        opt = pkg.FlatAdam(m, lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True)
        for _ in range(2):
            if by_hand:
                opt.zero_grad()
                y = m(x).reshape(t.shape)
                loss = crit(y, t, row_weights=rw)
                loss.backward()
                opt.step()
            else:
                loss, y = pkg.train_step(m, opt, x, t, criterion=crit, row_weights=rw)
        res.append([loss.detach().clone(), y.detach().clone()] + [v.detach().clone() for v in m.state_dict().values()])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    want, _ = orc.criterion("l1", res[0][1].reshape(8, 51).cpu().numpy(), t.reshape(8, 51).cpu().numpy(), 3,
                            orc.effective_weights(rwn, _weights(17)))
    assert abs(res[0][0].item() - want) <= 1e-5 * want


def test_eval_step_returns_the_criterions_loss(pkg):
    m = _model(pkg, 34, 51, 256, 1).eval()
    x, t = _batch(16, 34, 51)
    rw = _t(orc.weights(16, 17, seed=3))
    crit = _crit(pkg, "mpjpe", 3, _weights(17))
    loss, metric, y = pkg.eval_step(m, x.reshape(16, 17, 2), t.reshape(16, 17, 3), criterion=crit, row_weights=rw)
    assert torch.equal(loss, crit(y, t.reshape(16, 17, 3), row_weights=rw)) and metric.shape == (17,)
    plain, _, y0 = pkg.eval_step(m, x.reshape(16, 17, 2), t.reshape(16, 17, 3), criterion=crit)
    assert torch.equal(y0, y) and plain.item() != loss.item()
    mask = rw > 0                                                           # a bool mask is converted
    a = crit(y, t.reshape(16, 17, 3), row_weights=mask)
    assert torch.equal(a, crit(y, t.reshape(16, 17, 3), row_weights=mask.float()))
    # the masked mean through normalize_row_weights
    d = (y - t.reshape(16, 17, 3)).norm(dim=-1).double().cpu()
    wj = torch.from_numpy(_weights(17)).double()
    want = (d * wj * mask.cpu()).sum() / mask.sum().item()
    got = crit(y, t.reshape(16, 17, 3), row_weights=pkg.normalize_row_weights(mask))
    assert abs(got.item() - want.item()) <= 1e-5 * want.item()


# ------------------------------------------------------------------------------------------------- 11. the feeder
N_ROWS = 150
AUG = dict(p_flip=0.5, max_rot=0.4, scale_range=0.2, max_shift=0.05, jitter_sigma=0.01, seed=0xC0FFEE1234)


def _tables():
    rng = np.random.default_rng(8)
    x2d = rng.uniform(0.2, 0.8, (N_ROWS, 17, 2)).astype(np.float32)
    y3d = rng.standard_normal((N_ROWS, 17, 3)).astype(np.float32)
    y3d[:, :, 2] = np.arange(17, dtype=np.float32)[None, :]                 # z of joint j is j: no stage moves z
    return torch.from_numpy(x2d), torch.from_numpy(y3d)


@pytest.mark.parametrize("crop", [False, True])
@pytest.mark.parametrize("resident", [True, False])
def test_feeder_weights_follow_the_flip(pkg, resident, crop):
    """Every augmentation stage on, p_flip = 0.5: for every row of an epoch the joint order read from z of the 3-D batch equals
    the weights of w[n][j] = j; w is the tuple's last item, with and without a crop; both flip states occur."""
    x2d, y3d = _tables()
    w = torch.arange(17, dtype=torch.float32).repeat(N_ROWS, 1)
    kw = dict(crop=pkg.PersonCrop(), frame_hw=(480, 640)) if crop else {}
    f = pkg.PoseFeeder(x2d, y3d, 64, device=DEV, seed=1, resident=resident, augment=pkg.PoseAugment(**AUG), weights=w, **kw)
    f.set_epoch(2)
    seen, flips = 0, 0
    for batch in f:
        assert len(batch) == (4 if crop else 3)
        y2, wb = batch[1], batch[-1]
        if crop:
            assert batch[2].shape == (y2.shape[0], 4)
        assert wb.shape == (y2.shape[0], 17) and wb.dtype == torch.float32 and wb.device == y2.device
        assert torch.equal(wb, y2[:, :, 2])
        flips += int((wb[:, 1] == 4).sum().item())
        seen += wb.shape[0]
    assert seen == N_ROWS and 0 < flips < N_ROWS


def test_feeder_weights_are_a_function_of_row_and_epoch(pkg):
    """The weights of dataset row r in epoch e are the same bits under batch sizes 7 and 64 and in the resident and the streamed
    mode; they are gather_row_weights' on the same rows; augment=None is the plain table[idx]."""
    x2d, y3d = _tables()
    rng = np.random.default_rng(9)
    w = torch.from_numpy(rng.uniform(0.0, 2.0, (N_ROWS, 17)).astype(np.float32))
    w[:, 0] = torch.arange(N_ROWS, dtype=torch.float32)                    # joint 0 never swaps: the row's identity
    aug = pkg.PoseAugment(**AUG)
    per_config = []
    for bs in (7, 64):
        for resident in (True, False):
            f = pkg.PoseFeeder(x2d, y3d, bs, device=DEV, seed=1, resident=resident, augment=aug, weights=w)
            f.set_epoch(5)
            rows = {}
            for _, _, wb in f:
                for r in wb.cpu():
                    rows[int(r[0].item())] = r.clone()
            assert sorted(rows) == list(range(N_ROWS))
            per_config.append(torch.stack([rows[i] for i in range(N_ROWS)]))
    for other in per_config[1:]:
        assert torch.equal(per_config[0], other)
    ids = torch.arange(N_ROWS, device=DEV)
    again = pkg.gather_row_weights(w.to(DEV), augment=aug, row_ids=ids, epoch=5)
    assert torch.equal(again.cpu(), per_config[0])
    picked = pkg.gather_row_weights(w.to(DEV), augment=aug, epoch=5, src_idx=ids[10:20])          # row_ids default to src_idx
    assert torch.equal(picked.cpu(), per_config[0][10:20])
    for resident in (True, False):                 # no augmentation (a validation feeder): any J, no launch in the streamed mode
        f = pkg.PoseFeeder(x2d, y3d, 64, device=DEV, seed=1, shuffle=False, resident=resident, weights=w[:, :5].contiguous())
        at, kept = 0, []
        for y1, y2, wb in f:
            assert torch.equal(wb.cpu(), w[at:at + wb.shape[0], :5])
            kept.append(wb.clone())
            at += wb.shape[0]
            del wb                                  # the staged block goes back to the allocator while copies are in flight
        assert at == N_ROWS and torch.equal(torch.cat(kept).cpu(), w[:, :5])
        f = pkg.PoseFeeder(x2d, y3d, 7, device=DEV, seed=3, resident=resident, weights=w)          # shuffled: w[idx], row by row
        got = torch.cat([wb for _, _, wb in f]).cpu()
        assert torch.equal(got, w[got[:, 0].long()]) and sorted(got[:, 0].tolist()) == list(range(N_ROWS))
    assert torch.equal(pkg.gather_row_weights(w.to(DEV)).cpu(), w)
    bad = pkg.gather_row_weights(w.to(DEV), src_idx=torch.tensor([3, N_ROWS, -1]))
    assert torch.equal(bad[0].cpu(), w[3]) and bad[1:].isnan().all()
