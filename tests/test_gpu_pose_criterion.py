"""GPU tests of the train step's criterion (pl.PoseCriterion; include/poselift.h PLCriterion): the stand-alone
pass of every kind against the fp64 oracle of tests/pose_criterion_oracle.py on the same fp32 inputs, plain MSE bit for bit
what it always was, the fused step equal to forward -> criterion -> backward on every loss route of plan(), and the train /
graphed / eval steps."""
import ctypes

import numpy as np
import pytest
import torch

import pose_criterion_oracle as orc

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


# (B, O, G).  The pointwise element map puts 256 threads x <= 4 elements in a workgroup and the grouped one 256 threads x <= 4
# joints: one joint; under one workgroup; 1023 / 1025 elements and 1023 / 1025 joints (one short of / one past a workgroup of
# each map); 255 / 257 joints (one short of / one past its threads); several workgroups; 70 joints (more than 64); G = 1, 2, 3
SHAPES = [(1, 3, 3), (2, 51, 3), (64, 51, 3), (65, 34, 2), (257, 51, 3), (5, 70, 1), (20, 210, 3),
          (341, 3, 1), (205, 5, 1), (341, 9, 3), (205, 15, 3), (85, 6, 2), (257, 3, 3)]
# roundings between the fp32 inputs and one gradient element, in the expressions the header documents (each moves the
# result by at most U, relative; products and quotients only, so the relative errors add to first order):
#   mse         d, coef = s 2 / n, d * coef                                                        3   (+ 1: * w)
#   smooth_l1   d, coef = s / n, cb = coef / beta, d * cb  (the linear arm: coef alone)              4   (+ 1: * w)
#   mpjpe       d_g; ss: 2 from the d's squared + G from its G rounded steps, halved by the root: (2 + G) / 2; the root; coef
#               = s / (B J); cw / r; d_g * q                                                        5 + (2 + G) / 2   (+ 1: coef * w)
ROUNDINGS = {"mse": lambda G: 3, "smooth_l1": lambda G: 4, "mpjpe": lambda G: 5 + (2 + G) / 2}


@pytest.mark.parametrize("scale", [1.0, 1e3])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", orc.KINDS)
def test_standalone_pass_vs_fp64_oracle(pkg, kind, weighted, scale):
    """Loss to 1e-5 relative (the bound tests/test_gpu_losses.py derives for this structure: positive terms, per-thread chains
    of a few terms, fixed trees).  Gradient: mse to 2 ulp as there; l1 exactly the documented fp32 expression; smooth_l1 and
    mpjpe within ROUNDINGS x half an ulp (relative; second-order terms: a factor 1.001) of the fp64 gradient -- and mse,
    weighted, too.  Exact zeros where the table says 0; dpred = NULL (no gradient wanted) leaves the loss unchanged.
    The measured maxima are printed (and recorded in DESIGN 3d.2)."""
    worst = 0.0
    for B, O, G in SHAPES:
        J = O // G
        rng = np.random.default_rng(1000 * B + O)
        p = (rng.standard_normal((B, O)) * scale).astype(np.float32)
        t = (rng.standard_normal((B, O)) * scale).astype(np.float32)
        t[0, :G] = p[0, :G]                                             # an exactly-zero joint
        t[B - 1, O - 1] = p[B - 1, O - 1]                               # a zero coordinate (inside a non-zero joint where G > 1)
        beta = 0.5 * scale
        if O > G:
            p[0, G], t[0, G] = np.float32(1.5 * scale), np.float32(1.0 * scale)      # |d| == beta exactly
        w = _weights(J) if weighted else None
        crit = _crit(pkg, kind, G, w, beta)
        pd = _t(p).requires_grad_(True)
        loss = crit(pd, _t(t))
        loss.backward()
        got = pd.grad.cpu().numpy()
        with torch.no_grad():
            assert crit(_t(p), _t(t)).item() == loss.item()             # dpred = NULL
            assert crit(_t(p).reshape(B, J, G), _t(t).reshape(B, J, G)).item() == loss.item()
        want_l, want_g = orc.criterion(kind, p, t, G, w, beta=beta)
        rel = abs(loss.item() - want_l) / abs(want_l) if want_l != 0 else abs(loss.item())
        assert rel <= 1e-5, (B, O, G, loss.item(), want_l)
        if kind == "l1":
            assert np.array_equal(got, orc.grad_fp32(kind, p, t, G, w, beta=beta)), (B, O, G)
        else:
            k = ROUNDINGS[kind](G) + (1 if weighted else 0)
            err = np.abs(got.astype(np.float64) - want_g)
            nz = want_g != 0
            units = (err[nz] / (np.abs(want_g[nz]) * U)).max() if nz.any() else 0.0
            worst = max(worst, units)
            assert (err <= 1.001 * k * U * np.abs(want_g)).all(), (B, O, G, units, k)
            if kind == "mse" and not weighted and nz.any():
                ulps = err[nz] / np.spacing(np.abs(want_g[nz]).astype(np.float32)).astype(np.float64)
                assert ulps.max() <= 2.0
        zero = want_g == 0
        assert (got[zero] == 0).all()
        if kind in ("l1", "mpjpe"):
            assert zero[0, :G].all()
        if weighted and O > G:
            assert zero[:, :G].all() and not zero[:, G:].all()
    print(f"{kind} weighted={weighted} scale={scale}: gradient max {worst:.2f} x 2^-24 relative")


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("kind", orc.KINDS)
def test_nonfinite_set_is_torch_cpus(pkg, kind, bad):
    """One poisoned element: the non-finite loss and gradient values sit where torch's (fp32, CPU) do."""
    for w in (None, np.linspace(0.5, 1.5, 17).astype(np.float32)):
        rng = np.random.default_rng(5)
        p, t = rng.standard_normal((6, 51)).astype(np.float32), rng.standard_normal((6, 51)).astype(np.float32)
        p[2, 7] = bad
        want_l, want_g = orc.torch_criterion(kind, p, t, 3, w, 0.5, dtype=np.float32)
        pd = _t(p).requires_grad_(True)
        loss = _crit(pkg, kind, 3, w)(pd, _t(t))
        loss.backward()
        got = pd.grad.cpu().numpy()
        assert np.isnan(loss.item()) == np.isnan(want_l) and np.isinf(loss.item()) == np.isinf(want_l)
        assert np.array_equal(np.isnan(got), np.isnan(want_g)) and np.array_equal(np.isinf(got), np.isinf(want_g))
        fin = np.isfinite(want_g)
        np.testing.assert_allclose(got[fin], want_g[fin], rtol=1e-5, atol=0)


# ------------------------------------------------------------------------------------------------- the lifter's routes
def _model(pkg, i_dim, o_dim, H, S, dtype="fp32", p=0.5):
    torch.manual_seed(7)
    m = pkg.LinearModel(i_dim, o_dim, linear_size=H, num_stage=S, p_dropout=p, compute_dtype=dtype).to(DEV).train()
    m.manual_seed(3)
    return m


def _batch(B, i_dim, o_dim, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, i_dim, generator=g).to(DEV), (torch.rand(B, o_dim, generator=g) - 0.5).to(DEV)


# (route, in, out, H, stages, dtype, B, coords); the route of each is what plan() (csrc/api.hip) gives these shapes: SmallMse at
# B <= 64 with H a multiple of 256 and out <= 64; FromSlabs above that where H is a multiple of 64 and out is 51 or 34;
# PartialOnly for any other out (48: the reference's 16-joint prototype) or H (40)
ROUTES = [("small", 34, 51, 256, 1, "fp32", 8, 3), ("small", 34, 51, 256, 1, "fp32", 64, 3),
          ("slabs", 51, 34, 64, 2, "fp32", 100, 2), ("slabs", 34, 51, 64, 2, "fp32", 100, 3),
          ("partial", 34, 48, 64, 2, "fp32", 100, 3), ("partial", 34, 51, 40, 2, "fp32", 100, 3),
          ("slabs-f16x3", 34, 51, 1024, 2, "f16x3", 128, 3)]
ROUTE_IDS = [f"{r[0]}-{r[1]}-{r[2]}-H{r[3]}-B{r[6]}" for r in ROUTES]
# The SmallMse route forms y from the H / 16 slabs its last hidden layer's launch leaves; the separate training forward runs the
# output Linear as a GEMM.  The two y differ in the last bits with plain MSE already (measured on the code before the
# criterion: max |dy| 3.6e-7 at B = 8, 4.8e-7 at B = 64, and the gradient arenas with them), and MSE's bits may not move -- so
# there the fused step is compared bit for bit with what CAN equal it: the MSE step's y, and the stand-alone criterion on the
# returned y followed by pl_lifter_bwd on the state the fused forward saved.  The separate forward is held to round-off.
SEPARATE_FORWARD_IS_BITWISE = {"small": False, "slabs": True, "partial": True, "slabs-f16x3": True}


def _bwd_on_saved_state(pkg, m, x, y, t, crit):
    """stand-alone criterion on y -> dy -> pl_lifter_bwd on the workspace the model's last forward wrote: the gradient arena"""
    yd = y.detach().clone().requires_grad_(True)
    (crit(yd, t) if crit is not None else pkg.mse_loss(yd, t)).backward()
    ws, g = m.last_workspace, torch.zeros_like(m.flat_grads)
    rc = pkg.lib().pl_lifter_bwd(ctypes.byref(m._desc), x.data_ptr(), yd.grad.data_ptr(), x.shape[0], ws["buf"].data_ptr(),
                                 ws["bytes"], None, g.data_ptr(), pkg._lib.current_stream_ptr())
    pkg._lib.check(rc, "pl_lifter_bwd")
    return g


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_plain_mse_does_not_move(pkg, route):
    """criterion=None, PoseCriterion("mse"), all-ones weights on it, and forward -> pl.mse_loss -> backward (the entry points as
    they were; not on SmallMse, see above): loss, y and the whole gradient arena agree bit for bit; the stand-alone pass on that
    y is pl.mse_loss's bits."""
    name, i_dim, o_dim, H, S, dtype, B, G = route
    x, t = _batch(B, i_dim, o_dim)
    outs = []
    crits = [None, _crit(pkg, "mse", G), _crit(pkg, "mse", G, np.ones(o_dim // G, np.float32))]
    if SEPARATE_FORWARD_IS_BITWISE[name]:
        crits.append("separate")
    for c in crits:
        m = _model(pkg, i_dim, o_dim, H, S, dtype)
        if isinstance(c, str):
            y = m(x)
            loss = pkg.mse_loss(y, t)
            loss.backward()
        else:
            loss, y = m.fused_train_fwd_bwd(x, t, criterion=c)
        outs.append((loss.clone(), y.detach().clone(), m.flat_grads.clone()))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)
    y = outs[0][1]
    for c in crits[1:3]:
        yd = y.clone().requires_grad_(True)
        yo = y.clone().requires_grad_(True)
        a, b = c(yd, t), pkg.mse_loss(yo, t)
        a.backward()
        b.backward()
        assert torch.equal(a, b) and torch.equal(yd.grad, yo.grad)


@pytest.mark.parametrize("kind", ["l1", "smooth_l1", "mpjpe"])
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_fused_step_is_the_separate_calls(pkg, route, kind):
    """fused_train_fwd_bwd(criterion=) against the training forward, the stand-alone criterion and the backward in a row (same
    seed and step): y and the whole gradient arena bit for bit (SmallMse: see SEPARATE_FORWARD_IS_BITWISE); on every route the
    arena is also, bit for bit, the stand-alone criterion on the returned y + pl_lifter_bwd on the saved state, and y is the
    MSE step's.  The loss within 1e-5 relative of the fp64 oracle evaluated on the returned y (the fused routes sum their
    partials in another order than the stand-alone pass)."""
    name, i_dim, o_dim, H, S, dtype, B, G = route
    x, t = _batch(B, i_dim, o_dim)
    w = _weights(o_dim // G)
    crit = _crit(pkg, kind, G, w, beta=0.1)
    m = _model(pkg, i_dim, o_dim, H, S, dtype)
    loss, y = m.fused_train_fwd_bwd(x, t, criterion=crit)
    grads = m.flat_grads.clone()
    assert torch.equal(grads, _bwd_on_saved_state(pkg, m, x, y, t, crit))
    m0 = _model(pkg, i_dim, o_dim, H, S, dtype)
    assert torch.equal(y, m0.fused_train_fwd_bwd(x, t)[1])
    m2 = _model(pkg, i_dim, o_dim, H, S, dtype)
    y2 = m2(x)
    loss2 = crit(y2, t)
    loss2.backward()
    if SEPARATE_FORWARD_IS_BITWISE[name]:
        assert torch.equal(y, y2.detach())
        assert torch.equal(grads, m2.flat_grads)
    else:
        assert (y - y2.detach()).abs().max().item() <= 64 * U * y.abs().max().item()      # a different order of H products
    want, _ = orc.criterion(kind, y.cpu().numpy(), t.cpu().numpy(), G, w, beta=0.1)
    assert abs(loss.item() - want) <= 1e-5 * abs(want), (loss.item(), want)
    assert grads.abs().max().item() > 0


@pytest.mark.parametrize("kind", ["l1", "mpjpe"])
def test_adamw_riding_step_is_fused_plus_optimizer_step(pkg, kind):
    """B = 64: the AdamW update rides in the backward launches (pl_lifter_train_step_crit); bitwise fused_train_fwd_bwd(criterion=)
    + optimizer.step() on parameters, both moments and the losses of three steps."""
    B, out = 64, []
    crit = _crit(pkg, kind, 3, _weights(17))
    for in_call in (True, False):
        m = _model(pkg, 34, 51, 256, 1)
        opt = pkg.FlatAdamW(m, lr=1e-3, weight_decay=0.02)
        assert m.step_carries_adamw(B)
        losses = []
        for i in range(3):
            x, t = _batch(B, 34, 51, seed=40 + i)
            if in_call:
                loss, _ = pkg.train_step(m, opt, x, t, criterion=crit)
            else:
                loss, _ = m.fused_train_fwd_bwd(x, t, criterion=crit)
                opt.step()
            losses.append(loss.clone())
        assert opt.state_dict()["state"][0]["step"] == 3
        out.append((torch.stack(losses), m.flat_params.clone(), opt._m.clone(), opt._v.clone(), m.flat_grads.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert len(set(out[0][0].tolist())) == 3


@pytest.mark.parametrize("route", [ROUTES[3], ROUTES[4]], ids=[ROUTE_IDS[3], ROUTE_IDS[4]])
def test_layer_ranges_equal_the_single_call(pkg, route):
    """pl_lifter_train_fwd_bwd_crit over (L, cut) then (cut - 1, 0) -- the data-parallel overlap -- against (L, 0): bit for bit,
    on the routes where the MSE step's ranges are (at B <= 64 the layer that heads the second range runs its BatchNorm
    backward in another kernel, and the arenas differ in the last bits with plain MSE already: 8.8e-9 measured at B = 64)."""
    _, i_dim, o_dim, H, S, dtype, B, G = route
    x, t = _batch(B, i_dim, o_dim)
    crit = _crit(pkg, "mpjpe", G, _weights(o_dim // G))
    L, lib = 1 + 2 * S, pkg.lib()
    outs = []
    for ranges in (((L, 0),), ((L, 2), (1, 0))):
        m = _model(pkg, i_dim, o_dim, H, S, dtype)
        ws = m._acquire_workspace(B)
        y, loss = torch.empty(B, o_dim, device=DEV), torch.zeros((), device=DEV)
        st = crit.struct(o_dim, x.device)
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


# ------------------------------------------------------------------------------------------------- train / graphed / eval
def test_graphed_step_replays_the_eager_step_and_sees_weight_edits(pkg):
    """Three eager steps = three replays bit for bit with l1 (B = 8, H = 256); then joint_weights is edited in place on both
    sides and a fourth step still agrees -- and differs from the step the old weights give."""
    B = 8
    res = []
    for graphed in (False, True):
        m = _model(pkg, 34, 51, 256, 1)
        opt = pkg.FlatAdamW(m, lr=1e-3)
        crit = _crit(pkg, "l1", 3, _weights(17))
        x, t = _batch(B, 34, 51)
        step = pkg.GraphedTrainStep(m, opt, x, t, criterion=crit) if graphed else \
            (lambda a, b: pkg.train_step(m, opt, a, b, criterion=crit))
        out = []
        for i in range(4):
            if i == 3:
                crit.joint_weights.mul_(0.5)
                crit.joint_weights[5] = 3.0
            xi, ti = _batch(B, 34, 51, seed=20 + i)
            loss, y = step(xi, ti)
            out += [loss.clone(), y.clone()]
        res.append(out + [m.flat_params.clone(), opt._m.clone(), opt._v.clone()])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # the edit mattered: the same fourth step under the old weights gives another loss
    m = _model(pkg, 34, 51, 256, 1)
    opt = pkg.FlatAdamW(m, lr=1e-3)
    crit = _crit(pkg, "l1", 3, _weights(17))
    for i in range(4):
        loss, _ = pkg.train_step(m, opt, *_batch(B, 34, 51, seed=20 + i), criterion=crit)
    assert loss.item() != res[0][6].item()


def test_graphed_step_refuses_a_replaced_weight_tensor(pkg):
    m = _model(pkg, 34, 51, 256, 1)
    opt = pkg.FlatAdamW(m, lr=1e-3)
    crit = _crit(pkg, "mpjpe", 3, _weights(17))
    x, t = _batch(8, 34, 51)
    step = pkg.GraphedTrainStep(m, opt, x, t, criterion=crit)
    step(x, t)
    crit.joint_weights = crit.joint_weights.clone()
    with pytest.raises(pkg.PoseliftError, match="criterion"):
        step(x, t)


def test_train_step_on_another_model_is_the_autograd_composition(pkg):
    """train_step(MyViT, FlatAdam, criterion=l1) = zero_grad, forward, criterion, backward, step written by hand."""
    g = torch.Generator().manual_seed(2)
    x, t = torch.rand(8, 17, 2, generator=g).to(DEV), (torch.rand(8, 17, 3, generator=g) - 0.5).to(DEV)
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
                loss = crit(y, t)
                loss.backward()
                opt.step()
            else:
                loss, y = pkg.train_step(m, opt, x, t, criterion=crit)
        res.append([loss.detach().clone(), y.detach().clone()] + [v.detach().clone() for v in m.state_dict().values()])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    want, _ = orc.criterion("l1", res[0][1].reshape(8, 51).cpu().numpy(), t.reshape(8, 51).cpu().numpy(), 3, _weights(17))
    assert abs(res[0][0].item() - want) <= 1e-5 * want


def test_eval_step_returns_the_criterions_loss(pkg):
    m = _model(pkg, 34, 51, 256, 1).eval()
    x, t = _batch(16, 34, 51)
    crit = _crit(pkg, "mpjpe", 3, _weights(17))
    loss, metric, y = pkg.eval_step(m, x.reshape(16, 17, 2), t.reshape(16, 17, 3), criterion=crit)
    assert torch.equal(loss, crit(y, t.reshape(16, 17, 3))) and metric.shape == (17,)
    mse, _, y0 = pkg.eval_step(m, x.reshape(16, 17, 2), t.reshape(16, 17, 3))
    assert torch.equal(y0, y) and torch.equal(mse, pkg.mse_loss(y, t.reshape(16, 17, 3))) and mse.item() != loss.item()


def test_graphed_module_step_takes_a_pose_criterion(pkg):
    """GraphedModuleStep(loss_fn=PoseCriterion): three replays equal three eager steps of the same stock module."""
    res = []
    x, t = _batch(6, 7, 6)
    for graphed in (False, True):
        torch.manual_seed(12)
        mod = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Tanh(), torch.nn.Linear(5, 6)).to(DEV)
        crit = _crit(pkg, "smooth_l1", 3, np.array([0.5, 2.0], np.float32), beta=0.05)
        opt = pkg.FlatAdam(mod, lr=1e-2, capturable=True)
        if graphed:
            step = pkg.GraphedModuleStep(mod, opt, crit, x, t)
            for i in range(3):
                loss = step(x + i, t)
        else:
            for i in range(3):
                opt.zero_grad()
                loss = crit(mod(x + i), t)
                loss.backward()
                opt.step()
        res.append([loss.detach().clone()] + [p.detach().clone() for p in mod.parameters()])
    for a, b in zip(*res):
        assert torch.equal(a, b)
