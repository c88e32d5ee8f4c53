"""Gradient-norm clipping and non-finite skip of the flat optimizers on the MI355X: the norm kernel alone against the fp64
twin (tests/grad_clip_oracle.py), FlatAdamW / FlatAdam with clipping against torch.nn.utils.clip_grad_norm_ +
torch.optim.AdamW / Adam on the CPU, the bitwise properties of the routes (train_step, GraphedTrainStep, a skipped step), the
skip semantics, the weight-plane cache behind a skipped step, and the data-parallel gradient scale.

Where an optimizer is compared with torch, the CPU twin holds the same weights and is handed the library's own gradient of
each step (copied out of the gradient arena): what is compared is the norm, the coefficient and the update -- the subject
here -- at the bound tests/test_gpu_parity.py::test_flat_adamw_matches_oracle_and_torch_state_layout uses (parameters
rtol 1e-6 / atol 1e-8, moments 1e-6 / 1e-9).  The backward pass has its own tests."""

import numpy as np
import pytest
import torch
from torch import nn

import grad_clip_oracle as gco
from oracle.torch_twin import TwinLifter
from oracle.vit_twin import twin as vit_twin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the fp64 sum over n <= 2^25 terms contributes <= 2^-28, the sqrt and the rounding to fp32 2^-24: four times their sum
NORM_TOL = 2.0 ** -22


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


# ------------------------------------------------------------------------------------------------ the norm kernel alone
def _norm(pkg, g, ranges, gscale=1.0, clip=0, max_norm=0.0, skip=0, rec=None, max_dev=None):
    L, R = pkg.lib(), pkg._lib.PLGradRange
    arr = (R * len(ranges))(*[R(lo, hi) for lo, hi in ranges])
    rec = torch.zeros(6, dtype=torch.int32, device=DEV) if rec is None else rec
    scratch = torch.empty(L.pl_grad_norm_scratch_bytes(len(ranges)), dtype=torch.uint8, device=DEV)
    rc = L.pl_grad_norm_clip(g.data_ptr(), g.numel(), arr, len(ranges), gscale, clip, max_norm,
                             max_dev.data_ptr() if max_dev is not None else None, skip, rec.data_ptr(), scratch.data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.pl_last_error()
    return rec


def _read(rec):
    r = rec.cpu()
    f = r.view(torch.float32).numpy()
    return dict(norm=f[0], coef=f[1], finite=int(r[2]), skip=int(r[3]), skipped=int(r.view(torch.int64)[2]))


def _rel(got, want):
    return abs(float(got) - float(want)) / float(want)


REAL_LIFTER = 4296755          # floats of LinearModel(34, 51, linear_size=1024, num_stage=2): many partials, a ragged tail


@pytest.mark.parametrize("n", [1, 3, 4, 255, 256 * 4 + 1, REAL_LIFTER])
def test_norm_kernel_lengths_scales_nonfinite_and_determinism(pkg, n):
    rng = np.random.default_rng(n)
    g = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    gd = torch.from_numpy(g).to(DEV)
    for gscale in (1.0, 0.5, 1.0 / 3.0, -2.0):
        r1, r2 = _norm(pkg, gd, [(0, n)], gscale), _norm(pkg, gd, [(0, n)], gscale)
        assert torch.equal(r1, r2)                                         # two runs: bitwise equal records
        got, want = _read(r1), gco.grad_norm(g, [(0, n)], gscale)
        print(f"n={n} gscale={gscale:.4g}: norm {got['norm']:.9g} twin {want:.9g} rel {_rel(got['norm'], want):.3g}")
        assert _rel(got["norm"], want) <= NORM_TOL
        assert got["finite"] == 1 and got["skip"] == 0 and got["skipped"] == 0 and got["coef"] == 1.0
    # torch's coefficient in fp32, by value and from a device scalar
    want = gco.grad_norm(g, [(0, n)])
    for mx in (0.25 * float(want), 4.0 * float(want)):
        got = _read(_norm(pkg, gd, [(0, n)], clip=1, max_norm=mx))
        dev = _read(_norm(pkg, gd, [(0, n)], clip=1, max_norm=-1.0, max_dev=torch.tensor([mx], dtype=torch.float32, device=DEV)))
        assert got["coef"] == dev["coef"] == gco.clip_coef(got["norm"], mx), (mx, got, dev)
    # one inf or NaN at the first or the last active element
    rec = torch.zeros(6, dtype=torch.int32, device=DEV)
    for k, (pos, bad) in enumerate([(0, np.inf), (n - 1, np.nan), (0, np.nan), (n - 1, -np.inf)]):
        h = gd.clone()
        h[pos] = bad
        got = _read(_norm(pkg, h, [(0, n)], clip=1, max_norm=1.0, skip=1, rec=rec))
        assert got["finite"] == 0 and got["skip"] == 1 and got["skipped"] == k + 1 and not np.isfinite(got["norm"])
        assert _read(_norm(pkg, h, [(0, n)], clip=0, skip=0))["skip"] == 0
    got = _read(_norm(pkg, gd, [(0, n)], skip=1, rec=rec))                 # a finite step behind them: the count stays
    assert got["finite"] == 1 and got["skip"] == 0 and got["skipped"] == 4


@pytest.mark.parametrize("kind", ["zeros", "denormal", "1e19", "mixed"])
def test_norm_kernel_value_ranges(pkg, kind):
    n = 256 * 4 * 5 + 3
    rng = np.random.default_rng(7)
    sign = rng.choice([-1.0, 1.0], n)
    g = {"zeros": np.zeros(n),
         "denormal": sign * rng.uniform(1e-40, 1e-38, n),                  # every input below the smallest normal fp32
         "1e19": sign * 1e19,                                              # an fp32 square would overflow
         "mixed": sign * 10.0 ** rng.uniform(-20, 10, n)}[kind].astype(np.float32)
    if kind == "denormal":
        assert np.all(np.abs(g) < np.finfo(np.float32).tiny) and np.all(g != 0)
    gd = torch.from_numpy(g).to(DEV)
    got, want = _read(_norm(pkg, gd, [(0, n)], clip=1, max_norm=1.0)), gco.grad_norm(g)
    print(f"{kind}: norm {got['norm']:.9g} twin {want:.9g}")
    assert got["finite"] == 1 and np.isfinite(want)
    if kind == "zeros":
        assert got["norm"] == 0.0 and got["coef"] == 1.0                    # 1 / (0 + 1e-6) clamps to exactly 1
    else:
        assert want >= np.finfo(np.float32).tiny                           # (the norm itself is a normal fp32 number)
        assert _rel(got["norm"], want) <= NORM_TOL
        assert got["coef"] == gco.clip_coef(got["norm"], 1.0)


def test_norm_kernel_reads_only_its_ranges(pkg):
    """Five ranges with gaps that hold NaN and inf; starts at 4-float offsets that are not 16-float aligned; ragged ends; and
    more ranges than one launch takes (64), which makes a second partial launch."""
    n = 6000
    rng = np.random.default_rng(11)
    g = rng.standard_normal(n).astype(np.float32)
    ranges = [(4, 9), (20, 1047), (1052, 1053), (2000, 4099), (4100, 5999)]
    active = np.zeros(n, bool)
    for lo, hi in ranges:
        active[lo:hi] = True
    g[~active] = np.where(rng.random((~active).sum()) < 0.5, np.nan, np.inf).astype(np.float32)
    gd = torch.from_numpy(g).to(DEV)
    r1 = _norm(pkg, gd, ranges, 1.0, clip=1, max_norm=1.0, skip=1)
    got, want = _read(r1), gco.grad_norm(g, ranges)
    assert got["finite"] == 1 and got["skipped"] == 0 and _rel(got["norm"], want) <= NORM_TOL
    assert torch.equal(r1, _norm(pkg, gd, ranges, 1.0, clip=1, max_norm=1.0, skip=1))
    assert _read(_norm(pkg, gd, [(4, 9), (16, 24)]))["finite"] == 0        # (the gaps really are poisoned)
    many = [(8 * k, 8 * k + 5) for k in range(150)]                         # 3 launches of <= 64 ranges
    h = torch.from_numpy(np.where(np.arange(n) % 8 < 5, rng.standard_normal(n), np.nan).astype(np.float32)).to(DEV)
    got = _read(_norm(pkg, h, many))
    assert got["finite"] == 1 and _rel(got["norm"], gco.grad_norm(h.cpu().numpy(), many)) <= NORM_TOL


# ------------------------------------------------------------------------------------------------ the lifter vs torch
def _active(m):
    return [(s, p) for s, p in zip(m._slots, m._param_list) if p.requires_grad and (m.BN or "batch_norm" not in s.name)]


def _ranges(m):
    runs = []
    for k, s in enumerate(m._slots):
        if not any(s is a for a, _ in _active(m)):
            continue
        end = m._slots[k + 1].offset if k + 1 < len(m._slots) else m.flat_params.numel()
        if runs and runs[-1][1] == s.offset:
            runs[-1] = (runs[-1][0], end)
        else:
            runs.append((s.offset, end))
    return runs


def _cpu_twin(m, **kw):
    tw = TwinLifter(m.input_size, m.output_size, linear_size=m.linear_size, num_stage=m.num_stage, p_dropout=0.0, BN=m.BN)
    tw.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    return tw, torch.optim.AdamW(tw.parameters(), **kw)


def _hand_over_grads(m, tw, scale=1.0):
    """The library's gradient of this step (the active slots of the arena) as the CPU twin's .grad."""
    fg = m.flat_grads.detach().cpu()
    named = dict(tw.named_parameters())
    on = {s.name for s, _ in _active(m)}
    for s in m._slots:
        named[s.name].grad = (fg[s.offset:s.offset + s.numel].view(s.shape).clone() * scale) if s.name in on else None


def _assert_state_close(m, opt, tw, topt):
    named = dict(tw.named_parameters())
    for s, p in zip(m._slots, m._param_list):
        q = named[s.name]
        np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().numpy(), rtol=1e-6, atol=1e-8, err_msg=s.name)
        if q in topt.state:
            lo, hi = s.offset, s.offset + s.numel
            np.testing.assert_allclose(opt._m[lo:hi].cpu().numpy(), topt.state[q]["exp_avg"].numpy().reshape(-1),
                                       rtol=1e-6, atol=1e-9, err_msg=s.name)
            np.testing.assert_allclose(opt._v[lo:hi].cpu().numpy(), topt.state[q]["exp_avg_sq"].numpy().reshape(-1),
                                       rtol=1e-6, atol=1e-9, err_msg=s.name)


def _first_norm(pkg, m, x, y):
    """The norm of the first step's gradient, read once from the twin (the model is left as it was)."""
    snap = (m.flat_params.clone(), m._bn_running.clone(), m._bn_batches.clone(), m._step)
    m.fused_train_fwd_bwd(x.reshape(x.shape[0], -1).contiguous(), y.reshape(y.shape[0], -1).contiguous())
    n = float(gco.grad_norm(m.flat_grads.cpu().numpy(), _ranges(m)))
    m._bn_running.copy_(snap[1]); m._bn_batches.copy_(snap[2]); m._step = snap[3]
    return n


@pytest.mark.parametrize("dtype", ["f16x3", "fp32"])
@pytest.mark.parametrize("H,B", [(64, 8), (1024, 128)])
def test_lifter_clipping_vs_torch_clip_grad_norm_and_adamw(pkg, H, B, dtype):
    torch.manual_seed(21)
    m = pkg.LinearModel(34, 51, linear_size=H, p_dropout=0.0, compute_dtype=dtype).to(DEV).train()
    x, y = pkg.synth.synthetic_batch(B, 5, DEV)
    max_norm = 0.25 * _first_norm(pkg, m, x, y)
    opt = pkg.FlatAdamW(m, lr=3e-4, weight_decay=0.02, max_grad_norm=max_norm)
    tw, topt = _cpu_twin(m, lr=3e-4, weight_decay=0.02)
    for it in range(4):
        pkg.train_step(m, opt, x, y)
        want = gco.grad_norm(m.flat_grads.cpu().numpy(), _ranges(m))
        got, coef = opt.grad_norm.item(), opt.clip_coef.item()
        print(f"H={H} B={B} {dtype} step {it}: norm {got:.9g} twin {float(want):.9g} coef {coef:.6g}")
        assert _rel(got, want) <= NORM_TOL
        assert coef == gco.clip_coef(np.float32(got), max_norm) and coef < 1.0          # clipping binds
        _hand_over_grads(m, tw)
        torch.nn.utils.clip_grad_norm_(tw.parameters(), max_norm)
        topt.step()
        _assert_state_close(m, opt, tw, topt)
    assert opt.skipped_steps() == 0 and float(opt.state_dict()["state"][0]["step"]) == 4.0


def test_data_parallel_grad_scale_with_clipping(pkg):
    """optimizer.step(grad_scale=0.5) with clipping = the twin that halves the gradient first.  The kernel multiplies by
    gscale * coef, ONE fp32 product, where torch rounds twice: the coefficient agrees with the twin's to one fp32 ulp.
    (torch's own coefficient comes from its fp32-accumulated norm and may sit one ulp further away: seen 2 ulps, 1.5e-8 at
    0.1; the parameters and moments are held to torch at the AdamW bound all the same.)"""
    torch.manual_seed(2)
    m = pkg.LinearModel(34, 51, linear_size=64, p_dropout=0.0).to(DEV).train()
    rng = np.random.default_rng(3)
    g = (rng.standard_normal(m.flat_params.numel()) * 1e-2).astype(np.float32)
    real = np.zeros(g.size, bool)
    for s in m._slots:
        real[s.offset:s.offset + s.numel] = True
    g[~real] = 0.0                                                          # alignment padding holds no gradient
    max_norm = 0.3 * float(gco.grad_norm(g, _ranges(m), 0.5))
    opt = pkg.FlatAdamW(m, lr=3e-4, weight_decay=0.02, max_grad_norm=max_norm)
    tw, topt = _cpu_twin(m, lr=3e-4, weight_decay=0.02)
    tn = gco.ClipAdamW(m.flat_params.cpu().numpy(), lr=3e-4, weight_decay=0.02, max_grad_norm=max_norm)
    for it in range(3):
        m.flat_grads.copy_(torch.from_numpy(g * (1.0 + it)).to(DEV))
        opt.step(grad_scale=0.5)
        _hand_over_grads(m, tw, scale=0.5)                                  # (halving is exact)
        torch.nn.utils.clip_grad_norm_(tw.parameters(), max_norm)
        topt.step()
        tn.step(g * np.float32(1.0 + it) * np.float32(0.5), _ranges(m))    # the numpy twin on the halved gradient, scale 1
        assert _rel(opt.grad_norm.item(), tn.norm) <= NORM_TOL
        assert abs(opt.clip_coef.item() - float(tn.coef)) <= np.spacing(tn.coef) and tn.coef < 1.0
        _assert_state_close(m, opt, tw, topt)
        np.testing.assert_allclose(m.flat_params.cpu().numpy()[real], tn.p[real], rtol=1e-6, atol=1e-8)


# ------------------------------------------------------------------------------------------------ bitwise properties
def _maker(pkg, H, dtype):
    def make(**kw):
        torch.manual_seed(9)
        m = pkg.LinearModel(34, 51, linear_size=H, p_dropout=0.5, compute_dtype=dtype).to(DEV).train()
        m.manual_seed(77, step=0)
        return m, pkg.FlatAdamW(m, lr=1e-3, **kw)
    return make


def _same(a, b):
    (ma, oa), (mb, ob) = a, b
    return (torch.equal(ma.flat_params, mb.flat_params) and torch.equal(oa._m, ob._m) and torch.equal(oa._v, ob._v)
            and torch.equal(ma._bn_running, mb._bn_running))


@pytest.mark.parametrize("B", [8, 128])
def test_huge_max_norm_is_bitwise_the_unclipped_step(pkg, B):
    make = _maker(pkg, 256, "f16x3")
    plain, clipped = make(), make(max_grad_norm=1e30)
    for i in range(2):
        x, y = pkg.synth.synthetic_batch(B, 30 + i, DEV)
        l1, _ = pkg.train_step(*plain, x, y)
        l2, _ = pkg.train_step(*clipped, x, y)
        assert torch.equal(l1, l2)
    assert clipped[1].clip_coef.item() == 1.0 and clipped[1].grad_norm.item() > 0
    assert _same(plain, clipped)


@pytest.mark.parametrize("B", [8, 64])
def test_train_step_route_with_clipping_is_fwd_bwd_plus_optimizer_step(pkg, B):
    """B <= 64: without clipping the AdamW step would ride inside the backward launches; with it the route is
    fused_train_fwd_bwd, the norm pass, one AdamW launch -- the same as calling the two halves by hand."""
    make = _maker(pkg, 1024, "f16x3")
    a, b = make(max_grad_norm=0.05, skip_nonfinite=True), make(max_grad_norm=0.05, skip_nonfinite=True)
    assert a[0].step_carries_adamw(B)
    for i in range(2):
        x, y = pkg.synth.synthetic_batch(B, 50 + i, DEV)
        l1, y1 = pkg.train_step(*a, x, y)
        l2, y2 = b[0].fused_train_fwd_bwd(x.reshape(B, -1).contiguous(), y.reshape(B, -1).contiguous())
        b[1].step()
        assert torch.equal(l1, l2) and torch.equal(y1.reshape(B, -1), y2)
    assert a[1].clip_coef.item() < 1.0 and torch.equal(a[1]._clip.record, b[1]._clip.record)
    assert _same(a, b) and a[1]._t == b[1]._t == 2


@pytest.mark.parametrize("dtype,B,H", [("f16x3", 64, 1024), ("fp32", 128, 128)])
def test_graphed_train_step_with_clipping_and_a_skipped_step_is_bitwise_the_eager_one(pkg, dtype, B, H):
    make = _maker(pkg, H, dtype)
    kw = dict(max_grad_norm=0.05, skip_nonfinite=True)
    batches = [pkg.synth.synthetic_batch(B, 60 + i, DEV) for i in range(4)]
    batches[1][1][3, 2, 1] = float("inf")                                   # step 2: a non-finite gradient
    e, g = make(**kw), make(**kw)
    eager = []
    for i, (x, y) in enumerate(batches):
        if i == 3:
            e[1].param_groups[0]["max_grad_norm"] = 0.02                    # changed between steps, like lr
        loss, yh = pkg.train_step(*e, x, y)
        eager.append((loss.clone(), yh.clone(), e[1]._clip.record.clone()))
    step = pkg.GraphedTrainStep(*g, *batches[0])
    assert torch.equal(g[0].flat_params, make()[0].flat_params) and g[1].skipped_steps() == 0
    for i, (x, y) in enumerate(batches):
        if i == 3:
            g[1].param_groups[0]["max_grad_norm"] = 0.02
        loss, yh = step(x, y)
        assert torch.equal(loss, eager[i][0]) and torch.equal(yh, eager[i][1]), i
        assert torch.equal(g[1]._clip.record, eager[i][2]), i
    assert _same(e, g)
    assert e[1].skipped_steps() == g[1].skipped_steps() == 1
    assert float(g[1].state_dict()["state"][0]["step"]) == 3.0 and g[1]._t == 4
    g[1].param_groups[0]["max_grad_norm"] = None
    with pytest.raises(pkg.PoseliftError, match="after capture"):
        step(*batches[0])


# ------------------------------------------------------------------------------------------------ skip semantics
def test_skip_semantics_five_steps_one_nonfinite(pkg):
    """5 steps, the target of step 3 holds one inf: that step is not taken and not counted.  Steps 4-5 match the torch twin
    that did not call step() on iteration 3 (bias corrections with t = 3, 4)."""
    torch.manual_seed(4)
    m = pkg.LinearModel(34, 51, linear_size=64, p_dropout=0.0).to(DEV).train()
    x, y = pkg.synth.synthetic_batch(16, 8, DEV)
    max_norm = 0.5 * _first_norm(pkg, m, x, y)
    opt = pkg.FlatAdamW(m, lr=3e-4, weight_decay=0.02, max_grad_norm=max_norm, skip_nonfinite=True)
    tw, topt = _cpu_twin(m, lr=3e-4, weight_decay=0.02)
    for it in range(1, 6):
        yy = y.clone()
        if it == 3:
            yy[5, 7, 2] = float("inf")
            before = (m.flat_params.clone(), opt._m.clone(), opt._v.clone(), m._bn_running.clone())
        loss, _ = pkg.train_step(m, opt, x, yy)
        if it == 3:
            assert not torch.isfinite(loss) and not torch.isfinite(m.flat_grads).all()
            assert torch.equal(m.flat_params, before[0]) and torch.equal(opt._m, before[1]) and torch.equal(opt._v, before[2])
            # the forward does not read the target: the BatchNorm buffers moved as on any step, and stay finite
            assert torch.isfinite(m._bn_running).all() and not torch.equal(m._bn_running, before[3])
            assert not np.isfinite(opt.grad_norm.item())
            continue                                                        # the twin does not call step()
        _hand_over_grads(m, tw)
        torch.nn.utils.clip_grad_norm_(tw.parameters(), max_norm)
        topt.step()
        _assert_state_close(m, opt, tw, topt)
    assert opt.skipped_steps() == 1 and opt._t == 5
    sd = opt.state_dict()
    assert float(sd["state"][0]["step"]) == 4.0 == float(topt.state_dict()["state"][0]["step"])
    # load_state_dict: the loaded step counts taken steps, the skipped count starts again at 0 against it
    opt.load_state_dict(sd)
    assert opt.skipped_steps() == 0 and opt._t == 4
    pkg.train_step(m, opt, x, y)
    _hand_over_grads(m, tw)
    torch.nn.utils.clip_grad_norm_(tw.parameters(), max_norm)
    topt.step()
    _assert_state_close(m, opt, tw, topt)


def test_nonfinite_gradient_without_skip_gives_nan_parameters_as_torch(pkg):
    torch.manual_seed(4)
    m = pkg.LinearModel(34, 51, linear_size=64, p_dropout=0.0).to(DEV).train()
    opt = pkg.FlatAdamW(m, lr=3e-4, max_grad_norm=1.0)
    tw, topt = _cpu_twin(m, lr=3e-4)
    x, y = pkg.synth.synthetic_batch(16, 8, DEV)
    y[5, 7, 2] = float("inf")
    pkg.train_step(m, opt, x, y)
    _hand_over_grads(m, tw)
    torch.nn.utils.clip_grad_norm_(tw.parameters(), 1.0)                    # error_if_nonfinite=False
    topt.step()
    named, hit = dict(tw.named_parameters()), 0
    for s, p in zip(m._slots, m._param_list):                               # NaN where torch has NaN, nowhere else
        ours = torch.isnan(p.detach()).cpu()
        assert torch.equal(ours, torch.isnan(named[s.name].detach())), s.name
        hit += int(ours.sum())
    assert hit > 0 and torch.isnan(m.state_dict()["w2.weight"]).any()
    assert opt.skipped_steps() == 0


def test_bn_false_nan_in_an_unused_batchnorm_slot_does_not_skip(pkg):
    torch.manual_seed(4)
    m = pkg.LinearModel(34, 51, linear_size=64, p_dropout=0.0, BN=False).to(DEV).train()
    opt = pkg.FlatAdamW(m, lr=3e-4, max_grad_norm=1e-3, skip_nonfinite=True)
    x, y = pkg.synth.synthetic_batch(16, 8, DEV)
    p0 = m.flat_params.clone()
    m.fused_train_fwd_bwd(x.reshape(16, -1).contiguous(), y.reshape(16, -1).contiguous())
    assert len(opt._active_ranges()) > 1
    for s in m._slots:
        if "batch_norm" in s.name:
            m.flat_grads[s.offset] = float("nan")
            m.flat_grads[s.offset + s.numel - 1] = float("inf")
    opt.step()
    want = gco.grad_norm(m.flat_grads.cpu().numpy(), opt._active_ranges())
    assert np.isfinite(want) and _rel(opt.grad_norm.item(), want) <= NORM_TOL
    assert opt.skipped_steps() == 0 and torch.isfinite(m.flat_params).all() and not torch.equal(m.flat_params, p0)


# ------------------------------------------------------------------------------------------------ the plane trap
@pytest.mark.parametrize("when", ["before_the_step", "between_backward_and_step"])
def test_weight_planes_behind_a_skipped_step(pkg, when):
    """f16x3: the AdamW launch writes the operand planes and the host then marks them current.  A skipped step must still
    write them (from the unchanged parameters): load_state_dict made them stale."""
    torch.manual_seed(6)
    m = pkg.LinearModel(34, 51, linear_size=1024, p_dropout=0.0, compute_dtype="f16x3").to(DEV).train()
    opt = pkg.FlatAdamW(m, lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True)
    x, y = pkg.synth.synthetic_batch(128, 9, DEV)
    pkg.train_step(m, opt, x, y)                                            # planes written and marked current
    assert m._wplanes is not None and m._wplanes_ver == m._planes_key()
    torch.manual_seed(60)
    new = {k: v.clone() for k, v in pkg.LinearModel(34, 51, linear_size=1024, p_dropout=0.0).state_dict().items()}
    y[0, 0, 0] = float("inf")
    if when == "before_the_step":
        m.load_state_dict(new)
        pkg.train_step(m, opt, x, y)
    else:
        m.fused_train_fwd_bwd(x.reshape(128, -1).contiguous(), y.reshape(128, -1).contiguous())
        m.load_state_dict(new)                                              # the planes are stale when AdamW launches
        opt.step()
    assert opt.skipped_steps() == 1
    for k in ("w1.weight", "linear_stages.1.w2.weight"):
        assert torch.equal(m.state_dict()[k].cpu(), new[k])
    fresh = pkg.LinearModel(34, 51, linear_size=1024, p_dropout=0.0, compute_dtype="f16x3").to(DEV).eval()
    fresh.load_state_dict(m.state_dict())
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(x), fresh(x))


# ------------------------------------------------------------------------------------------------ six entry points, one kernel
@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("offset", [0, 1])
def test_the_six_adamw_entry_points_are_one_kernel_bitwise(pkg, offset, t):
    """The optimizers issue every step through pl_adamw_flat_planes_clip; with NULL planes and a NULL record it has to be the
    launch pl_adamw_flat / pl_adamw_flat_dev make.  n = 1027 from a 16-byte aligned base (float4 body + scalar tail) and from
    a base one float further (scalar path); by value, and with lr = *lr_dev, t = t_base + *t_dev."""
    L, n = pkg.lib(), 1027
    lr, hp, gs = float(np.float32(3e-4)), (0.9, 0.999, 1e-8, 0.02), 0.5
    g0 = torch.Generator().manual_seed(100 * offset + t)
    init = [torch.randn(n + 1, generator=g0) * s for s in (1.0, 1e-2, 1e-3)] + [torch.rand(n + 1, generator=g0) * 1e-4]
    lr_dev = torch.tensor([lr], dtype=torch.float32, device=DEV)
    t_dev = torch.tensor([t - 1], dtype=torch.int64, device=DEV)
    lp, tp = lr_dev.data_ptr(), t_dev.data_ptr()

    def run(name, *tail):
        bufs = [x.to(DEV) for x in init]
        p, g, m, v = (b[offset:offset + n] for b in bufs)
        assert all((x.data_ptr() % 16 == 0) == (offset == 0) for x in (p, g, m, v))
        rc = getattr(L, name)(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, *tail,
                              torch.cuda.current_stream().cuda_stream)
        assert rc == 0, (name, L.pl_last_error())
        return torch.stack([bufs[0], bufs[2], bufs[3]])      # whole buffers: the float outside [offset, offset + n) too

    want = run("pl_adamw_flat", lr, *hp, t, gs)
    assert not torch.equal(want[0], init[0].to(DEV))
    forms = {"flat_clip": run("pl_adamw_flat_clip", lr, *hp, t, gs, None),
             "flat_planes": run("pl_adamw_flat_planes", lr, None, *hp, t, None, gs, None),
             "flat_planes_clip": run("pl_adamw_flat_planes_clip", lr, None, *hp, t, None, gs, None, None),
             "flat_dev": run("pl_adamw_flat_dev", lp, *hp, 1, tp, gs),
             "flat_dev_clip": run("pl_adamw_flat_dev_clip", lp, *hp, 1, tp, gs, None),
             "flat_planes_clip, lr and t read on the device": run("pl_adamw_flat_planes_clip", 0.0, lp, *hp, 1, tp, gs, None, None)}
    for name, got in forms.items():
        assert torch.equal(got, want), name


# ------------------------------------------------------------------------------------------------ FlatAdam
@pytest.mark.parametrize("capturable", [False, True])
def test_flat_adam_small_module_vs_torch_adam_and_clip_grad_norm(pkg, capturable):
    """A stock module: its gradients arrive through gather_grads.  Steps: all gradients; one parameter without a gradient
    (several runs); an inf gradient (skipped: p, m, v bitwise unchanged); that parameter without a gradient again."""
    torch.manual_seed(12)
    mod = nn.Sequential(nn.Linear(7, 5), nn.Tanh(), nn.Linear(5, 3)).to(DEV)
    ref = nn.Sequential(nn.Linear(7, 5), nn.Tanh(), nn.Linear(5, 3))
    ref.load_state_dict({k: v.cpu() for k, v in mod.state_dict().items()})
    x, t = torch.randn(6, 7, device=DEV), torch.randn(6, 3, device=DEV)
    (mod(x) - t).pow(2).mean().backward()
    a = [p.grad.cpu().numpy().reshape(-1) for p in mod.parameters()]
    max_norm = 0.25 * float(np.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in a)))
    mod.zero_grad()
    opt = pkg.FlatAdam(mod, lr=1e-2, max_grad_norm=max_norm, skip_nonfinite=True, capturable=capturable)
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-2)
    arena = opt.arena
    for it, what in enumerate(["all", "missing", "inf", "missing"]):
        opt.zero_grad()
        tt = t.clone()
        if what == "inf":
            tt[1, 1] = float("inf")
        (mod(x) - tt).pow(2).mean().backward()
        if what == "missing":
            mod[0].bias.grad = None
        before = (arena.flat.clone(), opt._m.clone(), opt._v.clone())
        opt.step()
        runs = arena.gather_grads()
        assert len(runs) == (2 if what == "missing" else 1)
        want = gco.grad_norm(arena.grad.cpu().numpy(), runs)
        if what == "inf":
            assert not np.isfinite(opt.grad_norm.item())
            assert all(torch.equal(u, w) for u, w in zip(before, (arena.flat, opt._m, opt._v)))
            continue
        assert _rel(opt.grad_norm.item(), want) <= NORM_TOL and opt.clip_coef.item() < 1.0
        for p, q in zip(mod.parameters(), ref.parameters()):
            q.grad = p.grad.detach().cpu().clone() if p.grad is not None else None
        torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm)
        ropt.step()
        for (k, p), q in zip(mod.named_parameters(), ref.parameters()):
            np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().numpy(), rtol=1e-6, atol=1e-8, err_msg=f"{it} {k}")
            np.testing.assert_allclose(opt.state[p]["exp_avg"].cpu().numpy(), ropt.state[q]["exp_avg"].numpy(), rtol=1e-6,
                                       atol=1e-9, err_msg=f"{it} {k}")
    assert opt.skipped_steps() == 1
    sd = opt.state_dict()
    assert float(sd["state"][1]["step"]) == 3.0 and float(opt._step_tensor) == 4.0


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_myvit_one_clipped_step_vs_fp64_twin(pkg, mode):
    """One MyViT step at B = 3 with clipping binding, against the same construction (fp64 norm, torch's coefficient, AdamW) on
    oracle/vit_twin.py's gradients, at the bound tests/test_gpu_vit.py::test_g12_three_adamw_steps_vs_reference uses: 1e-5
    relative + 2e-7, but for at most 8 elements whose gradient is at round-off level (Adam normalises the gradient: such an
    element moves by up to lr in whichever direction its rounding points)."""
    tol = {"fp32": 1e-4, "f16x3": 5e-4}[mode]
    torch.manual_seed(103)
    m = pkg.MyViT(compute_dtype=mode)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    rng = np.random.default_rng(3)
    x = rng.uniform(0.0, 1.0, (3, 17, 2)).astype(np.float32)
    t = (0.2 * rng.standard_normal((3, 17, 3))).astype(np.float32)
    _, g64 = vit_twin(sd, x, t)
    norm64 = float(np.sqrt(sum(float((v ** 2).sum()) for v in g64.values())))
    max_norm, lr, wd = 0.25 * norm64, 1e-4, 0.01
    m = m.to(DEV).train()
    opt = pkg.FlatAdam(m, lr=lr, weight_decay=wd, decoupled_weight_decay=True, max_grad_norm=max_norm)
    pkg.train_step(m, opt, torch.as_tensor(x, device=DEV), torch.as_tensor(t, device=DEV))
    runs = opt.arena.gather_grads()
    own = gco.grad_norm(opt.arena.grad.cpu().numpy(), runs)
    assert _rel(opt.grad_norm.item(), own) <= NORM_TOL                      # against the library's own gradient
    print(f"myvit {mode}: norm {float(own):.9g}, fp64 twin's gradient {norm64:.9g}")
    assert opt.clip_coef.item() == gco.clip_coef(np.float32(opt.grad_norm.item()), max_norm) < 1.0
    coef = max_norm / (norm64 + 1e-6)
    got = {k: v.detach().cpu().numpy().reshape(-1) for k, v in m.state_dict().items()}
    odd = 0
    for k, g in g64.items():
        g = g.reshape(-1) * coef
        p = sd[k].double().numpy().reshape(-1) * (1.0 - lr * wd)
        mm, vv = 0.1 * g, 0.001 * g * g
        want = p - (lr / 0.1) * mm / (np.sqrt(vv) / np.sqrt(0.001) + 1e-8)
        bad = np.abs(got[k] - want) > 1e-5 * np.abs(want) + 2e-7
        if bad.any():
            gmax = np.abs(g64[k]).max()
            assert np.all(np.abs(g64[k].reshape(-1)[bad]) <= tol * gmax), k
            assert np.all(np.abs(got[k][bad] - want[bad]) <= 2 * lr), k
            odd += int(bad.sum())
    print(f"myvit {mode}: {odd} round-off-level elements")
    assert odd <= 8, odd
    assert torch.equal(m.pos_embed.detach().cpu(), sd["pos_embed"])          # no gradient: outside every run
