"""Averaged (EMA) weights kept inside the AdamW launches, on the MI355X.

The definition under test (csrc/adamw.h, include/poselift.h PLEma): for update n = 1, 2, ... of an element,

    e <- fmaf(p_new - e, omd_n, e) in fp32,   omd_n = (float)(1 - d_n),   d_n = decay  or  min(decay, (1 + n) / (10 + n))

The reference is the fp64 recurrence e64 += (p_k - e64) * omd_k advanced from the LIBRARY'S OWN fp32 parameters p_k (only the
averaging is under test; AdamW has its own tests) with the same omd_k (the fp32 value the definition names, widened).  Bound
after k updates, elementwise: |e - e64| <= k * 2^-22 * max(|p|, |e|) -- per update two fp32 roundings, each at most 2^-24
relative to a value of at most 2 * max (the difference p - e, the result), and earlier errors contract by d <= 1; max is taken
over the parameters and averages the element has seen so far.  Everything else here is bitwise (torch.equal): the EMA is an
observer of the step, every route of the step keeps the same average, a skipped step leaves it alone, the exchange of
averaged_weights() returns the parameters as they were, and a resumed run continues the uninterrupted one."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP2 = 2.0 ** -22


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


# ------------------------------------------------------------------------------------------------ the fp64 recurrence
def _omd(decay, warmup, n):
    d = float(np.float32(decay))
    if warmup:
        d = min(d, (1.0 + n) / (10.0 + n))
    return float(np.float32(1.0 - d))


class Recurrence:
    """e64 and the bound's max, advanced one update at a time from the library's fp32 parameters."""

    def __init__(self, e0, decay, warmup):
        self.e = e0.detach().double().cpu().numpy().copy()
        self.big = np.abs(self.e)
        self.decay, self.warmup, self.k = decay, warmup, 0

    def update(self, p_new, mask=None):
        p = p_new.detach().double().cpu().numpy()
        self.k += 1
        new = self.e + (p - self.e) * _omd(self.decay, self.warmup, self.k)
        self.e = new if mask is None else np.where(mask, new, self.e)
        self.big = np.maximum(self.big, np.maximum(np.abs(p), np.abs(self.e)))

    def check(self, e, what=""):
        got = e.detach().double().cpu().numpy()
        err, bound = np.abs(got - self.e), self.k * ULP2 * self.big
        worst = float((err - bound).max())
        print(f"{what}: k={self.k} max err {err.max():.3e}, max err/bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert worst <= 0.0, (what, self.k, float(err.max()), worst)


# ------------------------------------------------------------------------------------------------ 1. the kernel, through the C entry
@pytest.mark.parametrize("decay", [0.0, 0.9, 0.999])
@pytest.mark.parametrize("warmup", [0, 1])
def test_kernel_average_against_fp64_through_the_c_entry(pkg, warmup, decay):
    """n in {1, 3, 4, 5, 1027, 4099} from a 16-byte aligned base and from 4 floats further: float4 body, scalar tail, more
    than one workgroup.  Five consecutive calls (t = 1 .. 5, t0 = 0); the floats around [offset, offset + n) stay untouched."""
    L, lib = pkg.lib(), pkg._lib
    lr, hp, gs = 3e-3, (0.9, 0.999, 1e-8, 0.02), 0.5
    for n in (1, 3, 4, 5, 1027, 4099):
        for off in (0, 4):
            g0 = torch.Generator().manual_seed(1000 * n + off)
            size = off + n + 8
            p, g, m, e = (torch.randn(size, generator=g0).to(DEV) * s for s in (1.0, 1e-2, 1e-3, 1.0))
            v = (torch.rand(size, generator=g0) * 1e-4).to(DEV)
            e0 = e.clone()
            rec = Recurrence(e[off:off + n], decay, warmup)
            for t in range(1, 6):
                g.copy_(torch.randn(size, generator=g0) * 1e-2)
                ema = lib.PLEma(e.data_ptr() + 4 * off, decay, warmup, 0)
                args = [x.data_ptr() + 4 * off for x in (p, g, m, v)]
                assert all(a % 16 == 0 for a in args)
                rc = L.pl_adamw_flat_planes_clip_ema(*args, n, lr, None, *hp, t, None, gs, None, None, ctypes.byref(ema),
                                                     torch.cuda.current_stream().cuda_stream)
                assert rc == 0, L.pl_last_error()
                rec.update(p[off:off + n])
                rec.check(e[off:off + n], f"n={n} off={off} t={t}")
            assert torch.equal(e[:off], e0[:off]) and torch.equal(e[off + n:], e0[off + n:])


@pytest.mark.parametrize("off", [0, 4])
def test_null_ema_is_the_entry_without_it_bitwise(pkg, off):
    L, n = pkg.lib(), 1027
    g0 = torch.Generator().manual_seed(5)
    init = [torch.randn(off + n, generator=g0) * s for s in (1.0, 1e-2, 1e-3)] + [torch.rand(off + n, generator=g0) * 1e-4]

    def run(name, *tail):
        bufs = [x.to(DEV) for x in init]
        rc = getattr(L, name)(*(b.data_ptr() + 4 * off for b in bufs), n, 3e-4, None, 0.9, 0.999, 1e-8, 0.02, 3, None, 0.5, None, None,
                              *tail, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, L.pl_last_error()
        return torch.stack(bufs)

    want = run("pl_adamw_flat_planes_clip")
    assert not torch.equal(want[0], init[0].to(DEV))
    assert torch.equal(run("pl_adamw_flat_planes_clip_ema", None), want)


def test_swap_exchanges_two_ranges_in_place(pkg):
    L = pkg.lib()
    for n in (1, 3, 4, 5, 1027, 4099):
        for oa, ob in ((0, 0), (4, 0), (1, 0), (0, 3)):                     # float4 on both, and the scalar path
            a, b = torch.randn(oa + n + 4, device=DEV), torch.randn(ob + n + 4, device=DEV)
            a0, b0 = a.clone(), b.clone()
            rc = L.pl_swap_f32(a.data_ptr() + 4 * oa, b.data_ptr() + 4 * ob, n, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, L.pl_last_error()
            assert torch.equal(a[oa:oa + n], b0[ob:ob + n]) and torch.equal(b[ob:ob + n], a0[oa:oa + n])
            assert torch.equal(a[:oa], a0[:oa]) and torch.equal(a[oa + n:], a0[oa + n:])
            assert torch.equal(b[:ob], b0[:ob]) and torch.equal(b[ob + n:], b0[ob + n:])


# ------------------------------------------------------------------------------------------------ the lifter
# (64, 32): the narrow width, AdamW as its own launch; (1024, 64): AdamW rides in the backward launches, beside weight planes;
# (1024, 128): the AdamW launch refreshes the planes; (256, 32), (512, 16): the ride on the other two layer-kernel variants
SHAPES = [(64, 32), (1024, 64), (1024, 128), (256, 32), (512, 16)]


def _make(pkg, H, p_dropout=0.5, **kw):
    torch.manual_seed(9)
    m = pkg.LinearModel(34, 51, linear_size=H, p_dropout=p_dropout, compute_dtype="f16x3").to(DEV).train()
    m.manual_seed(77, step=0)
    return m, pkg.FlatAdamW(m, lr=1e-3, **kw)


def _batches(pkg, B, k, seed=300):
    return [pkg.synth.synthetic_batch(B, seed + i, DEV) for i in range(k)]


def _gpu_kernel_names(fn):
    """Names of the GPU kernels one call of fn() launches (torch.profiler; as in test_gpu_parity.py)."""
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


@pytest.mark.parametrize("H,B", SHAPES)
def test_the_average_is_an_observer_of_the_step(pkg, H, B):
    """Four train_steps with ema_decay=0.99 against four without: losses, parameters, moments, BatchNorm buffers and weight
    planes bitwise equal; the average follows the recurrence."""
    plain, ema = _make(pkg, H), _make(pkg, H, ema_decay=0.99)
    rec = None
    for i, (x, y) in enumerate(_batches(pkg, B, 4)):
        l0, y0 = pkg.train_step(*plain, x, y)
        if rec is None:
            rec = Recurrence(ema[0].flat_params, 0.99, False)
        l1, y1 = pkg.train_step(*ema, x, y)
        assert torch.equal(l0, l1) and torch.equal(y0, y1), i
        assert ema[1]._e is not None and "ema" in ema[1].state[ema[0]._param_list[0]]
        rec.update(ema[0].flat_params)
        rec.check(ema[1]._e, f"H={H} B={B} step {i + 1}")
    (m0, o0), (m1, o1) = plain, ema
    assert torch.equal(m0.flat_params, m1.flat_params) and torch.equal(o0._m, o1._m) and torch.equal(o0._v, o1._v)
    assert torch.equal(m0._bn_running, m1._bn_running) and torch.equal(m0._bn_batches, m1._bn_batches)
    assert o0._e is None and "ema" not in o0.state[m0._param_list[0]]
    assert (m0._wplanes is None) == (m1._wplanes is None) and (H != 1024 or m0._wplanes is not None)
    if m0._wplanes is not None:
        assert (m0._wplanes_ver == m0._planes_key()) == (m1._wplanes_ver == m1._planes_key())
        m0._ensure_wplanes(), m1._ensure_wplanes()           # (B <= 64 leaves them stale on both: refreshed from equal parameters)
        assert torch.equal(m0._wplanes, m1._wplanes)
    assert not torch.equal(o1._e, m1.flat_params)
    for s, p in zip(m1._slots, m1._param_list):              # state[p]["ema"] IS the arena
        assert o1.state[p]["ema"].data_ptr() == o1._e.data_ptr() + 4 * s.offset and o1.state[p]["ema"].shape == p.shape


@pytest.mark.parametrize("H,B,warmup", [(64, 32, True), (1024, 64, True), (1024, 128, False), (256, 32, False), (512, 16, True)])
def test_graph_replays_keep_the_average_of_the_eager_steps_bitwise(pkg, H, B, warmup):
    kw = dict(ema_decay=0.99, ema_warmup=warmup)
    e, g = _make(pkg, H, **kw), _make(pkg, H, **kw)
    batches = _batches(pkg, B, 4, seed=340)
    step = pkg.GraphedTrainStep(*g, *batches[0])
    assert torch.equal(g[1]._e, g[0].flat_params) and torch.equal(g[0].flat_params, _make(pkg, H)[0].flat_params)
    rec = Recurrence(e[0].flat_params, 0.99, warmup)
    for i, (x, y) in enumerate(batches):
        l0, _ = pkg.train_step(*e, x, y)
        l1, _ = step(x, y)
        assert torch.equal(l0, l1), i
        assert torch.equal(e[1]._e, g[1]._e) and torch.equal(e[0].flat_params, g[0].flat_params), i
        rec.update(e[0].flat_params)
        rec.check(e[1]._e, f"H={H} B={B} step {i + 1}")
    assert torch.equal(e[1]._m, g[1]._m) and torch.equal(e[1]._v, g[1]._v)
    assert e[1].state_dict()["param_groups"][0]["ema_updates"] == g[1].state_dict()["param_groups"][0]["ema_updates"] == 4
    # not one launch more than the step without the average -- where AdamW rides in the backward launches (B = 64 at
    # H = 1024 and the two narrower ride shapes) the average rides with it
    rides = (H, B) in ((1024, 64), (256, 32), (512, 16))
    assert e[0].step_carries_adamw(B) == rides == step._in_call
    off = _make(pkg, H)
    x, y = batches[0]
    pkg.train_step(*off, x, y)                                              # (first call: arenas, workspace)
    n_off = len(_gpu_kernel_names(lambda: pkg.train_step(*off, x, y)))
    names = _gpu_kernel_names(lambda: pkg.train_step(*e, x, y))
    print(f"H={H} B={B}: {len(names)} launches with the average, {n_off} without")
    assert 0 < len(names) <= n_off, (len(names), n_off)
    if rides:
        assert any("small_bwd_kernel" in n for n in names) and sum("adamw_kernel" in n for n in names) == 1
    # switching the average off (or changing it) after capture is refused, as switching clipping is
    g[1].param_groups[0]["ema_decay"] = None
    with pytest.raises(pkg.PoseliftError, match="after capture"):
        step(*batches[0])
    g[1].param_groups[0]["ema_decay"] = 0.5
    with pytest.raises(pkg.PoseliftError, match="after capture"):
        step(*batches[0])


@pytest.mark.parametrize("graphed", [False, True])
def test_a_skipped_step_leaves_the_average_alone_and_does_not_count(pkg, graphed):
    """Five steps, the third with a NaN target, skip_nonfinite and ema_warmup on: the average is bitwise unchanged across
    step 3 and follows the recurrence with n = 1, 2, 3, 4 (with warmup d_n depends on n: a miscount shows)."""
    torch.manual_seed(4)
    m = pkg.LinearModel(34, 51, linear_size=64, p_dropout=0.0).to(DEV).train()
    opt = pkg.FlatAdamW(m, lr=3e-3, weight_decay=0.02, skip_nonfinite=True, ema_decay=0.99, ema_warmup=True)
    x, y = pkg.synth.synthetic_batch(16, 8, DEV)
    do = pkg.GraphedTrainStep(m, opt, x, y) if graphed else (lambda a, b: pkg.train_step(m, opt, a, b))
    rec = Recurrence(m.flat_params, 0.99, True)
    for it in range(1, 6):
        yy = y.clone()
        if it == 3:
            yy[5, 7, 2] = float("nan")
        before = (opt._e.clone() if opt._e is not None else None, m.flat_params.clone())
        loss, _ = do(x, yy)
        if it == 3:
            assert not torch.isfinite(loss)
            assert torch.equal(opt._e, before[0]) and torch.equal(m.flat_params, before[1])
            continue
        assert not torch.equal(m.flat_params, before[1])
        rec.update(m.flat_params)
        rec.check(opt._e, f"graphed={graphed} step {it}")
    assert rec.k == 4 and opt.skipped_steps() == 1 and opt._t == 5
    sd = opt.state_dict()
    assert sd["param_groups"][0]["ema_updates"] == 4 == opt.param_groups[0]["ema_updates"]
    assert float(sd["state"][0]["step"]) == 4.0


# ------------------------------------------------------------------------------------------------ 5. the context and the caches
def _round_trip(pkg, m, opt, fwd, fresh, flat):
    """The averaged_weights() round trip on a model in eval mode: inside, the model computes what a fresh model loaded from
    ema_state_dict() computes, and not what it computed before; afterwards everything is bitwise as it was."""
    m.eval()
    with torch.no_grad():
        y_live = fwd(m).clone()
        p_live, e_live = flat.clone(), opt._e.clone()
        sd = opt.ema_state_dict()
        other = fresh().to(DEV).eval()
        other.load_state_dict(sd)
        y_want = fwd(other).clone()
        with opt.averaged_weights():
            y_avg = fwd(m).clone()
            assert torch.equal(flat, e_live) and torch.equal(opt._e, p_live)
            inside = opt.ema_state_dict()
            assert all(torch.equal(inside[k], sd[k]) for k in sd)
            with pytest.raises(pkg.PoseliftError, match="averaged_weights"):
                opt.step()
            with pytest.raises(pkg.PoseliftError, match="re-entrant"):
                with opt.averaged_weights():
                    pass
        assert torch.equal(y_avg, y_want) and not torch.equal(y_avg, y_live)
        assert torch.equal(fwd(m), y_live)
        assert torch.equal(flat, p_live) and torch.equal(opt._e, e_live)
    # buffers are the live ones, parameters the averages
    named, moved = dict(m.named_parameters()), 0
    for k, v in m.state_dict().items():
        if k in named:
            assert torch.equal(sd[k], opt.state[named[k]]["ema"]), k
            moved += int(not torch.equal(sd[k], v))
        else:
            assert torch.equal(sd[k], v), k
    assert moved > 0 and set(sd) == set(m.state_dict())
    return y_live, y_avg


def test_averaged_weights_context_on_the_lifter_with_weight_planes(pkg):
    m, opt = _make(pkg, 1024, ema_decay=0.9)
    batches = _batches(pkg, 128, 3, seed=380)
    step = pkg.GraphedTrainStep(m, opt, *batches[0])
    for x, y in batches:
        pkg.train_step(m, opt, x, y)
    assert m._wplanes_ver == m._planes_key()                  # the AdamW launch left the planes of the LIVE weights current
    x, y = batches[0]
    fresh = lambda: pkg.LinearModel(34, 51, linear_size=1024, p_dropout=0.5, compute_dtype="f16x3")
    y_live, y_avg = _round_trip(pkg, m, opt, lambda mod: mod(x), fresh, m.flat_params)
    metric = torch.zeros(17, device=DEV)
    with opt.averaged_weights():
        with pytest.raises(pkg.PoseliftError, match="averaged_weights"):
            pkg.train_step(m, opt, x, y)
        with pytest.raises(pkg.PoseliftError, match="averaged_weights"):
            step(x, y)
        m.train()
        with pytest.raises(pkg.PoseliftError, match="averaged_weights"):
            pkg.train_step(m, opt, x, y)                                    # (the fused route)
        m.eval()
        want = pkg.eval_step(m, x, y)
    got = pkg.eval_step(m, x, y, ema=opt)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and torch.equal(got[2].reshape(y_avg.shape), y_avg)
    live = pkg.eval_step(m, x, y)
    assert torch.equal(live[2].reshape(y_live.shape), y_live) and not torch.equal(live[0], got[0])
    # and training goes on from the live weights
    m.train()
    ref, ropt = _make(pkg, 1024, ema_decay=0.9)
    for xb, yb in batches:
        pkg.train_step(ref, ropt, xb, yb)
    l0, _ = pkg.train_step(ref, ropt, x, y)
    l1, _ = pkg.train_step(m, opt, x, y)
    assert torch.equal(l0, l1) and torch.equal(ref.flat_params, m.flat_params) and torch.equal(ropt._e, opt._e)
    plain = pkg.FlatAdamW(_make(pkg, 64)[0])
    with pytest.raises(pkg.PoseliftError, match="ema_decay"):
        with plain.averaged_weights():
            pass


def test_averaged_weights_context_on_myvit_bf16p(pkg):
    torch.manual_seed(164)
    m = pkg.MyViT(compute_dtype="bf16p").to(DEV).train()
    opt = pkg.FlatAdam(m, lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True, ema_decay=0.9)
    rng = np.random.default_rng(640)
    x = torch.as_tensor(rng.uniform(0.0, 1.0, (64, 17, 2)).astype(np.float32), device=DEV)
    y = torch.as_tensor((0.2 * rng.standard_normal((64, 17, 3))).astype(np.float32), device=DEV)
    for _ in range(3):
        pkg.train_step(m, opt, x, y)
    _round_trip(pkg, m, opt, lambda mod: mod(x), lambda: pkg.MyViT(compute_dtype="bf16p"), opt.arena.flat)


def _small(seed=12):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(7, 5), nn.Tanh(), nn.Linear(5, 3)).to(DEV)


def _small_step(mod, opt, x, t):
    opt.zero_grad()
    loss = (mod(x) - t).pow(2).mean()
    loss.backward()
    opt.step()
    return loss.detach()


def test_averaged_weights_context_on_a_stock_module(pkg):
    mod = _small()
    opt = pkg.FlatAdam(mod, lr=1e-2, ema_decay=0.9)
    x, t = torch.randn(6, 7, device=DEV), torch.randn(6, 3, device=DEV)
    for _ in range(3):
        _small_step(mod, opt, x, t)
    _round_trip(pkg, mod, opt, lambda m: m(x), lambda: _small(99), opt.arena.flat)


def test_averaged_weights_context_on_model_2d_follows_the_folded_bn_cache(pkg):
    m = pkg.Model_2D().train()
    m.load_state_dict(pkg.synth.seeded_state(m.state_dict(), 41))
    with torch.no_grad():
        m.final_layer.weight.mul_(1e-3)
    m = m.to(DEV)
    opt = pkg.FlatAdam(m, lr=1e-3, ema_decay=0.5)
    frames = pkg.synth.seeded_frames(2, 42, 32).permute(0, 3, 1, 2).contiguous().to(DEV)
    target = torch.rand(2, 17, 2, generator=torch.Generator().manual_seed(3)).to(DEV)
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        out = m(frames)
        (out.reshape(2, 17, 2) - target).pow(2).mean().backward()
        opt.step()
    m.eval()
    with torch.no_grad():
        m(frames)                                             # the eval forward folds BatchNorm into a cache keyed on versions

    def fresh():
        return pkg.Model_2D()
    _round_trip(pkg, m, opt, lambda mod: mod(frames), fresh, opt.arena.flat)


# ------------------------------------------------------------------------------------------------ 6. checkpoints
def _lifter_record(m, opt):
    sd = opt.state_dict()
    return (m.flat_params.clone(), opt._m.clone(), opt._v.clone(), opt._e.clone(), m._bn_running.clone(),
            sd["param_groups"][0]["ema_updates"], float(sd["state"][0]["step"]))


def _same_records(a, b):
    return all(torch.equal(u, v) if torch.is_tensor(u) else u == v for u, v in zip(a, b))


def test_lifter_checkpoint_resumes_the_average_bitwise(pkg):
    kw = dict(ema_decay=0.99, ema_warmup=True)
    batches = _batches(pkg, 32, 6, seed=420)
    m, opt = _make(pkg, 64, **kw)
    for x, y in batches:
        pkg.train_step(m, opt, x, y)
    want = _lifter_record(m, opt)
    assert want[5] == 6
    m, opt = _make(pkg, 64, **kw)
    for x, y in batches[:3]:
        pkg.train_step(m, opt, x, y)
    ck = {"model": {k: v.clone() for k, v in m.state_dict().items()}, "optimizer": opt.state_dict(), "dropout": m.dropout_state()}
    ck["optimizer"] = {"state": {i: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}
                                 for i, st in ck["optimizer"]["state"].items()},
                       "param_groups": [dict(g) for g in ck["optimizer"]["param_groups"]]}
    assert ck["optimizer"]["param_groups"][0]["ema_updates"] == 3 and "ema" in ck["optimizer"]["state"][0]
    torch.manual_seed(777)
    m2 = pkg.LinearModel(34, 51, linear_size=64, p_dropout=0.5, compute_dtype="f16x3").to(DEV).train()
    m2.load_state_dict(ck["model"])
    opt2 = pkg.FlatAdamW(m2, lr=1e-3, **kw)
    opt2.load_state_dict(ck["optimizer"])
    m2.manual_seed(**ck["dropout"])
    assert torch.equal(opt2._e, opt._e) and opt2.state_dict()["param_groups"][0]["ema_updates"] == 3
    for x, y in batches[3:]:
        pkg.train_step(m2, opt2, x, y)
    assert _same_records(_lifter_record(m2, opt2), want)

    # a state without the averages into an optimizer that keeps them: they start from the current parameters, 0 updates
    pm, popt = _make(pkg, 64)
    for x, y in batches[:2]:
        pkg.train_step(pm, popt, x, y)
    plain_sd = popt.state_dict()
    assert "ema" not in plain_sd["state"][0] and plain_sd["param_groups"][0].get("ema_updates") is None
    m3, opt3 = _make(pkg, 64, **kw)
    m3.load_state_dict(pm.state_dict())
    opt3.load_state_dict(plain_sd)
    assert opt3.param_groups[0]["ema_decay"] == 0.99 and opt3.param_groups[0]["ema_warmup"] is True
    assert torch.equal(opt3._e, m3.flat_params) and opt3.state_dict()["param_groups"][0]["ema_updates"] == 0
    rec = Recurrence(m3.flat_params, 0.99, True)
    pkg.train_step(m3, opt3, *batches[2])
    rec.update(m3.flat_params)                                # n = 1 although AdamW's t is 3
    rec.check(opt3._e, "fresh average behind a loaded state")
    assert float(opt3.state_dict()["state"][0]["step"]) == 3.0 and opt3.state_dict()["param_groups"][0]["ema_updates"] == 1

    # a state with the averages into a plain optimizer: loads, ignores them, and steps as the plain optimizer does
    m4, opt4 = _make(pkg, 64)
    m4.load_state_dict(ck["model"])
    opt4.load_state_dict(ck["optimizer"])
    m4.manual_seed(**ck["dropout"])
    assert opt4._e is None and opt4.param_groups[0]["ema_decay"] is None and "ema" not in opt4.state[m4._param_list[0]]
    for x, y in batches[3:]:
        pkg.train_step(m4, opt4, x, y)
    assert torch.equal(m4.flat_params, want[0]) and torch.equal(opt4._m, want[1]) and torch.equal(opt4._v, want[2])
    assert "ema" not in opt4.state_dict()["state"][0]


@pytest.mark.parametrize("capturable", [False, True])
def test_flat_adam_checkpoint_resumes_the_average_bitwise(pkg, capturable):
    kw = dict(lr=1e-2, ema_decay=0.9, ema_warmup=True, capturable=capturable)
    g0 = torch.Generator().manual_seed(8)
    data = [(torch.randn(6, 7, generator=g0).to(DEV), torch.randn(6, 3, generator=g0).to(DEV)) for _ in range(6)]

    def record(opt):
        sd = opt.state_dict()
        return (opt.arena.flat.clone(), opt._m.clone(), opt._v.clone(), opt._e.clone(), sd["param_groups"][0]["ema_updates"],
                float(sd["state"][0]["step"]))

    mod = _small()
    opt = pkg.FlatAdam(mod, **kw)
    for x, t in data:
        _small_step(mod, opt, x, t)
    want = record(opt)
    assert want[4] == 6 and want[5] == 6.0
    mod = _small()
    opt = pkg.FlatAdam(mod, **kw)
    for x, t in data[:3]:
        _small_step(mod, opt, x, t)
    msd = {k: v.clone() for k, v in mod.state_dict().items()}
    osd = opt.state_dict()
    osd = {"state": {i: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()} for i, st in osd["state"].items()},
           "param_groups": [dict(g) for g in osd["param_groups"]]}
    mod2 = _small(99)
    mod2.load_state_dict(msd)
    opt2 = pkg.FlatAdam(mod2, **kw)
    opt2.load_state_dict(osd)
    assert torch.equal(opt2._e, opt._e)
    for x, t in data[3:]:
        _small_step(mod2, opt2, x, t)
    assert _same_records(record(opt2), want)


# ------------------------------------------------------------------------------------------------ 7. FlatAdam in a graph
def test_flat_adam_graphed_module_step_keeps_the_average_and_a_frozen_parameter_keeps_its_copy(pkg):
    def build():
        mod = _small().train()
        mod[0].bias.requires_grad_(False)
        return mod, pkg.FlatAdam(mod, lr=1e-2, capturable=True, ema_decay=0.9)

    g0 = torch.Generator().manual_seed(21)
    data = [(torch.randn(6, 7, generator=g0).to(DEV), torch.randn(6, 3, generator=g0).to(DEV)) for _ in range(3)]
    (me, oe), (mg, og) = build(), build()
    e0 = og._e.clone()
    assert torch.equal(e0, og.arena.flat)
    step = pkg.GraphedModuleStep(mg, og, torch.nn.functional.mse_loss, data[0][0], data[0][1])
    assert torch.equal(og._e, e0) and torch.equal(og.arena.flat, e0)          # the warm-up steps were undone, the average too
    rec = Recurrence(oe.arena.flat, 0.9, False)
    frozen = np.zeros(oe.arena.numel, dtype=bool)
    for p, o in zip(oe.arena.params, oe.arena.offsets):
        if p.requires_grad:
            frozen[o:o + (p.numel() + 63) // 64 * 64] = True
    active = frozen                                                           # (True where the step updates)
    for i, (x, t) in enumerate(data):
        oe.zero_grad(set_to_none=True)
        le = torch.nn.functional.mse_loss(me(x), t)
        le.backward()
        oe.step()
        lg = step(x, t)
        assert torch.equal(le.detach(), lg), i
        assert torch.equal(oe._e, og._e) and torch.equal(oe.arena.flat, og.arena.flat), i
        rec.update(oe.arena.flat, mask=active)
        rec.check(oe._e, f"FlatAdam graph step {i + 1}")
    assert torch.equal(oe._m, og._m) and torch.equal(oe._v, og._v)
    b = me[0].bias
    assert torch.equal(oe.state[b]["ema"], og.state[mg[0].bias]["ema"])
    o = oe.arena.offsets[1]
    assert torch.equal(oe.state[b]["ema"].reshape(-1), e0[o:o + b.numel()]) and torch.equal(b.detach().reshape(-1), e0[o:o + b.numel()])
    assert not torch.equal(oe.state[me[0].weight]["ema"], me[0].weight.detach())
    assert og.state_dict()["param_groups"][0]["ema_updates"] == 3
    with og.averaged_weights():
        with pytest.raises(pkg.PoseliftError, match="averaged_weights"):
            step(*data[0])
