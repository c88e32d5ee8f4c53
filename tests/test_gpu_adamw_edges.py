"""Flat AdamW on every route against fp64, at the hyper-parameter and value edges (tests/adamw_oracle.py).

Every comparison is one step: the fp64 reference (adamw_oracle.step64) starts from the GPU'S OWN fp32 p, m, v of the step before
and the gradient the GPU read, with the hyper-parameters rounded to fp32 and t exact, and the GPU's result is held to
adamw_oracle.bounds (K = 16, u = 2^-24, tau = 2^-126) -- so step k of a run is held as tightly as step 1.  The worst ratio
per quantity is printed in units of those bounds.  tests/test_adamw_edges_host.py shows what the gate means: the kernel's
order emulated in numpy fp32 stays below 0.31 of it, and a bias correction from an fp32 pow, a fixed eps, swapped betas, t
off by one, a gradient scale that misses v, decay after the update, eps under 1 / sqrt(bc2) or a dropped clip coefficient
each leave it.

Routes: the C entry pl_adamw_flat_planes_clip_ema on plain tensors (float4 body, scalar tail, the scalar loop of misaligned
pointers, the grid-stride second pass, host t / lr against t_base + *t_dev / *lr_dev, the clip record, the averaged weights);
FlatAdamW.step() and arena.FlatAdam.step() (plain and capturable) with hyper-parameters changed in param_groups between
steps; the B <= 64 train_step that carries AdamW in its backward launches (BwdCtx::ride, FlatAdamW._step_struct); graph
replays of GraphedTrainStep (both routes) and GraphedModuleStep, which bake betas, eps and weight_decay into the captured
launches and therefore have to FOLLOW a change or REFUSE the replay; a loaded stock state at step 10^6."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

import adamw_oracle as ao

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 7.5                     # what the floats around [lead, lead + n) hold before and must hold after
LEAD, TRAIL = 4, 8


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


def _n(t):
    return t.detach().cpu().numpy()


def _hold(tag, before, after, g, hp, t, coef=1.0, mask=None, quiet=False):
    """(p, m, v) after one step from (p, m, v) before with gradient g: inside the bounds of the fp64 step at (hp, t, coef).
    Returns the ratios; prints them unless quiet."""
    p0, m0, v0 = (np.asarray(a, np.float32).reshape(-1) for a in before)
    p1, m1, v1 = (np.asarray(a, np.float32).reshape(-1) for a in after)
    g = np.asarray(g, np.float32).reshape(-1)
    if mask is not None:
        p0, m0, v0, p1, m1, v1, g = (a[mask] for a in (p0, m0, v0, p1, m1, v1, g))
    ref = ao.step64(p0, g, m0, v0, hp, t, coef)
    r = ao.ratios(p1, m1, v1, p0, m0, ref)
    if not quiet:
        print(f"    {tag}: p {r['p']:.3g} m {r['m']:.3g} v {r['v']:.3g} of the bounds")
    assert max(r.values()) <= 1.0, (tag, r, hp, t, coef)
    if ao.f32(hp[0]) == 0.0:
        assert np.array_equal(p1, p0), f"{tag}: lr = 0 must return p bitwise"
    return r


def _worse(worst, r, where):
    for q, x in r.items():
        if x > worst[q][0]:
            worst[q] = (x, where)


def _print_worst(tag, worst):
    for q, (x, where) in worst.items():
        print(f"    {tag} {q}: worst {x:.3g} of the bound   ({where})")


# ------------------------------------------------------------------------------------------------ a. the C entry on plain tensors
class Rows:
    """One device buffer of `rows` rows per quantity, each row = LEAD (+1 when misaligned) guard floats, n values, >= TRAIL
    guard floats; rows start 16-byte aligned."""

    def __init__(self, rows, n, misaligned=False):
        self.n, self.lead = n, LEAD + (1 if misaligned else 0)
        self.stride = (self.lead + n + TRAIL + 3) // 4 * 4
        self.host = np.full((rows, self.stride), GUARD, np.float32)

    def put(self, r, values):
        self.host[r, self.lead:self.lead + self.n] = values

    def upload(self):
        self.dev = torch.from_numpy(self.host).to(DEV)
        assert self.dev.data_ptr() % 16 == 0
        return self

    def ptr(self, r):
        return self.dev.data_ptr() + 4 * (r * self.stride + self.lead)

    def download(self):
        out = _n(self.dev)
        body = out[:, self.lead:self.lead + self.n]
        guards = np.concatenate([out[:, :self.lead], out[:, self.lead + self.n:]], axis=1)
        assert (guards == GUARD).all(), "floats outside [0, n) were written"
        return body


def _clip_record(coef, skipped):
    """A PLClipRecord on the device: {norm, coef, finite = 1, skip = 0, skipped}."""
    rec = torch.zeros(6, dtype=torch.int32)
    rec.view(torch.float32)[0] = 1.0
    rec.view(torch.float32)[1] = coef
    rec[2] = 1
    rec.view(torch.int64)[2] = skipped
    return rec.to(DEV)


def _adamw(pkg, bufs, r, n, hp, t, lr_dev=None, t_dev=None, clip=None, ema=None):
    """One pl_adamw_flat_planes_clip_ema on row r of bufs = (p, g, m, v); lr_dev / t_dev: device addresses (then t is t_base)."""
    lr, b1, b2, eps, wd, gs = hp
    P, G, M, V = bufs
    rc = pkg.lib().pl_adamw_flat_planes_clip_ema(P.ptr(r), G.ptr(r), M.ptr(r), V.ptr(r), n, 0.0 if lr_dev else lr, lr_dev, b1, b2,
                                                 eps, wd, t, t_dev, gs, None, clip.data_ptr() if clip is not None else None,
                                                 ctypes.byref(ema) if ema is not None else None, pkg._lib.current_stream_ptr())
    pkg._lib.check(rc, "pl_adamw_flat_planes_clip_ema")


def _fill(cases, n, misaligned=False, seed=0):
    bufs = tuple(Rows(len(cases), n, misaligned) for _ in range(4))
    vals = []
    for r, c in enumerate(cases):
        pgmv = ao.values(c.cls, n, c.t, seed)
        vals.append(pgmv)
        for b, a in zip(bufs, pgmv):
            b.put(r, a)
    return bufs, vals


@pytest.mark.parametrize("clip", [False, True], ids=["norecord", "cliprecord"])
@pytest.mark.parametrize("cls", ao.CLASSES)
def test_c_entry_over_the_case_grid(pkg, cls, clip):
    """Every (tuple, gscale, t) of the grid on one value class at n = 1027 (256 float4 + 3: one block and a tail), by value
    (host t, lr) and again from device memory (t_base + *t_dev, *lr_dev): the two are bitwise equal, and held to the bounds.
    With the record: coef = 0.37 folds into the gradient scale and skipped = 2 comes off a t passed two higher
    (adamw_consts_clip, the deliberate copy of adamw_consts)."""
    cases = ao.cases([cls])
    n = ao.N_GRID
    coef, skipped = (0.37, 2) if clip else (1.0, 0)
    rec = _clip_record(coef, skipped) if clip else None
    lrs = torch.tensor([hp[0] for hp in ao.HP_TUPLES], dtype=torch.float32, device=DEV)
    ticks = torch.tensor([1, 3], dtype=torch.int64, device=DEV)
    got = []
    for from_dev in (False, True):
        bufs, vals = _fill(cases, n)
        for b in bufs:
            b.upload()
        for r, c in enumerate(cases):
            t = c.t + skipped
            if from_dev:
                k = 0 if t < 4 else 1                       # *t_dev = 1 or 3, t_base = the rest
                i = ao.HP_TUPLES.index(c.hp[:5])
                _adamw(pkg, bufs, r, n, c.hp, t - (1, 3)[k], lr_dev=lrs.data_ptr() + 4 * i, t_dev=ticks.data_ptr() + 8 * k, clip=rec)
            else:
                _adamw(pkg, bufs, r, n, c.hp, t, clip=rec)
        torch.cuda.synchronize()
        got.append([b.download() for b in bufs])
    for a, b in zip(*got):
        assert np.array_equal(a, b), "t / lr by value and from device memory differ"
    P, G, M, V = got[0]
    worst = {"p": (0.0, ""), "m": (0.0, ""), "v": (0.0, "")}
    for r, c in enumerate(cases):
        p0, g0, m0, v0 = vals[r]
        assert np.array_equal(G[r], g0)
        _worse(worst, _hold(c.id, (p0, m0, v0), (P[r], M[r], V[r]), g0, c.hp, c.t, coef, quiet=True), c.id)
    _print_worst(f"C entry, {cls}, {'record' if clip else 'no record'}", worst)


# (n, tuple index, gscale, t, class): one tuple per size
SIZES = [(1, 0, 1.0, 1, "normal"), (3, 1, 0.125, 2, "mixed"), (4, 2, 3.7, 7, "normal"), (5, 3, 1.0, 1000, "mixed"),
         (255, 4, 0.125, 10 ** 6, "huge"), (None, 3, 3.7, 2, "mixed")]


@pytest.mark.parametrize("ema", [None, 0, 1], ids=["noema", "ema", "ema-warmup"])
@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "offbyone"])
def test_c_entry_sizes_alignment_and_the_average(pkg, misaligned, ema):
    """n in {1, 3, 4, 5, 255} and one n past the grid: 524288 + 7 aligned (a second pass of the 512 x 256 x 4 grid and a
    3-float tail), 131072 + 5 with every pointer one float further (the scalar loop, a second pass of 512 x 256).  With
    PLEma: the average follows from the new p within 4 u (|e| + |p'|), from its own 16-byte aligned arena."""
    worst = {"p": (0.0, ""), "m": (0.0, ""), "v": (0.0, "")}
    worst_e = 0.0
    for n, i, gs, t, cls in SIZES:
        n = n or (131072 + 5 if misaligned else 524288 + 7)
        c = ao.Case(f"n{n}/{cls}/hp{i}/gs{gs:g}/t{t}", cls, ao.HP_TUPLES[i] + (gs,), t)
        bufs, vals = _fill([c], n, misaligned, seed=3)
        for b in bufs:
            b.upload()
        assert (bufs[0].ptr(0) % 16 != 0) == misaligned
        E = st = None
        if ema is not None:
            E = Rows(1, n)
            e0 = np.random.default_rng(n).standard_normal(n).astype(np.float32)
            E.put(0, e0)
            E.upload()
            t0 = max(0, t - 3)
            st = pkg._lib.PLEma(E.ptr(0), 0.999, ema, t0)
        _adamw(pkg, bufs, 0, n, c.hp, t, ema=st)
        torch.cuda.synchronize()
        P, G, M, V = (b.download()[0] for b in bufs)
        p0, g0, m0, v0 = vals[0]
        assert np.array_equal(G, g0)
        _worse(worst, _hold(c.id, (p0, m0, v0), (P, M, V), g0, c.hp, t, quiet=True), c.id)
        if ema is not None:
            ref, bound = ao.ema64(e0, P, 0.999, ema, t - t0)
            ratio = float((np.abs(E.download()[0].astype(np.float64) - ref) / bound).max())
            worst_e = max(worst_e, ratio)
            assert ratio <= 1.0, (c.id, ratio)
    tag = f"C entry sizes, {'misaligned' if misaligned else 'aligned'}"
    _print_worst(tag, worst)
    if ema is not None:
        print(f"    {tag} e: worst {worst_e:.3g} of the bound")


# ------------------------------------------------------------------------------------------------ b. the optimizers' step()
def _hp_of(opt, grad_scale=1.0, lr=None):
    g = opt.param_groups[0]
    wd = g["weight_decay"] if g.get("decoupled_weight_decay", True) else 0.0
    return (float(g["lr"] if lr is None else lr), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(wd), grad_scale)


def _set_hp(opt, lr, b1, b2, eps, wd):
    g = opt.param_groups[0]
    g["lr"], g["betas"], g["eps"], g["weight_decay"] = lr, (b1, b2), eps, wd


def _mask_of(runs, n):
    mask = np.zeros(n, bool)
    for lo, hi in runs:
        mask[lo:hi] = True
    return mask


def _grad_values(n, k):
    """Gradients for step k of an optimizer test: N(0,1) 1e-2 with every fifth element at a decade from 1e-12 to 1e5."""
    rng = np.random.default_rng(100 + k)
    g = rng.standard_normal(n) * 1e-2
    g[::5] = rng.choice([-1.0, 1.0], g[::5].size) * 10.0 ** rng.integers(-12, 6, g[::5].size)
    return g.astype(np.float32)


STEPS = [(ao.HP_TUPLES[3], 3.7), (ao.HP_TUPLES[2], 0.125), (ao.HP_TUPLES[4], 1.0), (ao.HP_TUPLES[5], 3.7), (ao.HP_TUPLES[1], 1.0)]


def test_flat_adamw_step_follows_param_groups_and_leaves_inactive_ranges_alone(pkg):
    """LinearModel(linear_size=64, BN=False): the BatchNorm tensors hold no gradient, so the step is one launch per run of active
    tensors.  Built with one non-default tuple; betas, eps, weight_decay, lr and grad_scale change before every further step and
    the NEXT step uses the new values.  Inactive ranges of p, m and v stay bitwise."""
    torch.manual_seed(5)
    m = pkg.LinearModel(34, 51, linear_size=64, num_stage=1, p_dropout=0.0, BN=False).to(DEV).train()
    hp0, _ = STEPS[0]
    opt = pkg.FlatAdamW(m, lr=hp0[0], betas=hp0[1:3], eps=hp0[3], weight_decay=hp0[4])
    opt._bind()
    n = m.flat_params.numel()
    runs = opt._active_ranges()
    mask = _mask_of(runs, n)
    assert len(runs) > 1 and mask.any() and not mask.all()
    for k, (hp, gs) in enumerate(STEPS, 1):
        _set_hp(opt, *hp)
        g = _grad_values(n, k)
        m.flat_grads.copy_(torch.from_numpy(g))
        before = tuple(_n(a).copy() for a in (m.flat_params, opt._m, opt._v))
        opt.step(grad_scale=gs)
        after = tuple(_n(a) for a in (m.flat_params, opt._m, opt._v))
        _hold(f"FlatAdamW.step {k}", before, after, g, hp + (gs,), k, mask=mask)
        for a, b in zip(before, after):
            assert np.array_equal(a[~mask], b[~mask]), f"step {k}: an inactive range was written"
    assert float(opt.state_dict()["state"][0]["step"]) == len(STEPS)


def _tiny(seed=12):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(7, 16), nn.Tanh(), nn.Linear(16, 3)).to(DEV)


def _arena_grads(opt, g, skip=()):
    """Put g into FlatAdam's gradient arena and hand every parameter (not those in `skip`) its view of it as .grad."""
    opt.arena.grad.copy_(torch.from_numpy(g))
    for i, p in enumerate(opt.arena.params):
        p.grad = None if i in skip else p._pl_grad


@pytest.mark.parametrize("capturable", [False, True], ids=["plain", "capturable"])
def test_flat_adam_step_follows_param_groups_and_leaves_gradless_parameters_alone(pkg, capturable):
    """arena.FlatAdam (decoupled_weight_decay=True) on a stock module; the first bias holds no gradient: its slot of p, m, v stays
    bitwise.  capturable: t and lr are read from device memory."""
    mod = _tiny()
    hp0, _ = STEPS[0]
    opt = pkg.FlatAdam(mod, lr=hp0[0], betas=hp0[1:3], eps=hp0[3], weight_decay=hp0[4], decoupled_weight_decay=True,
                       capturable=capturable)
    n = opt.arena.numel
    o1, n1 = opt.arena.offsets[1], (opt.arena.params[1].numel() + 63) // 64 * 64
    mask = np.ones(n, bool)
    mask[o1:o1 + n1] = False
    for k, (hp, gs) in enumerate(STEPS, 1):
        _set_hp(opt, *hp)
        g = _grad_values(n, 10 + k)
        _arena_grads(opt, g, skip=(1,))
        before = tuple(_n(a).copy() for a in (opt.arena.flat, opt._m, opt._v))
        opt.step(grad_scale=gs)
        after = tuple(_n(a) for a in (opt.arena.flat, opt._m, opt._v))
        _hold(f"FlatAdam.step {k} ({'capturable' if capturable else 'plain'})", before, after, g, hp + (gs,), k, mask=mask)
        for a, b in zip(before, after):
            assert np.array_equal(a[~mask], b[~mask]), f"step {k}: a parameter without a gradient was written"
    assert float(opt.state_dict()["state"][0]["step"]) == len(STEPS)


@pytest.mark.parametrize("which", ["FlatAdamW", "FlatAdam-capturable"])
def test_clipped_step_after_a_skipped_one_counts_taken_steps_and_scales_by_the_coefficient(pkg, which):
    """max_grad_norm + skip_nonfinite with beta2 = 0.9, where bc2 at t = 2 and t = 3 differ by 1.4: a normal step, a step whose
    gradient holds an inf (skipped: p, m, v bitwise), a normal step -- held to t = 3 - 1 and g' = g * grad_scale * clip_coef."""
    hp = (1e-2, 0.5, 0.9, 1e-6, 0.1)
    if which == "FlatAdamW":
        torch.manual_seed(6)
        m = pkg.LinearModel(34, 51, linear_size=64, num_stage=1, p_dropout=0.0, BN=False).to(DEV).train()
        opt = pkg.FlatAdamW(m, lr=hp[0], betas=hp[1:3], eps=hp[3], weight_decay=hp[4], max_grad_norm=0.5, skip_nonfinite=True)
        opt._bind()
        flat, grads = m.flat_params, m.flat_grads
        mask = _mask_of(opt._active_ranges(), flat.numel())
        put = lambda g: grads.copy_(torch.from_numpy(g))
    else:
        mod = _tiny(13)
        opt = pkg.FlatAdam(mod, lr=hp[0], betas=hp[1:3], eps=hp[3], weight_decay=hp[4], decoupled_weight_decay=True,
                           capturable=True, max_grad_norm=0.5, skip_nonfinite=True)
        flat, grads = opt.arena.flat, opt.arena.grad
        mask = np.ones(flat.numel(), bool)
        put = lambda g: _arena_grads(opt, g)
    n, gs = flat.numel(), 0.25
    rng = np.random.default_rng(77)
    taken = 0
    for k, bad in enumerate((False, True, False), 1):
        g = (rng.standard_normal(n) * 0.3).astype(np.float32)
        if which != "FlatAdamW":                          # (alignment padding of a stock module's arena holds no gradient)
            pad = np.ones(n, bool)
            for p, o in zip(opt.arena.params, opt.arena.offsets):
                pad[o:o + p.numel()] = False
            g[pad] = 0.0
        if bad:
            g[np.flatnonzero(mask)[5]] = np.inf
        put(g)
        before = tuple(_n(a).copy() for a in (flat, opt._m, opt._v))
        opt.step(grad_scale=gs)
        after = tuple(_n(a) for a in (flat, opt._m, opt._v))
        if bad:
            for a, b in zip(before, after):
                assert np.array_equal(a, b), "a skipped step wrote p, m or v"
            continue
        taken += 1
        coef = float(opt.clip_coef.item())
        norm = gs * float(np.sqrt((g[mask].astype(np.float64) ** 2).sum()))
        assert 0.0 < coef < 1.0 and abs(coef - 0.5 / norm) <= 1e-4 * coef, (coef, 0.5 / norm)
        _hold(f"{which} clipped step {k} (t = {taken}, coef {coef:.4f})", before, after, g, hp + (gs,), taken, coef, mask=mask)
        for a, b in zip(before, after):
            assert np.array_equal(a[~mask], b[~mask])
    assert opt.skipped_steps() == 1
    assert float(opt.state_dict()["state"][0]["step"]) == 2


# ------------------------------------------------------------------------------------------------ c. AdamW inside the backward launches
def _real_slots(model):
    real = np.zeros(model.flat_params.numel(), bool)
    for s in model._slots:
        real[s.offset:s.offset + s.numel] = True
    return real


@pytest.mark.parametrize("hp_a,hp_b", [(ao.HP_TUPLES[3], ao.HP_TUPLES[2]), (ao.HP_TUPLES[4], ao.HP_TUPLES[1])], ids=["hp3-hp2", "hp4-hp1"])
@pytest.mark.parametrize("B,H,S", [(20, 256, 1), (9, 512, 0)])
def test_ride_carries_every_hyper_parameter(pkg, B, H, S, hp_a, hp_b):
    """train_step at B <= 64: FlatAdamW._step_struct fills PLAdamWStep and BwdCtx::ride() refills an AdamWRide from it field by
    field.  Two steps, the second with every hyper-parameter changed in param_groups; p, m, v before each step and the gradient
    arena after it hold the parameter slots to the bounds."""
    torch.manual_seed(0)
    m = pkg.LinearModel(34, 51, linear_size=H, num_stage=S, p_dropout=0.5).to(DEV).train()
    m.manual_seed(3)
    opt = pkg.FlatAdamW(m, lr=hp_a[0], betas=hp_a[1:3], eps=hp_a[3], weight_decay=hp_a[4])
    opt._bind()
    assert m.step_carries_adamw(B)
    real = _real_slots(m)
    for k, hp in enumerate((hp_a, hp_b), 1):
        _set_hp(opt, *hp)
        x, y = pkg.synth.synthetic_batch(B, 40 + k, DEV)
        before = tuple(_n(a).copy() for a in (m.flat_params, opt._m, opt._v))
        loss, _ = pkg.train_step(m, opt, x, y)
        assert torch.isfinite(loss)
        after = tuple(_n(a) for a in (m.flat_params, opt._m, opt._v))
        g = _n(m.flat_grads)
        assert np.abs(g[real]).max() > 0
        _hold(f"ride B={B} H={H} S={S} step {k}", before, after, g, hp + (1.0,), k, mask=real)
    assert float(opt.state_dict()["state"][0]["step"]) == 2


# ------------------------------------------------------------------------------------------------ d. graph replays
CAPTURED = (1e-3, 0.5, 0.9, 1e-3, 0.3)
CHANGES = [("weight_decay", 0.05), ("betas", (0.8, 0.95)), ("eps", 1e-6)]


def _replays_then_changes(pkg, tag, opt, replay, state, grads, t_now, mask=None):
    """Four replays held to the bounds at t0 + k; then weight_decay, betas, eps change in param_groups one after the other, and
    the next call must FOLLOW (the step with the new value, inside the bounds) or REFUSE (PoseliftError, nothing written; the
    value is then put back and the replay after it is held again) -- never use the captured value in silence; then a float lr
    changes and must be followed."""
    def held(what):
        before = tuple(_n(a).copy() for a in state())
        t = t_now() + 1
        replay()
        torch.cuda.synchronize()
        _hold(f"{tag} {what} (t = {t})", before, tuple(_n(a) for a in state()), _n(grads()), _hp_of(opt), t, mask=mask)

    for k in range(1, 5):
        held(f"replay {k}")
    g = opt.param_groups[0]
    outcome = {}
    for name, new in CHANGES:
        old = g[name]
        g[name] = new
        before = tuple(_n(a).copy() for a in state())
        t = t_now() + 1
        try:
            replay()
        except pkg.PoseliftError as e:
            assert "capture a new one" in str(e), str(e)
            torch.cuda.synchronize()
            for a, b in zip(before, state()):
                assert np.array_equal(a, _n(b)), f"{tag}: a refused replay wrote the state"
            assert t_now() + 1 == t
            g[name] = old
            outcome[name] = "refused"
            held(f"after the refused {name}")
        else:
            torch.cuda.synchronize()
            outcome[name] = "followed"
            _hold(f"{tag} new {name} (t = {t})", before, tuple(_n(a) for a in state()), _n(grads()), _hp_of(opt), t, mask=mask)
    print(f"    {tag}: {outcome}")
    g["lr"] = 7e-3
    held("new lr")
    return outcome


# (B = 64, H = 256 is the smallest fp32 step that carries AdamW in the call: the hidden layers' one-launch kernels need H to
# be a multiple of 256.  At H = 128 the same batch takes the separate launch, in fp32.)
@pytest.mark.parametrize("B,H,dtype,in_call", [(64, 256, "fp32", True), (64, 128, "fp32", False), (256, 256, "f16x3", False)])
def test_graphed_train_step_holds_every_replay_and_follows_or_refuses_hyper_parameter_changes(pkg, B, H, dtype, in_call):
    """Both routes of the captured step: AdamW inside the call's backward launches (PLAdamWStep baked into the graph) and the
    separate AdamW launch behind fwd + bwd."""
    torch.manual_seed(0)
    m = pkg.LinearModel(34, 51, linear_size=H, p_dropout=0.5, compute_dtype=dtype).to(DEV).train()
    m.manual_seed(3)
    opt = pkg.FlatAdamW(m, lr=CAPTURED[0], betas=CAPTURED[1:3], eps=CAPTURED[3], weight_decay=CAPTURED[4])
    x, y = pkg.synth.synthetic_batch(B, 40, DEV)
    step = pkg.GraphedTrainStep(m, opt, x, y)
    assert step._in_call == in_call == m.step_carries_adamw(B)
    _replays_then_changes(pkg, f"GraphedTrainStep B={B} H={H} {dtype}", opt, lambda: step(x, y),
                          lambda: (m.flat_params, opt._m, opt._v), lambda: m.flat_grads, lambda: opt._t, mask=_real_slots(m))
    assert float(opt.state_dict()["state"][0]["step"]) == opt._t


def test_graphed_module_step_with_flat_adam_holds_every_replay_and_follows_or_refuses(pkg):
    mod = _tiny(14).train()
    opt = pkg.FlatAdam(mod, lr=CAPTURED[0], betas=CAPTURED[1:3], eps=CAPTURED[3], weight_decay=CAPTURED[4],
                       decoupled_weight_decay=True, capturable=True)
    g0 = torch.Generator().manual_seed(21)
    x, t = torch.randn(6, 7, generator=g0).to(DEV), torch.randn(6, 3, generator=g0).to(DEV)
    step = pkg.GraphedModuleStep(mod, opt, torch.nn.functional.mse_loss, x, t)
    _replays_then_changes(pkg, "GraphedModuleStep FlatAdam", opt, lambda: step(x, t),
                          lambda: (opt.arena.flat, opt._m, opt._v), lambda: opt.arena.grad, lambda: int(opt._t_dev.item()))


# ------------------------------------------------------------------------------------------------ e. a loaded state at step 10^6
def _stock_state_at(ref, params, t):
    """ref's state_dict() after one stock step on random gradients, with every 'step' set to t."""
    g0 = torch.Generator().manual_seed(31)
    for p in params:
        p.grad = (torch.randn(p.shape, generator=g0) * 1e-2).to(DEV)
    ref.step()
    sd = ref.state_dict()
    for st in sd["state"].values():
        st["step"] = torch.full_like(st["step"], float(t))
    for p in params:
        p.grad = None
    return sd


def test_flat_adamw_from_a_stock_adamw_state_at_a_million_steps(pkg):
    torch.manual_seed(7)
    m = pkg.LinearModel(34, 51, linear_size=64, num_stage=1, p_dropout=0.0).to(DEV).train()
    kw = dict(lr=1e-3, betas=(0.9, 0.99999), eps=1e-8, weight_decay=0.01)
    sd = _stock_state_at(torch.optim.AdamW(m.parameters(), **kw), list(m.parameters()), 10 ** 6)
    opt = pkg.FlatAdamW(m, **kw)
    opt.load_state_dict(sd)
    n = m.flat_params.numel()
    g = _grad_values(n, 50)
    m.flat_grads.copy_(torch.from_numpy(g))
    before = tuple(_n(a).copy() for a in (m.flat_params, opt._m, opt._v))
    real = _real_slots(m)
    assert np.abs(before[1][real]).max() > 0 and before[2][real].max() > 0
    opt.step()
    after = tuple(_n(a) for a in (m.flat_params, opt._m, opt._v))
    _hold("FlatAdamW at t = 10^6 + 1", before, after, g, _hp_of(opt), 10 ** 6 + 1, mask=real)
    assert float(opt.state_dict()["state"][0]["step"]) == 10 ** 6 + 1


@pytest.mark.parametrize("capturable", [False, True], ids=["plain", "capturable"])
def test_flat_adam_from_a_stock_adam_state_at_a_million_steps(pkg, capturable):
    mod = _tiny(15)
    kw = dict(lr=1e-3, betas=(0.9, 0.99999), eps=1e-8, capturable=capturable)
    opt = pkg.FlatAdam(mod, **kw)                          # (first: it moves the parameters into its arena)
    sd = _stock_state_at(torch.optim.Adam(mod.parameters(), **kw), list(mod.parameters()), 10 ** 6)
    opt.load_state_dict(sd)
    n = opt.arena.numel
    g = _grad_values(n, 51)
    pad = np.ones(n, bool)
    for p, o in zip(opt.arena.params, opt.arena.offsets):
        pad[o:o + p.numel()] = False
    g[pad] = 0.0
    _arena_grads(opt, g)
    before = tuple(_n(a).copy() for a in (opt.arena.flat, opt._m, opt._v))
    assert np.abs(before[1]).max() > 0 and before[2].max() > 0
    opt.step()
    after = tuple(_n(a) for a in (opt.arena.flat, opt._m, opt._v))
    _hold(f"FlatAdam at t = 10^6 + 1 ({'capturable' if capturable else 'plain'})", before, after, g, _hp_of(opt), 10 ** 6 + 1)
    assert float(opt.state_dict()["state"][0]["step"]) == 10 ** 6 + 1
