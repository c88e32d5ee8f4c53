"""Resumed training is bit for bit the uninterrupted run, on every step route (tests/resume_cases.py holds the protocol).

    run(case, N + M)       N + M steps on a fixed list of different batches
    resume(case, N, M)     N steps, torch.save of {'epoch','batch_size','model','optimizer','dropout'[,'scheduler']}, every
                           object dropped, torch.load(weights_only=True), a FRESH model (other weights, other dropout key), a
                           fresh optimizer / scheduler / graph, the states loaded in a resuming script's order, M steps

Steps N+1 .. N+M must be torch.equal in everything recorded: loss, output, the parameter arena, exp_avg / exp_avg_sq of
every parameter, the BatchNorm buffers, the saved 'step', the learning rate.  What that walks: AdamW's step count on its four
routes to the kernels (by value, inside the small-batch backward launches, t_base + *t_dev in a graph, t - skipped behind
the clip record), the moment arenas rebuilt from per-parameter tensors, the Philox dropout position (not in state_dict():
LinearModel.dropout_state() / manual_seed), the persistent weight planes of f16x3 / bf16, graphs captured on a just-loaded
optimizer, and the scheduled learning rate.  No tolerance anywhere in that comparison.

Two equal wrong answers would pass it, so the resumed leg is also held to an independent reference: every resumed AdamW
step of the fp32 lifter cases against oracle.lifter_oracle.adamw_step on the device's own pre-step state and gradient with
t = taken steps + 1 (rtol 1e-5 / atol 1e-7, the bound of test_reduce_lr_on_plateau_drives_the_flat_optimizer), the gradient
of the first resumed step against the numpy oracle under that step number's Philox masks (relative L2 2e-4, as
test_small_batch_layer_kernels_dropout_modes_vs_oracle), and the first resumed FlatAdam step of the conv path and the ViT
against the stock torch optimizer loaded from the same file (<= 1e-3 lr per element, as
test_flat_adam_three_steps_of_model3d_vs_torch_adam -- one step only, for the reason given there).
And the comparison can fail: a resume without manual_seed, and one without optimizer.load_state_dict, differ at step N+1."""
import numpy as np
import pytest
import torch

import grad_clip_oracle as gco
import resume_cases as rc
from oracle import lifter_oracle as orc
from oracle import philox
from resume_cases import DEV, LR, WD

pytestmark = pytest.mark.gpu
N, M = 3, 3
NORM_TOL = 2.0 ** -22                  # tests/test_gpu_grad_clip.py: the fp64 sum, the sqrt and one rounding to fp32, four times


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


# Case 1 is here for the step whose AdamW rides in the backward launches.  That route needs the column-owning layer kernels
# (csrc/small_layer.hip: B <= 64 and H a multiple of 256), so its smallest shape is H = 256; at H = 128 a batch of 64 takes
# the small-batch BatchNorm launches with a separate AdamW launch -- kept as a case of its own (C1N).
C1 = rc.LifterCase("B64-H256-S1-fp32", 64, 256, 1)                           # AdamW rides in the backward launches
C1N = rc.LifterCase("B64-H128-S1-fp32", 64, 128, 1)                          # B = 64 without the ride
C2 = rc.LifterCase("B96-H128-S1-fp32", 96, 128, 1)                           # one separate AdamW launch
C3 = {dt: rc.LifterCase(f"B256-H256-S2-{dt}", 256, 256, 2, dtype=dt) for dt in ("f16x3", "bf16")}   # persistent weight planes
C5 = rc.LifterCase("B96-clip-skip", 96, 128, 1, clip=True, bad=1)            # step 2 of N is not taken
C6 = rc.LifterCase("B64-plateau", 64, 256, 1, sched=True)
C7 = rc.LifterCase("B64-noBN", 64, 256, 1, BN=False)
C8 = rc.LifterCase("B64-frozen-w1", 64, 256, 1, frozen=True)

_REF = {}


def _ref(pkg, case, n=None):
    """The EAGER uninterrupted run of a case, computed once and shared (never modified)."""
    if case.name not in _REF:
        _REF[case.name] = rc.run(pkg, case, case.steps)
    recs, counters = _REF[case.name]
    return (recs if n is None else recs[:n]), counters


def _assert_resumed(recs, ref, n=N, m=M, what=""):
    assert len(recs) == m
    for j, rec in enumerate(recs):
        rc.assert_same(rec, ref[n + j], f"{what} step {n + j + 1}")


def _close(a, b, rtol, atol):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


# ---------------------------------------------------------------------------------------------------- independent references
class AdamWOracle:
    """Around every resumed step of a lifter rig: oracle.lifter_oracle.adamw_step on the device's own pre-step parameters,
    moments and gradient, with t = (taken steps before the step) + 1 and the rate the step was scheduled to use.  With
    clipping, the gradient is multiplied by the device's coefficient, itself checked against the fp64 norm of the device
    gradient.  The ride-along step writes the parameters in the call that computes the gradient: the state is cloned
    before the step, the gradient read from the arena after it."""

    def __init__(self, with_gradient_of=None):
        self.with_gradient_of, self.checked = with_gradient_of, 0

    def before(self, rig, i):
        m, opt = rig.m, rig.opt
        named = list(m.named_parameters())
        pre = dict(p={k: p.detach().cpu().numpy().copy() for k, p in named},
                   m={k: opt.state[p]["exp_avg"].cpu().numpy().copy() for k, p in named},
                   v={k: opt.state[p]["exp_avg_sq"].cpu().numpy().copy() for k, p in named},
                   taken=float(opt.state_dict()["state"][0]["step"]))
        if i == self.with_gradient_of:
            pre["st"] = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
            pre["dropout"] = m.dropout_state()
        return pre

    def after(self, rig, i, pre, rec):
        m, opt, case = rig.m, rig.opt, rig.case
        coef = np.float32(1.0)
        if case.clip:
            g_all = m.flat_grads.cpu().numpy()
            norm = gco.grad_norm(g_all, [(s.offset, s.offset + s.numel) for s in m._slots])
            got_norm, coef = float(opt.grad_norm), np.float32(float(opt.clip_coef))
            assert abs(got_norm - float(norm)) <= NORM_TOL * float(norm), (i, got_norm, norm)
            assert coef == gco.clip_coef(np.float32(got_norm), case.max_norm(rig.pkg)) and coef < 1.0, (i, coef)
        assert rec["step"] == pre["taken"] + 1
        for k, p in m.named_parameters():
            g = p.grad.cpu().numpy() * coef
            want, wm, wv = orc.adamw_step(pre["p"][k], g, pre["m"][k], pre["v"][k], int(pre["taken"]) + 1, lr=rec["lr"], wd=WD)
            _close(p.detach().cpu().numpy(), want, 1e-5, 1e-7)
            _close(opt.state[p]["exp_avg"].cpu().numpy(), wm, 1e-5, 1e-7)
        if "st" in pre:
            self._gradient(rig, i, pre)
        self.checked += 1

    def _gradient(self, rig, i, pre):
        """The gradient of this step against the numpy oracle: the Philox masks of the step number the stream must be at
        (the loaded position + 1), the device's own ReLU decisions forced (a pre-activation within round-off of zero may
        fall either way; those must be few and tiny)."""
        m, case, pkg = rig.m, rig.case, rig.pkg
        B, H, L = case.B, case.H, 1 + 2 * case.S
        assert pre["dropout"]["step"] == i and m.dropout_state() == {"seed": pre["dropout"]["seed"], "step": i + 1}
        x, y = case.batches(pkg)[i]
        masks = [philox.dropout_keep_mask(pre["dropout"]["seed"], i + 1, l, B, H, 0.5) for l in range(L)]
        ws = m.last_workspace
        on = [pkg.layout.unpack_bitmap(m.workspace_view(ws, 2, l).cpu().numpy().view(np.uint64), H) for l in range(L)]
        opred, cache = orc.forward(pre["st"], x.cpu().numpy(), num_stage=case.S, train=True, p_dropout=0.5, keep_masks=masks,
                                   on_masks=on)
        for c in cache["layers"]:
            d = c["on_disagree"]
            assert d.size <= 1e-4 * c["z"].size + 2 and (d.size == 0 or d.max() < 1e-4), (d.size, d.max() if d.size else 0)
        _, dpred = orc.mse_loss(opred, y.cpu().numpy().reshape(B, -1))
        ograds, _ = orc.backward(pre["st"], cache, dpred)
        got = {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}
        for k, v in ograds.items():
            if k.endswith(".bias") and "batch_norm" not in k and k != "w2.bias":
                continue      # a Linear bias in front of BatchNorm: the true gradient is 0, both sides are round-off
            rel = np.linalg.norm((got[k] - v).astype(np.float64)) / (np.linalg.norm(v.astype(np.float64)) + 1e-30)
            print(f"{case.name} step {i + 1} grad {k}: rel L2 {rel:.3g}")
            assert rel < 2e-4, (k, rel)


class StockOptimizer:
    """Around the FIRST resumed FlatAdam step: torch.optim.Adam / AdamW on copies of the pre-step parameters, loaded from the
    same checkpoint, given the device's gradients."""

    def __init__(self, ck_holder, first):
        self.ck, self.first, self.checked = ck_holder, first, 0

    def before(self, rig, i):
        return [p.detach().clone() for p in rig.opt.arena.params] if i == self.first else None

    def after(self, rig, i, pre, rec):
        if pre is None:
            return
        params = rig.opt.arena.params
        twins = [q.requires_grad_(p.requires_grad) for p, q in zip(params, pre)]
        sd, g = self.ck["optimizer"], rig.opt.param_groups[0]
        decoupled = bool(g.get("decoupled_weight_decay", False))
        stock = (torch.optim.AdamW(twins, lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"]) if decoupled
                 else torch.optim.Adam(twins, lr=g["lr"], betas=g["betas"], eps=g["eps"]))
        # the checkpoint's state under the stock optimizer's own options; 'step' as the host float a stock state holds
        state = {k: {"step": torch.tensor(float(s["step"])), "exp_avg": s["exp_avg"], "exp_avg_sq": s["exp_avg_sq"]}
                 for k, s in sd["state"].items()}
        groups = stock.state_dict()["param_groups"]
        assert groups[0]["params"] == sd["param_groups"][0]["params"] and g["lr"] == sd["param_groups"][0]["lr"]
        stock.load_state_dict({"state": state, "param_groups": groups})
        moved = 0
        for p, q in zip(params, twins):
            q.grad = None if p.grad is None else p.grad.detach().clone()
        stock.step()
        for k, (p, q) in enumerate(zip(params, twins)):
            d = float((p.detach() - q.detach()).abs().max())
            assert d <= 1e-3 * g["lr"], (k, d)
            moved += int(p.grad is not None)
        assert moved > 0 and max(float(s["step"]) for s in stock.state_dict()["state"].values()) == rec["step"]
        self.checked += 1


# ---------------------------------------------------------------------------------------------------- the lifter, eager
def test_routes_of_the_lifter_cases(pkg):
    """Each case takes the route it is here for."""
    r1, r2, r3 = C1.rig(pkg, False), C2.rig(pkg, False), C3["f16x3"].rig(pkg, False)
    assert r1.m.step_carries_adamw(64) and r1.opt._step_struct(LR, None, 1, None) is not None
    assert not r2.m.step_carries_adamw(96) and not C1N.rig(pkg, False).m.step_carries_adamw(64)
    assert C6.rig(pkg, False).m.step_carries_adamw(64)
    for dt in C3:
        r = C3[dt].rig(pkg, False)
        assert not r.m.step_carries_adamw(256) and r.m._wplanes is not None and r.m.adamw_plane_segments() is not None
        r.eager(*C3[dt].batches(pkg)[0])
        assert r.m._wplanes_ver == r.m._planes_key()            # the AdamW launch left the persistent planes current
    assert r3.m._wplanes is not None and r1.m._wplanes is None
    r7, r8 = C7.rig(pkg, False), C8.rig(pkg, False)
    r7.opt._bind(), r8.opt._bind()
    assert len(r7.opt._active_ranges()) > 1 and r7.opt._step_struct(LR, None, 1, None) is None
    assert len(r8.opt._active_ranges()) == 1 and r8.opt._active_ranges()[0][0] > 0 and r8.opt._step_struct(LR, None, 1, None) is None
    assert C5.rig(pkg, False).opt._clipping()


@pytest.mark.parametrize("case", [C1, C2, C1N], ids=lambda c: c.name)
def test_lifter_resume_eager_with_oracle(pkg, tmp_path, case):
    """Cases 1 and 2 (and B = 64 at H = 128), with every resumed AdamW step against the oracle and (case 1) the first resumed
    gradient."""
    hook = AdamWOracle(with_gradient_of=N if case is C1 else None)
    recs, counters = rc.resume(pkg, case, N, M, tmp_path, hook=hook)
    ref, ref_counters = _ref(pkg, case)
    _assert_resumed(recs, ref, what=case.name)
    assert counters == ref_counters and hook.checked == M
    assert [r["step"] for r in recs] == [4.0, 5.0, 6.0]


@pytest.mark.parametrize("case", [C3["f16x3"], C3["bf16"], C7, C8], ids=lambda c: c.name)
def test_lifter_resume_eager(pkg, tmp_path, case):
    """Cases 3 (both plane types), 7 (BN=False: several AdamW runs) and 8 (one frozen tensor)."""
    seen = {}

    def on_loaded(rig, ck):
        seen["frozen"] = not rig.m.w1.weight.requires_grad
        seen["w1"] = rig.m.w1.weight.detach().clone()
        assert rig.m._slots[0].name == "w1.weight" and rig.m._slots[0].offset == 0

    recs, counters = rc.resume(pkg, case, N, M, tmp_path, on_loaded=on_loaded)
    ref, ref_counters = _ref(pkg, case)
    _assert_resumed(recs, ref, what=case.name)
    assert counters == ref_counters
    if case.frozen:                                            # the frozen tensor holds the loaded values, never stepped
        off, n = 0, seen["w1"].numel()
        assert seen["frozen"] and torch.equal(recs[-1]["params"][off:off + n].view_as(seen["w1"]), seen["w1"])
        assert not bool(recs[-1]["exp_avg"][0].any())


# ---------------------------------------------------------------------------------------------------- graphs across a resume
@pytest.mark.parametrize("first,second", [(True, True), (True, False), (False, True)],
                         ids=["graph-graph", "graph-eager", "eager-graph"])
@pytest.mark.parametrize("case", [C1, C3["f16x3"]], ids=lambda c: c.name)
def test_lifter_resume_through_graphs(pkg, tmp_path, case, first, second):
    """Case 4: GraphedTrainStep before and / or after the checkpoint, each mix equal to the EAGER uninterrupted run.  The
    graph after the resume is captured on the just-loaded optimizer: t0 = the loaded step, the dropout base the loaded
    position, its warm-up step on freshly bound moments."""
    recs, counters = rc.resume(pkg, case, N, M, tmp_path, first=first, second=second)
    ref, ref_counters = _ref(pkg, case)
    _assert_resumed(recs, ref, what=f"{case.name} {first}->{second}")
    assert counters == ref_counters == dict(skipped=0, t=N + M, dropout_step=N + M, step=float(N + M))


def test_a_graph_does_not_survive_load_state_dict(pkg):
    """The documented refusal: a GraphedTrainStep used across optimizer.load_state_dict raises; a new one resumes."""
    rig = C1.rig(pkg, False)
    b = C1.batches(pkg)
    step = pkg.GraphedTrainStep(rig.m, rig.opt, *b[0])
    step(*b[0])
    rig.opt.load_state_dict(rig.opt.state_dict())
    with pytest.raises(pkg.PoseliftError, match="capture a new"):
        step(*b[1])
    loss, _ = pkg.GraphedTrainStep(rig.m, rig.opt, *b[1])(*b[1])
    assert torch.equal(loss, _ref(pkg, C1)[0][1]["loss"])


# ---------------------------------------------------------------------------------------------------- clip + skip
@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph"])
def test_lifter_resume_behind_a_skipped_step(pkg, tmp_path, graphed):
    """Case 5: max_grad_norm = half the first gradient's norm (every step clips), skip_nonfinite, and step 2 of N has an inf
    in its target.  The checkpoint says N-1 taken steps; the loaded optimizer starts its skipped count at 0; the kernels of
    the resumed leg form t - skipped on the device and must arrive at the t of the uninterrupted run (attempted N+j, skipped
    1).  Eager: every resumed step also against the oracle with the clipped gradient."""
    saved = {}

    def on_saved(rig, env):
        saved.update(step=float(env["optimizer"]["state"][0]["step"]), skipped=rig.opt.skipped_steps(), t=rig.opt._t)

    def on_loaded(rig, ck):
        saved.update(loaded_skipped=rig.opt.skipped_steps(), loaded_t=rig.opt._t,
                     group=(rig.opt.param_groups[0]["max_grad_norm"], rig.opt.param_groups[0]["skip_nonfinite"]))

    hook = None if graphed else AdamWOracle()
    recs, counters = rc.resume(pkg, C5, N, M, tmp_path, first=graphed, second=graphed, hook=hook, on_saved=on_saved,
                               on_loaded=on_loaded)
    assert saved == dict(step=float(N - 1), skipped=1, t=N, loaded_skipped=0, loaded_t=N - 1,
                         group=(C5.max_norm(pkg), True))
    ref, ref_counters = _ref(pkg, C5)
    assert not torch.isfinite(ref[1]["loss"]) and torch.equal(ref[1]["params"], ref[0]["params"])   # the step was skipped
    _assert_resumed(recs, ref, what=f"{C5.name} graphed={graphed}")
    assert ref_counters == dict(skipped=1, t=N + M, dropout_step=N + M, step=float(N + M - 1))
    assert counters == dict(skipped=0, t=N + M - 1, dropout_step=N + M, step=float(N + M - 1))
    assert hook is None or hook.checked == M


# ---------------------------------------------------------------------------------------------------- scheduled rate
@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph"])
def test_lifter_resume_with_reduce_lr_on_plateau(pkg, tmp_path, graphed):
    """Case 6: ReduceLROnPlateau(factor .7, patience 1) stepped every training step with a metric that never improves: the
    rate drops after steps 3 and 5 -- once inside N (the first resumed step must already use the lower rate: it comes back in
    param_groups, the scheduler's counters in its own state) and once inside M.  A graph reads the rate from its device
    scalar."""
    hook = None if graphed else AdamWOracle()
    recs, counters = rc.resume(pkg, C6, N, M, tmp_path, first=graphed, second=graphed, hook=hook)
    ref, ref_counters = _ref(pkg, C6)
    want = [LR, LR, LR, LR * 0.7, LR * 0.7, LR * 0.7 * 0.7]
    assert [r["lr"] for r in ref] == want and [r["lr"] for r in recs] == want[N:]
    _assert_resumed(recs, ref, what=f"{C6.name} graphed={graphed}")
    assert counters == ref_counters
    # and the rate matters at this shape: the same steps at a constant rate end elsewhere
    assert not torch.equal(ref[N]["params"], _ref(pkg, C1)[0][N]["params"])


# ---------------------------------------------------------------------------------------------------- it can fail
def test_resume_without_manual_seed_differs(pkg, tmp_path):
    recs, _ = rc.resume(pkg, C1, N, 1, tmp_path, leave_out=("dropout",))
    ref = _ref(pkg, C1)[0][N]
    assert rc.differs(recs[0], ref) and not torch.equal(recs[0]["y_hat"], ref["y_hat"])
    assert recs[0]["step"] == ref["step"]                      # (the optimizer was loaded: only the masks are others)


def test_resume_without_optimizer_state_differs(pkg, tmp_path):
    recs, _ = rc.resume(pkg, C2, N, 1, tmp_path, leave_out=("optimizer",))
    ref = _ref(pkg, C2)[0][N]
    assert torch.equal(recs[0]["loss"], ref["loss"]) and torch.equal(recs[0]["y_hat"], ref["y_hat"])   # same forward ...
    assert not torch.equal(recs[0]["params"], ref["params"]) and recs[0]["step"] == 1.0                # ... another update


@pytest.mark.parametrize("dt", ["f16x3", "bf16"])
def test_first_forward_after_load_runs_on_rebuilt_weight_planes(pkg, tmp_path, dt):
    """Case 3: after the load and before the first resumed step, the fresh model's forward equals that of a model of the same
    arithmetic loaded from the same file on which no optimizer ever ran (its planes can only come from the loaded
    parameters) -- and differs from the fresh model's forward before the load.  The resumed steps behind that forward are
    still the uninterrupted run's."""
    case = C3[dt]
    x = case.batches(pkg)[N][0]
    out = {}

    def fwd(m):
        m.eval()
        with torch.no_grad():
            y = m(x).clone()
        m.train()
        return y

    def on_loaded(rig, ck):
        out["resumed"] = fwd(rig.m)
        assert rig.m._wplanes_ver == rig.m._planes_key()
        other = pkg.LinearModel(34, 51, linear_size=case.H, num_stage=case.S, p_dropout=0.5, compute_dtype=dt).to(DEV)
        out["unloaded"] = fwd(other)
        other.load_state_dict(ck["model"])
        out["other"] = fwd(other)

    recs, _ = rc.resume(pkg, case, N, M, tmp_path, on_loaded=on_loaded)
    assert torch.equal(out["resumed"], out["other"]) and not torch.equal(out["unloaded"], out["other"])
    _assert_resumed(recs, _ref(pkg, case)[0], what=case.name)


# ---------------------------------------------------------------------------------------------------- conv path
_MODEL3D = {(dt, cap): rc.ModuleCase("model3d", dt, capturable=cap) for dt in ("f16x3", "bf16p") for cap in (False, True)}


@pytest.mark.parametrize("how", ["host-eager", "capturable-eager", "capturable-graph-graph", "capturable-graph-eager"])
@pytest.mark.parametrize("dt", ["f16x3", "bf16p"])
def test_model3d_flat_adam_resume(pkg, tmp_path, dt, how):
    """Case 9: Model_3D + arena.FlatAdam, the step count on the host or (capturable) on the device, where the loaded count is
    what the kernel adds 1 to; inside GraphedModuleStep the graph is captured on the loaded state.  Eager legs: the first
    resumed step against torch.optim.Adam loaded from the same file."""
    cap = how != "host-eager"
    case = _MODEL3D[(dt, cap)]
    n, m = (3, 3) if how.endswith("-eager") and "graph" not in how else (2, 2)
    first, second = "graph-" in how, how.endswith("graph-graph")
    holder = {}
    hook = None if second else StockOptimizer(holder, first=n)
    recs, counters = rc.resume(pkg, case, n, m, tmp_path, first=first, second=second, hook=hook,
                               on_loaded=lambda rig, ck: holder.update(ck))
    ref, _ = _ref(pkg, case)
    _assert_resumed(recs, ref, n, m, what=f"{case.name} {how}")
    assert counters == dict(skipped=0, step=float(n + m)) and (hook is None or hook.checked == 1)


# ---------------------------------------------------------------------------------------------------- ViT
@pytest.mark.parametrize("mode", ["fp32", "f16x3", "bf16p"])
def test_vit_flat_adam_resume(pkg, tmp_path, mode):
    """Case 10: MyViT + FlatAdam (decoupled weight decay) through pkg.train_step; the weight-plane caches of the block
    Linears are rebuilt from the loaded parameters.  The first resumed step against torch.optim.AdamW from the same file."""
    case = rc.ModuleCase("vit", mode)
    holder = {}
    hook = StockOptimizer(holder, first=N)
    recs, counters = rc.resume(pkg, case, N, M, tmp_path, hook=hook, on_loaded=lambda rig, ck: holder.update(ck))
    ref, _ = rc.run(pkg, case, N + M)
    _assert_resumed(recs, ref, what=case.name)
    assert counters == dict(skipped=0, step=float(N + M)) and hook.checked == 1


# ---------------------------------------------------------------------------------------------------- the feeder's epoch
def test_pose_feeder_set_epoch_equals_having_iterated_the_epochs_before(pkg):
    """The envelope stores 'epoch': a fresh PoseFeeder(seed=s) after set_epoch(e) yields the batches of one that iterated
    epochs 0 .. e-1 first."""
    rng = np.random.default_rng(3)
    x, y = rng.random((200, 17, 2)).astype(np.float32), rng.standard_normal((200, 17, 3)).astype(np.float32)
    old = pkg.PoseFeeder(x, y, 48, device=DEV, seed=5)
    for e in range(2):
        old.set_epoch(e)
        for _ in old:
            pass
    old.set_epoch(2)
    new = pkg.PoseFeeder(x, y, 48, device=DEV, seed=5)
    new.set_epoch(2)
    got, want = list(new), list(old)
    assert len(got) == len(want) == 5
    for (a, b), (c, d) in zip(got, want):
        assert torch.equal(a, c) and torch.equal(b, d)
