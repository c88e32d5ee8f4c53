"""Resume protocol shared by tests/test_gpu_resume.py and tests/test_resume_host.py.  TEST INFRASTRUCTURE ONLY.

    train N steps, save, load into a FRESH model and a FRESH optimizer, train M more steps == N + M uninterrupted steps

written once: a Rig holds one model with its optimizer (and scheduler), knows how to take one step eagerly or through a
captured graph, what to record after a step, what goes into the checkpoint envelope and how a resuming script puts it back.
run() is the uninterrupted run, resume() the interrupted one; assert_same() compares two records with torch.equal -- the
kernels repeat bit for bit and a graph replays the eager step bit for bit (both asserted elsewhere in the suite), so a
difference of one ulp anywhere is a wrong step count, a wrong moment slot, a wrong dropout position or a stale weight plane.

Nothing here imports the package or touches a device at import time: the rigs take `pkg` (what __graft_entry__.build()
returns)."""
import gc

import numpy as np
import torch
import torch.nn.functional as F

DEV = "cuda:0"
LR, WD = 1e-3, 0.01


# ---------------------------------------------------------------------------------------------------- records
def assert_same(got, want, what=""):
    """Two records of one step: every tensor torch.equal, every number ==.  (A key that only one side recorded -- the
    output of a conv-path graph, which returns the loss alone -- is not compared.)"""
    keys = [k for k in want if k in got and got[k] is not None and want[k] is not None]
    assert {"loss", "params", "exp_avg", "exp_avg_sq", "bn", "step", "lr"} <= set(keys), (what, keys)
    for k in keys:
        a, b = got[k], want[k]
        if torch.is_tensor(b):
            assert torch.equal(a, b), (what, k)
        elif isinstance(b, list):
            assert len(a) == len(b), (what, k)
            for j, (u, v) in enumerate(zip(a, b)):
                assert torch.equal(u, v), (what, k, j)
        else:
            assert a == b, (what, k, a, b)


def differs(got, want):
    """Does any recorded tensor of the step differ (what a resume that left a piece out must show)."""
    try:
        assert_same(got, want)
    except AssertionError:
        return True
    return False


# ---------------------------------------------------------------------------------------------------- the lifter
class LifterCase:
    """LinearModel(34, 51, linear_size=H, num_stage=S, p_dropout=0.5) + FlatAdamW(lr=1e-3, weight_decay=0.01)."""

    def __init__(self, name, B, H, S, dtype="fp32", BN=True, frozen=False, clip=False, sched=False, bad=None, steps=6):
        self.name, self.B, self.H, self.S, self.dtype, self.BN = name, B, H, S, dtype, BN
        self.frozen, self.clip, self.sched, self.bad, self.steps = frozen, clip, sched, bad, steps
        self._batches = self._max_norm = None

    def batches(self, pkg):
        """A different batch for every step, drawn once; step `bad` (0-based) has one inf in its target."""
        if self._batches is None:
            out = []
            for i in range(self.steps):
                x, y = pkg.synth.synthetic_batch(self.B, 9000 + 17 * i + self.B, DEV)
                if i == self.bad:
                    y = y.clone()
                    y[5, 7, 2] = float("inf")
                out.append((x, y))
            self._batches = out
        return self._batches

    def max_norm(self, pkg):
        """Half the fp64 norm of the first step's gradient: every finite step of the case clips."""
        if self._max_norm is None:
            rig = LifterRig(pkg, self, fresh=False, clip_off=True)
            x, y = self.batches(pkg)[0]
            rig.m.fused_train_fwd_bwd(x.reshape(self.B, -1).contiguous(), y.reshape(self.B, -1).contiguous())
            g = rig.m.flat_grads.double()
            n2 = sum(float((g[s.offset:s.offset + s.numel] ** 2).sum()) for s in rig.m._slots)
            self._max_norm = 0.5 * float(np.sqrt(n2))
        return self._max_norm

    def rig(self, pkg, fresh):
        return LifterRig(pkg, self, fresh)


class LifterRig:
    def __init__(self, pkg, case, fresh, clip_off=False):
        self.pkg, self.case = pkg, case
        # a fresh model starts from OTHER weights and another dropout key: whatever the checkpoint does not bring shows
        torch.manual_seed(777 if fresh else 11)
        m = pkg.LinearModel(34, 51, linear_size=case.H, num_stage=case.S, p_dropout=0.5, BN=case.BN,
                            compute_dtype=case.dtype).to(DEV).train()
        if not fresh:
            m.manual_seed(0xC0FFEE12345, step=0)
        if case.frozen:
            m.w1.weight.requires_grad_(False)
        self.m, self.opt, self.sched, self.fresh = m, None, None, fresh
        self._clip = {}
        if case.clip and not clip_off:
            self._clip = dict(max_grad_norm=case.max_norm(pkg), skip_nonfinite=True)
        if not fresh:
            self.build_optimizer()

    def build_optimizer(self):
        self.opt = self.pkg.FlatAdamW(self.m, lr=LR, weight_decay=WD, **self._clip)
        if self.case.sched:
            self.sched = torch.optim.lr_scheduler.ReduceLROnPlateau(self.opt, factor=0.7, patience=1, cooldown=0)

    def envelope(self):
        env = {"epoch": 3, "batch_size": self.case.B, "model": self.m.state_dict(), "optimizer": self.opt.state_dict(),
               "dropout": self.m.dropout_state()}
        if self.sched is not None:
            env["scheduler"] = self.sched.state_dict()
        return env

    def load(self, ck, leave_out=()):
        """The resuming script: weights into the placed module, then the optimizer (and scheduler) on it and their states,
        then the dropout stream."""
        self.m.load_state_dict(ck["model"])
        self.build_optimizer()
        if "optimizer" not in leave_out:
            self.opt.load_state_dict(ck["optimizer"])
            if self.sched is not None:
                self.sched.load_state_dict(ck["scheduler"])
        if "dropout" not in leave_out:
            self.m.manual_seed(**ck["dropout"])

    def grapher(self, x, y):
        step = self.pkg.GraphedTrainStep(self.m, self.opt, x, y)
        return lambda a, b: step(a, b)

    def eager(self, x, y):
        return self.pkg.train_step(self.m, self.opt, x, y)

    def record(self, loss, y_hat):
        m, opt = self.m, self.opt
        sd = opt.state_dict()
        return dict(loss=loss.detach().clone(), y_hat=y_hat.detach().clone(), params=m.flat_params.clone(),
                    exp_avg=[opt.state[p]["exp_avg"].clone() for p in m._param_list],
                    exp_avg_sq=[opt.state[p]["exp_avg_sq"].clone() for p in m._param_list],
                    bn=[v.clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k],
                    step=float(sd["state"][0]["step"]))

    def after_step(self):
        if self.sched is not None:
            self.sched.step(1.0)                     # a metric that never improves

    def counters(self):
        return dict(skipped=self.opt.skipped_steps(), t=self.opt._t, dropout_step=self.m._step,
                    step=float(self.opt.state_dict()["state"][0]["step"]))


# ---------------------------------------------------------------------------------------------------- conv path and ViT
class ModuleCase:
    """kind "model3d": Model_3D(compute_dtype=mode) on 2 frames of 64 x 64 (the shape of
    test_graphed_module_step_replays_the_eager_step_bit_for_bit) + FlatAdam(lr=1e-3, capturable=...).
    kind "vit": MyViT(compute_dtype=mode) on 64 poses (test_weight_plane_caches_follow_flatadam_steps) +
    FlatAdam(lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True)."""

    def __init__(self, kind, mode, capturable=False, steps=6):
        self.kind, self.mode, self.capturable, self.steps = kind, mode, capturable, steps
        self.name = f"{kind}-{mode}-{'capturable' if capturable else 'host'}"
        self._batches = None

    def batches(self, pkg):
        if self._batches is None:
            if self.kind == "model3d":
                self._batches = [(pkg.synth.seeded_frames(2, 40 + i, 64).to(DEV),
                                  torch.randn(2, 51, generator=torch.Generator().manual_seed(50 + i)).to(DEV))
                                 for i in range(self.steps)]
            else:
                out = []
                for i in range(self.steps):
                    rng = np.random.default_rng(640 + i)
                    out.append((torch.as_tensor(rng.uniform(0.0, 1.0, (64, 17, 2)).astype(np.float32), device=DEV),
                                torch.as_tensor((0.2 * rng.standard_normal((64, 17, 3))).astype(np.float32), device=DEV)))
                self._batches = out
        return self._batches

    def rig(self, pkg, fresh):
        return ModuleRig(pkg, self, fresh)


class ModuleRig:
    def __init__(self, pkg, case, fresh):
        self.pkg, self.case, self.fresh = pkg, case, fresh
        if case.kind == "model3d":
            m = pkg.Model_3D(compute_dtype=case.mode).train()
            m.load_state_dict(pkg.synth.seeded_state(m.state_dict(), 77 if fresh else 31))
            with torch.no_grad():
                m.final_layer.weight.mul_(1e-3)
        else:
            torch.manual_seed(778 if fresh else 164)
            m = pkg.MyViT(compute_dtype=case.mode)
            with torch.no_grad():                                        # non-trivial LayerNorm affine parameters
                for name, p in m.named_parameters():
                    if "norm" in name:
                        p.add_(0.1 * torch.randn_like(p))
            m.train()
        self.m, self.opt, self.sched = m.to(DEV), None, None
        if not fresh:
            self.build_optimizer()

    def build_optimizer(self):
        """(on the module AFTER .to(device) and load_state_dict, as FlatAdam's arena demands)"""
        if self.case.kind == "model3d":
            self.opt = self.pkg.FlatAdam(self.m, lr=LR, capturable=self.case.capturable)
        else:
            self.opt = self.pkg.FlatAdam(self.m, lr=LR, weight_decay=WD, decoupled_weight_decay=True,
                                         capturable=self.case.capturable)

    def envelope(self):
        return {"epoch": 3, "batch_size": int(self.case.batches(self.pkg)[0][0].shape[0]), "model": self.m.state_dict(),
                "optimizer": self.opt.state_dict()}

    def load(self, ck, leave_out=()):
        self.m.load_state_dict(ck["model"])
        self.build_optimizer()
        if "optimizer" not in leave_out:
            self.opt.load_state_dict(ck["optimizer"])

    def grapher(self, x, y):
        step = self.pkg.GraphedModuleStep(self.m, self.opt, F.mse_loss, x, y)
        return lambda a, b: (step(a, b), None)

    def eager(self, x, y):
        if self.case.kind == "vit":
            return self.pkg.train_step(self.m, self.opt, x, y)
        self.opt.zero_grad(set_to_none=True)
        out = self.m(x)
        loss = F.mse_loss(out, y)
        loss.backward()
        self.opt.step()
        return loss.detach(), out.detach()

    def record(self, loss, y_hat):
        opt = self.opt
        a = opt.arena
        # the per-parameter state IS the arenas: one clone of each stands for all of them
        for p, o in zip(a.params, a.offsets):
            st = opt.state[p]
            assert st["exp_avg"].data_ptr() == opt._m.data_ptr() + 4 * o and st["step"] is opt._step_tensor
            assert st["exp_avg_sq"].data_ptr() == opt._v.data_ptr() + 4 * o and p.data_ptr() == a.flat.data_ptr() + 4 * o
        return dict(loss=loss.detach().clone(), y_hat=None if y_hat is None else y_hat.detach().clone(),
                    params=a.flat.clone(), exp_avg=opt._m.clone(), exp_avg_sq=opt._v.clone(),
                    bn=[b.detach().clone() for b in self.m.buffers()],
                    step=float(opt.state_dict()["state"][0]["step"]))

    def after_step(self):
        pass

    def counters(self):
        return dict(skipped=self.opt.skipped_steps(), step=float(self.opt.state_dict()["state"][0]["step"]))


# ---------------------------------------------------------------------------------------------------- the protocol
def _steps(rig, lo, hi, graphed, hook=None):
    """Steps lo .. hi-1 (0-based) of the case's batch list, eagerly or as replays of ONE graph captured here on batch lo.
    hook: an object with before(rig, i) -> pre and after(rig, i, pre, record), around every step."""
    batches = rig.case.batches(rig.pkg)
    do = rig.grapher(*batches[lo]) if graphed else rig.eager
    recs = []
    for i in range(lo, hi):
        lr = float(rig.opt.param_groups[0]["lr"])
        pre = hook.before(rig, i) if hook is not None else None
        loss, y_hat = do(*batches[i])
        rec = rig.record(loss, y_hat)
        rec["lr"] = lr
        if hook is not None:
            hook.after(rig, i, pre, rec)
        rig.after_step()
        recs.append(rec)
    return recs


def run(pkg, case, n_steps, graphed=False):
    """The uninterrupted run: (records of steps 1..n_steps, the rig's counters after the last)."""
    rig = case.rig(pkg, fresh=False)
    recs = _steps(rig, 0, n_steps, graphed)
    return recs, rig.counters()


def resume(pkg, case, N, M, tmp_path, first=False, second=False, leave_out=(), hook=None, on_saved=None, on_loaded=None):
    """N steps (graphed if `first`), torch.save of the envelope, every object dropped, torch.load(weights_only=True), a fresh
    model / optimizer / scheduler / graph, M steps (graphed if `second`) on batches N .. N+M-1.
    on_saved(rig, envelope) sees the first leg's rig as it saves, on_loaded(rig, ckpt) the fresh one before its first step;
    hook wraps the resumed steps.  Returns (records of steps N+1 .. N+M, the resumed rig's counters)."""
    rig = case.rig(pkg, fresh=False)
    _steps(rig, 0, N, first)
    env = rig.envelope()
    path = tmp_path / "ckpt.pt"
    torch.save(env, path)
    if on_saved is not None:
        on_saved(rig, env)
    del rig, env
    gc.collect()
    ck = torch.load(path, weights_only=True)
    assert set(ck) >= {"epoch", "batch_size", "model", "optimizer"}
    rig = case.rig(pkg, fresh=True)
    rig.load(ck, leave_out)
    if on_loaded is not None:
        on_loaded(rig, ck)
    recs = _steps(rig, N, N + M, second, hook)
    return recs, rig.counters()
