#!/usr/bin/env python
"""sha256 of everything the lifter's and the conv path's BatchNorm launches, the flat optimizers, the soft-argmax heads and
the GEMM launchers (every branch of their route tables) write, one line per (case, buffer):

    python tools/route_hashes.py > hashes.txt          (POSELIFT_LIB=... picks another build of the library)

The cases reach every Lin / Stats / Bwd route of plan() (csrc/api.hip) and every streaming / small-layer launcher at the
smallest shapes that do, through the Python package and the C ABI alone -- so the same script runs on two commits and the
two outputs can be compared line for line (a refactor of the launchers must not move a bit).  The whole workspace is
hashed too (zeroed before the case): saved pre-activations, bitmaps, statistics, operand planes, partials."""
import ctypes
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import importlib  # noqa: E402

pkg = importlib.import_module("3d_poseestimation_amd")
_lib = importlib.import_module("3d_poseestimation_amd._lib")
DEV = torch.device("cuda", 0)


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is None:
            h.update(b"none")
            continue
        t = t.detach()
        if t.dtype in (torch.float32, torch.int32):
            t = t.contiguous().view(torch.int32)
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def emit(case, **buffers):
    for k, v in buffers.items():
        print(f"{case}/{k} {sha(*v) if isinstance(v, (list, tuple)) else sha(v)}", flush=True)


# ------------------------------------------------------------------------------------------------ lifter
def make(B, H, S, dtype, p, i_dim=34, o_dim=51, bn=True):
    torch.manual_seed(1000 * S + H)
    m = pkg.LinearModel(i_dim, o_dim, linear_size=H, num_stage=S, p_dropout=p, BN=bn, compute_dtype=dtype).to(DEV).train()
    m.manual_seed(99, step=0)
    with torch.no_grad():                       # non-trivial BatchNorm parameters and running statistics
        g = torch.Generator().manual_seed(H + B)
        for name, t in m.state_dict().items():
            if "batch_norm" in name and "weight" in name:
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
            elif "batch_norm" in name and "bias" in name:
                t.copy_(torch.randn(t.shape, generator=g) * 0.1)
            elif "running_mean" in name:
                t.copy_(torch.randn(t.shape, generator=g) * 0.1)
            elif "running_var" in name:
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
    ws = m._acquire_workspace(B)                # the pool hands this buffer to the case's calls: zero what no launch writes
    ws["buf"].zero_()
    m._release_workspace(ws)
    g = torch.Generator().manual_seed(B)
    x = torch.rand(B, i_dim, generator=g).to(DEV)
    t = (torch.rand(B, o_dim, generator=g) - 0.5).to(DEV)
    return m, x, t


def state(m):
    return dict(params=m.flat_params, bn=[m._bn_running, m._bn_batches], ws=m.last_workspace["buf"])


def case_autograd(name, B, H, S, dtype, p, inject=False, **kw):
    """pl_lifter_fwd_train + pl_lifter_bwd (dx included)"""
    m, x, t = make(B, H, S, dtype, p, **kw)
    if inject:
        rng = np.random.default_rng(5)
        words = np.stack([pkg.layout.pack_keep_bitmap(rng.random((B, H)) < 0.5) for _ in range(1 + 2 * S)])
        m.debug_inject_keep(torch.from_numpy(words.view(np.int64)).to(DEV))
    x.requires_grad_(True)
    y = m(x)
    loss = pkg.mse_loss(y, t)
    loss.backward()
    torch.cuda.synchronize()
    emit(name, y=y, loss=loss, grads=m.flat_grads, dx=x.grad, **state(m))


def case_cut(name, B, H, S, dtype, p, cut):
    """pl_lifter_bwd_layers: the backward cut at one layer boundary"""
    m, x, t = make(B, H, S, dtype, p)
    ws = m._acquire_workspace(B)
    y = m._run_fwd_train(x, ws)
    gy = (y - t) / y.numel()
    grads, dx = m.flat_grads, torch.empty_like(x)
    L, n = _lib.lib(), 1 + 2 * S
    for hi, lo in ((n, cut), (cut - 1, 0)):
        rc = L.pl_lifter_bwd_layers(ctypes.byref(m._desc), x.data_ptr(), gy.data_ptr(), B, ws["buf"].data_ptr(), ws["bytes"],
                                    dx.data_ptr(), grads.data_ptr(), hi, lo, _lib.current_stream_ptr())
        _lib.check(rc, "pl_lifter_bwd_layers")
    torch.cuda.synchronize()
    emit(name, y=y, grads=grads, dx=dx, **state(m))


def case_step(name, B, H, S, dtype, p, graphed=False, steps=2, **kw):
    """pl_lifter_train_step / pl_lifter_train_fwd_bwd + AdamW, eager or replayed from a graph (step_dev != 0)"""
    m, x, t = make(B, H, S, dtype, p, **kw)
    opt = pkg.FlatAdamW(m, lr=1e-3)
    step = pkg.GraphedTrainStep(m, opt, x, t) if graphed else (lambda a, b: pkg.train_step(m, opt, a, b))
    out = []
    for _ in range(steps):
        loss, y = step(x, t)
        out += [loss.clone(), y.clone()]
    torch.cuda.synchronize()
    emit(name, loss_y=out, grads=m.flat_grads, moments=[opt._m, opt._v], **state(m))


def case_eval(name, B, H, S, dtype, grad=False, **kw):
    """pl_lifter_fwd_eval, or pl_lifter_fwd_eval_saved + pl_lifter_bwd_eval"""
    m, x, t = make(B, H, S, dtype, 0.5, **kw)
    m.eval()
    if not grad:
        with torch.no_grad():
            y = m(x)
        torch.cuda.synchronize()
        return emit(name, y=y, bn=[m._bn_running, m._bn_batches])
    x.requires_grad_(True)
    y = m(x)
    pkg.mse_loss(y, t).backward()
    torch.cuda.synchronize()
    emit(name, y=y, grads=m.flat_grads, dx=x.grad, **state(m))


def lifter_cases():
    # Stats InLayer / Bwd SmallLayerDw + InAbove, top_fused, the AdamW ride (B <= 64, H % 256 == 0)
    for dt in ("fp32", "f16x3"):
        case_autograd(f"small-layer/{dt}/B64/p0", 64, 256, 2, dt, 0.0)
        case_step(f"small-layer/{dt}/B64/p0.5/step", 64, 256, 2, dt, 0.5)
    case_autograd("small-layer/fp32/B4/p0.5/inject", 4, 256, 2, "fp32", 0.5, inject=True)
    case_autograd("small-layer/fp32/B4/p0.5", 4, 256, 2, "fp32", 0.5)
    case_step("small-layer/fp32/B64/p0.5/graph", 64, 256, 2, "fp32", 0.5, graphed=True, steps=3)
    case_cut("small-layer/fp32/B64/cut3", 64, 256, 2, "fp32", 0.5, 3)
    # Stats Small (bn_small_fwd / bn_small_bwd: H off the layer kernels' 256), 300 inputs / 70 outputs (row bitmap under tiles)
    case_autograd("bn-small/fp32/B64/H128/p0.5", 64, 128, 2, "fp32", 0.5)
    case_autograd("bn-small/bf16/B4/H128/inject", 4, 128, 1, "bf16", 0.5, inject=True)
    case_step("bn-small/fp32/B64/H128/graph", 64, 128, 2, "fp32", 0.5, graphed=True, steps=3)
    case_autograd("small-mixed/fp32/B32/in300-out70", 32, 256, 1, "fp32", 0.5, i_dim=300, o_dim=70)
    # F32Mid + InApply (ragged 100 rows), PlanesMid + InApply (128 / 256 rows), the thin GEMMs (bf16, ragged)
    for dt in ("fp32", "bf16x6", "f16x3", "bf16"):
        case_autograd(f"mid/{dt}/B100/p0.5", 100, 256, 2, dt, 0.5)
        case_autograd(f"tiles/{dt}/B256/p0", 256, 256, 2, dt, 0.0)
    case_autograd("tiles/f16x3/B128/p0.5/inject", 128, 256, 2, "f16x3", 0.5, inject=True)
    case_step("tiles/f16x3/B256/p0.5/step", 256, 256, 2, "f16x3", 0.5)
    case_step("tiles/f16x3/B256/p0.5/graph", 256, 256, 2, "f16x3", 0.5, graphed=True, steps=3)
    case_cut("tiles/f16x3/B256/cut2", 256, 256, 2, "f16x3", 0.5, 2)
    # Planes + Finalize + PlanesPair + the fused pass-1 epilogues (more than 4 groups), fp16 pairs and one bf16 plane
    for dt in ("f16x3", "bf16", "fp32"):
        case_autograd(f"planes/{dt}/B1024/p0.5", 1024, 256, 2, dt, 0.5)
    case_step("planes/f16x3/B1024/p0.5/step", 1024, 256, 2, "f16x3", 0.5)
    case_step("planes/f16x3/B1024/p0.5/graph", 1024, 256, 2, "f16x3", 0.5, graphed=True, steps=3)
    case_autograd("planes/f16x3/B1024/H1024/S1/p0", 1024, 1024, 1, "f16x3", 0.0)
    # no BatchNorm; generic dimensions (nothing specialised applies)
    case_autograd("nobn/fp32/B256/p0.5", 256, 128, 1, "fp32", 0.5, bn=False)
    case_autograd("generic/fp32/B100/H36", 100, 36, 0, "fp32", 0.5, i_dim=20, o_dim=7)
    # evaluation: the layer kernels (<= 512 rows), the folded GEMMs above; the saved-state forward with its backward
    for dt, B in (("fp32", 4), ("f16x3", 100), ("f16x3", 256), ("bf16", 1024), ("f16x3", 1024), ("fp32", 1024)):
        case_eval(f"eval/{dt}/B{B}", B, 256, 2, dt)
    for dt, B in (("fp32", 64), ("bf16x6", 100), ("f16x3", 256), ("f16x3", 1024)):
        case_eval(f"eval-grad/{dt}/B{B}", B, 256, 2, dt, grad=True)
    case_eval("eval/nobn/fp32/B256", 256, 128, 1, "fp32", bn=False)


# ------------------------------------------------------------------------------------------------ conv-path BatchNorm
def group_stats(z):
    """what a convolution's GEMM epilogue leaves: per 64-row group and column the sum and the M2 about the group mean"""
    rows, C = z.shape
    G = _lib.lib().pl_gemm_stat_groups(rows)
    st = torch.zeros(2, G, C, device=z.device)
    for g in range(G):
        blk = z[64 * g:64 * (g + 1)].double()
        st[0, g] = blk.sum(0).float()
        st[1, g] = ((blk - blk.mean(0)) ** 2).sum(0).float()
    return st


def case_conv_bn(name, rows, C, mode=0, join=False, gemm_stat=False, relu=1):
    L, s = _lib.lib(), _lib.current_stream_ptr()
    gen = torch.Generator().manual_seed(rows + C)
    z = torch.randn(rows, C, generator=gen).to(DEV)
    ident = torch.randn(rows, C, generator=gen).to(DEV) if join else None
    g = torch.randn(rows, C, generator=gen).to(DEV)
    g2 = torch.randn(rows, C, generator=gen).to(DEV)
    gamma, beta = (torch.rand(C, generator=gen) + 0.5).to(DEV), torch.randn(C, generator=gen).to(DEV)
    rm, rv, nb = torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV)
    y, yp = torch.zeros_like(z), torch.zeros_like(z)
    bits = torch.zeros(rows, 4 * ((C + 255) // 256), dtype=torch.int64, device=DEV)
    mean, rstd = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    scratch = torch.zeros(L.pl_bn_train_scratch_bytes(rows, C), dtype=torch.uint8, device=DEV)
    st = group_stats(z) if gemm_stat else None
    rc = L.pl_bn_train_fwd_ex(z.data_ptr(), rows, C, gamma.data_ptr(), beta.data_ptr(), 1e-5, 0.1, rm.data_ptr(), rv.data_ptr(),
                              nb.data_ptr(), relu, y.data_ptr(), bits.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                              scratch.data_ptr(), yp.data_ptr() if mode else None, mode, st.data_ptr() if gemm_stat else None,
                              ident.data_ptr() if join else None, s)
    _lib.check(rc, "pl_bn_train_fwd_ex")
    torch.cuda.synchronize()
    emit(name + "/fwd", y=y, planes=yp.view(torch.int32), bits=bits, stats=[mean, rstd], running=[rm, rv, nb])
    dx, dz, dzp = torch.zeros_like(z), torch.zeros_like(z), torch.zeros_like(z)
    dgam, dbet, dzs = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(2, device=DEV)
    scratch.zero_()
    tail = (dgam.data_ptr(), dbet.data_ptr(), scratch.data_ptr(), dzp.data_ptr() if mode else None, mode,
            dzs.data_ptr() if mode else None, s)
    if join and C >= 256:
        rc = L.pl_bn_join_bwd(g.data_ptr(), g2.data_ptr(), bits.data_ptr(), z.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                              gamma.data_ptr(), rows, C, dx.data_ptr(), dz.data_ptr(), *tail)
        _lib.check(rc, "pl_bn_join_bwd")
    else:
        rc = L.pl_bn_train_bwd_ex(g.data_ptr(), bits.data_ptr(), z.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                  gamma.data_ptr(), rows, C, dz.data_ptr(), *tail)
        _lib.check(rc, "pl_bn_train_bwd_ex")
    torch.cuda.synchronize()
    emit(name + "/bwd", dx=dx, dz=dz, planes=dzp.view(torch.int32), dscale=dzs, dparams=[dgam, dbet])


def conv_cases():
    F16, BF = _lib.PL_F16X3, _lib.PL_BF16
    for C in (64, 256):                          # 64: four column replicas
        case_conv_bn(f"conv-bn/C{C}/rows512", 512, C)
        case_conv_bn(f"conv-bn/C{C}/rows512/norelu", 512, C, relu=0)
        case_conv_bn(f"conv-bn/C{C}/rows512/gemm-stat", 512, C, gemm_stat=True)
        case_conv_bn(f"conv-bn/C{C}/rows512/f16x3", 512, C, mode=F16)
        case_conv_bn(f"conv-bn/C{C}/rows512/f16x3/gemm-stat", 512, C, mode=F16, gemm_stat=True)
    case_conv_bn("conv-bn/C256/rows512/bf16", 512, 256, mode=BF)
    case_conv_bn("conv-bn/C256/rows512/join", 512, 256, join=True)
    case_conv_bn("conv-bn/C256/rows512/join/f16x3", 512, 256, mode=F16, join=True)
    case_conv_bn("conv-bn/C64/rows512/join", 512, 64, join=True)
    case_conv_bn("conv-bn/C64/rows33792/gemm-stat", 33792, 64, gemm_stat=True)       # > 512 groups: bn_merge_groups
    case_conv_bn("conv-bn/C64/rows33792", 33792, 64)                                 # 256-row statistics groups


# ------------------------------------------------------------------------------------------------ the flat optimizers
def opt_state(m, opt):
    rec = opt._clip.record if opt._clip is not None else None
    return dict(params=m.flat_params, moments=[opt._m, opt._v], wplanes=m._wplanes, bn=[m._bn_running, m._bn_batches], clip=rec)


def case_opt(name, B, graphed=False, freeze=None, poison=None, steps=3, bn=True, **kw):
    """Three train steps of the 1024-wide f16x3 lifter (the AdamW launch writes its weight planes) with FlatAdamW(**kw);
    freeze: a parameter without a gradient (several runs, no planes); poison: the step whose target holds an inf."""
    m, x, t = make(B, 1024, 2, "f16x3", 0.5, bn=bn)
    if m._wplanes is not None:
        m._wplanes.zero_()                                # (not written yet: whatever no launch writes hashes as zero)
    if freeze:
        dict(m.named_parameters())[freeze].requires_grad_(False)
    opt = pkg.FlatAdamW(m, lr=1e-3, weight_decay=0.02, **kw)
    step = pkg.GraphedTrainStep(m, opt, x, t) if graphed else (lambda a, b: pkg.train_step(m, opt, a, b))
    losses = []
    for i in range(steps):
        tt = t.clone()
        if i == poison:
            tt[3, 7] = float("inf")
        losses.append(step(x, tt)[0].clone())
        if i == 1:
            opt.param_groups[0]["lr"] = 5e-4              # (a scheduler's change: the device scalar of a replay follows)
    torch.cuda.synchronize()
    emit(name, loss=losses, step=opt.state_dict()["state"][0]["step"].float(), **opt_state(m, opt))


def case_flat_adam(name, capturable=False, graphed=False, **kw):
    """arena.FlatAdam on a stock module (gradients arrive through gather_grads): all gradients, one parameter without,
    none at all (the counter still ticks), all again; graphed: three GraphedModuleStep replays."""
    torch.manual_seed(12)
    mod = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3)).to(DEV)
    x, t = torch.randn(6, 7, device=DEV), torch.randn(6, 3, device=DEV)
    opt = pkg.FlatAdam(mod, lr=1e-2, capturable=capturable, **kw)
    if graphed:
        step = pkg.GraphedModuleStep(mod, opt, torch.nn.functional.mse_loss, x, t)
        for i in range(3):
            step(x + i, t)
    else:
        for what in ("all", "missing", "none", "all"):
            opt.zero_grad()
            if what != "none":
                (mod(x) - t).pow(2).mean().backward()
            if what == "missing":
                mod[0].bias.grad = None
            opt.step()
    torch.cuda.synchronize()
    rec = opt._clip.record if opt._clip is not None else None
    emit(name, params=opt.arena.flat, moments=[opt._m, opt._v], clip=rec, step=opt.state_dict()["state"][0]["step"].float())


def optimizer_cases():
    CLIP = dict(max_grad_norm=0.05, skip_nonfinite=True)
    case_opt("opt/B256/planes", 256)                                    # a launch of its own, planes refreshed
    case_opt("opt/B256/planes/clip", 256, **CLIP)
    case_opt("opt/B64/in-call", 64)                                     # AdamW inside the backward launches + the remainder
    case_opt("opt/B64/clip", 64, **CLIP)                                # ... bypassed: norm pass + one launch
    case_opt("opt/B256/frozen", 256, freeze="w1.bias")
    case_opt("opt/B256/frozen/clip", 256, freeze="w1.bias", **CLIP)
    case_opt("opt/B256/nobn", 256, bn=False)
    case_opt("opt/B256/nobn/clip", 256, bn=False, **CLIP)
    case_opt("opt/B64/graph", 64, graphed=True)
    case_opt("opt/B64/graph/clip", 64, graphed=True, **CLIP)
    case_opt("opt/B256/graph", 256, graphed=True)
    case_opt("opt/B256/graph/clip", 256, graphed=True, **CLIP)
    case_opt("opt/B256/nonfinite-skip", 256, poison=1, **CLIP)
    case_opt("opt/B256/graph/nonfinite-skip", 256, graphed=True, poison=1, skip_nonfinite=True)
    for cap in (False, True):
        case_flat_adam(f"flat-adam/cap{int(cap)}", capturable=cap)
        case_flat_adam(f"flat-adam/cap{int(cap)}/clip", capturable=cap, **CLIP)
    case_flat_adam("flat-adam/graph", capturable=True, graphed=True)
    case_flat_adam("flat-adam/graph/clip", capturable=True, graphed=True, **CLIP)


# ------------------------------------------------------------------------------------------------ the soft-argmax heads
FILL = -7.0                                       # what no launch writes hashes as this


def heads_inputs(BJ, n, ncoord, centred, seed):
    """logits (BJ, n) with one -inf, targets with one at the map's edge and one NaN, upstream gradients of coords and sq"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(BJ, n, generator=g) * 3
    x[BJ - 1, n // 3] = float("-inf")
    t = torch.rand(BJ, ncoord, generator=g) * (1.6 if centred else 0.8) + (-0.8 if centred else 0.1)
    t[0] = 1.0                                    # mu = dim: the window hangs over the last index
    t[1, 0] = float("nan")
    gc, gs = torch.randn(BJ, ncoord, generator=g), torch.randn(BJ, generator=g)
    gs[0] = 0.0
    return [v.to(DEV) for v in (x, t, gc, gs)]


def hm_variants(centred):
    return (None, (0.5, "head"), (1.75, "reference" if centred else "head"))


def law_of(W, H, D, centred, centre):
    return (ctypes.c_float * 6)(*pkg.heatmap_law(W, H, D, centred, centre))


def full(*shape):
    return torch.full(shape, FILL, device=DEV)


def case_heads_nchw(BJ, D, H, W, ncoord, centred):
    L, s = _lib.lib(), _lib.current_stream_ptr()
    x, t, gc, gs = heads_inputs(BJ, D * H * W, ncoord, centred, 7 * D + W)
    for hm in hm_variants(centred):
        name = f"heads/abi/nchw/{BJ}x{D}x{H}x{W}/" + ("plain" if hm is None else f"hm-s{hm[0]}-{hm[1]}")
        coords, sq, stats, dl = full(BJ, ncoord), full(BJ), full(BJ, 5 if hm is None else 8), full(BJ, D * H * W)
        if hm is None:
            rc = L.pl_softargmax_fwd(x.data_ptr(), BJ, D, H, W, ncoord, centred, coords.data_ptr(), stats.data_ptr(), s)
            _lib.check(rc, "pl_softargmax_fwd")
            rc = L.pl_softargmax_bwd(x.data_ptr(), stats.data_ptr(), gc.data_ptr(), BJ, D, H, W, ncoord, centred, dl.data_ptr(), s)
            _lib.check(rc, "pl_softargmax_bwd")
        else:
            law = law_of(W, H, D, centred, hm[1])
            rc = L.pl_softargmax_hm_fwd(x.data_ptr(), t.data_ptr(), BJ, D, H, W, ncoord, centred, hm[0], law, coords.data_ptr(),
                                        sq.data_ptr(), stats.data_ptr(), s)
            _lib.check(rc, "pl_softargmax_hm_fwd")
            rc = L.pl_softargmax_hm_bwd(x.data_ptr(), t.data_ptr(), stats.data_ptr(), gc.data_ptr(), gs.data_ptr(), BJ, D, H, W,
                                        ncoord, centred, hm[0], law, dl.data_ptr(), s)
            _lib.check(rc, "pl_softargmax_hm_bwd")
        torch.cuda.synchronize()
        emit(name, stats=stats, coords=coords, sq=sq, dlogits=dl)


def case_heads_nhwc(B, H, W, J):
    L, s = _lib.lib(), _lib.current_stream_ptr()
    BJ, shape = B * J, (B, H, W, J * 64)
    x, t, gc, gs = heads_inputs(BJ, H * W * 64, 3, True, 11 * H + W)
    x = x.reshape(shape)                          # (the values' order does not matter: any layout of random logits)
    for hm in hm_variants(True):
        name = f"heads/abi/nhwc/{B}x{H}x{W}x{J}/" + ("plain" if hm is None else f"hm-s{hm[0]}-{hm[1]}")
        coords, sq, stats, scale = full(BJ, 3), full(BJ), full(BJ, 5 if hm is None else 8), full(2)
        law = None if hm is None else law_of(W, H, 64, True, hm[1])
        if hm is None:
            rc = L.pl_softargmax3d_nhwc_fwd(x.data_ptr(), B, J, H, W, coords.data_ptr(), stats.data_ptr(), s)
            _lib.check(rc, "pl_softargmax3d_nhwc_fwd")
            _lib.check(L.pl_softargmax_dl_scale(gc.data_ptr(), BJ, 3, scale.data_ptr(), s), "pl_softargmax_dl_scale")
        else:
            rc = L.pl_softargmax3d_nhwc_hm_fwd(x.data_ptr(), t.data_ptr(), B, J, H, W, hm[0], law, coords.data_ptr(),
                                               sq.data_ptr(), stats.data_ptr(), s)
            _lib.check(rc, "pl_softargmax3d_nhwc_hm_fwd")
            rc = L.pl_softargmax_hm_dl_scale(gc.data_ptr(), gs.data_ptr(), BJ, 3, scale.data_ptr(), s)
            _lib.check(rc, "pl_softargmax_hm_dl_scale")
        torch.cuda.synchronize()
        emit(name, stats=stats, coords=coords, sq=sq, scale=scale)
        forms = [("f32", True, False, 0), ("planes-bf16", False, True, 1), ("planes-f16x3", False, True, 3), ("both-f16x3", True, True, 3)]
        for form, want_f32, want_planes, mode in forms:
            dl, carrier = full(*shape), full(*shape)
            tail = (dl.data_ptr() if want_f32 else None, carrier.data_ptr() if want_planes else None, mode, scale.data_ptr(), s)
            if hm is None:
                rc = L.pl_softargmax3d_nhwc_bwd_ex(x.data_ptr(), stats.data_ptr(), gc.data_ptr(), B, J, H, W, *tail)
                _lib.check(rc, "pl_softargmax3d_nhwc_bwd_ex")
            else:
                rc = L.pl_softargmax3d_nhwc_hm_bwd_ex(x.data_ptr(), t.data_ptr(), stats.data_ptr(), gc.data_ptr(), gs.data_ptr(), B, J,
                                                      H, W, hm[0], law, *tail)
                _lib.check(rc, "pl_softargmax3d_nhwc_hm_bwd_ex")
            torch.cuda.synchronize()
            emit(f"{name}/bwd-{form}", dlogits=dl, planes=carrier.view(torch.int32))
        if hm is None:
            dl = full(*shape)
            rc = L.pl_softargmax3d_nhwc_bwd(x.data_ptr(), stats.data_ptr(), gc.data_ptr(), B, J, H, W, dl.data_ptr(), s)
            _lib.check(rc, "pl_softargmax3d_nhwc_bwd")
            torch.cuda.synchronize()
            emit(f"{name}/bwd-plain-entry", dlogits=dl)
    # the two scale kernels on a non-finite row
    gc[BJ - 1, 1] = float("inf")
    s1, s2 = full(2), full(2)
    _lib.check(L.pl_softargmax_dl_scale(gc.data_ptr(), BJ, 3, s1.data_ptr(), s), "pl_softargmax_dl_scale")
    _lib.check(L.pl_softargmax_hm_dl_scale(gc.data_ptr(), gs.data_ptr(), BJ, 3, s2.data_ptr(), s), "pl_softargmax_hm_dl_scale")
    torch.cuda.synchronize()
    emit(f"heads/abi/nhwc/{B}x{H}x{W}x{J}/scale-nonfinite", plain=s1, hm=s2)


def case_heads_public(name, x, J, fn, fn_hm, ncoord, centred, **kw):
    """coords, sq and x.grad of a public function and its _hm twin"""
    B = x.shape[0]
    _, t, gc, gs = heads_inputs(B * J, 1, ncoord, centred, 3 * J + ncoord)
    t, gc, gs = t.reshape(B, J * ncoord), gc.reshape(B, J * ncoord), gs.reshape(B, J)
    for hm in hm_variants(centred):
        xr = x.clone().requires_grad_(True)
        if hm is None:
            coords, sq = fn(xr, num_joints=J, **kw), None
            (coords * gc).sum().backward()
        else:
            coords, sq = fn_hm(xr, t, hm[0], hm[1], num_joints=J, **kw)
            ((coords * gc).sum() + (sq * gs).sum()).backward()
        torch.cuda.synchronize()
        emit(f"heads/public/{name}/" + ("plain" if hm is None else f"hm-s{hm[0]}-{hm[1]}"), coords=coords, sq=sq, dx=xr.grad)


def case_heads_model(dtype):
    """one Model_3D training step (the NHWC head behind the final convolution, with its plane link where the route has one)"""
    frames = pkg.synth.seeded_frames(2, 32).to(DEV)
    y = (torch.rand(2, 51, generator=torch.Generator().manual_seed(1)) * 1.6 - 0.8).to(DEV)
    for with_hm in (False, True):
        m = pkg.Model_3D(compute_dtype=dtype)
        m.load_state_dict(pkg.synth.seeded_state(m.state_dict(), 51))
        m = m.to(DEV).train()
        if with_hm:
            coords, sq = m(frames, heatmap_target=y)
            (((coords - y) ** 2).mean() + 1000 * pkg.heatmap_mse(sq, 64 * 64 * 64)).backward()
        else:
            coords, sq = m(frames), None
            ((coords - y) ** 2).mean().backward()
        torch.cuda.synchronize()
        emit(f"heads/model3d/{dtype}/" + ("hm" if with_hm else "plain"), coords=coords, sq=sq,
             final_grads=[m.final_layer.weight.grad, m.final_layer.bias.grad])


def heads_cases():
    # (BJ, D, H, W): one chunk; 16384 voxels = two chunks of the backward; a map smaller than the workgroup; the 2-D head
    for BJ, D, H, W, ncoord, centred in ((6, 8, 4, 8, 3, 1), (6, 16, 16, 64, 3, 1), (2, 1, 3, 4, 3, 1), (6, 1, 12, 16, 2, 0)):
        case_heads_nchw(BJ, D, H, W, ncoord, centred)
    for B, H, W, J in ((2, 3, 5, 3), (2, 8, 8, 3)):          # 15 pixels: a ragged last pass of the four wavefronts
        case_heads_nhwc(B, H, W, J)
    for BJ, D, H, W in ((4, 8, 4, 8), (4, 1, 12, 16)):
        ncoord = 3 if D > 1 else 2
        _, t, _, _ = heads_inputs(BJ, 1, ncoord, D > 1, 5)
        for sigma, centre in hm_variants(D > 1)[1:]:
            out = full(BJ, D, H, W)
            rc = _lib.lib().pl_heatmap_gaussian(t.data_ptr(), BJ, D, H, W, ncoord, sigma, law_of(W, H, D, D > 1, centre),
                                                out.data_ptr(), _lib.current_stream_ptr())
            _lib.check(rc, "pl_heatmap_gaussian")
            torch.cuda.synchronize()
            emit(f"heads/abi/gaussian/{BJ}x{D}x{H}x{W}/s{sigma}-{centre}", out=out)
    g = torch.Generator().manual_seed(77)
    for D, H, W in ((8, 4, 8), (16, 16, 64)):
        x = (torch.randn(2, 3 * D, H, W, generator=g) * 3).to(DEV)
        case_heads_public(f"3d/2x3x{D}x{H}x{W}", x, 3, pkg.soft_argmax_3d, pkg.soft_argmax_3d_hm, 3, True, depth_dim=D)
    x = (torch.randn(1, 2, 3, 4, generator=g) * 3).to(DEV)
    case_heads_public("3d/1x2x1x3x4", x, 2, pkg.soft_argmax_3d, pkg.soft_argmax_3d_hm, 3, True, depth_dim=1)
    x = (torch.randn(2, 3, 12, 16, generator=g) * 3).to(DEV)
    case_heads_public("2d/2x3x12x16", x, 3, pkg.soft_argmax_2d, pkg.soft_argmax_2d_hm, 2, False)
    for H, W in ((3, 5), (8, 8)):
        x = (torch.randn(2, H, W, 3 * 64, generator=g) * 3).to(DEV)
        x[1, H - 1, W - 1, 70] = float("-inf")
        case_heads_public(f"nhwc/2x{H}x{W}x3", x, 3, pkg.soft_argmax_3d_nhwc, pkg.soft_argmax_3d_nhwc_hm, 3, True)
    for dtype in ("f16x3", "bf16x6"):                         # the plane link; the fp32-grade direct route
        case_heads_model(dtype)


# ------------------------------------------------------------------------------------------------ GEMM launchers
def gemm_planes_case(name, layout, mode, M, N, K):
    """pl_gemm_planes (launch_gemm_planes behind two plane splits)"""
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K + layout)
    A = torch.randn((K, M) if layout == 2 else (M, K), generator=g).to(DEV)
    Bm = (torch.randn((N, K) if layout == 0 else (K, N), generator=g) * 0.05).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    C = full(M, N)
    L = _lib.lib()
    scratch = torch.zeros(L.pl_gemm_planes_scratch_bytes(M, N, K), dtype=torch.uint8, device=DEV)
    rc = L.pl_gemm_planes(layout, mode, A.data_ptr(), Bm.data_ptr(), C.data_ptr(), M, N, K, bias.data_ptr(), 1.0, 16.0,
                          scratch.data_ptr(), _lib.current_stream_ptr())
    _lib.check(rc, "pl_gemm_planes")
    torch.cuda.synchronize()
    emit(f"gemm/planes/{name}/mode{mode}/l{layout}-{M}x{N}x{K}", C=C, scratch=scratch.view(torch.int32))


def gemm_arith_case(arith, layout, M, N, K, splits=1):
    """pl_gemm_arith (launch_gemm_f32), slabs included"""
    g = torch.Generator().manual_seed(M + N + K + layout)
    A = torch.randn((K, M) if layout == 2 else (M, K), generator=g).to(DEV)
    Bm = torch.randn((N, K) if layout == 0 else (K, N), generator=g).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV) if splits == 1 else None
    C, slabs = full(M, N), full(splits, M, N) if splits > 1 else None
    rc = _lib.lib().pl_gemm_arith(layout, arith, A.data_ptr(), Bm.data_ptr(), C.data_ptr(), M, N, K,
                                  bias.data_ptr() if bias is not None else None, splits,
                                  slabs.data_ptr() if slabs is not None else None, _lib.current_stream_ptr())
    _lib.check(rc, "pl_gemm_arith")
    torch.cuda.synchronize()
    emit(f"gemm/arith{arith}/l{layout}-{M}x{N}x{K}-s{splits}", C=C, slabs=slabs)


def conv_planes_case(mode, B, H, W, Cin, Cout, K, stride, pad):
    """pl_conv2d_planes_fwd (with the epilogue's statistics) and pl_conv2d_planes_wgrad (slabs included)"""
    cv, L, s = pkg.conv, _lib.lib(), _lib.current_stream_ptr()
    g = torch.Generator().manual_seed(B * 131 + H * 17 + Cin + Cout + K)
    x = torch.randn(B, H, W, Cin, generator=g).to(DEV)
    w = (torch.randn(Cout, K, K, Cin, generator=g) * 0.05).to(DEV)
    Ho, Wo = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    dz = torch.randn(B, Ho, Wo, Cout, generator=g).to(DEV)
    xp, wp, dzp = cv._planes_of(x, 1.0, mode), cv._planes_of(w, 16.0, mode), cv._planes_of(dz, 1.0, mode)
    y, stat = full(B, Ho, Wo, Cout), full(2, L.pl_gemm_stat_groups(B * Ho * Wo), Cout)
    rc = L.pl_conv2d_planes_fwd(mode, xp.data_ptr(), x.numel(), B, H, W, Cin, wp.data_ptr(), w.numel(), Cout, K, K, stride, pad,
                                y.data_ptr(), 1.0 / 16.0, None, stat.data_ptr(), s)
    _lib.check(rc, "pl_conv2d_planes_fwd")
    name = f"gemm/conv-planes/mode{mode}/{B}x{H}x{W}x{Cin}-{Cout}-k{K}s{stride}"
    torch.cuda.synchronize()
    emit(name, y=y, stat=stat)
    if (B * Ho * Wo) % 32 == 0:
        splits = L.pl_gemm_planes_splits(Cout, K * K * Cin, B * Ho * Wo)
        slabs = full(splits, Cout * K * K * Cin) if splits > 1 else None
        dw = full(Cout, K, K, Cin)
        rc = L.pl_conv2d_planes_wgrad(mode, dzp.data_ptr(), dz.numel(), xp.data_ptr(), x.numel(), B, H, W, Cin, Cout, K, K, stride,
                                      pad, dw.data_ptr(), 1.0, None, slabs.data_ptr() if slabs is not None else None, s)
        _lib.check(rc, "pl_conv2d_planes_wgrad")
        torch.cuda.synchronize()
        emit(name + f"/wgrad-s{splits}", dw=dw, slabs=slabs)


def deconv_planes_case(mode, B, H, W, Cin, Cout):
    cv, L = pkg.conv, _lib.lib()
    g = torch.Generator().manual_seed(B + 7 * H + Cin + 3 * Cout)
    x = torch.randn(B, H, W, Cin, generator=g).to(DEV)
    w = (torch.randn(Cin, Cout, 4, 4, generator=g) * 0.05).to(DEV)
    xp, wsub = cv._planes_of(x, 1.0, mode), cv._planes_of(cv.deconv_subkernels(w), 16.0, mode)
    y = full(B, 2 * H, 2 * W, Cout)
    rc = L.pl_deconv4x4s2_planes_fwd(mode, xp.data_ptr(), x.numel(), B, H, W, Cin, wsub.data_ptr(), wsub.numel(), Cout, y.data_ptr(),
                                     1.0 / 16.0, None, _lib.current_stream_ptr())
    _lib.check(rc, "pl_deconv4x4s2_planes_fwd")
    torch.cuda.synchronize()
    emit(f"gemm/deconv-planes/mode{mode}/{B}x{H}x{W}x{Cin}-{Cout}", y=y)


def conv_nhwc_case(arith, B, H, Cin, Cout, K, stride, pad):
    """pl_conv2d_nhwc_fwd / _wgrad (launch_conv_nhwc, launch_conv_wgrad; 1x1: launch_gemm_f32) through the package"""
    g = torch.Generator().manual_seed(B + H + Cin + Cout + K)
    x = torch.randn(B, H, H, Cin, generator=g).to(DEV)
    w = (torch.randn(Cout, K, K, Cin, generator=g) * 0.05).to(DEV)
    y = pkg.conv.conv2d_nhwc(x, w, stride, pad, arith=arith)
    dw = pkg.conv.conv2d_nhwc_wgrad(x, torch.randn(y.shape, generator=g).to(DEV), K, stride, pad, arith=arith)
    torch.cuda.synchronize()
    emit(f"gemm/conv-nhwc/{arith}/{B}x{H}x{H}x{Cin}-{Cout}-k{K}s{stride}", y=y, dw=dw)


def gemm_cases():
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    # every branch of planes_route (tests/test_gpu_planes.py test_planes_gemm_routes), both modes
    for mode in (3, 1):
        for name, layout, M, N, K in (("one-item", 0, 128, 128, 32), ("one-item", 1, 128, 128, 32), ("one-item", 2, 128, 128, 32),
                                      ("one-item-edge", 0, 200, 192, 64), ("t64", 0, 256, 64, 32), ("t64-edge", 0, 1, 8, 32),
                                      ("t64-persistent", 0, 256 * 2 * ncu, 64, 32), ("wide", 0, 128, 128, 1024),
                                      ("wide-edge", 0, 136, 128, 1024), ("wide-persistent", 0, 128 * 2 * ncu, 128, 1024),
                                      ("persistent", 0, 128 * 2 * ncu, 128, 32), ("persistent-edge", 0, 128 * 2 * ncu + 8, 128, 32),
                                      ("below-persistent", 0, 128 * (2 * ncu - 1), 128, 32)):
            gemm_planes_case(name, layout, mode, M, N, K)
    # every branch of f32_route that pl_gemm_arith reaches (tests/test_gpu_parity.py test_gemm_arith_routes)
    for arith, layout, M, N, K, splits in ((0, 0, 128, 128, 32, 1), (0, 1, 128, 128, 32, 1), (0, 2, 128, 128, 32, 1),
                                           (0, 0, 130, 72, 40, 1), (1, 0, 128, 128, 32, 1), (2, 0, 128, 128, 32, 1),
                                           (5, 1, 128, 128, 32, 1), (6, 0, 128, 128, 32, 1), (2, 0, 128, 72, 32, 1),
                                           (0, 2, 128, 128, 256, 2), (2, 2, 128, 128, 256, 2)):
        gemm_arith_case(arith, layout, M, N, K, splits)
    # ... the bf16-planes GEMM (a 1x1 convolution in PL_BF16, whole and ragged N) and the implicit-GEMM launchers: 3x3 whole,
    # ragged (Cout = 72 / 189 pixels) and split-K (128 pixels of 1152 k), weight gradients
    for arith in ("bf16", "bf16x6"):
        for B, H, Cin, Cout, K, stride, pad in ((2, 8, 32, 128, 1, 1, 0), (2, 8, 32, 72, 1, 1, 0), (2, 8, 128, 128, 3, 1, 1),
                                                (2, 16, 64, 72, 3, 2, 1), (2, 32, 128, 128, 3, 1, 1)):
            conv_nhwc_case(arith, B, H, Cin, Cout, K, stride, pad)
        g = torch.Generator().manual_seed(8)
        x = torch.randn(2, 8, 8, 64, generator=g).to(DEV)
        for cout in (128, 72):                                  # launch_conv_nhwc_group4, whole and ragged
            wsub = pkg.conv.deconv_subkernels((torch.randn(64, cout, 4, 4, generator=g) * 0.05).to(DEV))
            y = pkg.conv.deconv4x4s2_nhwc(x, wsub, arith=arith)
            torch.cuda.synchronize()
            emit(f"gemm/deconv-nhwc/{arith}/2x8x8x64-{cout}", y=y)
    # the planes convolutions (tests/test_gpu_conv.py's smallest shapes: t64 / edge / row gather / ragged M / split-K wgrad)
    for mode in (3, 1):
        for shape in ((2, 16, 16, 64, 64, 3, 1, 1), (2, 16, 24, 32, 128, 3, 2, 1), (2, 8, 8, 128, 72, 1, 2, 0),
                      (3, 9, 7, 64, 96, 3, 1, 1), (1, 32, 32, 96, 256, 3, 1, 1)):
            conv_planes_case(mode, *shape)
        for shape in ((2, 8, 8, 64, 128), (1, 6, 10, 96, 64), (3, 4, 4, 256, 256)):
            deconv_planes_case(mode, *shape)
    # the thin GEMM (65 rows of a 64-wide fp32 lifter) and the backward pair, chained (five dX tiles, five dW items) and dual
    case_autograd("gemm/thin/fp32/B65/H64", 65, 64, 2, "fp32", 0.0)
    for dtype in ("f16x3", "bf16", "fp32", "bf16x6"):
        for H in (128, 256):
            case_autograd(f"gemm/pair/{dtype}/B640/H{H}", 640, H, 2, dtype, 0.5)


if __name__ == "__main__":
    lifter_cases()
    conv_cases()
    optimizer_cases()
    heads_cases()
    gemm_cases()
