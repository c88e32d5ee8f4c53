"""The "f16x3" range guard on the device (include/poselift.h pl_range_monitor, range_guard.py): in-range results are bitwise
what they are without it, an overflow is reported with its site and size, the record is sticky and holds the maximum,
non-finite sources are not recorded, a captured graph keeps reporting, and the conv path's sites work.

Every case sets the guard's state explicitly.  Batches: one per route of the lifter that stores fp16 planes at H = 1024 --
64 rows (the layer kernels of small_layer.hip), 128 (65 ... 512 rows on the planes: launch_small_linear_stats + bn_apply) and
640 (the smallest whole-tile batch above 512: the planes tile GEMM) -- plus, for the bitwise case, 65 rows (the ragged
65 ... 512-row route: exact fp32, no fp16 planes at all).  No fault is provoked anywhere: an fp16 inf is an ordinary value."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H = 1024
SITE_W, SITE_CONV_ACT = 8, 9


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


@pytest.fixture(autouse=True)
def _guard_state(pkg):
    """Every case starts from an enabled, clean guard; afterwards the guard is back in the state it was found in (off,
    unless somebody enabled it), so the modules that run behind this one see the library's default."""
    was = pkg.range_guard.enabled(DEV)
    pkg.range_guard.enable(DEV)
    pkg.range_guard.clear(DEV)
    yield
    pkg.range_guard.clear(DEV)
    (pkg.range_guard.enable if was else pkg.range_guard.disable)(DEV)


def _mags(pkg):
    return pkg.range_guard.status(DEV).cpu().numpy().view(np.float32)


def _lifter(pkg, dtype, p=0.0, S=2, seed=5):
    torch.manual_seed(seed)
    return pkg.LinearModel(34, 51, linear_size=H, num_stage=S, p_dropout=p, compute_dtype=dtype).to(DEV)


def _batch(B, seed=11):
    g = torch.Generator().manual_seed(seed + B)
    return torch.rand(B, 34, generator=g).to(DEV), (torch.rand(B, 51, generator=g) - 0.5).to(DEV)


# ---------------------------------------------------------------------------------------------------------------
# 1. in range: bitwise unchanged, record clean
# ---------------------------------------------------------------------------------------------------------------
def _lifter_results(pkg, B, p, guard):
    (pkg.range_guard.enable if guard else pkg.range_guard.disable)(DEV)
    assert pkg.range_guard.enabled(DEV) == guard
    m = _lifter(pkg, "f16x3", p).train()
    x, t = _batch(B)
    x.requires_grad_(True)
    m.manual_seed(17, step=2)
    y = m(x)
    pkg.mse_loss(y, t).backward()
    out = {"y": y.detach().clone(), "dx": x.grad.clone()}
    out.update({"g:" + k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None})
    out.update({"b:" + k: v.clone() for k, v in m.named_buffers()})
    m.eval()
    with torch.no_grad():
        out["y_eval"] = m(x.detach()).clone()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("B", [64, 65, 128, 640])
def test_in_range_lifter_is_bitwise_unchanged(pkg, B, p):
    on = _lifter_results(pkg, B, p, True)
    assert not pkg.range_guard.status(DEV).any().item(), pkg.range_guard.describe(pkg.range_guard.status(DEV).cpu().numpy())
    off = _lifter_results(pkg, B, p, False)
    assert on.keys() == off.keys() and len(on) > 20
    for k in on:
        assert torch.equal(on[k], off[k]), k
    assert torch.isfinite(on["y"]).all()


def _bottleneck_results(pkg, guard):
    (pkg.range_guard.enable if guard else pkg.range_guard.disable)(DEV)
    bb, cv = pkg.backbone, pkg.conv
    torch.manual_seed(3)
    blk = bb.Bottleneck(256, 64, stride=1).train().to(DEV)
    x = torch.randn(1, 8, 8, 256).to(DEV).requires_grad_(True)
    dy = torch.randn(1, 8, 8, 256).to(DEV)
    assert bb._bottleneck_planes_ok(blk, x.shape)
    out, outp = bb._bottleneck_train_planes(blk, x, cv.to_planes(x, pkg._lib.PL_F16X3), pkg._lib.PL_F16X3)
    out.backward(dy)
    res = {"y": out.detach().clone(), "yp": outp.detach().clone().view(torch.int32), "dx": x.grad.clone()}
    res.update({"g:" + k: v.grad.clone() for k, v in blk.named_parameters()})
    res.update({"b:" + k: v.clone() for k, v in blk.named_buffers()})
    torch.cuda.synchronize()
    return res


def _deconv_results(pkg, guard):
    (pkg.range_guard.enable if guard else pkg.range_guard.disable)(DEV)
    cv = pkg.conv
    torch.manual_seed(4)
    deconv = torch.nn.ConvTranspose2d(256, 64, kernel_size=4, stride=2, padding=1, bias=False).to(DEV)
    bn = torch.nn.BatchNorm2d(64).train().to(DEV)
    x = torch.randn(1, 8, 8, 256).to(DEV).requires_grad_(True)
    assert cv.planes_deconv_supported(1, 8, 8, 256, 64)
    lk = cv.PlaneLink(pkg._lib.PL_F16X3)
    out = cv.batchnorm_relu_train_planes(cv.deconv4x4s2_planes(cv.to_planes(x, pkg._lib.PL_F16X3), deconv.weight, lk), bn, True,
                                         False, lk)
    out.backward(torch.randn(1, 16, 16, 64, generator=torch.Generator().manual_seed(9)).to(DEV))
    res = {"y": out.detach().clone(), "dx": x.grad.clone(), "gw": deconv.weight.grad.clone(), "gg": bn.weight.grad.clone(),
           "gb": bn.bias.grad.clone(), "rm": bn.running_mean.clone(), "rv": bn.running_var.clone()}
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("results", [_bottleneck_results, _deconv_results])
def test_in_range_conv_path_is_bitwise_unchanged(pkg, results):
    on = results(pkg, True)
    assert not pkg.range_guard.status(DEV).any().item()
    off = results(pkg, False)
    for k in on:
        assert torch.equal(on[k], off[k]), k
    assert torch.isfinite(on["y"]).all()


# ---------------------------------------------------------------------------------------------------------------
# 2. activation overflow: the right site, the right size; just inside the range: silence and agreement
# ---------------------------------------------------------------------------------------------------------------
def _gamma(m, k):
    return m._named_holders()[k][1].weight


def _fwd_train(m, x):
    with torch.no_grad():
        return m(x)


def _act_max(m, k):
    return float(m.workspace_view(m.last_workspace, 1, k).abs().max())


def _gamma_factor(ref, k, target):
    """The factor on layer k's gamma (beta = 0) that takes the maximum of its activation to `target`: target / m for a plain
    layer; a block output is skip + gamma-part, of which only the second scales, so the factor is iterated on the reference's
    own tensors (both parts are ReLU outputs: the maximum grows with the factor)."""
    act = ref.workspace_view(ref.last_workspace, 1, k).clone()
    skip = ref.workspace_view(ref.last_workspace, 1, k - 2).clone() if (k >= 2 and k % 2 == 0) else torch.zeros_like(act)
    part, s = act - skip, 1.0
    for _ in range(8):
        s *= target / float((skip + s * part).abs().max())
    return s


def _pair(pkg, B):
    """The same weights (beta = 0, no dropout) in "bf16x6" -- the reference -- and "f16x3"."""
    ref = _lifter(pkg, "bf16x6").train()
    with torch.no_grad():
        for _, bn in ref._named_holders():
            bn.bias.zero_()
    m = _lifter(pkg, "f16x3").train()
    m.load_state_dict(ref.state_dict())
    return ref, m


# Measured on an MI355X, |reported / bf16x6 maximum - 1| (the bound 1e-3 is set by the feature's specification; both sides are
# fp32 values of the same tensor, computed by two arithmetics up to layer k):
#   B = 64:  k = 0: 0 (70000.008 both), k = 3: 3.4e-7      B = 128: k = 0: 0, k = 3: 0      B = 640: k = 0: 0, k = 3: 5.6e-7
#   k = 2 (block output): no figure recorded yet -- the case prints it (pytest -s)
# In range (60000), |y - y_bf16x6| / max|y|: 4.3e-8 ... 9.2e-7 (bound 2e-5).  Layers 0, 2 (a block output: carries the residual) and 3 (the
# last hidden layer that IS stored as fp16 planes); layer 4, the last hidden layer, feeds the 51-wide output Linear in fp32 and
# has no plane: test_last_hidden_layer_has_no_plane_to_overflow.
@pytest.mark.parametrize("k", [0, 2, 3])
@pytest.mark.parametrize("B", [64, 128, 640])
def test_activation_overflow_names_layer_and_magnitude(pkg, B, k):
    rg = pkg.range_guard
    ref, m = _pair(pkg, B)
    x, _ = _batch(B)
    _fwd_train(ref, x)
    g0 = _gamma(ref, k).detach().clone()
    factor = {t: _gamma_factor(ref, k, t) for t in (70000.0, 60000.0)}
    for target, over in ((70000.0, True), (60000.0, False)):
        with torch.no_grad():
            for mod in (ref, m):
                _gamma(mod, k).copy_(g0 * factor[target])
        y_ref = _fwd_train(ref, x)
        want = _act_max(ref, k)                       # the rescaled model's maximum in the reference arithmetic
        assert torch.isfinite(y_ref).all()            # the overflow belongs to the mode, not to the model
        assert (want > 65504.0) == over and abs(want / target - 1.0) < 0.01
        rg.clear(DEV)
        y = _fwd_train(m, x)
        if over:
            with pytest.raises(pkg.PoseliftRangeError) as ei:
                rg.check(DEV)
            sites = dict(ei.value.sites)
            # (behind k everything is NaN, as in torch: ReLU keeps the NaN of the layer after k, and the guard does not record
            #  non-finite sources -- so k is the first, and usually the only, site named)
            assert k in sites and min(sites) == k, ei.value
            assert f"hidden activation of layer {k}" in str(ei.value) and "bf16x6" in str(ei.value)
            dev = abs(sites[k] / want - 1.0)
            print(f"B={B} k={k}: reported {sites[k]:.8g}, bf16x6 {want:.8g}, deviation {dev:.3g}")
            assert dev < 1e-3
            rg.check(DEV)                             # raised once, clean now
        else:
            rg.check(DEV)                             # silent
            scale = float(y_ref.abs().max())
            err = float((y - y_ref).abs().max()) / scale
            print(f"B={B} k={k}: in range, |y - y_bf16x6| / max|y| = {err:.3g}")
            assert err <= 2e-5                        # test_ragged_shapes_vs_oracle's bound for the f16x3 forward


@pytest.mark.parametrize("B", [64, 640])
def test_last_hidden_layer_has_no_plane_to_overflow(pkg, B):
    """The output of the last hidden layer goes to the 51-wide output Linear in fp32: at 70000 nothing is stored as fp16, so
    nothing is reported and the result stays finite and agrees with "bf16x6"."""
    ref, m = _pair(pkg, B)
    x, _ = _batch(B)
    _fwd_train(ref, x)
    s = _gamma_factor(ref, 4, 70000.0)
    with torch.no_grad():
        for mod in (ref, m):
            _gamma(mod, 4).mul_(s)
    y_ref, y = _fwd_train(ref, x), _fwd_train(m, x)
    assert _act_max(ref, 4) > 65504.0
    pkg.range_guard.check(DEV)
    assert torch.isfinite(y).all() and float((y - y_ref).abs().max()) <= 2e-5 * float(y_ref.abs().max())


# ---------------------------------------------------------------------------------------------------------------
# 3. weights
# ---------------------------------------------------------------------------------------------------------------
def test_weight_overflow_after_refresh_and_after_adamw(pkg):
    rg = pkg.range_guard
    B = 128
    m = _lifter(pkg, "f16x3").train()
    opt = pkg.FlatAdamW(m, lr=1e-4)
    x, t = _batch(B)
    pkg.train_step(m, opt, x, t)                      # in range: finite gradients and moments
    rg.check(DEV)
    w = m.linear_stages[0].w1.weight
    with torch.no_grad():
        w[5, 7] = 5000.0                              # 5000 x 16 > 65504
    _fwd_train(m, x)                                  # the forward refreshes the stale planes first
    assert _mags(pkg)[SITE_W] == 5000.0
    with pytest.raises(pkg.PoseliftRangeError, match="weight planes"):
        rg.check(DEV)
    assert not rg.status(DEV).any().item()
    opt.step()                                        # pl_adamw_flat_planes rewrites the planes (the gradients are the first step's)
    got = float(_mags(pkg)[SITE_W])
    assert abs(got / float(w[5, 7]) - 1.0) < 1e-6 and abs(got / 5000.0 - 1.0) < 1e-3


def test_weight_overflow_in_the_small_batch_layer_kernels(pkg):
    """64 rows: no weight planes in memory -- the layer kernels split W on the way to LDS, the same guard."""
    m = _lifter(pkg, "f16x3").train()
    with torch.no_grad():
        m.linear_stages[1].w2.weight[1000, 1023] = -5000.0
    _fwd_train(m, _batch(64)[0])
    assert _mags(pkg)[SITE_W] == 5000.0


# ---------------------------------------------------------------------------------------------------------------
# 4. sticky, maximum, clear; two sites
# ---------------------------------------------------------------------------------------------------------------
def test_sticky_maximum_and_clear(pkg):
    rg = pkg.range_guard
    B = 128
    ref, m = _pair(pkg, B)
    x, _ = _batch(B)
    _fwd_train(ref, x)
    base, g0 = _act_max(ref, 1), _gamma(m, 1).detach().clone()
    seen = []
    for target in (90000.0, 70000.0):                 # the larger first: the second step must not lower the record
        with torch.no_grad():
            _gamma(m, 1).copy_(g0 * (target / base))
        _fwd_train(m, x)
        seen.append(float(_mags(pkg)[1]))
    assert abs(seen[0] / 90000.0 - 1.0) < 1e-2 and seen[1] == seen[0]
    with pytest.raises(pkg.PoseliftRangeError):
        rg.check(DEV)
    rg.check(DEV)
    _fwd_train(m, x)
    assert abs(float(_mags(pkg)[1]) / 70000.0 - 1.0) < 1e-2
    rg.clear(DEV)
    assert not rg.status(DEV).any().item()


def test_two_layers_two_slots(pkg):
    B = 64
    torch.manual_seed(5)
    ref = _lifter(pkg, "bf16x6", S=3).train()          # 7 hidden layers: layer 4 is stored as planes
    with torch.no_grad():
        for _, bn in ref._named_holders():
            bn.bias.zero_()
    m = _lifter(pkg, "f16x3", S=3).train()
    m.load_state_dict(ref.state_dict())
    x, _ = _batch(B)
    _fwd_train(ref, x)
    for k in (1, 4):                                  # one step each: behind an overflowing layer everything is NaN
        g0 = _gamma(m, k).detach().clone()
        with torch.no_grad():
            _gamma(m, k).mul_(_gamma_factor(ref, k, 70000.0))
        _fwd_train(m, x)
        with torch.no_grad():
            _gamma(m, k).copy_(g0)
    mags = _mags(pkg)
    assert mags[1] > 65504.0 and mags[4] > 65504.0
    # behind 1 and 4 the values are NaN, which the guard does not record: 5 and the block output 6 stay empty too (6 used to
    # carry 4's value through the skip connection when ReLU turned layer 5's NaN into 0)
    assert not mags[[0, 2, 3, 5, 6, 8]].any()


# ---------------------------------------------------------------------------------------------------------------
# 5. non-finite sources
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [64, 128])
def test_non_finite_sources_are_not_recorded(pkg, B):
    m = _lifter(pkg, "f16x3").train()
    x, _ = _batch(B)
    x[0, 0] = float("inf")                            # row 0 of the first pre-activation is +-inf in fp32
    _fwd_train(m, x)
    assert not torch.isfinite(m.workspace_view(m.last_workspace, 0, 0)).all()     # the pre-activation: inf / NaN
    assert not pkg.range_guard.status(DEV).any().item()


def test_non_finite_values_of_a_split_are_not_recorded(pkg):
    x = torch.zeros(64, device=DEV)
    x[3], x[9], x[17] = float("inf"), float("-inf"), float("nan")
    pkg.conv._planes_of(x, 1.0, pkg._lib.PL_F16X3)
    assert not pkg.range_guard.status(DEV).any().item()
    x[40] = -1e5
    pkg.conv._planes_of(x, 1.0, pkg._lib.PL_F16X3)
    assert _mags(pkg)[11] == np.float32(1e5) and not np.delete(_mags(pkg), 11).any()


def test_a_direct_call_of_the_c_entry_does_not_disarm_the_guard(pkg):
    """The wrapper hands the record over before every launching call: pl_range_monitor(NULL) from elsewhere on this thread
    lasts until the next one."""
    assert pkg.lib().pl_range_monitor(None) == 0
    x = torch.zeros(64, device=DEV)
    x[40] = 1e5
    pkg.conv._planes_of(x, 1.0, pkg._lib.PL_F16X3)
    assert _mags(pkg)[11] == np.float32(1e5)


# ---------------------------------------------------------------------------------------------------------------
# 6. graph replay
# ---------------------------------------------------------------------------------------------------------------
def test_graph_replay_reports(pkg):
    rg = pkg.range_guard
    B = 64
    m = _lifter(pkg, "f16x3").train()
    opt = pkg.FlatAdamW(m, lr=1e-4)
    x, t = _batch(B)
    step = pkg.GraphedTrainStep(m, opt, x, t.reshape(B, 17, 3))
    step(x, t.reshape(B, 17, 3))
    torch.cuda.synchronize()
    rg.check(DEV)                                     # captured and replayed in range
    with torch.no_grad():
        m.batch_norm1.weight.mul_(1e6)                # in place in the parameter arena: relu(gamma zhat) reaches ~1e6
    step(x, t.reshape(B, 17, 3))
    torch.cuda.synchronize()
    assert _mags(pkg)[0] > 65504.0


# ---------------------------------------------------------------------------------------------------------------
# 7. conv sites
# ---------------------------------------------------------------------------------------------------------------
def _block_eval(pkg, blk, x, xp):
    cv, mode = pkg.conv, pkg._lib.PL_F16X3
    out = xp
    for name, pad, last in (("conv1", 0, False), ("conv2", 1, False), ("conv3", 0, True)):
        w = cv.to_ohwi(getattr(blk, name).weight.detach().float())
        s, b = (t.detach() for t in cv.fold_bn(getattr(blk, "bn" + name[-1])))
        y, out = cv.conv2d_planes_eval(out, cv._planes_of(w, cv.WEIGHT_PLANE_SCALE, mode), w.shape, 1, pad, s, b,
                                       relu=2 if last else 1, resid=x if last else None, want_f32=last, want_planes=True, mode=mode)
    return y


@pytest.mark.parametrize("big, flagged", [(5e6, True), (4e6, False)])
def test_conv_activation_site(pkg, big, flagged):
    rg, cv = pkg.range_guard, pkg.conv
    torch.manual_seed(6)
    blk = pkg.backbone.Bottleneck(256, 64, stride=1).eval().to(DEV)
    x = torch.randn(1, 8, 8, 256).to(DEV)
    x[0, 3, 4, 17] = big
    # the generic split at the conv scale
    xp = cv._planes_of(x, cv.ACT_PLANE_SCALE, pkg._lib.PL_F16X3)
    mags = _mags(pkg)
    assert mags[SITE_CONV_ACT] == (np.float32(big) if flagged else 0.0) and not np.delete(mags, SITE_CONV_ACT).any()
    rg.clear(DEV)
    # one Bottleneck eval forward fed that map
    with torch.no_grad():
        _block_eval(pkg, blk, x, cv._planes_of(x, cv.ACT_PLANE_SCALE, pkg._lib.PL_F16X3))
    assert _mags(pkg)[SITE_CONV_ACT] == (np.float32(big) if flagged else 0.0)
    rg.clear(DEV)
    # ... and the GEMM epilogue as the writer: the input in range (4e6), the join relu(0 * conv3 + shift + x) lifts that
    # element to 4e6 + shift exactly -- 5e6 is flagged with that magnitude, 4e6 is not
    x[0, 3, 4, 17] = 4e6
    with torch.no_grad():
        blk.bn3.weight.zero_()
        blk.bn3.bias.fill_(big - 4e6)
        y = _block_eval(pkg, blk, x, cv._planes_of(x, cv.ACT_PLANE_SCALE, pkg._lib.PL_F16X3))
    assert float(y[0, 3, 4, 17]) == big
    assert _mags(pkg)[SITE_CONV_ACT] == (np.float32(big) if flagged else 0.0)
    if flagged:
        with pytest.raises(pkg.PoseliftRangeError, match="conv-path feature map"):
            rg.check(DEV)
