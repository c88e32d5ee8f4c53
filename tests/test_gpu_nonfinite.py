"""GPU tests of the non-finite contract ("Non-finite values"): a NaN or an infinity leaves every kernel where
torch's same operation leaves one.  O(1) random inputs with ONE poisoned element, one test with NaN and one with +inf; the
references and the case tables are tests/nonfinite_oracle.py (stock torch, CPU, fp64), whose patterns
tests/test_nonfinite_host.py asserts on their own.

Compute kernels: the set of non-finite outputs equals torch's exactly (so what torch has finite is finite here), and what the
poison cannot reach is bit-identical to the same call without it.  Kernels that move or select values (max-pool, add_relu,
the flips, the transpose, the bitmaps): the exact value, NaN and the sign of an infinity included.

+inf in a split arithmetic ("bf16x6", "f16x3", "bf16"; the conv path's tile GEMMs run "bf16x6"): an operand is a sum of
16-bit planes and the low plane of an infinity is inf - inf = NaN, so only the mask is compared, never the class -- and where
a ReLU follows, the mask in front of it (`reach`): torch's ReLU turns an exact -inf into 0, a NaN stays."""
import ctypes

import numpy as np
import pytest
import torch

import nonfinite_oracle as nfo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = sorted(nfo.POISONS)


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


def _gpu_kernel_names(fn):
    """Names of the GPU kernels one call of fn() launches (torch.profiler; as in test_gpu_eval_backward.py)."""
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def _short(names):
    """The library's kernels among profiler event names, without namespaces, template and call arguments."""
    import re
    return sorted({m.group(1) for n in names for m in [re.search(r"(\w+_kernel)\b", n)] if m})


def _t(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rows(mask):
    return mask.reshape(mask.shape[0], -1)


def _assert_mask(got, want, what):
    g, w = nfo.bad(got), nfo.bad(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), f"{what}: {int((g & ~w).sum())} non-finite where torch is finite, " \
                                 f"{int((w & ~g).sum())} finite where torch is not (of {int(w.sum())})"


# ================================================================================================== lifter
def _model(pkg, case, st, train=False):
    i_dim, o_dim = case.dims
    m = pkg.LinearModel(i_dim, o_dim, linear_size=case.H, num_stage=case.S, p_dropout=0.0, BN=case.bn,
                        compute_dtype=case.dtype).to(DEV)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in st.items()})
    return m.train(train)


def _poison_weight(m, value):
    name, i, j = nfo.MID_WEIGHT
    with torch.no_grad():
        old = dict(m.named_parameters())[name][i, j].item()
        dict(m.named_parameters())[name][i, j] = value
    return old


@pytest.mark.parametrize("where", ["x", "w"])
@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("case,kernel", nfo.EVAL_FWD_CASES, ids=[c.id for c, _ in nfo.EVAL_FWD_CASES])
def test_lifter_eval_forward(pkg, case, kernel, poison, where):
    """pl_lifter_fwd_eval.  One poisoned element of one input row: that row of y is non-finite (NaN for a NaN), every other
    row has the bits of the clean call.  One poisoned weight of a middle layer: every row."""
    value = nfo.POISONS[poison]
    st, x, t = nfo.lifter_inputs(case)
    m = _model(pkg, case, st)
    with torch.no_grad():
        clean = m(_t(x))
        assert torch.isfinite(clean).all()
        stp, xp, _ = nfo.poisoned(case, where, value)
        if where == "w":
            _poison_weight(m, value)
        out = []
        names = _gpu_kernel_names(lambda: out.append(m(_t(xp))))
    y = out[0]
    print(f"{case.id}: {_short(names)}")
    assert any(kernel in n for n in names), (case.id, _short(names))
    want = nfo.twin_step(stp, xp, t, case, train=False)["y"]
    _assert_mask(y, want, f"{case.id} y")
    if where == "x":
        r = nfo.poison_row(case)
        keep = np.arange(case.B) != r
        assert nfo.bad(y)[r].all() and nfo.same_bits(y[keep], clean[keep])
        if poison == "nan":
            assert np.array_equal(nfo.classes(y), nfo.classes(want))
    else:
        assert nfo.bad(y).all()


@pytest.mark.parametrize("where", ["x", "w"])
@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("case", nfo.EVAL_BWD_CASES, ids=[c.id for c in nfo.EVAL_BWD_CASES])
def test_lifter_eval_saved_forward_and_backward(pkg, case, poison, where):
    """model.eval() inside an autograd graph (pl_lifter_fwd_eval_saved / pl_lifter_bwd_eval): y and dx of the poisoned row are
    non-finite, the other rows' are finite (y: the clean call's bits); a NaN reaches every parameter gradient torch's reaches."""
    value = nfo.POISONS[poison]
    st, x, t = nfo.lifter_inputs(case)
    m = _model(pkg, case, st)
    stp, xp, _ = nfo.poisoned(case, where, value)

    def step(xin):
        m.zero_grad(set_to_none=True)
        a = _t(xin).requires_grad_(True)
        y = m(a)
        ((y - _t(t)) ** 2).mean().backward()
        return y.detach(), a.grad

    y0, dx0 = step(x)
    assert torch.isfinite(y0).all() and torch.isfinite(dx0).all()
    if where == "w":
        _poison_weight(m, value)
    y, dx = step(xp)
    tw = nfo.twin_step(stp, xp, t, case, train=False)
    _assert_mask(y, tw["y"], f"{case.id} y")
    _assert_mask(dx, tw["dx"], f"{case.id} dx")
    if where == "x":
        r = nfo.poison_row(case)
        keep = np.arange(case.B) != r
        assert nfo.bad(dx)[r].all() and not nfo.bad(dx)[keep].any() and nfo.same_bits(y[keep], y0[keep])
    if poison == "nan":
        for n, p in m.named_parameters():
            if n in tw["grads"]:
                _assert_mask(p.grad, tw["grads"][n], f"{case.id} d{n}")
    assert all(torch.isfinite(b).all() for n, b in m.state_dict().items() if "running" in n)     # eval: buffers untouched


def _bits_of(*ts):
    return [t.detach().clone() for t in ts]


def _cpu_twin_adamw(pkg, m, **kw):
    from oracle.torch_twin import TwinLifter
    tw = TwinLifter(m.input_size, m.output_size, linear_size=m.linear_size, num_stage=m.num_stage, p_dropout=0.0, BN=m.BN)
    tw.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    return tw, torch.optim.AdamW(tw.parameters(), **kw)


def _used(m, s):
    return m.BN or "batch_norm" not in s.name


def _hand_over_grads(m, tw):
    """The library's gradient of this step as the CPU twin's .grad (as tests/test_gpu_grad_clip.py)."""
    fg = m.flat_grads.detach().cpu()
    named = dict(tw.named_parameters())
    for s in m._slots:
        named[s.name].grad = fg[s.offset:s.offset + s.numel].view(s.shape).clone() if _used(m, s) else None


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


def _train(pkg, m, opt, x, t, route):
    """One step on the fused entry (train_step's library route) or through autograd (an input that requires a gradient is not
    fusable: model(x), mse_loss, backward, optimizer.step)."""
    xd = _t(x)
    if route == "autograd":
        xd.requires_grad_(True)
    return pkg.train_step(m, opt, xd, _t(t))


@pytest.mark.parametrize("route", ["fused", "autograd"])
@pytest.mark.parametrize("where", ["x", "w"])
@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("case", nfo.TRAIN_CASES, ids=[c.id for c in nfo.TRAIN_CASES])
def test_lifter_train_step_is_skipped(pkg, case, poison, where, route):
    """A clean step, the poisoned step, a clean step, with skip_nonfinite=True: the poisoned step's loss, gradient arena and
    gradient norm are non-finite (a NaN: every gradient's mask is the twin's), parameters, m and v keep their bits, and the
    step after it matches the torch twin that did not step."""
    value = nfo.POISONS[poison]
    st, x, t = nfo.lifter_inputs(case)
    m = _model(pkg, case, st, train=True)
    opt = pkg.FlatAdamW(m, lr=3e-4, weight_decay=0.02, max_grad_norm=1e3, skip_nonfinite=True)
    tw, topt = _cpu_twin_adamw(pkg, m, lr=3e-4, weight_decay=0.02)
    _, xp, _ = nfo.poisoned(case, where, value)
    for it in range(3):
        if it == 1:
            before = _bits_of(m.flat_params, opt._m, opt._v)
            old = _poison_weight(m, value) if where == "w" else None
            if where == "w":
                before[0] = m.flat_params.detach().clone()
            out = []
            names = _gpu_kernel_names(lambda: out.append(_train(pkg, m, opt, xp, t, route)))
            loss, yh = out[0]
            print(f"{case.id} {route}: {_short(names)}")
            assert set(nfo.TRAIN_KERNELS[case.id]) <= set(_short(names)), (case.id, _short(names))
            if case.id == "f16x3-16x256-small":                  # Linear + BatchNorm + ReLU in one launch: fwd_tail's ReLU alone
                assert not any("bn_apply" in n or "bn_small" in n for n in names), _short(names)
            # the twin on the weights and buffers as they are now, one AdamW step from the seeded ones
            now = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
            ref = nfo.twin_step(now, xp, t, case, train=True)
            assert not torch.isfinite(loss).item() and not np.isfinite(opt.grad_norm.item())
            _assert_mask(yh.reshape(case.B, -1), ref["y"], f"{case.id} y")
            fg = m.flat_grads
            assert not torch.isfinite(fg).all()
            if poison == "nan":
                for s in m._slots:
                    if _used(m, s):
                        _assert_mask(fg[s.offset:s.offset + s.numel].view(s.shape), ref["grads"][s.name], f"{case.id} d{s.name}")
            for a, b in zip(before, (m.flat_params, opt._m, opt._v)):
                assert nfo.same_bits(a, b)
            assert opt.skipped_steps() == 1
            if where == "w":
                _poison_weight(m, old)
            continue                                                        # the twin does not call step()
        loss, _ = _train(pkg, m, opt, x, t, route)
        assert torch.isfinite(loss).item() and torch.isfinite(m.flat_grads).all()
        _hand_over_grads(m, tw)
        torch.nn.utils.clip_grad_norm_(tw.parameters(), 1e3)
        topt.step()
        _assert_state_close(m, opt, tw, topt)
    assert opt.skipped_steps() == 1 and float(opt.state_dict()["state"][0]["step"]) == 2.0


@pytest.mark.parametrize("case", nfo.TRAIN_CASES, ids=[c.id for c in nfo.TRAIN_CASES])
def test_lifter_train_step_without_skip_gives_nan_parameters_as_torch(pkg, case):
    st, x, t = nfo.poisoned(case, "x", nfo.NAN)
    m = _model(pkg, case, st, train=True)
    opt = pkg.FlatAdamW(m, lr=3e-4, max_grad_norm=1.0)
    tw, topt = _cpu_twin_adamw(pkg, m, lr=3e-4)
    _train(pkg, m, opt, x, t, "fused")
    _hand_over_grads(m, tw)
    torch.nn.utils.clip_grad_norm_(tw.parameters(), 1.0)                    # error_if_nonfinite=False
    topt.step()
    named, hit = dict(tw.named_parameters()), 0
    for s, p in zip(m._slots, m._param_list):                               # NaN where torch has NaN, nowhere else
        ours = torch.isnan(p.detach()).cpu()
        assert torch.equal(ours, torch.isnan(named[s.name].detach())), s.name
        hit += int(ours.sum())
    assert hit > 0 and torch.isnan(m.state_dict()["w2.weight"]).all() and opt.skipped_steps() == 0


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("cid", ["f16x3-16x128-small", "f16x3-128x128-tile"])
def test_graphed_train_step_replay_with_a_poisoned_batch_is_skipped(pkg, cid, poison):
    case = next(c for c in nfo.TRAIN_CASES if c.id == cid)
    st, x, t = nfo.lifter_inputs(case)
    _, xp, _ = nfo.poisoned(case, "x", nfo.POISONS[poison])
    m = _model(pkg, case, st, train=True)
    opt = pkg.FlatAdamW(m, lr=3e-4, weight_decay=0.02, max_grad_norm=1e3, skip_nonfinite=True)
    step = pkg.GraphedTrainStep(m, opt, _t(x), _t(t))
    step(_t(x), _t(t))
    before = _bits_of(m.flat_params, opt._m, opt._v)
    loss, yh = step(_t(xp), _t(t))
    assert not torch.isfinite(loss).item() and not torch.isfinite(yh).any()
    for a, b in zip(before, (m.flat_params, opt._m, opt._v)):
        assert nfo.same_bits(a, b)
    assert opt.skipped_steps() == 1 and not np.isfinite(opt.grad_norm.item())
    loss, _ = step(_t(x), _t(t))
    assert torch.isfinite(loss).item() and opt.skipped_steps() == 1 and not nfo.same_bits(before[0], m.flat_params)


@pytest.mark.parametrize("case,kernel", nfo.DROPOUT_CASES, ids=[c.id for c, _ in nfo.DROPOUT_CASES])
def test_dropout_on_a_nan_is_pinned_to_the_select_form(pkg, case, kernel):
    """PINNED BEHAVIOUR THAT IS NOT TORCH'S.  Dropout(0.5) with injected keep masks on a unit that is NaN in every row (a NaN
    bias of a middle layer), on each kernel that applies Dropout (bn_small_fwd_kernel, small_fwd_kernel, bn_apply_kernel) and
    without BatchNorm.  torch's Dropout is the product relu(.) * mask / (1 - p): a DROPPED NaN is NaN * 0 = NaN, and so is
    the gradient of a dropped element when a NaN gradient arrives.  The library selects, keep ? . / (1 - p) : 0, in both
    directions (one bit per element, "kept and positive"): a dropped NaN is 0.  The forward could multiply instead; measured,
    that costs 0.8 % of the B = 4096 step and 2.9 % of the cycle step, outside the parent's spread
    (profiles/nonfinite_relu_ab.txt, C), so the select stays -- DESIGN.md, "Non-finite values".
    Asserted: the layer's output, its bitmap, y, dx and every gradient have exactly the non-finite set of the twin whose
    Dropout selects (nonfinite_oracle._SelectDropout), which is never more than stock torch's; at the dropped row 0 the
    unit is finite here and NaN in torch; the kept NaN's bit is set; the loss is NaN as in torch."""
    st, x, t = nfo.lifter_inputs(case)
    st = {k: np.array(v) for k, v in st.items()}
    st[nfo.DROPOUT_BIAS][nfo.DROPOUT_UNIT] = nfo.NAN
    masks = nfo.dropout_masks(case)
    i_dim, o_dim = case.dims
    m = pkg.LinearModel(i_dim, o_dim, linear_size=case.H, num_stage=case.S, p_dropout=0.5, BN=case.bn,
                        compute_dtype=case.dtype).to(DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    m.train()
    m.debug_inject_keep(_t(np.stack([pkg.layout.pack_keep_bitmap(k) for k in masks]).view(np.int64)))
    xd = _t(x).requires_grad_(True)
    out = []
    names = _gpu_kernel_names(lambda: out.append(m(xd)))
    assert kernel in _short(names), (case.id, _short(names))
    y = out[0]
    L, u = nfo.DROPOUT_LAYER, nfo.DROPOUT_UNIT
    ws = m.last_workspace
    act = m.workspace_view(ws, 1, L).clone()
    bits = pkg.layout.unpack_bitmap(m.workspace_view(ws, 2, L).cpu().numpy().view(np.uint64), case.H)
    loss = pkg.mse_loss(y, _t(t))
    loss.backward()
    stock = nfo.dropout_twin_step(st, x, t, case, masks)
    pinned = nfo.dropout_twin_step(st, x, t, case, masks, select=True)
    _assert_mask(act, pinned["acts"][L], f"{case.id} output of layer {L}")
    assert not masks[L][0, u] and np.isfinite(act[0, u].item()) and np.isnan(float(stock["acts"][L][0, u]))   # torch: NaN
    assert masks[L][1, u] and np.isnan(act[1, u].item())
    assert np.array_equal(bits[:, u], masks[L][:, u])            # a kept NaN counts as positive; a dropped one has no bit
    _assert_mask(y, pinned["y"], f"{case.id} y")
    assert np.isnan(loss.item()) and np.isnan(float(stock["loss"]))
    _assert_mask(xd.grad, pinned["dx"], f"{case.id} dx")
    assert not (nfo.bad(pinned["y"]) & ~nfo.bad(stock["y"])).any() and not (nfo.bad(pinned["dx"]) & ~nfo.bad(stock["dx"])).any()
    for n, p_ in m.named_parameters():
        if n in pinned["grads"] and p_.grad is not None:
            _assert_mask(p_.grad, pinned["grads"][n], f"{case.id} d{n}")
            assert not (nfo.bad(pinned["grads"][n]) & ~nfo.bad(stock["grads"][n])).any(), n


def test_bad_gather_index_gives_a_nan_pose_and_a_skipped_step(pkg):
    """pl_pose_augment_gather: a source index outside the table yields a NaN pose row (as tests/test_gpu_pose_augment.py); one
    train_step on that batch with skip_nonfinite=True is skipped -- the NaN reaches the loss."""
    import pose_augment_oracle as pao
    from test_pose_augment_host import TABLE_ROWS, aug_struct, make_table
    a, b, idx = make_table(pkg)
    a_t, b_t = torch.tensor(a).to(DEV), torch.tensor(b).to(DEV)
    src = idx[:16].copy()
    src[5] = TABLE_ROWS
    s = torch.tensor(src, device=DEV)
    rid = torch.arange(16, dtype=torch.int64, device=DEV)
    oa, ob = torch.zeros(16, 17, 2, device=DEV), torch.zeros(16, 17, 3, device=DEV)
    cfg = aug_struct(pkg, pao.config())
    rc = pkg.lib().pl_pose_augment_gather(a_t.data_ptr(), b_t.data_ptr(), s.data_ptr(), rid.data_ptr(), 16, TABLE_ROWS,
                                          oa.data_ptr(), ob.data_ptr(), ctypes.byref(cfg), 0, pkg._lib.current_stream_ptr())
    assert rc == 0, pkg.lib().pl_last_error()
    bad = np.arange(16) == 5
    assert np.array_equal(_rows(np.isnan(oa.cpu().numpy())).all(1), bad) and np.array_equal(_rows(nfo.bad(ob)).any(1), bad)
    torch.manual_seed(4)
    m = pkg.LinearModel(34, 51, linear_size=128, p_dropout=0.0, compute_dtype="f16x3").to(DEV).train()
    opt = pkg.FlatAdamW(m, lr=3e-4, skip_nonfinite=True)
    p0 = m.flat_params.detach().clone()
    loss, _ = pkg.train_step(m, opt, oa, ob)
    assert torch.isnan(loss).item() and opt.skipped_steps() == 1 and nfo.same_bits(p0, m.flat_params)


# ================================================================================================== conv path
def _conv(pkg, case, x, w, scale, shift, relu, r):
    dv = lambda t: None if t is None else t.to(DEV)
    return pkg.conv.conv2d_nhwc(dv(x), pkg.conv.to_ohwi(w).to(DEV), case[7], case[8], dv(scale), dv(shift), None, relu, dv(r))


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("relu,resid", nfo.CONV_VARIANTS)
@pytest.mark.parametrize("case", nfo.CONV_CASES, ids=[c[0] for c in nfo.CONV_CASES])
def test_conv2d_nhwc_relu_epilogue(pkg, case, relu, resid, poison):
    """conv2d_nhwc with the folded BatchNorm and ReLU in the epilogue on each forward route, one poisoned input element."""
    value = nfo.POISONS[poison]
    x, w, scale, shift, r = nfo.conv_inputs(case, resid)
    xp = x.clone()
    xp[nfo.CONV_POISON] = value
    clean = _conv(pkg, case, x, w, scale, shift, relu, r)
    out = []
    names = _gpu_kernel_names(lambda: out.append(_conv(pkg, case, xp, w, scale, shift, relu, r)))
    y = out[0]
    direct_stem = case[0] == "stem" and relu == 1 and not resid    # (with a residual or relu == 2: the im2col route)
    kernel = case[9] if (case[0] != "stem" or direct_stem) else "im2col_nhwc_kernel"
    print(f"{case[0]} relu={relu} resid={resid}: {_short(names)}")
    assert any(kernel in n for n in names), (case[0], _short(names))
    want, pre = nfo.conv_ref(xp, w, case[7], case[8], scale, shift, relu, r)
    split = case[10] or not direct_stem
    # +inf in a split arithmetic: NaN wherever the poison enters, in front of the ReLU (module docstring)
    _assert_mask(y, pre if (poison == "inf" and split) else want, f"{case[0]} relu={relu} resid={resid}")
    reach = nfo.bad(pre)
    assert torch.isfinite(clean).all() and nfo.same_bits(y.cpu()[torch.from_numpy(~reach)], clean.cpu()[torch.from_numpy(~reach)])
    if poison == "nan":
        assert np.isnan(y.cpu().numpy()[reach]).all()


@pytest.mark.parametrize("poison", POISON)
def test_deconv4x4s2_bn_relu(pkg, poison):
    x, w, scale, shift = nfo.deconv_inputs()
    xp = x.clone()
    xp[0, 2, 3, 5] = nfo.POISONS[poison]
    run = lambda xin: pkg.conv.deconv4x4s2_nhwc(xin.to(DEV), pkg.conv.deconv_subkernels(w).to(DEV), scale.to(DEV), shift.to(DEV), 1)
    clean, y = run(x), run(xp)
    want, pre = nfo.deconv_ref(xp, w, scale, shift)
    _assert_mask(y, pre, "deconv")                    # (the four sub-convolutions run "bf16x6": the mask in front of the ReLU)
    if poison == "nan":
        _assert_mask(y, want, "deconv")
    keep = torch.from_numpy(~nfo.bad(pre))
    assert nfo.same_bits(y.cpu()[keep], clean.cpu()[keep])


@pytest.mark.parametrize("rows,C,planes", [(r, c, False) for r, c in nfo.ADD_RELU_SHAPES] +
                         [(r, c, True) for r, c in nfo.ADD_RELU_PLANES_SHAPES])
def test_add_relu_value_bitmap_bit_and_backward(pkg, rows, C, planes):
    """relu(a + b) with a NaN, a +inf and a -inf sum: the exact value; the stored bitmap bit of the NaN element is SET (torch's
    threshold_backward passes the gradient there); the backward through pl_mask_add_by_bits."""
    g = torch.Generator().manual_seed(rows * 1000 + C)
    a, b, dy = (torch.randn(rows, C, generator=g) for _ in range(3))
    a[rows - 1, C - 3] = nfo.NAN
    a[0, C - 1], a[0, C - 2] = nfo.INF, -nfo.INF
    want, dwant = nfo.add_relu_ref(a, b, dy)
    ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    out = pkg.conv.add_relu_planes(ad, bd)[0] if planes else pkg.conv.add_relu(ad, bd)
    assert nfo.same_values(out, want)
    out.backward(dy.to(DEV))
    assert nfo.same_values(ad.grad, dwant) and nfo.same_values(bd.grad, dwant)
    assert float(ad.grad[rows - 1, C - 3]) == float(dy[rows - 1, C - 3])
    # the bitmap itself
    o2, bits = torch.empty(rows, C, device=DEV), pkg.conv._bits(rows, C, DEV)
    rc = pkg.lib().pl_add_relu_fwd_ex(ad.data_ptr(), bd.data_ptr(), rows, C, o2.data_ptr(), bits.data_ptr(), None, 0,
                                      pkg._lib.current_stream_ptr())
    assert rc == 0
    on = pkg.layout.unpack_bitmap(bits.cpu().numpy().view(np.uint64), C)
    assert np.array_equal(on, ~(want.numpy() <= 0)) and on[rows - 1, C - 3] and on[0, C - 1] and not on[0, C - 2]


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("rows,C", nfo.BN_RELU_SHAPES)
def test_batchnorm_relu_train(pkg, rows, C, poison):
    """Training-mode BatchNorm2d + ReLU, one poisoned element: its whole column of y and dz, dgamma and the running statistics of
    that channel -- and dbeta of that channel FINITE, the plain sum of dy (ReLU's backward passes at a NaN).  Every other
    channel: the bits of the clean call."""
    g = torch.Generator().manual_seed(rows + C)
    z, dy = torch.randn(rows, C, generator=g) * 2 + 0.5, torch.randn(rows, C, generator=g)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5); bn.bias.copy_(torch.randn(C, generator=g) * 0.2)
    zp = z.clone()
    zp[rows // 2, 3] = nfo.POISONS[poison]
    ref = nfo.bn_relu_train_ref(zp, bn, dy)

    def run(zin):
        import copy
        bnd = copy.deepcopy(bn).to(DEV).train()
        zd = zin.to(DEV).requires_grad_(True)
        y = pkg.conv.batchnorm_relu_train(zd.reshape(1, rows, 1, C), bnd, True)
        y.backward(dy.to(DEV).reshape(1, rows, 1, C))
        return dict(y=y.detach().reshape(rows, C), dz=zd.grad, dgamma=bnd.weight.grad, dbeta=bnd.bias.grad,
                    running_mean=bnd.running_mean, running_var=bnd.running_var)

    clean, got = run(z), run(zp)
    other = torch.arange(C) != 3
    for k in ref:
        _assert_mask(got[k], ref[k], k)
        assert nfo.same_bits(got[k].cpu()[..., other], clean[k].cpu()[..., other]), k
    want = float(ref["dbeta"][3])
    assert abs(float(got["dbeta"][3]) - want) < 2e-5 * max(1.0, abs(want))


TAPS = [(kh, kw) for kh in range(3) for kw in range(3)] + [None]


@pytest.mark.parametrize("shape", nfo.MAXPOOL_SHAPES)
def test_maxpool_forwards_and_backwards(pkg, shape):
    """Both forwards (pl_maxpool3x3s2_nhwc, and _idx: the training one) and both backwards (from the recorded tap, and
    recomputed from x) with a NaN at each of the nine taps of one window in turn, and a window of -inf only, against
    F.max_pool2d and its autograd: exact values; the two forwards agree bit for bit."""
    B, H, W, C = shape
    L = pkg.lib()
    for tap in TAPS:
        x, dy = nfo.maxpool_inputs(shape, tap, nfo.NAN)
        want, dwant = nfo.maxpool_ref(x, dy)
        xd, dyd = x.to(DEV).requires_grad_(True), dy.to(DEV)
        y1 = pkg.conv.maxpool3x3s2_nhwc(xd.detach())
        y2 = pkg.conv.maxpool3x3s2_nhwc_autograd(xd)
        assert nfo.same_values(y1, want), tap
        assert nfo.same_bits(y1, y2), tap
        y2.backward(dyd)
        assert nfo.same_values(xd.grad, dwant), tap
        dx = torch.empty(B, H, W, C, device=DEV)
        rc = L.pl_maxpool3x3s2_nhwc_bwd(xd.data_ptr(), dyd.data_ptr(), B, H, W, C, dx.data_ptr(), pkg._lib.current_stream_ptr())
        assert rc == 0 and nfo.same_values(dx, dwant), tap
    for value in (nfo.INF, -nfo.INF):                            # an infinite tap is a pure select: the exact class
        for tap in ((0, 0), (1, 1), (2, 2)):
            x, dy = nfo.maxpool_inputs(shape, tap, value)
            want, dwant = nfo.maxpool_ref(x, dy)
            xd, dyd = x.to(DEV).requires_grad_(True), dy.to(DEV)
            y1, y2 = pkg.conv.maxpool3x3s2_nhwc(xd.detach()), pkg.conv.maxpool3x3s2_nhwc_autograd(xd)
            assert nfo.same_values(y1, want) and nfo.same_bits(y1, y2), (value, tap)
            y2.backward(dyd)
            dx = torch.empty(B, H, W, C, device=DEV)
            rc = L.pl_maxpool3x3s2_nhwc_bwd(xd.data_ptr(), dyd.data_ptr(), B, H, W, C, dx.data_ptr(), pkg._lib.current_stream_ptr())
            assert rc == 0 and nfo.same_values(xd.grad, dwant) and nfo.same_values(dx, dwant), (value, tap)
    # two NaNs in one window: torch hands the gradient to the LAST one
    x, dy = nfo.maxpool_inputs(shape, (0, 1), nfo.NAN)
    oh, ow = nfo.MAXPOOL_WINDOW
    x[B - 1, 2 * oh - 1 + 2, 2 * ow - 1 + 0, 1] = nfo.NAN
    want, dwant = nfo.maxpool_ref(x, dy)
    xd, dyd = x.to(DEV).requires_grad_(True), dy.to(DEV)
    pkg.conv.maxpool3x3s2_nhwc_autograd(xd).backward(dyd)
    dx = torch.empty(B, H, W, C, device=DEV)
    rc = L.pl_maxpool3x3s2_nhwc_bwd(xd.data_ptr(), dyd.data_ptr(), B, H, W, C, dx.data_ptr(), pkg._lib.current_stream_ptr())
    assert rc == 0 and nfo.same_values(xd.grad, dwant) and nfo.same_values(dx, dwant)


@pytest.mark.parametrize("poison", POISON)
def test_bottleneck_training_step_and_flat_adam_skip(pkg, poison):
    """One Bottleneck(256, 64) training step on (2, 8, 8, 256) with one NaN pixel against the stock module: the output's, every
    gradient's and the running statistics' masks (bn3.bias: finite in torch -- the join's ReLU passes dy at a NaN -- and the
    same value here); arena.FlatAdam(skip_nonfinite=True) skips the step."""
    torch.manual_seed(3)
    blk = pkg.backbone.Bottleneck(256, 64, stride=1).train()
    x, dy = torch.randn(*nfo.BOTTLENECK_SHAPE), torch.randn(*nfo.BOTTLENECK_SHAPE)
    x[1, 2, 5, 9] = nfo.POISONS[poison]                       # (+inf: bn1's batch statistics turn it into NaN everywhere, as a NaN)
    out_ref, dx_ref, grads, buffers = nfo.bottleneck_ref(blk, x, dy)
    b = blk.to(DEV)
    opt = pkg.arena.FlatAdam(b, lr=1e-3, skip_nonfinite=True)
    p0 = opt.arena.flat.detach().clone()
    xd = x.to(DEV).requires_grad_(True)
    o, ident = pkg.backbone._bottleneck_train_direct(b, xd, "bf16x6")
    out = pkg.conv.add_relu(o, ident)
    out.backward(dy.to(DEV))
    _assert_mask(out, out_ref, "out")
    _assert_mask(xd.grad, dx_ref, "dx")
    for n, p in b.named_parameters():
        _assert_mask(p.grad, grads[n], n)
    for n, v in b.named_buffers():
        if "running" in n:
            _assert_mask(v, buffers[n], n)
    want = grads["bn3.bias"]
    assert float((b.bn3.bias.grad.cpu().double() - want).abs().max()) < 2e-4 * max(1.0, float(want.abs().max()))
    opt.step()
    assert opt.skipped_steps() == 1 and not np.isfinite(opt.grad_norm.item()) and nfo.same_bits(p0, opt.arena.flat)


def test_flips_and_transpose_move_non_finite_values_exactly(pkg):
    g = torch.Generator().manual_seed(9)
    for D in (2, 3):
        p = torch.randn(5, 17, D, generator=g)
        p[1, 4, 0], p[2, 13, D - 1], p[3, 0, 1] = nfo.NAN, nfo.INF, -nfo.INF
        want = p.clone()                                        # (fp32: 1 - x rounds once, here as on the device)
        want[..., 0] = (1.0 - want[..., 0]) if D == 2 else -want[..., 0]
        left, right = [4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]
        want[:, left + right] = want[:, right + left].clone()
        assert nfo.same_values(pkg.flip_pose(p.to(DEV)), want.double())
    x = torch.randn(2, 8, 12, 68, generator=g)
    x[1, 3, 7, 5], x[0, 0, 0, 67], x[1, 7, 11, 0] = nfo.NAN, nfo.INF, -nfo.INF
    assert nfo.same_values(pkg.conv.nhwc_to_nchw(x.to(DEV)), x.permute(0, 3, 1, 2).double())


# ================================================================================================== ViT token head
@pytest.mark.parametrize("poison", POISON)
def test_vit_token_head(pkg, poison):
    """pl_vit_head_fwd / _bwd, one NaN (or +inf) in z at T = 3, K = 32, out_d = 3: row t of y is non-finite; dz is finite
    everywhere (ReLU's backward passes dy W there) and matches the twin; column k of dW is non-finite.  (Exact fp32 on the
    vector unit: with +inf the masks are torch's as well.)"""
    T, K, out_d = nfo.VIT_HEAD
    g = torch.Generator().manual_seed(11)
    z, W, b, dy = (torch.randn(T, K, generator=g), torch.randn(out_d, K, generator=g), torch.randn(out_d, generator=g),
                   torch.randn(T, out_d, generator=g))
    L, s = pkg.lib(), pkg._lib.current_stream_ptr

    def run(zin):
        zd, Wd, bd, dyd = (t.to(DEV) for t in (zin, W, b, dy))
        y = torch.empty(T, out_d, device=DEV)
        assert L.pl_vit_head_fwd(zd.data_ptr(), T, K, Wd.data_ptr(), bd.data_ptr(), out_d, y.data_ptr(), s()) == 0
        dz, dwb = torch.empty(T, K, device=DEV), torch.empty(out_d * K + out_d, device=DEV)
        scratch = torch.empty(L.pl_vit_head_bwd_scratch_bytes(T, K, out_d), dtype=torch.uint8, device=DEV)
        assert L.pl_vit_head_bwd(dyd.data_ptr(), zd.data_ptr(), T, K, Wd.data_ptr(), out_d, dz.data_ptr(), dwb.data_ptr(),
                                 scratch.data_ptr(), s()) == 0
        torch.cuda.synchronize()
        return y.cpu(), dz.cpu(), dwb[:out_d * K].view(out_d, K).cpu(), dwb[out_d * K:].cpu()

    clean = run(z)
    zp = z.clone()
    zp[1, 17] = nfo.POISONS[poison]
    got, want = run(zp), nfo.vit_head_ref(zp, W, b, dy)
    for name, a, w_ in zip(("y", "dz", "dW", "db"), got, want):
        _assert_mask(a, w_, name)
    y, dz, dW, db = got
    assert nfo.bad(y[1]).all() and nfo.same_bits(y[[0, 2]], clean[0][[0, 2]])
    if poison == "inf":
        assert np.array_equal(nfo.classes(y), nfo.classes(want[0]))
    assert float((dz.double() - want[1]).abs().max()) <= 1e-5 * float(want[1].abs().max())
    other = torch.arange(K) != 17
    assert nfo.same_bits(dW[:, other], clean[2][:, other]) and nfo.same_bits(db, clean[3])


# ================================================================================================== losses
@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("n", nfo.LOSS_SIZES)
def test_mse_loss(pkg, n, poison):
    g = torch.Generator().manual_seed(n)
    p, t = torch.randn(n, generator=g), torch.randn(n, generator=g)

    def run(pin):
        pd = pin.to(DEV).requires_grad_(True)
        loss = pkg.mse_loss(pd, t.to(DEV))
        loss.backward()
        return loss.detach().cpu(), pd.grad.cpu()

    _, dclean = run(p)
    p[n // 2] = nfo.POISONS[poison]
    loss, dp = run(p)
    lref, dref = nfo.mse_ref(p, t)
    assert nfo.classes(loss) == nfo.classes(lref) != 0           # NaN for a NaN, +inf for +inf
    _assert_mask(dp, dref, "dpred")
    keep = torch.arange(n) != n // 2
    assert nfo.classes(dp[n // 2]) == nfo.classes(dref[n // 2]) != 0 and nfo.same_bits(dp[keep], dclean[keep])


def test_l1_terms(pkg):
    """Six terms, a NaN in one: that term is NaN, the others keep their bits, and the gradient at the NaN element is what
    torch.nn.functional.l1_loss gives (sign(NaN) = 0)."""
    sizes = nfo.LOSS_SIZES + [63, 64 * 256 + 1, 2]
    g = torch.Generator().manual_seed(7)
    A, Bs = [torch.randn(n, generator=g) for n in sizes], [torch.randn(n, generator=g) for n in sizes]

    def run(As):
        ta = [a.to(DEV).requires_grad_(True) for a in As]
        tb = [b.to(DEV).requires_grad_(True) for b in Bs]
        losses = pkg.losses.l1_terms(*zip(ta, tb))
        losses.sum().backward()
        return losses.detach().cpu(), [a.grad.cpu() for a in ta], [b.grad.cpu() for b in tb]

    clean = run(A)
    for k in (0, 1, 4):                                          # 1 and 257 elements; one past the 64 x 256 sweep of the grid
        Ap = [a.clone() for a in A]
        Ap[k][sizes[k] // 2] = nfo.NAN
        losses, da, db = run(Ap)
        lref, daref, dbref = nfo.l1_ref(Ap[k], Bs[k])
        bad = np.arange(len(sizes)) == k
        assert np.array_equal(nfo.bad(losses), bad) and np.isnan(lref.item())
        assert nfo.same_bits(losses[~torch.from_numpy(bad)], clean[0][~torch.from_numpy(bad)])
        for j in range(len(sizes)):
            if j != k:
                assert nfo.same_bits(da[j], clean[1][j]) and nfo.same_bits(db[j], clean[2][j])
        assert np.array_equal(da[k].double().numpy(), daref.float().double().numpy())
        assert np.array_equal(db[k].double().numpy(), dbref.float().double().numpy())
        assert da[k][sizes[k] // 2].item() == 0.0 == daref[sizes[k] // 2].item()


@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("B", [1, 257, 64 * 256 + 1])
def test_loss_mpjpe(pkg, B, poison):
    g = torch.Generator().manual_seed(B)
    p, t = torch.randn(B, 17, 3, generator=g), torch.randn(B, 17, 3, generator=g)
    clean = pkg.loss_MPJPE(p.to(DEV), t.to(DEV)).cpu()
    p[B // 2, 6, 1] = nfo.POISONS[poison]
    got, want = pkg.loss_MPJPE(p.to(DEV), t.to(DEV)).cpu(), nfo.mpjpe_ref(p, t)
    _assert_mask(got, want, "metric")
    keep = torch.arange(17) != 6
    assert nfo.classes(got[6]) == nfo.classes(want[6]) != 0 and nfo.same_bits(got[keep], clean[keep])


# ================================================================================================== soft-argmax heads
@pytest.mark.parametrize("poison", POISON)
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_soft_argmax_heads(pkg, layout, poison):
    """One NaN (or +inf: exp(inf - inf)) logit: that (b, j) is NaN in the coordinates and in dlogits, no other pair is
    touched (the clean call's bits).  NCHW on the 8 x 16 x 32 map.  The NHWC head exists for depth 64 alone (head_nhwc
    refuses any other channel count: it reads Model_3D's final convolution in place), so the 8-deep map cannot be given to
    it: 64 x 4 x 8 there, the map of test_soft_argmax_3d_nhwc_with_minus_infinity_logits."""
    J = 17
    D, H, W = (8, 16, 32) if layout == "nchw" else (64, 4, 8)
    g = torch.Generator().manual_seed(21)
    x, dy = torch.randn(2, J * D, H, W, generator=g) * 3, torch.randn(2, J * 3, generator=g)

    def run(xin):
        if layout == "nchw":
            xd = xin.to(DEV).requires_grad_(True)
            c = pkg.soft_argmax_3d(xd, J, D)
            c.backward(dy.to(DEV))
            return c.detach().cpu(), xd.grad.cpu()
        xd = xin.permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
        c = pkg.soft_argmax_3d_nhwc(xd, J)
        c.backward(dy.to(DEV))
        return c.detach().cpu(), xd.grad.permute(0, 3, 1, 2).contiguous().cpu()

    c0, d0 = run(x)
    x[1, 4 * D + 3, H // 2, W // 2] = nfo.POISONS[poison]
    c, d = run(x)
    cref, dref = nfo.soft_argmax_ref(x, J, D, dy)
    _assert_mask(c, cref, "coordinates")
    _assert_mask(d, dref, "dlogits")
    pair = torch.zeros(2, J, dtype=torch.bool)
    pair[1, 4] = True
    assert np.isnan(c.reshape(2, J, 3)[pair].numpy()).all() and np.isnan(d.reshape(2, J, -1)[pair].numpy()).all()
    assert nfo.same_bits(c.reshape(2, J, 3)[~pair], c0.reshape(2, J, 3)[~pair])
    assert nfo.same_bits(d.reshape(2, J, -1)[~pair], d0.reshape(2, J, -1)[~pair])
