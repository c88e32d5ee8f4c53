"""Contiguous inputs that do not start on a 16-byte boundary, on every public entry.

Every other GPU test hands the library fresh allocations (data_ptr() % 256 == 0); a contiguous VIEW -- table[n:], a dropped
first row, table[i * B:(i + 1) * B] -- need not be 16-byte aligned.  Here every caller tensor sits 4, 8 and 12 bytes past a
16-byte boundary (tests/alignment_cases.py) between guard elements.

Python-level cases: outputs, returned gradients, the .grad of the misaligned leaves and every piece of state the call
updates must be torch.equal (on the bits) to the same call on aligned clones from the same seeds, and the guards must be
intact.  Bitwise equality is the right gate whatever a wrapper does with such a view -- hands it to element kernels as it
is, or copies it first (_lib.aligned16): the same kernel on the same values.  The aligned calls themselves are held to
fp64 by the rest of the suite; no tolerance is introduced here.

C-ABI cases behind a launcher's own gate (pl_gemm_f32, pl_gemm_arith, pl_colsum, pl_colsum_planes): the misaligned pointer
goes to the library as it is, takes the element path and is held to the fp64 result at the bound the aligned test uses.
No test here hands a pointer to an entry point that refuses it: the refusals are tested on the host with made-up addresses
(tests/test_alignment_host.py)."""
import numpy as np
import pytest
import torch

import alignment_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _rand(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


# ================================================================================================ the lifter
def _model_state(m):
    return [m.flat_params, m._bn_running, m._bn_batches]


def _grads(m):
    return [p.grad for p in m.parameters() if p.grad is not None]


def _build_lifter(pkg, case, warm=False, opt=False):
    B, H, S, dt, i_dim, o_dim = case

    def build():
        m = pkg.LinearModel(i_dim, o_dim, linear_size=H, num_stage=S, p_dropout=0.5, compute_dtype=dt).to(DEV)
        if warm:                              # running statistics that are not the initial (0, 1): the eval forward has work to do
            m.train()
            with torch.no_grad():
                m(_rand(5, B, i_dim))
        return (m, pkg.FlatAdamW(m, lr=1e-3)) if opt else m
    return build


@pytest.mark.parametrize("case", ac.LIFTER, ids=ac.LIFTER_IDS)
def test_lifter_autograd_forward_backward(pkg, case):
    """model(x) under autograd with x.requires_grad, then backward with a MISALIGNED incoming gradient: y, x.grad, every
    parameter gradient, the BatchNorm buffers.  Dropout 0.5: the masks come from the model's seed, the same in every run."""
    B, H, S, dt, i_dim, o_dim = case

    def call(m, x, gy):
        m.train()
        y = m(x)
        y.backward(gy)
        return [y] + _grads(m) + _model_state(m)
    ref = ac.run_aligned_and_off(_build_lifter(pkg, case), call, [_rand(1, B, i_dim), _randn(2, B, o_dim)], grad_idx=(0,))
    assert ref[-1].abs().max() > 0                                                # (x.grad is not trivially zero)


@pytest.mark.parametrize("case", ac.LIFTER, ids=ac.LIFTER_IDS)
def test_lifter_fused_train_fwd_bwd_and_train_step(pkg, case):
    """fused_train_fwd_bwd (x and the target both off), then two train_step calls with FlatAdamW: loss, prediction, the
    gradient arena, parameters, moments, BatchNorm buffers."""
    B, H, S, dt, i_dim, o_dim = case

    def call(st, x, t):
        m, opt = st
        m.train()
        loss0, y0 = m.fused_train_fwd_bwd(x, t)
        out = [loss0.clone(), y0.clone(), m.flat_grads.clone()]
        for _ in range(2):
            loss, pred = pkg.train_step(m, opt, x, t)
            out += [loss.clone(), pred.clone()]
        return out + _model_state(m) + opt._capture_state()
    ac.run_aligned_and_off(_build_lifter(pkg, case, opt=True), call, [_rand(3, B, i_dim), _randn(4, B, o_dim)])


@pytest.mark.parametrize("case", ac.LIFTER, ids=ac.LIFTER_IDS)
def test_lifter_eval_forward_with_and_without_grad(pkg, case):
    B, H, S, dt, i_dim, o_dim = case

    def call(m, x, gy):
        m.eval()
        with torch.no_grad():
            y0 = m(x)
        y = m(x)                              # eval mode inside an autograd graph: pl_lifter_fwd_eval_saved / _bwd_eval
        y.backward(gy)
        return [y0, y] + _grads(m) + _model_state(m)
    ac.run_aligned_and_off(_build_lifter(pkg, case, warm=True), call, [_rand(6, B, i_dim), _randn(7, B, o_dim)], grad_idx=(0,))


@pytest.mark.parametrize("case", ac.LIFTER[:4], ids=ac.LIFTER_IDS[:4])
def test_lifter_flip_tta_and_eval_step_with_a_meter(pkg, case):
    """predict_flip_tta and eval_step (MSE, loss_MPJPE with out=, a PoseMetrics meter with int32 group ids at a 4-byte
    offset): the meter's three accumulators are state."""
    B, H, S, dt, i_dim, o_dim = case

    def call(m, y1, y2, gid):
        m.eval()
        tta = pkg.predict_flip_tta(m, y1)
        meter = pkg.PoseMetrics(joints=17, groups=3, device=DEV)
        metric = torch.zeros(17, device=DEV)
        loss, met, y2_hat = pkg.eval_step(m, y1, y2, metric_out=metric, meter=meter, group_ids=gid)
        assert met is metric
        loss_f, _, y_f = pkg.eval_step(m, y1, y2, flip=True)
        return [tta, loss, metric, y2_hat, loss_f, y_f, meter.sums, meter.counts, meter.n_poses]
    gid = (torch.arange(B, dtype=torch.int32) % 3).to(DEV)
    ref = ac.run_aligned_and_off(_build_lifter(pkg, case, warm=True), call, [_rand(8, B, 17, 2), _randn(9, B, 17, 3), gid])
    assert int(ref[-1][:3].sum()) == B and int(ref[-1][3]) == 0


def test_lifter_on_rows_of_resident_tables_the_natural_form(pkg):
    """x = table2d[1:1 + B], t = table3d[1:1 + B] on (B + 1, 34) / (B + 1, 51) tables: 8 and 12 bytes off."""
    case = ac.LIFTER[0]
    B = case[0]
    t2, t3 = _rand(10, B + 1, 34), _randn(11, B + 1, 51)
    x, t = t2[1:1 + B], t3[1:1 + B]
    assert t2.data_ptr() % 16 == 0 and t3.data_ptr() % 16 == 0
    assert x.is_contiguous() and t.is_contiguous() and x.data_ptr() % 16 == 8 and t.data_ptr() % 16 == 12

    def run(x, t):
        torch.manual_seed(77)
        m, opt = _build_lifter(pkg, case, opt=True)()
        m.train()
        loss, pred = pkg.train_step(m, opt, x, t)
        m.eval()
        with torch.no_grad():
            y = m(x)
        return [loss, pred, y] + _model_state(m) + opt._capture_state()
    got, ref = run(x, t), run(x.clone(), t.clone())
    assert len(got) == len(ref) and all(ac.same_bits(g, r) for g, r in zip(got, ref))
    assert torch.equal(t2[1:1 + B], x) and torch.equal(t2[0], _rand(10, B + 1, 34)[0])        # the table is untouched


def test_graphed_train_step_replay_fed_misaligned_tensors(pkg):
    case = ac.LIFTER[3]                       # (37, 256, 1): the step carries AdamW
    B, H, S, dt, i_dim, o_dim = case

    def call(st, x, t):
        m, opt = st
        m.train()
        step = pkg.GraphedTrainStep(m, opt, _rand(14, B, i_dim), _randn(15, B, o_dim))      # (aligned examples)
        out = []
        for _ in range(2):
            loss, y = step(x, t)
            out += [loss.clone(), y.clone()]
        return out + _model_state(m) + opt._capture_state()
    ac.run_aligned_and_off(_build_lifter(pkg, case, opt=True), call, [_rand(12, B, i_dim), _randn(13, B, o_dim)])


# ================================================================================================ losses and criteria
B5 = 5


def test_mse_l1_and_mpjpe_losses(pkg):
    def call(_, p, t):
        a = pkg.mse_loss(p, t)
        b = pkg.l1_loss(p, t)
        terms = pkg.l1_terms((p, t), (p * 2.0, t))
        (a + b + terms.sum()).backward()
        m0 = pkg.loss_MPJPE(p, t)
        acc = torch.ones(17, device=DEV)
        assert pkg.loss_MPJPE(p, t, out=acc) is acc
        xf = pkg.PoseTransform(torch.linspace(-1, 1, 51).reshape(17, 3), torch.linspace(0.5, 2, 51).reshape(17, 3))
        return [a, b, terms, m0, acc, pkg.loss_MPJPE(p, t, denorm=xf)]
    ac.run_aligned_and_off(lambda: None, call, [_randn(20, B5, 17, 3), _randn(21, B5, 17, 3)], grad_idx=(0, 1))


def test_mpjpe_out_tensor_off_alignment_accumulates_in_place(pkg):
    """loss_MPJPE(out=) goes to element code: a misaligned accumulator is written in place, never copied."""
    p, t = _randn(22, B5, 17, 3), _randn(23, B5, 17, 3)
    want = pkg.loss_MPJPE(p, t) + 1.0
    for k in ac.OFFSETS:
        ov = ac.OffViews()
        acc = ov.off_view(torch.ones(17, device=DEV), k)
        assert pkg.loss_MPJPE(p, t, out=acc) is acc
        assert torch.equal(acc, want)
        ov.guards_intact(values_too=False)


def test_triangle_loss_and_heatmap_mse(pkg):
    def call(_, p2, p3, l2g, l2p, g2, g3, sq):
        tri = pkg.TriangleLoss(era="lifter")
        loss = tri(p2, p3, l2g, l2p, g2, g3) + pkg.heatmap_mse(sq, 64 ** 3)
        loss.backward()
        return [loss, tri._log[0]]
    ts = [_rand(30, B5, 34), _randn(31, B5, 51), _randn(32, B5, 51), _randn(33, B5, 51), _rand(34, B5, 34), _randn(35, B5, 51),
          _rand(36, B5, 17)]
    ac.run_aligned_and_off(lambda: None, call, ts, grad_idx=(0, 1, 2, 3, 6))


@pytest.mark.parametrize("kind", ["mse", "l1", "smooth_l1", "mpjpe"])
def test_pose_criterion_standing_alone(pkg, kind):
    def build():
        return pkg.PoseCriterion(kind, beta=0.5, joint_weights=torch.linspace(0.0, 2.0, 17), coords=3).to(DEV)

    def call(crit, p, t):
        loss = crit(p, t)
        loss.backward()
        return [loss]
    ac.run_aligned_and_off(build, call, [_randn(40, B5, 17, 3), _randn(41, B5, 17, 3)], grad_idx=(0,))


# ================================================================================================ pose ops
def test_flip_pose_flip_average_crop_and_uncrop(pkg):
    def call(_, a, b, boxes):
        f = pkg.flip_pose(a)
        avg = pkg.flip_average(a, b)
        c = pkg.crop_poses(a, boxes, (256, 256))
        u = pkg.uncrop_poses(c, boxes, (256, 256))
        (f.sum() + (avg * avg).sum() + (c * u).sum()).backward()
        return [f, avg, c, u]
    boxes = torch.tensor([[10.0, 20.0, 110.0, 110.0]] * B5).to(DEV) + _rand(52, B5, 1)        # (x0, y0, side, side)
    ac.run_aligned_and_off(lambda: None, call, [_rand(50, B5, 17, 2), _rand(51, B5, 17, 2), boxes], grad_idx=(0, 1))


def test_flip_frames_nhwc_on_a_dropped_first_frame(pkg):
    frames = _rand(53, 3, 5, 7, 3)
    v = frames[1:]
    assert v.is_contiguous() and v.data_ptr() % 16 == 4                           # one frame is 420 bytes
    assert torch.equal(pkg.flip_frames_nhwc(v), pkg.flip_frames_nhwc(v.clone()))
    assert torch.equal(pkg.flip_frames_nhwc(v), v.flip(2))
    ac.run_aligned_and_off(lambda: None, lambda _, f: [pkg.flip_frames_nhwc(f)], [v.clone()])


# ================================================================================================ metrics
@pytest.mark.parametrize("B", [3, 70])
def test_pose_errors_procrustes_and_meter_update(pkg, B):
    """pose_errors on such views used to raise "not 16-byte aligned" at the caller (pose_errors(pred[1:], tgt[1:]))."""
    def call(_, p, t, gid):
        meter = pkg.PoseMetrics(joints=17, groups=4, device=DEV)
        meter.update(p, t, gid)
        meter.update(p, t)
        xf = pkg.PoseTransform(torch.zeros(17, 3), torch.full((17, 3), 2.0))
        return [pkg.pose_errors(p, t), pkg.procrustes_align(p, t), pkg.pose_errors(p, t, denorm=xf), meter.sums, meter.counts,
                meter.n_poses]
    gid = (torch.arange(B, dtype=torch.int32) % 4).to(DEV)
    ac.run_aligned_and_off(lambda: None, call, [_randn(60, B, 17, 3), _randn(61, B, 17, 3), gid])
    p, t = _randn(62, B + 1, 17, 3), _randn(63, B + 1, 17, 3)
    assert p[1:].data_ptr() % 16 == 12
    assert torch.equal(pkg.pose_errors(p[1:], t[1:]), pkg.pose_errors(p[1:].clone(), t[1:].clone()))


# ================================================================================================ heads
@pytest.mark.parametrize("dims", ac.HEADS_NCHW, ids=lambda d: "B{}D{}H{}W{}".format(*d))
def test_soft_argmax_heads_nchw(pkg, dims):
    B, D, H, W = dims

    def call(_, logits, target, g, gsq):
        if D > 1:
            c0 = pkg.soft_argmax_3d(logits, 17, D)
            c1, sq = pkg.soft_argmax_3d_hm(logits, target, sigma=0.7, num_joints=17, depth_dim=D)
        else:
            c0 = pkg.soft_argmax_2d(logits, 17)
            c1, sq = pkg.soft_argmax_2d_hm(logits, target, sigma=0.7, num_joints=17)
        torch.autograd.backward([c0, c1, sq], [g, g * 0.5, gsq])                  # misaligned incoming gradients
        return [c0, c1, sq]
    nc = 3 if D > 1 else 2
    target = (_rand(71, B, 17 * nc) * 2 - 1) if D > 1 else _rand(71, B, 17 * nc)
    ac.run_aligned_and_off(lambda: None, call, [_randn(70, B, 17 * D, H, W), target, _randn(72, B, 17 * nc), _randn(73, B, 17)],
                           grad_idx=(0,))


@pytest.mark.parametrize("dims", ac.HEADS_NHWC, ids=lambda d: "B{}H{}W{}".format(*d))
def test_soft_argmax_heads_nhwc(pkg, dims):
    B, H, W = dims

    def call(_, logits, target, g, gsq):
        c0 = pkg.soft_argmax_3d_nhwc(logits, 17)
        c1, sq = pkg.soft_argmax_3d_nhwc_hm(logits, target, sigma=0.7, num_joints=17)
        torch.autograd.backward([c0, c1, sq], [g, g * 0.5, gsq])
        return [c0, c1, sq]
    ac.run_aligned_and_off(lambda: None, call, [_randn(74, B, H, W, 17 * 64), _rand(75, B, 51) * 2 - 1, _randn(76, B, 51),
                                                _randn(77, B, 17)], grad_idx=(0,))


# ================================================================================================ MyViT
VIT_SMALLEST = dict(chw=(1, 1, 1), n_blocks=1, hidden_d=64, n_heads=1, out_d=1)        # tests/test_gpu_vit_envelope.py CONFIGS[0]
VIT_LIFT = dict(chw=(1, 17, 2), n_blocks=2, hidden_d=256, n_heads=4, out_d=3)


@pytest.mark.parametrize("mode", ["fp32", "f16x3", "bf16p"])
@pytest.mark.parametrize("cfg,B", [(VIT_SMALLEST, 1), (VIT_LIFT, 3)], ids=["smallest", "lifter-B3"])
def test_myvit_forward_backward(pkg, cfg, B, mode):
    seq, in_d = cfg["chw"][1], cfg["chw"][2]

    def build():
        return pkg.MyViT(compute_dtype=mode, **cfg).to(DEV)

    def call(m, x, gy):
        with torch.no_grad():
            y0 = m(x)
        y = m(x)
        y.backward(gy)
        return [y0, y] + _grads(m)
    ac.run_aligned_and_off(build, call, [_rand(80, B, seq, in_d), _randn(81, B, seq, cfg["out_d"])], grad_idx=(0,))


# ================================================================================================ the conv path
def test_stem_convolution_on_a_dropped_first_frame(pkg):
    """conv2d_nhwc as the stem (7x7 stride 2, Cin 3) on (3, 15, 21, 3)[1:]: a frame is 3780 bytes, frame 1 starts 4 bytes off."""
    frames = _rand(90, 3, 15, 21, 3)
    v = frames[1:]
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    w, s, b = _randn(91, 64, 7, 7, 3) * 0.1, _rand(92, 64) + 0.5, _randn(93, 64)

    def call(_, x, w, s, b):
        y = pkg.conv.conv2d_nhwc(x, w, 2, 3, s, b, relu=1)
        dw = pkg.conv.conv2d_nhwc_wgrad(x, y, 7, 2, 3)
        return [y, dw, pkg.conv.maxpool3x3s2_nhwc(y)]
    assert all(ac.same_bits(g, r) for g, r in zip(call(None, v, w, s, b), call(None, v.clone(), w, s, b)))
    ac.run_aligned_and_off(lambda: None, call, [v.clone(), w, s, b])


def test_direct_convolutions_with_residual_off_alignment(pkg):
    """The implicit-GEMM route (conv_shape_cases "3x3 s2 odd x even": Cin 32, a residual, relu 2) and a transposed
    convolution: x, the filter and the residual all off."""
    def call(_, x, w, resid, xd, wd):
        y = pkg.conv.conv2d_nhwc(x, w, 2, 1, relu=2, resid=resid)
        return [y, pkg.conv.deconv4x4s2_nhwc(xd, wd)]
    ac.run_aligned_and_off(lambda: None, call, [_randn(94, 2, 9, 14, 32), _randn(95, 64, 3, 3, 32) * 0.1, _randn(96, 2, 5, 7, 64),
                                                _randn(97, 1, 3, 5, 32), _randn(98, 4, 16, 2, 2, 32) * 0.1])


def test_conv_building_blocks_with_autograd_off_alignment(pkg):
    """The functional building blocks backbone.py assembles, called with a user's own views: maxpool3x3s2_nhwc_autograd,
    batchnorm_relu_train (BatchNorm buffers are state), add_relu, add_relu_planes and to_planes -- forward, and backward
    with MISALIGNED incoming gradients (conv.add_relu(a, b).backward(g[1:]))."""
    C = 24

    def build():
        bn = torch.nn.BatchNorm2d(C).to(DEV)
        with torch.no_grad():
            bn.weight.copy_(torch.linspace(0.5, 1.5, C))
            bn.bias.copy_(torch.linspace(-0.3, 0.3, C))
        return bn.train()

    def call(bn, x, z, a, b, g_pool, g_bn, g_add, g_addp):
        cv = pkg.conv
        y_pool = cv.maxpool3x3s2_nhwc_autograd(x)
        y_bn = cv.batchnorm_relu_train(z, bn)
        y_add = cv.add_relu(a, b)
        y_addp, carrier = cv.add_relu_planes(a, z)
        planes = cv.to_planes(x)
        torch.autograd.backward([y_pool, y_bn, y_add, y_addp], [g_pool, g_bn, g_add, g_addp])
        return [y_pool, y_bn, y_add, y_addp, carrier, planes, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var,
                bn.num_batches_tracked]
    ts = [_randn(130, 2, 9, 13, C), _randn(131, 2, 5, 7, C), _randn(132, 2, 5, 7, C), _randn(133, 2, 5, 7, C),
          _randn(134, 2, 5, 7, C), _randn(135, 2, 5, 7, C), _randn(136, 2, 5, 7, C), _randn(137, 2, 5, 7, C)]
    ac.run_aligned_and_off(build, call, ts, grad_idx=(0, 1, 2, 3))


def test_batchnorm_join_with_wide_channels_off_alignment(pkg):
    """C = 256: no column replication in the BatchNorm kernels' view, and add_relu's backward with BOTH of its outputs'
    gradients present (the fp32 one and the carrier's), each off alignment."""
    C = 256

    def build():
        return torch.nn.BatchNorm2d(C).to(DEV).train()

    def call(bn, z, a, g, gp):
        y = pkg.conv.batchnorm_relu_train(z, bn, relu=False)
        s, sp = pkg.conv.add_relu_planes(y, a)
        torch.autograd.backward([s, sp], [g, gp])
        return [y, s, sp, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var]
    ts = [_randn(140, 3, 2, 5, C), _randn(141, 3, 2, 5, C), _randn(142, 3, 2, 5, C), _randn(143, 3, 2, 5, C)]
    ac.run_aligned_and_off(build, call, ts, grad_idx=(0, 1))


_M2D = {}


def _model_2d(pkg):
    """ONE Model_2D for the module (building a ResNet-50 takes longer than the test), put back to its saved state for every
    run.  compute_dtype "bf16x6": the direct kernels, where the frames themselves reach the stem kernel (the planes route
    pads them into a pixel-pair view first: a fresh tensor)."""
    if not _M2D:
        m = pkg.Model_2D(compute_dtype="bf16x6")
        m.load_state_dict(pkg.synth.seeded_state(m.state_dict(), 41))
        with torch.no_grad():
            m.final_layer.weight.mul_(1e-3)
        _M2D["m"] = m.to(DEV)
        _M2D["sd"] = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = _M2D["m"]
    m.load_state_dict(_M2D["sd"])
    m.zero_grad(set_to_none=True)
    return m


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_model_2d_on_frames_off_alignment(pkg, train):
    """Model_2D on 64 x 64 NHWC frames (the map tests/test_gpu_conv.py trains it at) that start off alignment: eval, and one
    training forward + backward with a misaligned incoming gradient (BatchNorm buffers are state)."""
    def call(m, frames, g):
        m.train(train)
        if not train:
            return [m.predict_nhwc(frames)]
        out = m.predict_nhwc(frames)
        out.backward(g)
        return [out] + _grads(m) + [b for b in m.buffers()]
    ac.run_aligned_and_off(lambda: _model_2d(pkg), call, [_rand(99, 2, 64, 64, 3), _randn(100, 2, 34)])


# ================================================================================================ feeders and tables
@pytest.mark.parametrize("resident", [True, False], ids=["resident", "streamed"])
def test_pose_feeder_on_tables_off_alignment(pkg, resident):
    N = 11

    def call(_, a, b):
        feeder = pkg.PoseFeeder(a, b, 4, device=DEV, shuffle=True, seed=3, resident=resident)
        out = []
        for y1, y2 in feeder:
            out += [y1.clone(), y2.clone()]
        aug = pkg.PoseFeeder(a, b, 4, device=DEV, seed=3, augment=pkg.PoseAugment(p_flip=0.5, max_rot=0.2, seed=5))
        for y1, y2 in aug:
            out += [y1.clone(), y2.clone()]
        return out
    if resident:
        ac.run_aligned_and_off(lambda: None, call, [_rand(110, N, 17, 2), _randn(111, N, 17, 3)])
    else:                                     # host tables: the views are host memory, pinned and copied by the feeder
        a, b = _rand(110, N, 17, 2).cpu(), _randn(111, N, 17, 3).cpu()
        ref = call(None, a, b)
        for k in ac.OFFSETS:
            ov = ac.OffViews()
            got = call(None, ov.off_view(a, k), ov.off_view(b, k))
            ov.guards_intact()
            assert len(got) == len(ref) and all(ac.same_bits(g, r) for g, r in zip(got, ref))


def test_prepare_poses_pose_stats_and_transform_on_tables_off_alignment(pkg):
    def call(_, raw, table):
        prepared = pkg.prepare_poses(raw, joints=pkg.H36M_17_OF_32, zero_centre=True, device=DEV)
        st = pkg.pose_stats(table)
        xf = pkg.PoseTransform(st.mean, st.std)
        z = xf.apply(table)
        return [prepared, st.mean.to(DEV), st.std.to(DEV), st.min.to(DEV), st.max.to(DEV), z, xf.invert(z)]
    ac.run_aligned_and_off(lambda: None, call, [_randn(120, 6, 32, 3), _randn(121, 9, 17, 3)])


# ================================================================================================ C ABI behind existing gates
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _gemm(pkg, layout, arith, a, b, bias, off, splits=1):
    """One pl_gemm_arith call with the pointers named in `off` moved k elements off a 16-byte boundary (splits > 1: layout 2
    over K slices into aligned slabs, summed into C by launch_reduce_slabs -- its vec gate, reduce.hip:179, is C's).  Gates read from the
    code before this ran: A / B -- gemm_f32.hip a_vec / b_vec (:280) in the edge kernel, operands_vec4 (:1065) keeps a
    misaligned operand off every whole-tile and planes kernel; C -- epilogue_vec_ok (:234), else the element epilogue; bias
    is read by element in both epilogues."""
    M, K = a.shape
    N = b.shape[1]
    ov = ac.OffViews()
    place = lambda t, key: ov.off_view(t, off[key], key) if key in off else t     # noqa: E731
    A = place(_t(a if layout != 2 else a.T), "A")
    Bm = place(_t(b.T if layout == 0 else b), "B")
    C = place(torch.full((M, N), float("nan"), device=DEV), "C")
    bt = place(_t(bias), "bias") if bias is not None else None
    slabs = torch.full((splits, M, N), float("nan"), device=DEV) if splits > 1 else None
    rc = pkg.lib().pl_gemm_arith(layout, arith, A.data_ptr(), Bm.data_ptr(), C.data_ptr(), M, N, K,
                                 bt.data_ptr() if bt is not None else None, splits, slabs.data_ptr() if splits > 1 else None,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, pkg.lib().pl_last_error()
    torch.cuda.synchronize()
    ov.guards_intact(values_too=False)        # (C is the call's output; the inputs are compared below)
    assert torch.equal(A, _t(a if layout != 2 else a.T)) and torch.equal(Bm, _t(b.T if layout == 0 else b))
    return C.cpu().numpy()


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("M,N,K", ac.GEMM_SHAPES)
def test_gemm_f32_with_each_pointer_off_alignment(pkg, layout, M, N, K):
    """tests/test_gpu_parity.py::test_gemm_layouts' own bound, 2e-6 |a| |b| + 1e-6, against the fp64 product."""
    rng = np.random.default_rng(M * 7 + N * 3 + K + layout)
    a = rng.standard_normal((M, K)).astype(np.float32)
    b = rng.standard_normal((K, N)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32) if layout != 2 else None
    want = a.astype(np.float64) @ b.astype(np.float64) + (bias if bias is not None else 0)
    bound = 2e-6 * (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)) + 1e-6
    names = ["A", "B", "C"] + (["bias"] if bias is not None else [])
    for off in [{n: k} for n in names for k in ac.OFFSETS] + [{n: 1 + (i % 3) for i, n in enumerate(names)}]:
        got = _gemm(pkg, layout, pkg._lib.PL_F32, a, b, bias, off)
        err = np.abs(got - want)
        assert np.all(err <= bound), (off, float((err / bound).max()))


@pytest.mark.parametrize("M,N,K,splits", [(128, 128, 512, 4), (51, 130, 777, 5)])
def test_gemm_f32_split_k_with_c_off_alignment(pkg, M, N, K, splits):
    """pl_gemm_f32's slabs route (layout 2, split_k > 1): the slab sum into a misaligned C goes through launch_reduce_slabs'
    element branch ((128, 128): n % 4 == 0, so only C's address decides; (51, 130, 777): ragged everything).  The bound of
    tests/test_gpu_parity.py::test_gemm_tn_split_k."""
    rng = np.random.default_rng(K + splits)
    a = rng.standard_normal((M, K)).astype(np.float32)
    b = rng.standard_normal((K, N)).astype(np.float32)
    want = a.astype(np.float64) @ b.astype(np.float64)
    bound = 2e-6 * (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)) + 1e-6
    for off in [{"C": k} for k in ac.OFFSETS] + [{"A": 1, "B": 2, "C": 3}]:
        err = np.abs(_gemm(pkg, 2, pkg._lib.PL_F32, a, b, None, off, splits=splits) - want)
        assert np.all(err <= bound), (off, float((err / bound).max()))


@pytest.mark.parametrize("arith,tol", [(1, 2e-2), (2, 2e-6)])
@pytest.mark.parametrize("layout,M,N,K", ac.GEMM_ARITH)
def test_gemm_arithmetic_modes_with_each_pointer_off_alignment(pkg, arith, tol, layout, M, N, K):
    """tests/test_gpu_parity.py::test_gemm_bf16_arithmetic_modes' tolerances.  (A misaligned A or B leaves the bf16 / bf16x6
    main loops for the exact-fp32 edge kernel, which is inside both bounds; a misaligned C keeps the arithmetic.)"""
    rng = np.random.default_rng(M + N + K + layout)
    a = rng.standard_normal((M, K)).astype(np.float32)
    b = rng.standard_normal((K, N)).astype(np.float32)
    want = a.astype(np.float64) @ b.astype(np.float64)
    bound = tol * (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)) + 1e-6
    for off in [{n: k} for n in ("A", "B", "C") for k in ac.OFFSETS] + [{"A": 1, "B": 2, "C": 3}]:
        err = np.abs(_gemm(pkg, layout, arith, a, b, None, off) - want)
        assert np.all(err <= bound), (off, float((err / bound).max()))


@pytest.mark.parametrize("rows,cols", [(130, 51), (130, 52), (64, 128), (3000, 128)])
def test_colsum_and_colsum_planes_off_alignment(pkg, rows, cols):
    """pl_colsum with X and out off: conv.hip tests X itself and takes colsum_partial_kernel; out goes through
    launch_reduce_slabs -- its vec gate (reduce.hip:179) for the 1 ... 3 row chunks of the first three shapes, the element
    kernel reduce_rows_kernel for the 47 chunks of (3000, 128).  pl_colsum_planes with out and inv_scale off (its planes are
    refused unless aligned: never passed off).  Against the fp64 sum at the bound of the entry points' existing test
    (tests/test_gpu_conv.py::test_softargmax_bwd_planes_and_colsum_planes_match_the_fp32_forms): 1e-5 max |want|, and for the
    planes max |x| rows 2^-21 on top (what two fp16 planes drop of each value)."""
    L = pkg.lib()
    x = _randn(rows * 1000 + cols, rows, cols)
    want = x.double().sum(0).cpu().numpy()
    bound = 1e-5 * float(np.abs(want).max())
    s = torch.cuda.current_stream().cuda_stream
    for k in ac.OFFSETS:
        ov = ac.OffViews()
        X = ov.off_view(x, k, "X")
        out = ov.off_view(torch.zeros(cols, device=DEV), k, "out")
        scratch = torch.empty(L.pl_colsum_scratch_bytes(rows, cols), dtype=torch.uint8, device=DEV)
        assert L.pl_colsum(X.data_ptr(), rows, cols, out.data_ptr(), scratch.data_ptr(), s) == 0, L.pl_last_error()
        torch.cuda.synchronize()
        ov.guards_intact(values_too=False)
        assert torch.equal(X, x)
        assert float(np.abs(out.cpu().numpy() - want).max()) <= bound, k
        if cols % 4 == 0:
            carrier = pkg.conv._planes_of(x, 1.0)
            ov = ac.OffViews()
            inv = ov.off_view(torch.ones(1, device=DEV), k, "inv_scale")
            out = ov.off_view(torch.zeros(cols, device=DEV), k, "out")
            rc = L.pl_colsum_planes(carrier.data_ptr(), pkg._lib.PL_F16X3, rows, cols, inv.data_ptr(), out.data_ptr(),
                                    scratch.data_ptr(), s)
            assert rc == 0, L.pl_last_error()
            torch.cuda.synchronize()
            ov.guards_intact(values_too=False)
            assert float(np.abs(out.cpu().numpy() - want).max()) <= bound + float(x.abs().max()) * rows * 2.0 ** -21, k
