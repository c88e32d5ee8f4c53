"""GPU tests of the direct convolution route (csrc/conv.hip, the gathering loaders of csrc/gemm_f32.hip, conv.py's dgrad /
wgrad forms) on maps that are NOT square and not even: FrameFeeder(out_hw=...), the frame warp and PersonCrop hand the image
networks frames of any shape, and every kernel here decodes a GEMM row m -> (b, oh, ow) on its own -- a swap of Ho / Wo or
H / W is invisible on the square maps of tests/test_gpu_conv.py and tests/test_gpu_bf16_exact.py.

One case per route (tests/conv_shape_cases.py), the kernel families that ran asserted by name (torch.profiler), the result
against F.conv2d / F.conv_transpose2d in fp64 on the CPU with the bounds the square tests already hold:
    forward            test_conv2d_nhwc_vs_torch's per-element 4e-6 mag |scale| + 1e-6, mag = conv(|x|, |w|)
    dW, dx             test_conv2d_backward_vs_torch_autograd's 2e-5 max|want|
    arith="bf16"       test_gpu_bf16_exact.py's forms around the bf16-rounded operands (inside) and the unrounded ones (outside)
then the stride-2 data gradient on odd maps (the 2 Ho x 2 Wo transposed convolution cropped to H x W), and one whole
Bottleneck on both routes at a rectangular and an odd map."""
import copy
from importlib import import_module

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bf16_oracle as bo
import conv_shape_cases as cs
from test_gpu_bf16_exact import CONV_FAMILIES, _families
from test_gpu_planes import _gpu_kernel_names

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FAMILIES = CONV_FAMILIES + ("stem7x7_c3_wgrad_kernel", "deconv_interleave_kernel", "upsample2x_zero_kernel")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


def _ids(cases):
    return [c[0].replace(" ", "-") for c in cases]


def _dv(t):
    return None if t is None else t.to(DEV)


def _ran(fn):
    """(what fn() returned, the kernel families of FAMILIES it launched)."""
    out = []
    names = _gpu_kernel_names(lambda: out.append(fn()))
    return out[0], _families(names, FAMILIES), names


def _fwd_inputs(geom, bn, res, bias):
    B, H, W, Cin, Cout, k, stride, pad = geom
    Ho, Wo = cs.out_hw(geom)
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + W * 7 + Cin + Cout + k + stride + int(res))
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / np.sqrt(Cin * k * k)
    scale = torch.rand(Cout, generator=g) + 0.5 if bn else None
    shift = torch.randn(Cout, generator=g) if bn else None
    bs = torch.randn(Cout, generator=g) if bias else None
    resid = torch.randn(B, Ho, Wo, Cout, generator=g) if res else None
    return x, w, scale, shift, bs, resid


def _grad_inputs(geom, w_scale=None):
    B, H, W, Cin, Cout, k, stride, pad = geom
    Ho, Wo = cs.out_hw(geom)
    g = torch.Generator().manual_seed(B * 131 + H * 17 + W * 5 + Cin + Cout + k + stride)
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * (w_scale if w_scale is not None else 1.0 / np.sqrt(Cin * k * k))
    dy = torch.randn(B, Ho, Wo, Cout, generator=g)
    return x, w, dy


# ---------------------------------------------------------------------------- 1. the entry points, one case per route
@pytest.mark.parametrize("name,geom,bn,relu,res,bias,kernels,scratch", cs.FWD_CASES, ids=_ids(cs.FWD_CASES))
def test_conv2d_nhwc_rectangular_vs_fp64(pkg, name, geom, bn, relu, res, bias, kernels, scratch):
    """conv2d_nhwc on H != W, the route by kernel name: F.conv2d in fp64 with the epilogue in fp64, per element within
    4e-6 conv(|x|, |w|) |scale| + 1e-6."""
    B, H, W, Cin, Cout, k, stride, pad = geom
    x, w, scale, shift, bs, resid = _fwd_inputs(geom, bn, res, bias)
    y, ran, names = _ran(lambda: pkg.conv.conv2d_nhwc(_dv(x), pkg.conv.to_ohwi(w).to(DEV), stride, pad, _dv(scale), _dv(shift),
                                                      _dv(bs), relu, _dv(resid)))
    assert ran == kernels, (name, sorted(set(names)))
    want, mag = bo.conv_reference(x, w, stride, pad, scale, shift, bs, relu, resid, rounded=False)
    assert tuple(y.shape) == (B, *cs.out_hw(geom), Cout) == tuple(want.shape)
    err = (y.cpu().double() - want).abs()
    bound = 4e-6 * mag + 1e-6
    print(f"{name}: err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), (name, float((err / bound).max()))


@pytest.mark.parametrize("name,geom,kernels,scratch,dgrad", cs.WGRAD_CASES, ids=_ids(cs.WGRAD_CASES))
def test_conv2d_wgrad_and_dgrad_rectangular_vs_fp64(pkg, name, geom, kernels, scratch, dgrad):
    """conv2d_nhwc_wgrad (the gathered TN kernel at Ho != Wo, stride 2, an uneven K split; the im2col fallback; the plain TN
    GEMM; the stem's kernel up to and past the widest row it stages) and conv2d_nhwc_dgrad on the same shapes against torch
    autograd in fp64: 2e-5 max|want| each."""
    B, H, W, Cin, Cout, k, stride, pad = geom
    x, w, dy = _grad_inputs(geom)
    wantx, wantw = bo.conv_grads_reference(x, w, dy, stride, pad, rounded=False)
    dw, ran, names = _ran(lambda: pkg.conv.conv2d_nhwc_wgrad(x.to(DEV), dy.to(DEV), k, stride, pad))
    assert ran == kernels, (name, sorted(set(names)))
    want = wantw.permute(0, 2, 3, 1)                                    # OIHW -> OHWI
    assert dw.shape == want.shape
    ew = float((dw.cpu().double() - want).abs().max()) / (2e-5 * float(want.abs().max()))
    print(f"{name}: dW err / bound = {ew:.3f}")
    assert ew < 1.0, (name, ew)
    if dgrad is None:
        return
    dx, ran, names = _ran(lambda: pkg.conv.conv2d_nhwc_dgrad(dy.to(DEV), pkg.conv.to_ohwi(w).to(DEV), (H, W), stride, pad))
    assert ran == dgrad, (name, sorted(set(names)))
    assert dx.shape == wantx.shape
    ex = float((dx.cpu().double() - wantx).abs().max()) / (2e-5 * float(wantx.abs().max()))
    print(f"{name}: dx err / bound = {ex:.3f}")
    assert ex < 1.0, (name, ex)


@pytest.mark.parametrize("name,geom,kernels", cs.DGRAD_S2_CASES, ids=_ids(cs.DGRAD_S2_CASES))
def test_conv2d_dgrad_1x1_stride2_rectangular_vs_fp64(pkg, name, geom, kernels):
    """The stride-2 downsample's data gradient on an even rectangular map: one GEMM at Ho x Wo spread over the even pixels
    by upsample2x_zero_kernel; 2e-5 max|want|."""
    B, H, W, Cin, Cout, k, stride, pad = geom
    x, w, dy = _grad_inputs(geom)
    wantx, _ = bo.conv_grads_reference(x, w, dy, stride, pad, rounded=False)
    dx, ran, names = _ran(lambda: pkg.conv.conv2d_nhwc_dgrad(dy.to(DEV), pkg.conv.to_ohwi(w).to(DEV), (H, W), stride, pad))
    assert ran == kernels, (name, sorted(set(names)))
    assert dx.shape == wantx.shape
    assert float((dx.cpu().double() - wantx).abs().max()) < 2e-5 * float(wantx.abs().max())


@pytest.mark.parametrize("bn", [False, True], ids=["plain", "bn-relu"])
@pytest.mark.parametrize("B,Hi,Wi,Cin,Cout", cs.DECONV_CASES)
def test_deconv4x4s2_rectangular_vs_fp64(pkg, B, Hi, Wi, Cin, Cout, bn):
    """deconv4x4s2_nhwc on Hi != Wi (the four-parity gather + deconv_interleave_kernel) against
    F.conv_transpose2d(..., 4, 2, 1) in fp64, with and without scale / shift + ReLU: test_deconv4x4s2_vs_torch's
    4e-6 conv_transpose(|x|, |w|) |scale| + 1e-6."""
    g = torch.Generator().manual_seed(Hi * 13 + Wi + Cin + Cout)
    x = torch.randn(B, Hi, Wi, Cin, generator=g)
    w = torch.randn(Cin, Cout, 4, 4, generator=g) / np.sqrt(Cin * 4)
    scale = torch.rand(Cout, generator=g) + 0.5 if bn else None
    shift = torch.randn(Cout, generator=g) if bn else None
    want = F.conv_transpose2d(x.permute(0, 3, 1, 2).double(), w.double(), stride=2, padding=1)
    mag = F.conv_transpose2d(x.permute(0, 3, 1, 2).abs().double(), w.abs().double(), stride=2, padding=1)
    if bn:
        want = (want * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)).clamp_min(0)
        mag = mag * scale.double().view(1, -1, 1, 1)
    got, ran, names = _ran(lambda: pkg.conv.deconv4x4s2_nhwc(x.to(DEV), pkg.conv.deconv_subkernels(w).to(DEV), _dv(scale),
                                                             _dv(shift), 1 if bn else 0))
    assert ran == {"conv_x6_planes_group4_kernel", "deconv_interleave_kernel"}, sorted(set(names))
    assert tuple(got.shape) == (B, 2 * Hi, 2 * Wi, Cout)
    err = (got.cpu().double() - want.permute(0, 2, 3, 1)).abs()
    bound = 4e-6 * mag.permute(0, 2, 3, 1) + 1e-6
    assert bool((err <= bound).all()), float((err / bound).max())


# ---- the same entry points in arith="bf16": one forward, one gathered dW, one stride-2 dx, one transposed convolution
def test_conv2d_nhwc_rectangular_bf16_vs_rounded_operands(pkg):
    """The stride-2 odd x even forward case with arith="bf16" (conv_bf16_planes_kernel): inside 4e-6 mag |scale| + 1e-6 around
    the fp64 result of the bf16-rounded x and w, outside it around the unrounded ones
    (test_conv2d_nhwc_bf16_vs_rounded_operands)."""
    name, geom, bn, relu, res, bias, _, _ = cs.FWD_CASES[1]
    B, H, W, Cin, Cout, k, stride, pad = geom
    x, w, scale, shift, bs, resid = _fwd_inputs(geom, bn, res, bias)
    y, ran, names = _ran(lambda: pkg.conv.conv2d_nhwc(_dv(x), pkg.conv.to_ohwi(w).to(DEV), stride, pad, _dv(scale), _dv(shift),
                                                      _dv(bs), relu, _dv(resid), arith="bf16"))
    assert ran == {"conv_bf16_planes_kernel"}, sorted(set(names))
    y = y.cpu().double()
    inside = {}
    for rounded in (True, False):
        want, mag = bo.conv_reference(x, w, stride, pad, scale, shift, bs, relu, resid, rounded=rounded)
        assert y.shape == want.shape
        inside[rounded] = bool(((y - want).abs() <= 4e-6 * mag + 1e-6).all())
    assert inside[True] and not inside[False], inside


def _grad_ratios(got, want, terms):
    """max error over test_conv2d_nhwc_wgrad_and_dgrad_bf16_vs_rounded_operands' bound 3e-6 max|want| sqrt(terms)."""
    return float((got - want).abs().max()) / (3e-6 * float(want.abs().max()) * terms ** 0.5)


def test_conv2d_wgrad_and_dgrad_rectangular_bf16_vs_rounded_operands(pkg):
    """arith="bf16": dW of the gathered Wo = 8 case (conv_wgrad_x6_planes_kernel with one plane) and dx of the gathered
    stride-2 case (the four-parity transposed convolution with one plane) within 3e-6 max|want| sqrt(terms) of torch's fp64
    gradients on bf16_round(x), bf16_round(w), bf16_round(dy) -- terms = pixels for dW, k k Cout for dx -- and outside it
    around the unrounded operands."""
    name, geom, _, _, _ = cs.WGRAD_CASES[0]
    B, H, W, Cin, Cout, k, stride, pad = geom
    x, w, dy = _grad_inputs(geom, w_scale=0.05)
    dw, ran, names = _ran(lambda: pkg.conv.conv2d_nhwc_wgrad(x.to(DEV), dy.to(DEV), k, stride, pad, arith="bf16"))
    assert ran == {"conv_wgrad_x6_planes_kernel"}, sorted(set(names))
    dw = dw.permute(0, 3, 1, 2).cpu().double()                          # OHWI -> OIHW
    for rounded in (True, False):
        _, wantw = bo.conv_grads_reference(x, w, dy, stride, pad, rounded=rounded)
        ew = _grad_ratios(dw, wantw, B * dy.shape[1] * dy.shape[2])
        print(f"{name}: rounded={rounded} dW err / bound = {ew:.3f}")
        assert (ew <= 1.0) == rounded, (name, rounded, ew)
    name, geom, _, _, _ = cs.WGRAD_CASES[1]
    B, H, W, Cin, Cout, k, stride, pad = geom
    assert stride == 2
    x, w, dy = _grad_inputs(geom, w_scale=0.05)
    dx, ran, names = _ran(lambda: pkg.conv.conv2d_nhwc_dgrad(dy.to(DEV), pkg.conv.to_ohwi(w).to(DEV), (H, W), stride, pad,
                                                            arith="bf16"))
    assert ran == {"conv_x6_planes_group4_kernel", "deconv_interleave_kernel"}, sorted(set(names))
    dx = dx.cpu().double()
    for rounded in (True, False):
        wantx, _ = bo.conv_grads_reference(x, w, dy, stride, pad, rounded=rounded)
        ex = _grad_ratios(dx, wantx, k * k * Cout)
        print(f"{name}: rounded={rounded} dx err / bound = {ex:.3f}")
        assert (ex <= 1.0) == rounded, (name, rounded, ex)


def test_deconv4x4s2_rectangular_bf16_vs_rounded_operands(pkg):
    """deconv4x4s2_nhwc(arith="bf16") on the 4 x 2 map with scale / shift and ReLU: test_deconv4x4s2_nhwc_bf16_vs_rounded_operands'
    3e-6 max|conv| sqrt(4 Cin) |scale| around conv_transpose2d in fp64 on the rounded operands, not around the unrounded."""
    B, Hi, Wi, Cin, Cout = cs.DECONV_CASES[1]
    g = torch.Generator().manual_seed(Hi * 13 + Wi + Cin + Cout)
    x = torch.randn(B, Hi, Wi, Cin, generator=g)
    w = torch.randn(Cin, Cout, 4, 4, generator=g) / np.sqrt(Cin * 4)
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    y, ran, names = _ran(lambda: pkg.conv.deconv4x4s2_nhwc(x.to(DEV), pkg.conv.deconv_subkernels(w).to(DEV), scale.to(DEV),
                                                           shift.to(DEV), 1, arith="bf16"))
    assert ran == {"conv_x6_planes_group4_kernel", "deconv_interleave_kernel"}, sorted(set(names))
    y = y.cpu().double()
    for rounded in (True, False):
        lin = bo.deconv_reference(x, w, rounded=rounded)
        want = (lin * scale.double() + shift.double()).clamp_min(0)
        bound = 3e-6 * float(lin.abs().max()) * (4 * Cin) ** 0.5 * scale.double()
        assert bool(((y - want).abs() <= bound).all()) == rounded, rounded


# ---------------------------------------------------------------------------- 2. stride-2 data gradient on odd maps
# arith="bf16" on the 1x1 case: its GEMM has 40 rows, off the tile grid -- launch_gemm_f32 sends that to the exact-fp32 edge
# kernel whatever arith says (test_gpu_bf16_exact.py, "final 1x1 bias 64px"), so it meets the fp32 bound around the UNROUNDED
# operands and not the bf16 one around the rounded ones
ODD_BF16_ARITHMETIC = {"3x3 9x13": "bf16", "1x1 7x10": "fp32", "3x3 5x8 one odd side": "bf16"}


@pytest.mark.parametrize("arith", ["bf16x6", "bf16"])
@pytest.mark.parametrize("name,geom", cs.DGRAD_ODD_CASES, ids=_ids(cs.DGRAD_ODD_CASES))
def test_conv2d_dgrad_stride2_odd_map_vs_fp64(pkg, name, geom, arith):
    """dx of a 3x3 / pad 1 or 1x1 / pad 0 stride-2 convolution whose input has an odd height or width (layer2.0 ... layer4.0 on
    a 72 x 104 frame: 9 x 13, 5 x 7 maps): the transposed convolution (or GEMM + zero spread) at 2 Ho x 2 Wo, cropped to
    H x W -- the dropped row / column is the padding the forward read as zero.  Against torch autograd in fp64: 2e-5 max|want|
    in bf16x6; in bf16 the 3e-6 max|want| sqrt(k k Cout) of the even case around the rounded operands (and not around the
    unrounded ones), except where the route leaves the bf16 arithmetic (ODD_BF16_ARITHMETIC)."""
    B, H, W, Cin, Cout, k, stride, pad = geom
    assert stride == 2 and (H % 2 or W % 2)
    x, w, dy = _grad_inputs(geom, w_scale=0.05 if arith == "bf16" else None)
    dx, ran, names = _ran(lambda: pkg.conv.conv2d_nhwc_dgrad(dy.to(DEV), pkg.conv.to_ohwi(w).to(DEV), (H, W), stride, pad,
                                                            arith=arith))
    assert ran == ({"conv_x6_planes_group4_kernel", "deconv_interleave_kernel"} if k == 3 else
                   {"gemm_f32_kernel", "upsample2x_zero_kernel"}), sorted(set(names))
    assert tuple(dx.shape) == (B, H, W, Cin) and dx.is_contiguous()
    dx = dx.cpu().double()
    wantx, _ = bo.conv_grads_reference(x, w, dy, stride, pad, rounded=False)
    e32 = float((dx - wantx).abs().max()) / (2e-5 * float(wantx.abs().max()))
    if arith == "bf16x6":
        print(f"{name}: dx err / bound = {e32:.3f}")
        assert e32 < 1.0, (name, e32)
        return
    wantr, _ = bo.conv_grads_reference(x, w, dy, stride, pad, rounded=True)
    er, eu = _grad_ratios(dx, wantr, k * k * Cout), _grad_ratios(dx, wantx, k * k * Cout)
    print(f"{name}: bf16 err / bound = {er:.3f} (rounded operands), {eu:.3f} (unrounded); fp32 bound {e32:.3f}")
    if ODD_BF16_ARITHMETIC[name] == "bf16":
        assert er <= 1.0 and eu > 1.0, (name, er, eu)
    else:
        assert e32 < 1.0 and er > 1.0, (name, e32, er)


def test_conv2d_dgrad_still_refuses_other_geometries(pkg):
    """What conv2d_nhwc_dgrad has no route for says so, naming the geometry: a 5x5 stride-2 kernel, stride 3, a dy that is not
    the stride-2 output of the stated input."""
    dy = torch.zeros(1, 4, 4, 32, device=DEV)
    with pytest.raises(NotImplementedError, match="stride 2, kernel 5x5, padding 2, input 8x8"):
        pkg.conv.conv2d_nhwc_dgrad(dy, torch.zeros(32, 5, 5, 32, device=DEV), (8, 8), 2, 2)
    with pytest.raises(NotImplementedError, match="stride 3"):
        pkg.conv.conv2d_nhwc_dgrad(dy, torch.zeros(32, 3, 3, 32, device=DEV), (12, 12), 3, 1)
    with pytest.raises(NotImplementedError, match="kernel 3x3, padding 0"):
        pkg.conv.conv2d_nhwc_dgrad(dy, torch.zeros(32, 3, 3, 32, device=DEV), (9, 9), 2, 0)
    with pytest.raises(ValueError, match="not the stride-2 output"):
        pkg.conv.conv2d_nhwc_dgrad(dy, torch.zeros(32, 3, 3, 32, device=DEV), (9, 13), 2, 1)


# ---------------------------------------------------------------------------- 3. one Bottleneck, both routes
def _bottleneck_case(pkg, shape):
    """Bottleneck(256, 128, stride 2, downsample) in training mode, its input and output gradient, and the stock module under
    torch autograd on the CPU in `dtype`: (block, x, dy, run) with run(dtype) -> dict of output, dx, parameter gradients and
    running statistics (NHWC / the parameters' own layouts)."""
    torch.manual_seed(3 + shape[1])
    blk = pkg.backbone.Bottleneck(256, 128, stride=2, downsample=nn.Sequential(
        nn.Conv2d(256, 512, kernel_size=1, stride=2, bias=False), nn.BatchNorm2d(512))).train()
    B, H, W, C = shape
    x = torch.randn(B, H, W, C)
    dy = torch.randn(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 512)

    def run(dtype):
        ref = copy.deepcopy(blk).to(dtype)
        xr = x.permute(0, 3, 1, 2).to(dtype).requires_grad_(True)
        o = torch.relu(ref.bn1(ref.conv1(xr)))
        o = torch.relu(ref.bn2(ref.conv2(o)))
        out = torch.relu(ref.bn3(ref.conv3(o)) + ref.downsample(xr))
        out.backward(dy.permute(0, 3, 1, 2).to(dtype))
        return _collect(ref, out.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1))
    return blk, x, dy, run


def _collect(blk, out, dx):
    r = {"out": out, "dx": dx}
    for n, p in blk.named_parameters():
        r["grad:" + n] = p.grad
    for n, b in blk.named_buffers():
        if n.endswith("running_mean") or n.endswith("running_var"):
            r["stat:" + n] = b
    return {k: v.detach().cpu().double() for k, v in r.items()}


def _bottleneck_tol(key):
    """test_bottleneck_train_step_from_the_building_blocks_vs_torch's bounds, relative to max(1, max|ref|)."""
    return 5e-5 if key == "out" else 1e-5 if key.startswith("stat:") else 2e-4


BOTTLENECK_SHAPES = [(2, 8, 16, 256),        # even, rectangular
                     (32, 9, 13, 256)]       # odd: 3,744 input and 1,120 output pixels, both whole 32-row tiles


@pytest.mark.parametrize("route", ["direct-bf16x6", "planes-f16x3"])
@pytest.mark.parametrize("shape", BOTTLENECK_SHAPES, ids=["2x8x16", "32x9x13"])
def test_bottleneck_stride2_train_step_rectangular_and_odd_vs_torch(pkg, shape, route):
    """One stride-2 Bottleneck with its downsample branch (layer3.0's shape in small) in TRAINING mode on both routes of
    ResNet._forward_train -- backbone._bottleneck_train_direct + conv.add_relu at bf16x6, backbone._bottleneck_train_planes at
    f16x3 (where _bottleneck_planes_ok holds at both shapes) -- on a rectangular and on an odd map, where conv2 and the
    downsample take the cropped / zero-spread stride-2 data gradient inside a whole block.  Against the stock module under
    torch autograd in fp64 on the CPU: output (5e-5), dx, every convolution and BatchNorm gradient (2e-4), running mean and
    variance (1e-5), each of max(1, max|ref|) -- the bounds of test_bottleneck_train_step_from_the_building_blocks_vs_torch.
    The distance of stock fp32 from its own fp64 on the same inputs is printed beside each error."""
    cv = import_module("3d_poseestimation_amd.conv")
    blk, x, dy, run = _bottleneck_case(pkg, shape)
    want, floor = run(torch.float64), run(torch.float32)
    b = blk.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    if route.startswith("direct"):
        out = cv.add_relu(*pkg.backbone._bottleneck_train_direct(b, xd, "bf16x6"))
    else:
        assert pkg.backbone._bottleneck_planes_ok(b, tuple(shape))
        mode = pkg._lib.PL_F16X3
        out, _ = pkg.backbone._bottleneck_train_planes(b, xd, cv.to_planes(xd, mode), mode)
    out.backward(dy.to(DEV))
    got = _collect(b, out.detach(), xd.grad)
    assert set(got) == set(want) and len(got) == 2 + 12 + 8
    bad = []
    for k in sorted(want):
        assert got[k].shape == want[k].shape, k
        scale = max(1.0, float(want[k].abs().max()))
        err, fl = float((got[k] - want[k]).abs().max()) / scale, float((floor[k] - want[k]).abs().max()) / scale
        print(f"{route} {tuple(shape)} {k}: err {err:.2e} (bound {_bottleneck_tol(k):.0e}), stock fp32 {fl:.2e}")
        if not err < _bottleneck_tol(k):
            bad.append((k, err, fl))
    assert not bad, bad
