"""GPU tests that hold every route into the bf16 arithmetic (PL_BF16 planes, pl_gemm_arith's arith 1, the bf16-planes
GEMM of launch_gemm_f32, arith="bf16" on the direct convolution kernels, "bf16p" planes convolutions, the lifter in
compute_dtype="bf16") to the bounds of the
fp32-grade rows of the existing tests, around the fp64 result of the bf16-ROUNDED operands (tests/bf16_oracle.py): every
rounding in the library is an RNE `(__bf16)` cast, the products of bf16 values are exact in fp32 and the accumulation is
fp32, so nothing but fp32 accumulation error separates a correct kernel from that reference.  A 2e-2 bound around the
unrounded result -- what these instantiations had -- passes truncation instead of rounding and, at K = 4096, a dropped
k tile (tests/test_bf16_oracle_host.py shows both on these inputs).

Where a route silently leaves the bf16 arithmetic (launch_gemm_f32 sends what is off the tile grid to the exact-fp32
edge kernel; the stem's own kernel is fp32) the case says so: it must then meet the fp32 bound around the UNROUNDED
operands and must not meet the bf16 one."""
from importlib import import_module

import numpy as np
import pytest
import torch

import bf16_oracle as bo
from test_gpu_planes import PLANES_FAMILIES, ROUTE_CASES, _gpu_kernel_names, _ncu, _planes_families, _planes_gemm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PL_BF16 = 1


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


@pytest.fixture(scope="module")
def cv(pkg):
    return import_module("3d_poseestimation_amd.conv")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _families(names, families):
    """The kernel templates of `families` among launched kernel names (no identifier is a substring of another)."""
    return {f for f in families for n in names if f in n}


def _gemm_ref_on_device(a, b, bias, rounded, tol=2e-6, floor=1e-7, bias_in_mag=True):
    """(want, bound) in fp64 on the device: operands rounded to bf16 first (rounded) or as they are."""
    q = bo.bf16_round if rounded else (lambda v: v)
    a64, b64 = q(_t(a)).double(), q(_t(b)).double()
    bias64 = _t(bias).double() if bias is not None else torch.zeros(b.shape[1], dtype=torch.float64, device=DEV)
    want = a64 @ b64 + bias64
    bound = tol * (a64.abs() @ b64.abs() + (bias64.abs() if bias_in_mag else 0.0)) + floor
    return want, bound


# ---------------------------------------------------------------------------- 2.1 raw GEMMs
def _planes_cases():
    out = [(name, kernel, layout, rows, N, K) for name, kernel, layout, rows, N, K in ROUTE_CASES]
    for layout, M, N, K in bo.PLANES_GEMM_CASES:
        # (the route of these shapes is not the subject: whichever planes family runs, and only planes families)
        out.append((f"{'NT NN TN'.split()[layout]} {M}x{N}x{K}", None, layout, (lambda m: (lambda n: m))(M), N, K))
    return out


PLANES_CASES = _planes_cases()


@pytest.mark.parametrize("name,kernel,layout,rows,N,K", PLANES_CASES, ids=[c[0].replace(" ", "-") for c in PLANES_CASES])
def test_planes_gemm_bf16_vs_rounded_operands(pkg, name, kernel, layout, rows, N, K):
    """pl_gemm_planes in PL_BF16 on every row of test_planes_gemm_routes' table (the kernel family by name) and on one
    whole-tile and one overhanging shape per layout of test_planes_gemm_vs_fp64 plus one long contraction per pipeline
    phase: bf16_round(a) @ bf16_round(b) + bias in fp64 within the f16x3 row's bound of those tests,
    2e-6 (|a_r| @ |b_r| + |bias|) + 1e-7 (reference and bound formed in fp64 on the device)."""
    M = rows(_ncu())
    a, b, bias = bo.gemm_inputs(layout, M, N, K)
    got = []
    names = _gpu_kernel_names(lambda: got.append(_planes_gemm(pkg, layout, PL_BF16, a, b, bias, sa=1.0, sb=16.0)))
    ran = _planes_families(names)
    assert ran == {kernel} if kernel else (len(ran) == 1 and ran <= set(PLANES_FAMILIES)), (name, names)
    want, bound = _gemm_ref_on_device(a, b, bias, rounded=True)
    err = (_t(got[0]).double() - want).abs()
    print(f"{name}: err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), (name, float((err / bound).max()))
    # ... and really one bf16 product: the unrounded result is outside the same bound somewhere
    want32, bound32 = _gemm_ref_on_device(a, b, bias, rounded=False)
    assert not bool(((_t(got[0]).double() - want32).abs() <= bound32).all()), name


F32_FAMILIES = ("gemm_f32_kernel", "gemm_x6_planes_kernel", "gemm_x6_planes_nedge_kernel", "gemm_bf16_planes_kernel",
                "gemm_f32_dual_kernel", "gemm_x6_planes_dual_kernel", "thin_gemm_kernel")

# (name, layout, M, N, K, splits, the arithmetic f32_route prescribes for a kArithBf16 problem of this shape)
ARITH_CASES = [(f"whole {'NT NN TN'.split()[lay]} {M}x{N}x{K}", lay, M, N, K, 1, "bf16")
               for lay in (0, 1, 2) for M, N, K in ((128, 128, 32), (256, 384, 96))] + [
    ("TN split-K", 2, 128, 128, 256, 2, "bf16"),
    # off the tile grid: gemm_body's EDGE form has no bf16 main loop -- f32_route sends the problem to the exact-fp32
    # edge kernel (r.ar = 0 whatever a.arith says)
    ("ragged NT", 0, 130, 72, 40, 1, "fp32"),
    ("ragged NN", 1, 130, 51, 34, 1, "fp32"),
    ("ragged TN", 2, 130, 51, 34, 1, "fp32"),
]


@pytest.mark.parametrize("name,layout,M,N,K,splits,arith", ARITH_CASES, ids=[c[0].replace(" ", "-") for c in ARITH_CASES])
def test_gemm_arith_bf16_vs_rounded_operands(pkg, name, layout, M, N, K, splits, arith):
    """pl_gemm_arith with arith 1 (kArithBf16) runs gemm_f32_kernel: on whole tiles its AR = 1 main loop -- the
    rounded-operand result within 2e-6 (|a_r| @ |b_r| + |bias|) + 1e-7 --, off the tile grid the exact-fp32 edge form:
    there test_gemm_layouts' fp32 bound 2e-6 |a| @ |b| + 1e-6 around the UNROUNDED operands holds and the bf16 bound does
    not."""
    a, b, bias = bo.gemm_inputs(layout, M, N, K, b_scale=1.0)
    if splits > 1:
        bias = None                                            # (the split launch takes no bias)
    A = _t(a if layout != 2 else a.T)
    Bm = _t(b.T if layout == 0 else b)
    C = torch.full((M, N), float("nan"), device=DEV)
    bt = _t(bias) if bias is not None else None
    slabs = torch.full((splits, M, N), float("nan"), device=DEV) if splits > 1 else None

    def run():
        rc = pkg.lib().pl_gemm_arith(layout, 1, A.data_ptr(), Bm.data_ptr(), C.data_ptr(), M, N, K,
                                     bt.data_ptr() if bt is not None else None, splits,
                                     slabs.data_ptr() if splits > 1 else None, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, pkg.lib().pl_last_error()
    assert _families(_gpu_kernel_names(run), F32_FAMILIES) == {"gemm_f32_kernel"}, name
    want_r, bound_r = _gemm_ref_on_device(a, b, bias, rounded=True)
    want_u, bound_u = _gemm_ref_on_device(a, b, bias, rounded=False, floor=1e-6, bias_in_mag=False)
    in_r = (C.double() - want_r).abs() <= bound_r
    in_u = (C.double() - want_u).abs() <= bound_u
    print(f"{name}: in rounded bound {float(in_r.double().mean()):.4f}, in unrounded bound {float(in_u.double().mean()):.4f}")
    if arith == "bf16":
        assert bool(in_r.all()) and not bool(in_u.all()), name
    else:
        assert bool(in_u.all()) and not bool(in_r.all()), name


@pytest.mark.parametrize("Cout", [128, 72])
def test_conv1x1_bf16_planes_gemm_vs_rounded_operands(pkg, Cout):
    """gemm_bf16_planes_kernel, the route of launch_gemm_f32 that pl_gemm_arith cannot select: a 1x1 convolution with
    arith="bf16" on 128 pixels, whole and ragged N (inputs of test_conv1x1_bf16_takes_the_bf16_planes_gemm)."""
    rng = np.random.default_rng(Cout)
    x = rng.standard_normal((2, 8, 8, 32)).astype(np.float32)
    w = rng.standard_normal((Cout, 1, 1, 32)).astype(np.float32)
    got = []
    names = _gpu_kernel_names(lambda: got.append(pkg.conv.conv2d_nhwc(_t(x), _t(w), arith="bf16")))
    assert _families(names, F32_FAMILIES) == {"gemm_bf16_planes_kernel"}, names
    a, b = x.reshape(128, 32), np.ascontiguousarray(w.reshape(Cout, 32).T)
    want, bound = _gemm_ref_on_device(a, b, None, rounded=True)
    err = (got[0].reshape(128, Cout).double() - want).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    want_u, bound_u = _gemm_ref_on_device(a, b, None, rounded=False)
    assert not bool(((got[0].reshape(128, Cout).double() - want_u).abs() <= bound_u).all())


# ---------------------------------------------------------------------------- 2.2 direct conv kernels, arith="bf16"
CONV_FAMILIES = ("conv_bf16_planes_kernel", "conv_x6_planes_kernel", "conv_wgrad_x6_planes_kernel",
                 "conv_x6_planes_group4_kernel", "stem7x7_c3_kernel", "im2col_nhwc_kernel", "reduce_slabs_epi_kernel") + F32_FAMILIES

# (name, B, H, Cin, Cout, k, stride, pad, bn, relu, res, bias, kernels, arithmetic) -- rows of test_conv2d_nhwc_vs_torch's
# table at their sizes there or smaller
CONV_FWD_CASES = [
    ("3x3 s1", 2, 16, 128, 128, 3, 1, 1, True, 1, False, False, {"conv_bf16_planes_kernel"}, "bf16"),
    ("3x3 s2", 2, 16, 128, 128, 3, 2, 1, True, 1, False, False, {"conv_bf16_planes_kernel"}, "bf16"),
    ("3x3 residual relu", 2, 16, 256, 256, 3, 1, 1, True, 2, True, False, {"conv_bf16_planes_kernel"}, "bf16"),
    ("1x1 s2 bn", 2, 16, 256, 512, 1, 2, 0, True, 0, False, False, {"conv_bf16_planes_kernel"}, "bf16"),
    # the final 1x1: a plain GEMM.  128 pixels take the bf16-planes GEMM (ragged N: 1088 = 8.5 tiles); the row of
    # test_conv2d_nhwc_vs_torch (one 8x8 frame: 64 pixels, M off the tile grid) leaves bf16 for the exact-fp32 edge kernel
    ("final 1x1 bias 128px", 2, 8, 256, 1088, 1, 1, 0, False, 0, False, True, {"gemm_bf16_planes_kernel"}, "bf16"),
    ("final 1x1 bias 64px", 1, 8, 256, 1088, 1, 1, 0, False, 0, False, True, {"gemm_f32_kernel"}, "fp32"),
    ("8x8 borders", 4, 8, 64, 128, 3, 1, 1, False, 0, False, False, {"conv_bf16_planes_kernel"}, "bf16"),
    ("nothing aligned", 3, 10, 32, 40, 3, 2, 1, False, 2, True, True, {"conv_bf16_planes_kernel"}, "bf16"),
    # bf16x6 splits K for this shape (conv_fwd_splits); PL_BF16 never splits: one launch with the epilogue in the kernel
    ("layer4 no split-K", 4, 8, 512, 512, 3, 1, 1, True, 2, True, False, {"conv_bf16_planes_kernel"}, "bf16"),
    # the stem as the backbone calls it has its own exact-fp32 kernel whatever arith says ...
    ("stem", 2, 32, 3, 64, 7, 2, 3, True, 1, False, False, {"stem7x7_c3_kernel"}, "fp32"),
    # ... with an epilogue that kernel does not fold, im2col + the bf16-planes GEMM (K = 147 padded to 160; ragged N = 64)
    ("stem unfolded epilogue", 2, 32, 3, 64, 7, 2, 3, True, 2, True, False, {"im2col_nhwc_kernel", "gemm_bf16_planes_kernel"},
     "bf16"),
    ("64 to 64", 2, 16, 64, 64, 3, 1, 1, True, 1, False, False, {"conv_bf16_planes_kernel"}, "bf16"),
]


def _conv_inputs(B, H, Cin, Cout, k, stride, pad, bn, res, bias):
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + Cin + Cout + k + stride)
    x = torch.randn(B, H, H, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / np.sqrt(Cin * k * k)
    Ho = (H + 2 * pad - k) // stride + 1
    scale = torch.rand(Cout, generator=g) + 0.5 if bn else None
    shift = torch.randn(Cout, generator=g) if bn else None
    bs = torch.randn(Cout, generator=g) if bias else None
    resid = torch.randn(B, Ho, Ho, Cout, generator=g) if res else None
    return x, w, scale, shift, bs, resid


@pytest.mark.parametrize("name,B,H,Cin,Cout,k,stride,pad,bn,relu,res,bias,kernels,arith", CONV_FWD_CASES,
                         ids=[c[0].replace(" ", "-") for c in CONV_FWD_CASES])
def test_conv2d_nhwc_bf16_vs_rounded_operands(pkg, name, B, H, Cin, Cout, k, stride, pad, bn, relu, res, bias, kernels, arith):
    """conv2d_nhwc(arith="bf16"): F.conv2d in fp64 on bf16_round(x) and bf16_round(w), epilogue in fp64, within
    test_conv2d_nhwc_vs_torch's 4e-6 mag |scale| + 1e-6 (mag from the rounded operands).  Each case names the kernels
    that run and the arithmetic the route prescribes; an "fp32" case meets that bound around the unrounded operands and
    not around the rounded ones, a "bf16" case the other way round."""
    x, w, scale, shift, bs, resid = _conv_inputs(B, H, Cin, Cout, k, stride, pad, bn, res, bias)
    dv = lambda t: None if t is None else t.to(DEV)                                  # noqa: E731
    got = []
    names = _gpu_kernel_names(lambda: got.append(pkg.conv.conv2d_nhwc(
        dv(x), pkg.conv.to_ohwi(w).to(DEV), stride, pad, dv(scale), dv(shift), dv(bs), relu, dv(resid), arith="bf16")))
    assert _families(names, CONV_FAMILIES) == kernels, (name, names)
    y = got[0].cpu().double()
    inside = {}
    for rounded in (True, False):
        want, mag = bo.conv_reference(x, w, stride, pad, scale, shift, bs, relu, resid, rounded=rounded)
        assert y.shape == want.shape
        err = (y - want).abs()
        bound = 4e-6 * mag + 1e-6
        inside[rounded] = bool((err <= bound).all())
        print(f"{name}: rounded={rounded} err / bound = {float((err / bound).max()):.3f}")
    assert inside[arith == "bf16"] and not inside[arith != "bf16"], (name, inside)


def test_conv2d_nhwc_bf16_is_not_split_over_k(pkg):
    """(4, 8, 512, 512, 3x3): the fp32-grade arithmetic cuts K into slices summed by reduce_slabs_epi_kernel
    (conv_fwd_splits); conv_fwd_check refuses slices for PL_BF16, and conv_core asks for none: the Python side sizes the
    scratch for the split all the same (pl_conv2d_nhwc_scratch_bytes_ex does not know the arithmetic) and the bf16 call
    leaves it unused -- one conv_bf16_planes_kernel launch (its result: the "layer4 no split-K" case above)."""
    x, w, scale, shift, _, resid = _conv_inputs(4, 8, 512, 512, 3, 1, 1, True, True, False)
    wd, args = pkg.conv.to_ohwi(w).to(DEV), (1, 1, scale.to(DEV), shift.to(DEV), None, 2, resid.to(DEV))
    assert pkg.lib().pl_conv2d_nhwc_scratch_bytes_ex(4, 8, 8, 512, 512, 3, 3, 1, 1, 0, 1, 2) > 0
    split = _families(_gpu_kernel_names(lambda: pkg.conv.conv2d_nhwc(x.to(DEV), wd, *args, arith="bf16x6")), CONV_FAMILIES)
    assert split == {"conv_x6_planes_kernel", "reduce_slabs_epi_kernel"}, split
    whole = _families(_gpu_kernel_names(lambda: pkg.conv.conv2d_nhwc(x.to(DEV), wd, *args, arith="bf16")), CONV_FAMILIES)
    assert whole == {"conv_bf16_planes_kernel"}, whole


# (name, B, H, Cin, Cout, k, stride, pad, does the weight gradient run the gathered bf16 kernel)
GRAD_CASES = [("aligned", 2, 16, 128, 128, 3, 1, 1, True),     # 512 pixels, whole tiles everywhere
              ("ragged", 3, 16, 32, 64, 3, 2, 1, True),        # 192 output pixels, Cout = 64, 9 x 32 = 288 columns: tiles overhang
              # output rows of 10 pixels: the gathered weight-gradient kernel wants Wo % 8 == 0 -- pl_conv2d_nhwc_wgrad falls
              # back to im2col + the generic TN GEMM, which "stays fp32-grade" (conv.hip) whatever arith says; dx is bf16
              ("wgrad fallback", 2, 10, 32, 64, 3, 1, 1, False)]


@pytest.mark.parametrize("name,B,H,Cin,Cout,k,stride,pad,dw_bf16", GRAD_CASES, ids=[c[0].replace(" ", "-") for c in GRAD_CASES])
def test_conv2d_nhwc_wgrad_and_dgrad_bf16_vs_rounded_operands(pkg, name, B, H, Cin, Cout, k, stride, pad, dw_bf16):
    """conv2d_nhwc_wgrad / conv2d_nhwc_dgrad with arith="bf16" (the gathered TN kernel with one plane; the forward kernel
    on dy with the flipped filter for stride 1, the four-parity transposed convolution for stride 2): torch's fp64
    gradients of conv2d on bf16_round(x), bf16_round(w), bf16_round(dy), within the planes tests' 3e-6 max|want|
    sqrt(terms) (test_conv_planes_fwd_dgrad_wgrad_vs_torch_fp64: terms = pixels for dW, k k Cout for dx)."""
    g = torch.Generator().manual_seed(B * 131 + H * 17 + Cin + Cout + k)
    x = torch.randn(B, H, H, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * 0.05
    Ho = (H + 2 * pad - k) // stride + 1
    dy = torch.randn(B, Ho, Ho, Cout, generator=g)
    got = {}
    names = _gpu_kernel_names(lambda: got.update(dw=pkg.conv.conv2d_nhwc_wgrad(x.to(DEV), dy.to(DEV), k, stride, pad, arith="bf16")))
    ran = _families(names, CONV_FAMILIES)
    assert ran == {"conv_wgrad_x6_planes_kernel"} if dw_bf16 else ("im2col_nhwc_kernel" in ran and
                                                                    "conv_wgrad_x6_planes_kernel" not in ran), names
    names = _gpu_kernel_names(lambda: got.update(dx=pkg.conv.conv2d_nhwc_dgrad(
        dy.to(DEV), pkg.conv.to_ohwi(w).to(DEV), (H, H), stride, pad, arith="bf16")))
    assert _families(names, CONV_FAMILIES) == {"conv_bf16_planes_kernel" if stride == 1 else "conv_x6_planes_group4_kernel"}, names
    dw = got["dw"].permute(0, 3, 1, 2).cpu().double()                   # OHWI -> OIHW
    dx = got["dx"].cpu().double()
    for rounded in (True, False):
        wantx, wantw = bo.conv_grads_reference(x, w, dy, stride, pad, rounded=rounded)
        ew = float((dw - wantw).abs().max()) / (3e-6 * float(wantw.abs().max()) * (B * Ho * Ho) ** 0.5)
        ex = float((dx - wantx).abs().max()) / (3e-6 * float(wantx.abs().max()) * (k * k * Cout) ** 0.5)
        print(f"{name}: rounded={rounded} dW err / bound = {ew:.3f}, dx err / bound = {ex:.3f}")
        assert (ex <= 1.0) == rounded and (ew <= 1.0) == (rounded == dw_bf16), (name, rounded, ew, ex)


@pytest.mark.parametrize("B,Hi,Cin,Cout", [(2, 8, 64, 128), (3, 5, 32, 40)], ids=["aligned", "ragged"])
def test_deconv4x4s2_nhwc_bf16_vs_rounded_operands(pkg, B, Hi, Cin, Cout):
    """deconv4x4s2_nhwc(arith="bf16") with BatchNorm scale / shift and ReLU (the group-of-four gather kernel with one
    plane): conv_transpose2d in fp64 on the rounded operands, the epilogue in fp64; bound of
    test_deconv_planes_fwd_dgrad_wgrad_vs_torch_fp64, 3e-6 max|conv| sqrt(4 Cin), times |scale|."""
    g = torch.Generator().manual_seed(Hi + Cin + Cout)
    x = torch.randn(B, Hi, Hi, Cin, generator=g)
    w = torch.randn(Cin, Cout, 4, 4, generator=g) / np.sqrt(Cin * 4)
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    got = []
    names = _gpu_kernel_names(lambda: got.append(pkg.conv.deconv4x4s2_nhwc(
        x.to(DEV), pkg.conv.deconv_subkernels(w).to(DEV), scale.to(DEV), shift.to(DEV), 1, arith="bf16")))
    assert _families(names, CONV_FAMILIES) == {"conv_x6_planes_group4_kernel"}, names
    y = got[0].cpu().double()
    for rounded in (True, False):
        lin = bo.deconv_reference(x, w, rounded=rounded)
        want = (lin * scale.double() + shift.double()).clamp_min(0)
        bound = 3e-6 * float(lin.abs().max()) * (4 * Cin) ** 0.5 * scale.double()
        err = (y - want).abs()
        print(f"deconv {B}x{Hi}x{Cin}x{Cout}: rounded={rounded} err / bound = {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()) == rounded


# ---------------------------------------------------------------------------- 2.3 planes convolutions, PL_BF16
def _bf16_planes(cv, t):
    return cv._planes_of(t, 1.0, PL_BF16)


def _decode_bf16_plane(carrier):
    """The values of a PL_BF16 carrier: one bf16 plane in the first half of its bytes."""
    n = carrier.numel()
    return carrier.reshape(-1).view(torch.bfloat16)[:n].float().reshape(carrier.shape)


@pytest.mark.parametrize("B,H,W,Cin,Cout,K,stride,pad", [
    (2, 16, 16, 64, 64, 3, 1, 1), (2, 16, 24, 32, 128, 3, 2, 1), (2, 8, 8, 128, 72, 1, 2, 0), (3, 9, 7, 64, 96, 3, 1, 1),
    (1, 32, 32, 96, 256, 3, 1, 1)])
def test_conv_planes_bf16_fwd_dgrad_wgrad_vs_rounded_operands(pkg, cv, B, H, W, Cin, Cout, K, stride, pad):
    """The body of test_conv_planes_fwd_dgrad_wgrad_vs_torch_fp64 at its shapes with mode PL_BF16 (the MODE = kBf16
    instantiations of the gathered forward, data-gradient and weight-gradient kernels): planes from
    _planes_of(t, 1, PL_BF16), output scale 1, against conv2d in fp64 on the rounded x, w and dz with that test's own
    f16x3 bounds; the epilogue statistics by its 1e-4 rule against the statistics of the reference output."""
    L = pkg.lib()
    g = torch.Generator().manual_seed(B * 131 + H * 17 + Cin + Cout + K)
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(Cout, K, K, Cin, generator=g) * 0.05
    Ho, Wo = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    dz = torch.randn(B, Ho, Wo, Cout, generator=g)
    xd, wd, dzd = x.to(DEV), w.to(DEV), dz.to(DEV)
    xp, wp, dzp = _bf16_planes(cv, xd), _bf16_planes(cv, wd), _bf16_planes(cv, dzd)
    assert torch.equal(_decode_bf16_plane(xp), bo.bf16_round(xd))          # the planes ARE the RNE rounding
    s = torch.cuda.current_stream().cuda_stream
    y = torch.full((B, Ho, Wo, Cout), float("nan"), device=DEV)
    G = L.pl_gemm_stat_groups(B * Ho * Wo)
    stat = torch.full((2, G, Cout), float("nan"), device=DEV)
    rc = L.pl_conv2d_planes_fwd(PL_BF16, xp.data_ptr(), x.numel(), B, H, W, Cin, wp.data_ptr(), w.numel(), Cout,
                                K, K, stride, pad, y.data_ptr(), 1.0, None, stat.data_ptr(), s)
    assert rc == 0, L.pl_last_error()
    w_oihw = w.permute(0, 3, 1, 2)
    ref, mag = bo.conv_reference(x, w_oihw, stride, pad)
    err = (y.cpu().double() - ref).abs()
    assert bool((err <= 2e-6 * mag + 1e-7).all()), float((err / (2e-6 * mag + 1e-7)).max())
    ref_u, mag_u = bo.conv_reference(x, w_oihw, stride, pad, rounded=False)
    assert not bool(((y.cpu().double() - ref_u).abs() <= 2e-6 * mag_u + 1e-7).all())       # really bf16 operands
    r2 = ref.reshape(-1, Cout)
    for gi in range(G):
        blk = r2[64 * gi:64 * (gi + 1)]
        want_s = blk.sum(0) if len(blk) else torch.zeros(Cout, dtype=torch.float64)
        want_q = ((blk - blk.mean(0)) ** 2).sum(0) if len(blk) else torch.zeros(Cout, dtype=torch.float64)
        assert float((stat[0, gi].cpu().double() - want_s).abs().max()) <= 1e-4 * max(1.0, float(want_s.abs().max()))
        assert float((stat[1, gi].cpu().double() - want_q).abs().max()) <= 1e-4 * max(1.0, float(want_q.abs().max()))
    wantx, wantw = bo.conv_grads_reference(x, w_oihw, dz, stride, pad)
    if stride == 1:
        wf = w.flip(1, 2).permute(3, 1, 2, 0).contiguous().to(DEV)            # [Cin][KH][KW][Cout]
        wfp = _bf16_planes(cv, wf)
        dx = torch.full((B, H, W, Cin), float("nan"), device=DEV)
        rc = L.pl_conv2d_planes_fwd(PL_BF16, dzp.data_ptr(), dz.numel(), B, Ho, Wo, Cout, wfp.data_ptr(), wf.numel(),
                                    Cin, K, K, 1, K - 1 - pad, dx.data_ptr(), 1.0, None, None, s)
        assert rc == 0, L.pl_last_error()
        assert float((dx.cpu().double() - wantx).abs().max()) <= 3e-6 * float(wantx.abs().max()) * (K * K * Cout) ** 0.5
    if (B * Ho * Wo) % 32 == 0:
        n = Cout * K * K * Cin
        splits = L.pl_gemm_planes_splits(Cout, K * K * Cin, B * Ho * Wo)
        slabs = torch.empty(splits * n, device=DEV) if splits > 1 else None
        dw = torch.full((Cout, K, K, Cin), float("nan"), device=DEV)
        rc = L.pl_conv2d_planes_wgrad(PL_BF16, dzp.data_ptr(), dz.numel(), xp.data_ptr(), x.numel(), B, H, W, Cin, Cout,
                                      K, K, stride, pad, dw.data_ptr(), 1.0, None, slabs.data_ptr() if slabs is not None else None, s)
        assert rc == 0, L.pl_last_error()
        want = wantw.permute(0, 2, 3, 1)
        assert float((dw.cpu().double() - want).abs().max()) <= 3e-6 * float(want.abs().max()) * (B * Ho * Wo) ** 0.5


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 8, 8, 64, 128), (1, 6, 10, 96, 64), (3, 4, 4, 256, 256)])
def test_deconv_planes_bf16_fwd_dgrad_wgrad_vs_rounded_operands(pkg, cv, B, H, W, Cin, Cout):
    """The body of test_deconv_planes_fwd_dgrad_wgrad_vs_torch_fp64 at its shapes with mode PL_BF16, against
    conv_transpose2d in fp64 on the rounded x, w and dy with that test's bounds."""
    L = pkg.lib()
    g = torch.Generator().manual_seed(B + 7 * H + Cin + 3 * Cout)
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(Cin, Cout, 4, 4, generator=g) * 0.05
    dy = torch.randn(B, 2 * H, 2 * W, Cout, generator=g)
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
    s = torch.cuda.current_stream().cuda_stream
    xp, dyp = _bf16_planes(cv, xd), _bf16_planes(cv, dyd)
    wsub = _bf16_planes(cv, cv.deconv_subkernels(wd))
    y = torch.full((B, 2 * H, 2 * W, Cout), float("nan"), device=DEV)
    rc = L.pl_deconv4x4s2_planes_fwd(PL_BF16, xp.data_ptr(), x.numel(), B, H, W, Cin, wsub.data_ptr(), wsub.numel(), Cout,
                                     y.data_ptr(), 1.0, None, s)
    assert rc == 0, L.pl_last_error()
    want, wantx, wantw = bo.deconv_reference(x, w, dy)
    assert float((y.cpu().double() - want).abs().max()) <= 3e-6 * float(want.abs().max()) * (4 * Cin) ** 0.5
    want_u = bo.deconv_reference(x, w, rounded=False)
    assert float((y.cpu().double() - want_u).abs().max()) > 3e-6 * float(want_u.abs().max()) * (4 * Cin) ** 0.5
    wc = _bf16_planes(cv, wd.permute(0, 2, 3, 1))
    dx = torch.full((B, H, W, Cin), float("nan"), device=DEV)
    rc = L.pl_conv2d_planes_fwd(PL_BF16, dyp.data_ptr(), dy.numel(), B, 2 * H, 2 * W, Cout, wc.data_ptr(), w.numel(), Cin, 4, 4,
                                2, 1, dx.data_ptr(), 1.0, None, None, s)
    assert rc == 0, L.pl_last_error()
    assert float((dx.cpu().double() - wantx).abs().max()) <= 3e-6 * float(wantx.abs().max()) * (16 * Cout) ** 0.5
    if (B * H * W) % 32 == 0:
        n = Cin * 16 * Cout
        splits = L.pl_gemm_planes_splits(Cin, 16 * Cout, B * H * W)
        slabs = torch.empty(splits * n, device=DEV) if splits > 1 else None
        dwc = torch.full((Cin, 4, 4, Cout), float("nan"), device=DEV)
        rc = L.pl_conv2d_planes_wgrad(PL_BF16, xp.data_ptr(), x.numel(), dyp.data_ptr(), dy.numel(), B, 2 * H, 2 * W, Cout, Cin,
                                      4, 4, 2, 1, dwc.data_ptr(), 1.0, None, slabs.data_ptr() if slabs is not None else None, s)
        assert rc == 0, L.pl_last_error()
        ww = wantw.permute(0, 2, 3, 1)                               # [Cin][4][4][Cout]
        assert float((dwc.cpu().double() - ww).abs().max()) <= 3e-6 * float(ww.abs().max()) * (B * H * W) ** 0.5


def _assert_stored_plane(yp, y32, want, delta):
    """A kernel that stores its result as a bf16 plane rounds its fp32 value v, |v - want| <= delta: the plane equals
    bf16_round(want) except where want lies within delta of a rounding midpoint, where the neighbouring bf16 value (one
    bf16 ulp) is allowed -- for at most 1 % of the elements (the inputs have under 0.5 % such elements:
    tests/test_bf16_oracle_host.py)."""
    got = _decode_bf16_plane(yp).cpu().double().numpy()
    want, delta = want.numpy(), delta.numpy()
    assert np.all(np.abs(y32.cpu().double().numpy() - want) <= delta)           # the fp32 output of the same launch
    np.testing.assert_array_equal(got, bo.bf16_round(y32.cpu().numpy()).astype(np.float64))   # plane = RNE(fp32 output)
    exact = bo.bf16_round(want.astype(np.float32)).astype(np.float64)
    differs = got != exact
    amb = bo.ambiguous(want, delta + 2.0 ** -24 * np.abs(want))                 # (+ the fp32 cast of want above)
    assert not np.any(differs & ~amb), int((differs & ~amb).sum())
    assert np.all(np.abs(got - exact)[differs] <= bo.ulp_bf16(np.maximum(np.abs(got), np.abs(exact)))[differs])
    assert differs.mean() <= 0.01, float(differs.mean())


def test_conv2d_planes_eval_stores_the_bf16_rounding_of_its_result(pkg, cv):
    """conv2d_planes_eval with y_planes in PL_BF16, scale, shift, residual and ReLU after the add."""
    x, w, scale, shift, resid = bo.planes_eval_conv_inputs()
    want, delta = bo.planes_eval_conv_reference()
    ohwi = cv.to_ohwi(w).to(DEV)
    y, yp = cv.conv2d_planes_eval(_bf16_planes(cv, x.to(DEV)), _bf16_planes(cv, ohwi), tuple(ohwi.shape), 1, 1,
                                  scale.to(DEV), shift.to(DEV), None, 2, resid.to(DEV), want_f32=True, want_planes=True,
                                  mode=PL_BF16)
    _assert_stored_plane(yp, y, want, delta)


def test_deconv_planes_eval_stores_the_bf16_rounding_of_its_result(pkg, cv):
    """deconv_planes_eval with y_planes in PL_BF16, scale, shift and ReLU."""
    x, w, scale, shift = bo.planes_eval_deconv_inputs()
    want, delta = bo.planes_eval_deconv_reference()
    wsub = _bf16_planes(cv, cv.deconv_subkernels(w.to(DEV)))
    y, yp = cv.deconv_planes_eval(_bf16_planes(cv, x.to(DEV)), wsub, 72, scale.to(DEV), shift.to(DEV), 1, want_f32=True,
                                  want_planes=True, mode=PL_BF16)
    _assert_stored_plane(yp, y, want, delta)


# ---------------------------------------------------------------------------- 2.4 the lifter, compute_dtype="bf16"
LIFTER_FAMILIES = PLANES_FAMILIES + F32_FAMILIES
# the one-launch forms of a hidden layer's backward pair (tests/eval_backward_oracle.py PAIR_KERNELS)
PAIR_KERNELS = ("planes_gemm_chain_kernel", "planes_gemm_dual_kernel", "gemm_f32_dual_kernel", "gemm_x6_planes_dual_kernel")


def _lifter_step(pkg, name, B, H, bn):
    """One training forward + MSE + backward of LinearModel(compute_dtype="bf16") on bo.lifter_inputs, the kernels of the
    forward and of the backward by name: (model, state, x, t, keep masks, (pred, loss, grads, dx), fwd names, bwd names)."""
    st, x, t = bo.lifter_inputs(B, H, bn)
    m = pkg.LinearModel(34, 51, linear_size=H, num_stage=2, p_dropout=0.5, BN=bn, compute_dtype="bf16").to(DEV)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in st.items()})
    m.train().manual_seed(bo.LIFTER_DROPOUT_SEED, step=bo.LIFTER_STEP - 1)
    xd = _t(x).requires_grad_(True)
    out = []
    fwd = _gpu_kernel_names(lambda: out.append(m(xd)))
    loss = pkg.mse_loss(out[0], _t(t))
    bwd = _gpu_kernel_names(loss.backward)
    grads = {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}
    got = (out[0].detach().cpu().numpy(), float(loss.detach()), grads, xd.grad.cpu().numpy())
    return m, st, x, t, bo.lifter_keep_masks(B, H), got, fwd, bwd


def _decisions(pkg, m, H):
    """The device's own positive-and-kept decisions of the last training forward (test_gpu_parity._gpu_decisions)."""
    ws = m.last_workspace
    return [pkg.layout.unpack_bitmap(m.workspace_view(ws, 2, l).cpu().numpy().view(np.uint64), H) for l in range(5)]


def _template_args_say(names, kernel, args):
    """A launch of `kernel` whose template arguments start with `args` is among the names -- where the profiler's names
    carry template arguments at all (else there is nothing to read from a name: the numbers hold the arithmetic)."""
    mine = [n for n in names if kernel in n]
    assert mine, (kernel, sorted(set(names)))
    return any(args in n for n in mine) or not any("<" in n for n in mine)


@pytest.mark.parametrize("name,B,H,bn", bo.LIFTER_CASES, ids=[c[0] for c in bo.LIFTER_CASES])
def test_lifter_bf16_train_step_vs_emulated_oracle(pkg, name, B, H, bn):
    """compute_dtype="bf16" end to end against the EMULATED oracle -- oracle/lifter_oracle.py in fp64 with the operands of
    the hidden x hidden GEMMs rounded to bf16 (q(a) q(W)^T, q(dz)^T q(a), q(dz) q(W); first and output Linear, biases,
    BatchNorm and their gradients unrounded: csrc/api.hip writes planes of activations, dz and the weights of layers
    1 ... and of nothing else; off the planes path gemm_body's AR = 1 loop rounds the same operands as it stages them),
    the device's own ReLU decisions forced: prediction, loss, dx and every gradient, norm-wise (the zero-true-gradient
    biases skipped as in test_ragged_shapes_vs_oracle).

    Gates: those of the fp32-grade branch of the same comparison -- 2e-2 mm MPJPE, 2e-5 relative loss, 2e-4 relative L2
    -- or, if larger, twice what rounding ties cost the reference alone (an fp32-perturbed activation or dz may round to
    the neighbouring bf16 value), measured on the CPU as the emulated oracle in fp32 against the same in fp64
    (bo.lifter_reference_alone, recorded in bo.LIFTER_MEASURED, re-measured by tests/test_bf16_oracle_host.py):
        planes (B = 256, H = 256, BatchNorm):  0.167 mm, 2.3e-6, 2.55e-3  ->  gates 0.334 mm, 2e-5, 5.1e-3
        dual (B = 512, H = 512, no BatchNorm): 4.8e-4 mm, 1.2e-8, 1.16e-4 ->  gates 2e-2 mm, 2e-5, 2.32e-4
        two-launches (B = 256, H = 256, none): 6.6e-4 mm, 7.2e-8, 9.3e-5  ->  gates 2e-2 mm, 2e-5, 2e-4
    (Ties cascade: one activation that lands on the neighbouring bf16 value moves its whole row of the next z by an ulp of
    bf16 times a weight, and that row then flips a tenth of its own activations -- 6, 5, 46, 305 differing inputs at layers
    1 ... 4 of the planes case.  test_lifter_bf16_planes_layers_teacher_forced is the check without that cascade.)
    The device's result was never used to set them.  The 8e-2 gates of test_bf16_mode_train_and_eval_vs_oracle and
    test_ragged_shapes_vs_oracle, against the unrounded oracle, stay where they are.

    The kernels, by name: on the planes path the hidden Linears run planes tile GEMMs and the backward pairs
    planes_gemm_dual_kernel; without BatchNorm gemm_f32_kernel forward and, with 8 | tiles, gemm_f32_dual_kernel at AR = 1
    backward, else two gemm_f32_kernel launches per layer."""
    m, st, x, t, masks, got, fwd, bwd = _lifter_step(pkg, name, B, H, bn)
    ran_f, pair = _families(fwd, LIFTER_FAMILIES), _families(bwd, PAIR_KERNELS)
    if name == "planes":
        assert _planes_families(fwd) and "gemm_bf16_planes_kernel" not in ran_f, sorted(set(fwd))   # (the ends: gemm_f32_kernel)
        assert pair == {"planes_gemm_dual_kernel"}, sorted(set(bwd))
    else:
        # (the 34- and 51-wide ends are off the tile grid: their gemm_f32_kernel launches are the exact-fp32 edge form)
        assert ran_f == {"gemm_f32_kernel"}, sorted(set(fwd))
        assert _template_args_say(fwd, "gemm_f32_kernel", "<false, false, false, 1,")            # NT, whole tiles, AR = 1
        assert pair == ({"gemm_f32_dual_kernel"} if name == "dual" else set()), sorted(set(bwd))
        if name == "dual":
            assert _template_args_say(bwd, "gemm_f32_dual_kernel", "gemm_f32_dual_kernel<1,")
        else:
            assert _template_args_say(bwd, "gemm_f32_kernel", "<false, true, false, 1,")          # dX: NN, whole, AR = 1
            assert _template_args_say(bwd, "gemm_f32_kernel", "<true, true, false, 1,")           # dW: TN, whole, AR = 1
    on = _decisions(pkg, m, H)
    want = bo.lifter_emulated(st, x, t, bn, masks, on_masks=on)
    for c in want[4]["layers"]:
        d = c["on_disagree"]                # few, and small (the fraction of test_ragged_shapes_vs_oracle, the size of the bf16 rule)
        assert d.size <= 1e-3 * c["z"].size + 2 and (d.size == 0 or d.max() < 0.2), (d.size, d.max() if d.size else 0)
    mm, loss, rel, worst = bo.lifter_differences(got, want, bn)
    g_mm, g_loss, g_rel = bo.lifter_gates(name)
    print(f"lifter {name}: MPJPE {mm:.3e} mm (gate {g_mm:.3e}), loss {loss:.3e} (gate {g_loss:.1e}), worst relative L2 {rel:.3e} "
          f"({worst}; gate {g_rel:.2e})")
    assert mm <= g_mm and loss <= g_loss and rel <= g_rel, (mm, loss, rel, worst)
    # really the bf16 arithmetic: the unrounded oracle under the same decisions is far outside the same gates
    from oracle import lifter_oracle as orc
    pred_u, _ = orc.forward({k: v.copy() for k, v in st.items()}, x, num_stage=2, train=True, use_bn=bn, p_dropout=0.5,
                            keep_masks=masks, on_masks=on, dtype=np.float64)
    assert orc.mpjpe_mm(got[0], pred_u) > 3 * g_mm


def test_lifter_bf16_planes_layers_teacher_forced(pkg):
    """Layer by layer on the planes path (B = 256, H = 256, dropout from the Philox masks), each hidden x hidden Linear on
    the device's OWN saved input: z_l = q(a_{l-1}) q(W_l)^T + b_l within the GEMM bound of the raw planes GEMM cases,
    2e-6 (|q(a)| |q(W)|^T + |b|) + 1e-7.
      * odd l: a_{l-1} is materialised in fp32 (workspace_view which = 1: the residual stream) -- its plane is its rounding.
      * even l: a_{l-1} exists as a plane only.  It is rebuilt in fp64 from the saved z, mean, rstd and bitmap,
        a = on ? ((z - mean) rstd gamma + beta) / (1 - p) : 0; the device formed it in fp32 as z s + t with s = gamma rstd,
        t = beta - mean s (or in the centred form): up to eight roundings of at most 2^-24 of |z s| + |mean s| + |beta|
        each, delta = 2^-21 (|z s| + |mean s| + |beta|) / (1 - p).  Where a lies within delta of a rounding midpoint the
        device may hold the neighbouring bf16 value: the bound grows, per output, by sum_k amb[r,k] ulp_bf16(a[r,k]) |q(W)[n,k]|."""
    name, B, H, bn = bo.LIFTER_CASES[0]
    m, st, x, t, masks, got, fwd, bwd = _lifter_step(pkg, name, B, H, bn)
    from oracle import lifter_oracle as orc
    ws = m.last_workspace
    names = orc.hidden_layer_names(2)
    view = lambda which, l: m.workspace_view(ws, which, l).double()                      # noqa: E731
    on = [_t(np.ascontiguousarray(o)) for o in _decisions(pkg, m, H)]
    for l in range(1, 5):
        lin, _ = names[l]
        Wq = bo.bf16_round(_t(st[lin + ".weight"])).double()
        bias = _t(st[lin + ".bias"]).double()
        extra = 0.0
        if (l - 1) % 2 == 0:
            a = view(1, l - 1)
        else:
            bnp = names[l - 1][1]
            gamma, beta = _t(st[bnp + ".weight"]).double(), _t(st[bnp + ".bias"]).double()
            z, mean, rstd = view(0, l - 1), view(3, l - 1), view(4, l - 1)
            s = gamma * rstd
            a = torch.where(on[l - 1], ((z - mean) * rstd * gamma + beta) * 2.0, torch.zeros_like(z))
            delta = 2.0 ** -21 * ((z * s).abs() + (mean * s).abs() + beta.abs()) * 2.0
            amb = _t(bo.ambiguous(a.cpu().numpy(), delta.cpu().numpy())) & on[l - 1]
            ulp = _t(bo.ulp_bf16(a.cpu().numpy()))
            extra = (amb.double() * ulp) @ Wq.abs().T
            print(f"layer {l}: {int(amb.sum())} of {amb.numel()} rebuilt inputs within delta of a midpoint")
            assert float(amb.double().mean()) < 1e-3
        aq = bo.bf16_round(a.float()).double()
        want = aq @ Wq.T + bias
        bound = 2e-6 * (aq.abs() @ Wq.abs().T + bias.abs()) + 1e-7 + extra
        err = (view(0, l) - want).abs()
        print(f"layer {l}: err / bound = {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (l, float((err / bound).max()))
    with pytest.raises(pkg.PoseliftError, match="planes"):
        m.workspace_view(ws, 1, 1)                                   # (odd layers: planes only, as the case assumes)
