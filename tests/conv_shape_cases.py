"""The rectangular / odd-map cases of the direct convolution route, one row per route of conv_core (csrc/conv.hip),
pl_conv2d_nhwc_wgrad and conv.conv2d_nhwc_dgrad.  Shared by tests/test_gpu_conv_shapes.py (the kernels that run, by name,
and the fp64 result) and tests/test_conv_planes_host.py (the scratch the two size queries answer for the same route).

geom = (B, H, W, Cin, Cout, k, stride, pad) with H != W throughout: every kernel of this route decodes a GEMM row
m -> (b, oh, ow) or a column -> (kh, kw, ci) on its own, and on a square map a swap of Ho / Wo or H / W is invisible.

scratch: ("none",) | ("slabs", splits) | ("im2col",) | ("stem partials",) -- turned into bytes by fwd_scratch_bytes /
wgrad_scratch_bytes below from the formulas of the route, not from the library."""

STEM_WGRAD_WGS = 512                 # csrc/conv.hip: workgroups of stem7x7_c3_wgrad_kernel, one [64][147] partial each
STEM_WGRAD_MAX_WO = 152              # the widest output row that kernel stages in 64 KB of LDS


def out_hw(geom):
    B, H, W, Cin, Cout, k, stride, pad = geom
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


# (name, geom, BatchNorm scale/shift, relu, residual, bias, kernel families that run, scratch)
FWD_CASES = [
    # M = 120 pixels: one ragged 128-row tile whose rows decode with Wo = 20, Ho = 6
    ("3x3 ragged tile", (1, 6, 20, 32, 48, 3, 1, 1), True, 1, False, False, {"conv_x6_planes_kernel"}, ("none",)),
    # stride 2 on an odd x even map: Ho, Wo = 5, 7; the last row / column of taps falls on the padding
    ("3x3 s2 odd x even", (2, 9, 14, 32, 64, 3, 2, 1), True, 2, True, False, {"conv_x6_planes_kernel"}, ("none",)),
    # the 1x1 stride-2 row gather (the downsample): Ho, Wo = 5, 3
    ("1x1 s2 gather", (2, 10, 6, 64, 32, 1, 2, 0), True, 0, False, True, {"conv_x6_planes_kernel"}, ("none",)),
    # Cin % 32 != 0: explicit im2col (K = 72 padded to 96) + the generic GEMM's edge form
    ("im2col Cin 8", (1, 7, 11, 8, 24, 3, 1, 1), True, 2, True, True, {"im2col_nhwc_kernel", "gemm_f32_kernel"}, ("im2col",)),
    # the stem's own kernel: Ho, Wo = 5, 15
    ("stem", (1, 10, 30, 3, 64, 7, 2, 3), True, 1, False, False, {"stem7x7_c3_kernel"}, ("none",)),
    # ... and with an epilogue that kernel does not fold: im2col (K = 147 padded to 160)
    ("stem residual", (1, 10, 30, 3, 64, 7, 2, 3), True, 1, True, False, {"im2col_nhwc_kernel", "gemm_f32_kernel"}, ("im2col",)),
    # one whole 128 x 128 tile, 144 K tiles: conv_fwd_splits cuts K 8 ways; reduce_slabs_epi_kernel carries the epilogue
    ("split-K 8 slices", (1, 8, 16, 512, 128, 3, 1, 1), True, 2, True, True, {"conv_x6_planes_kernel", "reduce_slabs_epi_kernel"},
     ("slabs", 8)),
    # 1x1 stride 1: no gather at all, M = N = 128, K = 256
    ("1x1 plain GEMM", (1, 4, 32, 256, 128, 1, 1, 0), True, 1, False, False, {"gemm_x6_planes_kernel"}, ("none",)),
]

# (name, geom, kernel families of the weight gradient, scratch, kernel families of the data gradient or None: the stem has none)
WGRAD_CASES = [
    ("gathered Wo 8", (2, 6, 8, 32, 64, 3, 1, 1), {"conv_wgrad_x6_planes_kernel"}, ("none",), {"conv_x6_planes_kernel"}),
    ("gathered s2", (2, 8, 16, 32, 32, 3, 2, 1), {"conv_wgrad_x6_planes_kernel"}, ("none",),
     {"conv_x6_planes_group4_kernel", "deconv_interleave_kernel"}),
    # 544 pixels = 17 tiles, wgrad_splits: 2 slices of 9 and 8 tiles -- the last K slice is the shorter one
    ("gathered split 9 + 8", (1, 17, 32, 32, 64, 3, 1, 1), {"conv_wgrad_x6_planes_kernel"}, ("slabs", 2), {"conv_x6_planes_kernel"}),
    # Wo = 12: the gathered loader wants octets of pixels inside one output row
    ("im2col Wo 12", (2, 4, 12, 32, 64, 3, 1, 1), {"im2col_nhwc_kernel", "gemm_f32_kernel"}, ("im2col",), {"conv_x6_planes_kernel"}),
    # 1x1 stride 1 with whole tiles: dW = dy^T x, the plain TN GEMM (its dx: 32 pixels, the generic GEMM's edge form)
    ("1x1 plain TN", (1, 4, 8, 128, 128, 1, 1, 0), {"gemm_x6_planes_kernel"}, ("none",), {"gemm_f32_kernel"}),
    ("stem", (1, 6, 20, 3, 64, 7, 2, 3), {"stem7x7_c3_wgrad_kernel"}, ("stem partials",), None),
    # Wo = 152 = STEM_WGRAD_MAX_WO: 152 * 64 + 7 * 309 * 3 floats = 64,868 of 65,536 bytes of dynamic LDS
    ("stem widest row", (1, 4, 304, 3, 64, 7, 2, 3), {"stem7x7_c3_wgrad_kernel"}, ("stem partials",), None),
    # one pixel past it: im2col (306 pixels x 147 columns) + the generic TN GEMM's edge form
    ("stem past the widest row", (1, 4, 306, 3, 64, 7, 2, 3), {"im2col_nhwc_kernel", "gemm_f32_kernel"}, ("im2col",), None),
]

# stride-2 data gradients beside WGRAD_CASES' "gathered s2": (name, geom, kernel families)
DGRAD_S2_CASES = [
    ("1x1 s2 even", (2, 10, 6, 64, 32, 1, 2, 0), {"gemm_f32_kernel", "upsample2x_zero_kernel"}),
]

# stride 2 on maps with an odd side: the 2 Ho x 2 Wo result cropped to H x W (conv.conv2d_nhwc_dgrad)
DGRAD_ODD_CASES = [
    ("3x3 9x13", (2, 9, 13, 32, 64, 3, 2, 1)),
    ("1x1 7x10", (2, 7, 10, 64, 32, 1, 2, 0)),
    ("3x3 5x8 one odd side", (1, 5, 8, 32, 32, 3, 2, 1)),
]

# (B, Hi, Wi, Cin, Cout) of deconv4x4s2_nhwc
DECONV_CASES = [(1, 3, 5, 32, 16), (2, 4, 2, 64, 32)]


def fwd_scratch_bytes(geom, scratch):
    B, H, W, Cin, Cout, k, stride, pad = geom
    Ho, Wo = out_hw(geom)
    M, K = B * Ho * Wo, k * k * Cin
    if scratch[0] == "none":
        return 0
    if scratch[0] == "slabs":
        return scratch[1] * M * Cout * 4
    Kp = (K + 31) // 32 * 32                    # im2col rows and the weight rows, zero-padded to whole K tiles
    return (M * Kp + Cout * Kp) * 4


def wgrad_scratch_bytes(geom, scratch):
    B, H, W, Cin, Cout, k, stride, pad = geom
    Ho, Wo = out_hw(geom)
    pixels, N = B * Ho * Wo, k * k * Cin
    if scratch[0] == "none":
        return 0
    if scratch[0] == "slabs":
        return scratch[1] * Cout * N * 4
    if scratch[0] == "stem partials":
        return STEM_WGRAD_WGS * 64 * 147 * 4
    return pixels * N * 4                       # im2col, unpadded: the TN GEMM contracts over the pixels
