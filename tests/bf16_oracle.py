"""What the bf16 arithmetic (PL_BF16, arith="bf16", "bf16p") is held to: every bf16 rounding in the library is a
`(__bf16)` cast of an fp32 value -- round to nearest, ties to even, what torch's `.to(torch.bfloat16)` does -- the
product of two bf16 values is exact in fp32 and the accumulation is fp32.  So "round the operands to bf16, then compute
in fp64" is the exact result up to fp32 accumulation, and the bf16 kernels can be held to the bounds of the fp32-grade
rows of the same tests instead of "bf16-sized" ones.  Shared by tests/test_bf16_oracle_host.py (no GPU) and
tests/test_gpu_bf16_exact.py."""
import numpy as np
import torch


def bf16_round(x):
    """fp32 -> the fp32 value of its bf16 rounding (RNE), through torch's CPU cast for numpy arrays and on the tensor's
    own device for torch tensors; the result has the type of the argument (numpy float32 / torch float32)."""
    if isinstance(x, torch.Tensor):
        return x.to(torch.float32).to(torch.bfloat16).to(torch.float32)
    v = np.ascontiguousarray(x, np.float32)
    return torch.from_numpy(v).to(torch.bfloat16).to(torch.float32).numpy().reshape(v.shape)


def ulp_bf16(v):
    """Spacing of the bf16 values around |v| (fp64 numpy array): 8 significant bits, 2^-133 in the subnormal range."""
    _, e = np.frexp(np.abs(np.asarray(v, np.float64)))            # |v| = m 2^e, m in [0.5, 1)
    return np.ldexp(1.0, np.maximum(e, -125) - 8)


def ambiguous(v, delta):
    """Elements of the fp64 array `v` that lie within `delta` (scalar or array) of a bf16 rounding midpoint: a value
    that is known only to `delta` may round to either neighbour there."""
    v = np.abs(np.asarray(v, np.float64))
    _, e = np.frexp(v)
    e = np.maximum(e, -125)
    ulp = np.ldexp(1.0, e - 8)
    q = v / ulp
    dist = np.abs(q - np.floor(q) - 0.5) * ulp                    # the midpoints of v's own binade [2^(e-1), 2^e)
    below = np.ldexp(1.0, e - 1) - 0.25 * ulp                     # the last one of the binade below (spacing ulp / 2)
    above = np.ldexp(1.0, e) + ulp                                # the first one of the binade above (spacing 2 ulp)
    return np.minimum(dist, np.minimum(np.abs(v - below), np.abs(v - above))) <= delta


# ---- the raw GEMM cases of tests/test_gpu_bf16_exact.py whose size does not depend on the device (layout, M, N, K):
# layout 0 = NT (A [M][K], B [N][K]), 1 = NN (B [K][N]), 2 = TN (A [K][M])
PLANES_GEMM_CASES = [
    (0, 256, 128, 96), (0, 200, 192, 64),              # test_planes_gemm_vs_fp64: whole tiles and an overhang per layout
    (1, 128, 384, 64), (1, 130, 64, 128),
    (2, 256, 128, 160), (2, 200, 72, 256),
    (0, 128, 128, 1024), (2, 128, 128, 4096),          # one long contraction per pipeline phase
]


def gemm_inputs(layout, M, N, K, b_scale=0.05):
    """a [M][K], b [K][N], bias [N] of test_planes_gemm_vs_fp64 (seeded standard normal; b times b_scale)."""
    rng = np.random.default_rng(M + 3 * N + 7 * K + layout)
    a = rng.standard_normal((M, K)).astype(np.float32)
    b = (rng.standard_normal((K, N)) * b_scale).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    return a, b, bias


def gemm_reference(a, b, bias, tol=2e-6, floor=1e-7):
    """(exact result of the bf16-rounded operands, the f16x3 row's bound around it) in fp64 (numpy)."""
    ar, br = bf16_round(a).astype(np.float64), bf16_round(b).astype(np.float64)
    b64 = 0.0 if bias is None else bias.astype(np.float64)
    return ar @ br + b64, tol * (np.abs(ar) @ np.abs(br) + np.abs(b64)) + floor


# ---- convolutions: torch's fp64 conv2d / conv_transpose2d on the CPU, operands rounded first
def _q(t, rounded):
    return (bf16_round(t) if rounded else t).double()


def epilogue64(v_nchw, scale, shift, relu, resid_nhwc):
    """conv2d_nhwc's epilogue in fp64: BatchNorm scale / shift, relu 1 = ReLU then + resid, 2 = + resid then ReLU."""
    if scale is not None:
        v_nchw = v_nchw * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    if relu == 1:
        v_nchw = v_nchw.clamp_min(0)
    if resid_nhwc is not None:
        v_nchw = v_nchw + resid_nhwc.permute(0, 3, 1, 2).double()
    if relu == 2:
        v_nchw = v_nchw.clamp_min(0)
    return v_nchw.permute(0, 2, 3, 1)


def conv_reference(x_nhwc, w_oihw, stride, pad, scale=None, shift=None, bias=None, relu=0, resid=None, rounded=True):
    """(want, mag), NHWC fp64: F.conv2d on x and w (rounded to bf16 first unless rounded=False; bias, scale, shift and
    resid are never rounded: the kernels apply them in fp32) with the epilogue in fp64, and the magnitude
    conv(|x|, |w|) |scale| that test_conv2d_nhwc_vs_torch's bound is formed from."""
    import torch.nn.functional as F
    x, w = _q(x_nhwc, rounded).permute(0, 3, 1, 2), _q(w_oihw, rounded)
    v = F.conv2d(x, w, None if bias is None else bias.double(), stride=stride, padding=pad)
    mag = F.conv2d(x.abs(), w.abs(), stride=stride, padding=pad).permute(0, 2, 3, 1)
    if scale is not None:
        mag = mag * scale.abs().double().view(1, 1, 1, -1)
    return epilogue64(v, scale, shift, relu, resid), mag


def conv_grads_reference(x_nhwc, w_oihw, dy_nhwc, stride, pad, rounded=True):
    """(dx NHWC, dw OIHW) of F.conv2d in fp64 on (rounded) x, w and dy."""
    import torch.nn.functional as F
    x = _q(x_nhwc, rounded).permute(0, 3, 1, 2).requires_grad_(True)
    w = _q(w_oihw, rounded).requires_grad_(True)
    F.conv2d(x, w, stride=stride, padding=pad).backward(_q(dy_nhwc, rounded).permute(0, 3, 1, 2))
    return x.grad.permute(0, 2, 3, 1), w.grad


def deconv_reference(x_nhwc, w_iohw, dy_nhwc=None, rounded=True):
    """ConvTranspose2d(4, 2, 1) in fp64 on (rounded) operands: y NHWC, and with dy also (dx NHWC, dw IOHW)."""
    import torch.nn.functional as F
    x = _q(x_nhwc, rounded).permute(0, 3, 1, 2).requires_grad_(True)
    w = _q(w_iohw, rounded).requires_grad_(True)
    y = F.conv_transpose2d(x, w, stride=2, padding=1)
    if dy_nhwc is None:
        return y.detach().permute(0, 2, 3, 1)
    y.backward(_q(dy_nhwc, rounded).permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1), x.grad.permute(0, 2, 3, 1), w.grad


# ---- kernels that store their output as a bf16 plane (conv2d_planes_eval / deconv_planes_eval with y_planes): the
# stored value is the bf16 rounding of the fp32 result, which is known to `delta` around the fp64 reference
def planes_eval_conv_inputs():
    """3x3 convolution 32 -> 72 channels on a 2 x 9 x 12 map (216 pixels: ragged M and N) with scale, shift, a residual
    and the ReLU after the add."""
    g = torch.Generator().manual_seed(2024)
    x = torch.randn(2, 9, 12, 32, generator=g)
    w = torch.randn(72, 32, 3, 3, generator=g) * 0.05
    scale = torch.rand(72, generator=g) + 0.5
    shift = torch.randn(72, generator=g) + 3.0        # most outputs well away from zero, where bf16 midpoints crowd
    resid = torch.randn(2, 9, 12, 72, generator=g)
    return x, w, scale, shift, resid


def planes_eval_deconv_inputs():
    """ConvTranspose2d(4, 2, 1) 32 -> 72 channels on a 3 x 5 x 6 map (90 pixels) with scale, shift and ReLU."""
    g = torch.Generator().manual_seed(2025)
    x = torch.randn(3, 5, 6, 32, generator=g)
    w = torch.randn(32, 72, 4, 4, generator=g) * 0.05
    scale = torch.rand(72, generator=g) + 0.5
    shift = torch.randn(72, generator=g) + 1.5
    return x, w, scale, shift


def stored_plane_delta(mag_scaled, pre_relu_terms):
    """How far the fp32 value a planes kernel rounds to bf16 may lie from the fp64 reference: the f16x3 row's GEMM bound
    2e-6 mag |scale| + 1e-7 (test_conv_planes_fwd_dgrad_wgrad_vs_torch_fp64), plus the fp32 epilogue -- a scale
    multiply, a shift add and a residual add, each rounding by at most 2^-24 of its result, which the sum of the
    absolute values of the terms (`pre_relu_terms`) bounds."""
    return 2e-6 * mag_scaled + 1e-7 + 3 * 2.0 ** -24 * pre_relu_terms


def planes_eval_conv_reference():
    x, w, scale, shift, resid = planes_eval_conv_inputs()
    want, mag = conv_reference(x, w, 1, 1, scale, shift, None, 2, resid)
    lin, _ = conv_reference(x, w, 1, 1)
    terms = lin.abs() * scale.abs().double() + shift.abs().double() + resid.abs().double()
    return want, stored_plane_delta(mag, terms)


def planes_eval_deconv_reference():
    import torch.nn.functional as F
    x, w, scale, shift = planes_eval_deconv_inputs()
    lin = deconv_reference(x, w)
    want = (lin * scale.double() + shift.double()).clamp_min(0)
    mag = F.conv_transpose2d(bf16_round(x).double().abs().permute(0, 3, 1, 2), bf16_round(w).double().abs(), stride=2,
                             padding=1).permute(0, 2, 3, 1) * scale.abs().double()
    return want, stored_plane_delta(mag, lin.abs() * scale.abs().double() + shift.abs().double())


# ---- the lifter in compute_dtype="bf16": oracle/lifter_oracle.py with operand_round (the emulated oracle)
def operand_round(v):
    """The operand_round of oracle.lifter_oracle.forward: the bf16 rounding of the fp32 value of each operand (the
    library rounds fp32 tensors), returned in the dtype the oracle runs in."""
    v = np.asarray(v)
    return bf16_round(v.astype(np.float32)).astype(v.dtype)


# (id, B, H, BatchNorm): the planes path (one bf16 plane per activation, dz and weight); off it -- no BatchNorm -- the
# tile GEMMs' bf16 main loop, backward pair in one launch (8 | tiles) and in two
LIFTER_CASES = [("planes", 256, 256, True), ("dual", 512, 512, False), ("two-launches", 256, 256, False)]
LIFTER_DROPOUT_SEED, LIFTER_STEP = 23, 1


def lifter_inputs(B, H, bn):
    """(state, x [B][34], target [B][51]) of a LinearModel(34, 51, linear_size=H, num_stage=2, BN=bn)."""
    from oracle import lifter_oracle as orc
    st = orc.init_state(34, 51, H, 2, rng=np.random.default_rng(H + 3 * B + int(bn)), nontrivial_bn=bn)
    rng = np.random.default_rng(B + 7 * H)
    x = rng.random((B, 34), dtype=np.float32)
    t = rng.random((B, 51), dtype=np.float32) - np.float32(0.5)
    return st, x, t


def lifter_keep_masks(B, H):
    from oracle import philox
    return [philox.dropout_keep_mask(LIFTER_DROPOUT_SEED, LIFTER_STEP, l, B, H, 0.5) for l in range(5)]


def lifter_emulated(st, x, t, bn, keep_masks, on_masks=None, dtype=np.float64):
    """One training forward + MSE + backward of the emulated oracle: (pred, loss, grads, dx, cache)."""
    from oracle import lifter_oracle as orc
    pred, cache = orc.forward({k: v.copy() for k, v in st.items()}, x, num_stage=2, train=True, use_bn=bn, p_dropout=0.5,
                              keep_masks=keep_masks, on_masks=on_masks, dtype=dtype, operand_round=operand_round)
    loss, dpred = orc.mse_loss(pred, t, dtype)
    grads, dx = orc.backward(st, cache, dpred)
    return pred, loss, grads, dx, cache


def lifter_differences(got, want, bn):
    """(MPJPE in mm between the predictions, relative loss difference, largest relative L2 difference over dx and the
    parameter gradients -- the zero-true-gradient pre-BatchNorm biases left out, as in test_ragged_shapes_vs_oracle)."""
    from oracle import lifter_oracle as orc
    rel = {"dx": np.linalg.norm(np.float64(got[3]) - want[3]) / np.linalg.norm(np.float64(want[3]))}
    for k, v in want[2].items():
        if bn and k.endswith(".bias") and "batch_norm" not in k and k != "w2.bias":
            continue
        rel[k] = np.linalg.norm(np.float64(got[2][k]) - v) / (np.linalg.norm(np.float64(v)) + 1e-30)
    worst = max(rel, key=rel.get)
    return orc.mpjpe_mm(got[0], want[0]), abs(float(got[1]) - float(want[1])) / abs(float(want[1])), float(rel[worst]), worst


def lifter_reference_alone(B, H, bn):
    """What rounding ties cost the REFERENCE: the emulated oracle in fp32 against the same in fp64 (its ReLU decisions
    forced on the fp32 run) -- an fp32-perturbed activation or dz may round to the neighbouring bf16 value."""
    st, x, t = lifter_inputs(B, H, bn)
    masks = lifter_keep_masks(B, H)
    want = lifter_emulated(st, x, t, bn, masks)
    on = [c["rmask"] & c["keep"] for c in want[4]["layers"]]
    got = lifter_emulated(st, x, t, bn, masks, on_masks=on, dtype=np.float32)
    return lifter_differences(got, want, bn)


# lifter_reference_alone() when the gates were set: (MPJPE mm, relative loss difference, worst relative L2)
LIFTER_MEASURED = {"planes": (0.167, 2.3e-6, 2.55e-3), "dual": (4.8e-4, 1.2e-8, 1.16e-4), "two-launches": (6.6e-4, 7.2e-8, 9.3e-5)}


def lifter_gates(name):
    """Twice the reference-alone difference, or the bound of the fp32-grade branch of the same comparison if that is
    larger: 2e-2 mm (test_bf16_mode_train_and_eval_vs_oracle's e32), 2e-5 relative loss and 2e-4 relative L2
    (test_ragged_shapes_vs_oracle)."""
    mm, loss, rel = LIFTER_MEASURED[name]
    return max(2 * mm, 2e-2), max(2 * loss, 2e-5), max(2 * rel, 2e-4)
