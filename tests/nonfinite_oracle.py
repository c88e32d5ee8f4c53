"""Where a NaN or an infinity comes out, according to stock torch on the CPU in fp64.  TEST INFRASTRUCTURE ONLY.

The contract ("Non-finite values"): a non-finite value leaves every kernel of the library where torch's same
operation leaves one.  This module runs that same operation -- oracle/torch_twin.TwinLifter for the lifter, stock
conv2d / conv_transpose2d / batch_norm / max_pool2d / relu and the Bottleneck of backbone.py for the conv path,
mse_loss / l1_loss for the losses, the head of oracle/vit_twin.py for the ViT token head -- on an input with ONE poisoned
element and returns what came out.  tests/test_nonfinite_host.py asserts, on the CPU, that each reference alone shows the
clean pattern the GPU tests assert (exactly the poisoned row, the whole batch, the receptive field, ...), and that the
numpy oracle agrees with the twin; tests/test_gpu_nonfinite.py compares the device with it.

Split arithmetics and +inf.  "bf16x6", "f16x3" (and the conv path's GEMMs, which run "bf16x6") carry an fp32 operand as a
sum of 16-bit planes; the low plane of an infinity is inf - inf = NaN.  So where exact arithmetic gives +-inf these give
NaN: the CLASS of a non-finite result may differ from torch's, and a ReLU behind it cannot turn a -inf into 0 the way
torch does.  For +inf in a split arithmetic the expectation is therefore the mask alone, taken in FRONT of that ReLU
(`reach`: every output the poison enters); everywhere else the expectation is torch's mask itself."""
import copy

import numpy as np
import torch
import torch.nn.functional as F

import eval_backward_oracle as ebo
from oracle import lifter_oracle as orc
from oracle.torch_twin import TwinLifter

NAN, INF = float("nan"), float("inf")
POISONS = {"nan": NAN, "inf": INF}
SPLIT_DTYPES = ("bf16x6", "f16x3", "bf16")          # (bf16 rounds the operand: one plane, but products of bf16 roundings)


# ------------------------------------------------------------------------------------------------ classes and masks
def bad(t):
    """Boolean numpy mask of the non-finite elements."""
    return ~np.isfinite(np.asarray(torch.as_tensor(t).detach().cpu().numpy(), dtype=np.float64))


def classes(t):
    """0 finite, 1 NaN, 2 +inf, 3 -inf, elementwise (int8 numpy)."""
    a = np.asarray(torch.as_tensor(t).detach().cpu().numpy(), dtype=np.float64)
    c = np.zeros(a.shape, np.int8)
    c[np.isnan(a)] = 1
    c[np.isposinf(a)] = 2
    c[np.isneginf(a)] = 3
    return c


def same_values(got, want):
    """Exact equality for kernels that move or select values: the same class everywhere (NaN, +inf, -inf) and the same fp32
    value wherever that is finite (want: an fp64 reference of fp32-exact values)."""
    g = torch.as_tensor(got).detach().cpu().double().numpy()
    w = torch.as_tensor(want).detach().cpu().double().numpy()
    return g.shape == w.shape and np.array_equal(classes(g), classes(w)) and np.array_equal(g[np.isfinite(w)], w[np.isfinite(w)])


def same_bits(a, b):
    a, b = (np.ascontiguousarray(torch.as_tensor(t).detach().cpu().numpy()) for t in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------ lifter
_BY_ID = {c.id: c for c in ebo.CASES}
# pl_lifter_fwd_eval, one case per forward family of tests/eval_backward_oracle.CASES.  Up to 512 rows an evaluation with
# BatchNorm and a hidden size of 256 or 512 runs on the layer kernels of small_layer.hip whatever the batch (api.hip plan():
# eval_small; small_layer_ok wants whole 256-wide contraction steps), so those shapes end in eval_tail's ReLU; the GEMM
# epilogues are reached at H = 128, past 512 rows, off the tile grid and without BatchNorm.  kernel: a name the forward must
# launch.
EVAL_FWD_CASES = [
    (_BY_ID["fp32-2x128"], "thin_reduce_kernel"),                                           # gemm_thin.hip
    (_BY_ID["f16x3-100x256-ragged"], "small_fwd_kernel"),
    (_BY_ID["f16x3-128x128-chain"], "planes_gemm"),
    (_BY_ID["f16x3-256x256-dual-mid"], "small_fwd_kernel"),
    (_BY_ID["bf16-256x256-dual"], "small_fwd_kernel"),
    (_BY_ID["fp32-512x256-tile-dual"], "small_fwd_kernel"),
    (_BY_ID["bf16x6-512x256-x6-dual"], "small_fwd_kernel"),
    (_BY_ID["f16x3-640x128-chain"], "planes_gemm"),                                         # staged epilogue, gemm_planes.hip
    (_BY_ID["f16x3-640x128-chain"]._replace(id="bf16-640x128", dtype="bf16"), "planes_gemm"),
    (_BY_ID["f16x3-640x128-chain"]._replace(id="fp32-640x128", dtype="fp32"), "gemm_f32_kernel"),      # gemm_epilogue.h
    (_BY_ID["f16x3-640x128-chain"]._replace(id="bf16x6-640x128", dtype="bf16x6"), "gemm_x6_planes"),   # gemm_epilogue_vec
    (_BY_ID["fp32-520x128-ragged"], "gemm_f32_kernel"),                                     # edge tiles
    (_BY_ID["fp32-64x128-noBN"], "thin_reduce_kernel"),                                     # gemm_thin.hip
]
# the eval-mode autograd graph (pl_lifter_fwd_eval_saved / pl_lifter_bwd_eval): ReLU in bn_apply at every batch size
EVAL_BWD_CASES = [_BY_ID[k] for k in ("fp32-2x128", "f16x3-100x256-ragged", "f16x3-128x128-chain", "f16x3-256x256-dual-mid",
                                      "bf16-256x256-dual", "fp32-512x256-tile-dual", "bf16x6-512x256-x6-dual",
                                      "fp32-64x128-noBN")]
# one training step: the small-batch routes, the thin route, a whole-tile route per arithmetic, no BatchNorm
_T = _BY_ID["fp32-2x128"]
TRAIN_CASES = [
    _T._replace(id="fp32-16x64-small", B=16, H=64),
    _T._replace(id="f16x3-16x128-small", dtype="f16x3", B=16, H=128),
    _T._replace(id="f16x3-16x256-small", dtype="f16x3", B=16, H=256),      # the layer kernels of small_layer.hip (fwd_tail's ReLU)
    _T._replace(id="f16x3-100x256-thin", dtype="f16x3", B=100, H=256),
    _T._replace(id="f16x3-128x128-tile", dtype="f16x3", B=128, H=128),
    _T._replace(id="bf16-256x256-tile", dtype="bf16", B=256, H=256),
    _T._replace(id="fp32-512x256-tile", dtype="fp32", B=512, H=256),
    _T._replace(id="bf16x6-512x256-tile", dtype="bf16x6", B=512, H=256),
    _T._replace(id="fp32-64x128-noBN", B=64, H=128, bn=False),
]
# id -> kernels the training step must launch: the one that holds the layer's ReLU (bn_small_fwd_kernel and bn_apply_kernel
# both run bn_apply_row; small_fwd_kernel runs fwd_tail) and the one that names the route of its Linears
TRAIN_KERNELS = {
    "fp32-16x64-small": ("bn_small_fwd_kernel", "thin_gemm_kernel"),
    "f16x3-16x128-small": ("bn_small_fwd_kernel", "thin_gemm_kernel"),
    "f16x3-16x256-small": ("small_fwd_kernel", "small_bwd_kernel"),
    "f16x3-100x256-thin": ("bn_apply_kernel", "thin_gemm_kernel"),
    "f16x3-128x128-tile": ("bn_apply_kernel", "planes_gemm_kernel"),
    "bf16-256x256-tile": ("bn_apply_kernel", "planes_gemm_kernel"),
    "fp32-512x256-tile": ("bn_apply_kernel", "gemm_f32_dual_kernel"),
    "bf16x6-512x256-tile": ("bn_apply_kernel", "gemm_x6_planes_dual_kernel"),
    "fp32-64x128-noBN": ("bn_apply_kernel", "thin_gemm_kernel"),
}
# Dropout (p = 0.5, injected keep masks) on a NaN: one case per kernel that applies it, and one without BatchNorm, where
# rows stay apart and the difference from torch reaches the output (dropout_twin_step).  The poison is the bias of unit
# DROPOUT_UNIT of hidden layer DROPOUT_LAYER (a block output, kept in fp32): that unit is NaN in every row, the layers in
# front of it stay finite.
DROPOUT_CASES = [
    (_T._replace(id="fp32-16x64-drop", B=16, H=64), "bn_small_fwd_kernel"),
    (_T._replace(id="fp32-16x256-drop", B=16, H=256), "small_fwd_kernel"),
    (_T._replace(id="fp32-100x128-drop", B=100, H=128), "bn_apply_kernel"),
    (_T._replace(id="fp32-64x128-noBN-drop", B=64, H=128, bn=False), "bn_apply_kernel"),
]
DROPOUT_LAYER, DROPOUT_UNIT, DROPOUT_BIAS = 2, 7, "linear_stages.0.w2.bias"
MID_WEIGHT = ("linear_stages.0.w2.weight", 3, 7)      # a weight of a middle layer (every case here has num_stage = 2)
POISON_COL = 5


def poison_row(case):
    return case.B // 2


def lifter_inputs(case):
    """(st, x, t): the seeded weights, inputs and targets of eval_backward_oracle.make_inputs."""
    st, xa, ta, _, _ = ebo.make_inputs(case)
    return st, xa, ta


def poisoned(case, where, value):
    """(st, x, t) with one element poisoned: where = "x" (input row poison_row(case)) or "w" (MID_WEIGHT)."""
    st, x, t = lifter_inputs(case)
    st, x = {k: np.array(v) for k, v in st.items()}, x.copy()
    if where == "x":
        x[poison_row(case), POISON_COL] = value
    else:
        name, i, j = MID_WEIGHT
        st[name][i, j] = value
    return st, x, t


def twin_of(st, case):
    i_dim, o_dim = case.dims
    tw = TwinLifter(i_dim, o_dim, linear_size=case.H, num_stage=case.S, p_dropout=0.0, BN=case.bn).double()
    tw.load_state_dict({k: torch.from_numpy(np.array(v)).double() if np.asarray(v).dtype.kind == "f"
                        else torch.from_numpy(np.array(v)) for k, v in st.items()})
    return tw


def twin_step(st, x, t, case, train):
    """One forward + MSE + backward of the twin in fp64: y, loss, dx, every gradient and the buffers afterwards."""
    tw = twin_of(st, case)
    tw.train(train)
    xr = torch.from_numpy(x).double().requires_grad_(True)
    y = tw(xr)
    loss = F.mse_loss(y, torch.from_numpy(t).double())
    loss.backward()
    used = {n for n, _ in tw.named_parameters() if case.bn or "batch_norm" not in n}
    return dict(y=y.detach(), loss=loss.detach(), dx=xr.grad,
                grads={n: p.grad for n, p in tw.named_parameters() if n in used},
                buffers={n: b.detach().clone() for n, b in tw.named_buffers()})


def dropout_masks(case, p=0.5):
    """Seeded keep masks, one (B, H) boolean per hidden layer; of the poisoned unit row 0 is dropped and row 1 kept."""
    rng = np.random.default_rng(case.B + case.H)
    masks = [rng.random((case.B, case.H)) >= p for _ in range(1 + 2 * case.S)]
    masks[DROPOUT_LAYER][0, DROPOUT_UNIT], masks[DROPOUT_LAYER][1, DROPOUT_UNIT] = False, True
    return masks


class _SelectDropout(torch.autograd.Function):
    """Dropout as the library computes it: a SELECT in both directions -- keep ? r / (1 - p) : 0 forward, keep ? g / (1 - p) : 0
    backward -- where torch multiplies by the mask.  The two differ only where a dropped element, or the gradient arriving
    at one, is not finite: NaN * 0 = NaN in torch, 0 here."""

    @staticmethod
    def forward(ctx, r, keep, scale):
        ctx.save_for_backward(keep)
        ctx.scale = scale
        return torch.where(keep, r * scale, torch.zeros_like(r))

    @staticmethod
    def backward(ctx, g):
        (keep,) = ctx.saved_tensors
        return torch.where(keep, g * ctx.scale, torch.zeros_like(g)), None, None


def dropout_twin_step(st, x, t, case, masks, p=0.5, select=False):
    """The training step of the twin's architecture in fp64 with the keep masks given: Linear, BatchNorm (batch statistics),
    ReLU, Dropout as the product relu(.) * mask / (1 - p) -- stock torch's F.dropout with its mask made explicit.
    select: Dropout as a select instead (_SelectDropout: the library's form).  Returns y, loss, dx, gradients and the activation
    behind every hidden layer."""
    P = {k: torch.from_numpy(np.array(v)).double().requires_grad_(np.asarray(v).dtype.kind == "f" and "running" not in k)
         for k, v in st.items()}
    scale = 1.0 / (1.0 - p)
    acts = []

    def group(i, lin, bn, a):
        z = F.linear(a, P[lin + ".weight"], P[lin + ".bias"])
        if case.bn:
            z = F.batch_norm(z, None, None, P[bn + ".weight"], P[bn + ".bias"], training=True, eps=orc.BN_EPS)
        keep = torch.from_numpy(masks[i])
        r = torch.relu(z)
        out = _SelectDropout.apply(r, keep, scale) if select else r * (keep.double() * scale)
        acts.append(out)
        return out

    names = orc.hidden_layer_names(case.S)
    xr = torch.from_numpy(x).double().requires_grad_(True)
    h = group(0, *names[0], xr)
    for s_ in range(case.S):
        i1, i2 = 1 + 2 * s_, 2 + 2 * s_
        h = h + group(i2, *names[i2], group(i1, *names[i1], h))
        acts[i2] = h                                             # what the library keeps of a block's second layer: its output
    y = F.linear(h, P["w2.weight"], P["w2.bias"])
    loss = F.mse_loss(y, torch.from_numpy(t).double())
    loss.backward()
    return dict(y=y.detach(), loss=loss.detach(), dx=xr.grad, acts=[a.detach() for a in acts],
                grads={k: v.grad for k, v in P.items() if v.requires_grad and v.grad is not None})


def numpy_oracle_step(st, x, t, case, train):
    """The same step on oracle/lifter_oracle.py (fp64), for the host test: its masks must be the twin's."""
    st = {k: np.array(v) for k, v in st.items()}
    with np.errstate(invalid="ignore", over="ignore"):           # (inf - inf and 0 * inf are the point here)
        y, cache = orc.forward(st, x, num_stage=case.S, train=train, use_bn=case.bn, p_dropout=0.0, dtype=np.float64)
        loss, dy = orc.mse_loss(y, t, dtype=np.float64)
        grads, dx = orc.backward(st, cache, dy)
    return dict(y=y, loss=loss, dx=dx, grads=grads, buffers={k: v for k, v in st.items() if "running" in k})


# ------------------------------------------------------------------------------------------------ conv path
# conv2d_nhwc, one case per forward route (conv.hip conv_core): id, B, H, W, Cin, Cout, k, stride, pad, the kernel that runs
# for relu = 1 without a residual, and whether that route's arithmetic is split ("bf16x6": the tile GEMMs, the ragged-N form
# the im2col fallback's 128-pixel problem takes included) or exact fp32 (the direct stem kernel alone; with a residual or
# relu = 2 the stem's shape takes the im2col route)
CONV_CASES = [
    ("stem", 2, 16, 16, 3, 64, 7, 2, 3, "stem7x7_c3_kernel", False),
    ("implicit", 2, 8, 8, 32, 40, 3, 1, 1, "conv_x6_planes_kernel", True),
    ("1x1-gemm", 2, 8, 8, 64, 128, 1, 1, 0, "gemm_x6_planes", True),
    ("im2col", 2, 8, 8, 8, 16, 3, 1, 1, "im2col_nhwc_kernel", True),
    ("split-k", 1, 8, 16, 64, 128, 3, 1, 1, "reduce_slabs_epi_kernel", True),
]
CONV_VARIANTS = [(1, False), (2, True), (1, True)]            # (relu, residual): ReLU, + resid then ReLU, ReLU then + resid
CONV_POISON = (-1, 3, 4, 1)                                    # (b, h, w, c) of the poisoned input element


def conv_inputs(case, resid):
    _, B, H, W, Cin, Cout, k, stride, pad, _, _ = case
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + Cin + Cout + k)
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / np.sqrt(Cin * k * k)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.3
    r = torch.randn(B, Ho, Wo, Cout, generator=g) if resid else None
    return x, w, scale, shift, r


def conv_ref(x, w, stride, pad, scale, shift, relu, resid):
    """(y, pre): conv2d + folded BatchNorm + ReLU / residual in the two orders, NHWC fp64, and the value in front of the
    first ReLU (its non-finite mask is `reach`)."""
    pre = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), stride=stride, padding=pad)
    pre = pre * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    v = torch.relu(pre) if relu == 1 else pre
    if resid is not None:
        v = v + resid.permute(0, 3, 1, 2).double()
    if relu == 2:
        v = torch.relu(v)
    return v.permute(0, 2, 3, 1), pre.permute(0, 2, 3, 1)


def conv_window_mask(case, poison=CONV_POISON):
    """Geometry alone: the output pixels whose window holds the poisoned input pixel (every channel of them)."""
    _, B, H, W, Cin, Cout, k, stride, pad, _, _ = case
    b, h, w_, _ = poison
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    m = np.zeros((B, Ho, Wo, Cout), bool)
    for oh in range(Ho):
        for ow in range(Wo):
            if 0 <= h - (oh * stride - pad) < k and 0 <= w_ - (ow * stride - pad) < k:
                m[b % B, oh, ow, :] = True
    return m


DECONV_CASE = (1, 4, 6, 32, 64)                                # B, Hi, Wi, Cin, Cout: ConvTranspose2d(4, 2, 1) + BN + ReLU


def deconv_inputs():
    B, Hi, Wi, Cin, Cout = DECONV_CASE
    g = torch.Generator().manual_seed(Hi + Wi + Cin + Cout)
    x = torch.randn(B, Hi, Wi, Cin, generator=g)
    w = torch.randn(Cin, Cout, 4, 4, generator=g) / np.sqrt(Cin * 4)
    return x, w, torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.3


def deconv_ref(x, w, scale, shift):
    pre = F.conv_transpose2d(x.permute(0, 3, 1, 2).double(), w.double(), stride=2, padding=1)
    pre = pre * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    return torch.relu(pre).permute(0, 2, 3, 1), pre.permute(0, 2, 3, 1)


ADD_RELU_SHAPES = [(rows, C) for C in (4, 68, 320) for rows in (1, 3, 5)]
# add_relu_planes: the library takes maps of a multiple of 8 elements only (its second plane starts rows * C fp16 values in,
# and is written 16 bytes at a time; anything else is refused with "planes misaligned")
ADD_RELU_PLANES_SHAPES = [(rows, C) for rows, C in ADD_RELU_SHAPES if rows * C % 8 == 0] + \
                         [(rows, C) for C in (4, 68) for rows in (2, 4, 6)]


def add_relu_ref(a, b, g):
    """relu(a + b) and the gradient both inputs receive, torch autograd in fp64 (the fp32 sum is exact in fp64 and rounds
    back to the fp32 sum: the values are compared exactly)."""
    ar = a.double().requires_grad_(True)
    out = torch.relu((ar + b.double()).float().double())
    out.backward(g.double())
    return out.detach(), ar.grad


BN_RELU_SHAPES = [(6, 8), (130, 256)]


def bn_relu_train_ref(z, bn, dy):
    """Training-mode BatchNorm2d + ReLU over the rows of z [rows][C] (as test_batchnorm2d_train_fwd_bwd_vs_torch): output,
    the three gradients and the running statistics."""
    rows, C = z.shape
    ref = copy.deepcopy(bn).double().train()
    zr = z.double().requires_grad_(True)
    y = torch.relu(ref(zr.t().reshape(1, C, rows, 1)))
    y.backward(dy.double().t().reshape(1, C, rows, 1))
    return dict(y=y.detach().reshape(C, rows).t(), dz=zr.grad, dgamma=ref.weight.grad, dbeta=ref.bias.grad,
                running_mean=ref.running_mean.clone(), running_var=ref.running_var.clone())


MAXPOOL_SHAPES = [(1, 5, 6, 4), (2, 9, 7, 8)]
MAXPOOL_WINDOW = (1, 1)                                        # the output pixel whose nine taps are poisoned in turn


def maxpool_ref(x, dy):
    """F.max_pool2d(3, 2, 1) and its autograd on an NHWC map, in fp32: the values are selected, never rounded, and a pixel's
    gradient is the fp32 sum of at most four window gradients (bit for bit in tests/test_gpu_conv.py as well)."""
    xr = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.max_pool2d(xr, 3, 2, 1)
    y.backward(dy.permute(0, 3, 1, 2).contiguous())
    return y.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1)


def maxpool_inputs(shape, tap, value):
    """A seeded map with `value` at tap (kh, kw) of window MAXPOOL_WINDOW, channel 1, last sample; tap None: that window holds
    -inf only (channel 1)."""
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g)
    B, H, W, C = shape
    oh, ow = MAXPOOL_WINDOW
    if tap is None:
        x[B - 1, 2 * oh - 1:2 * oh + 2, 2 * ow - 1:2 * ow + 2, 1] = -INF
    else:
        x[B - 1, 2 * oh - 1 + tap[0], 2 * ow - 1 + tap[1], 1] = value
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return x, torch.randn(B, Ho, Wo, C, generator=g)


BOTTLENECK_SHAPE = (2, 8, 8, 256)


def bottleneck_ref(blk, x, dy):
    """One training step of the stock Bottleneck(256, 64) (backbone.py, Resnet.py:65-93) under torch autograd, NCHW fp64."""
    ref = copy.deepcopy(blk).double().train()
    xr = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    o = torch.relu(ref.bn1(ref.conv1(xr)))
    o = torch.relu(ref.bn2(ref.conv2(o)))
    out = torch.relu(ref.bn3(ref.conv3(o)) + xr)
    out.backward(dy.permute(0, 3, 1, 2).double())
    grads = {n: p.grad for n, p in ref.named_parameters()}
    buffers = {n: b.clone() for n, b in ref.named_buffers() if "running" in n}
    return out.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1), grads, buffers


# ------------------------------------------------------------------------------------------------ ViT token head
VIT_HEAD = (3, 32, 3)                                          # T, K, out_d


def vit_head_ref(z, W, b, dy):
    """oracle/vit_twin.forward's last line, mlp.2(ReLU(.)): y, dz, dW, db."""
    zr, Wr, br = (t.double().requires_grad_(True) for t in (z, W, b))
    y = F.linear(torch.relu(zr), Wr, br)
    y.backward(dy.double())
    return y.detach(), zr.grad, Wr.grad, br.grad


# ------------------------------------------------------------------------------------------------ losses
LOSS_SIZES = [1, 257, 1024 * 1024 + 3]                         # one element, one past a workgroup, one past MSE's grid cap


def mse_ref(p, t):
    pr = p.double().requires_grad_(True)
    loss = F.mse_loss(pr, t.double())
    loss.backward()
    return loss.detach(), pr.grad


def l1_ref(a, b):
    ar, br = a.double().requires_grad_(True), b.double().requires_grad_(True)
    loss = F.l1_loss(ar, br)
    loss.backward()
    return loss.detach(), ar.grad, br.grad


def mpjpe_ref(p, t):
    """loss_MPJPE (train_1.py:19-23): per joint, the sum over the batch of the L2 error."""
    return torch.sqrt(((p.double() - t.double()) ** 2).sum(-1)).sum(0)


# ------------------------------------------------------------------------------------------------ soft-argmax heads
def soft_argmax_ref(x, J, D, g):
    """Coordinates (B, J*3) of (B, J*D, H, W) logits and dlogits for the output gradient g, torch autograd in fp64."""
    B, _, H, W = x.shape
    xr = x.double().requires_grad_(True)
    hm = torch.softmax(xr.reshape(B, J, -1), 2).reshape(B, J, D, H, W)
    cx = (hm.sum((2, 3)) * torch.arange(W, dtype=torch.float64)).sum(2, keepdim=True)
    cy = (hm.sum((2, 4)) * torch.arange(H, dtype=torch.float64)).sum(2, keepdim=True)
    cz = (hm.sum((3, 4)) * torch.arange(D, dtype=torch.float64)).sum(2, keepdim=True)
    pred = torch.cat(((cx / W - .5) * 2, (cy / H - .5) * 2, (cz / D - .5) * 2), 2).reshape(B, J * 3)
    (pred * g.double()).sum().backward()
    return pred.detach(), xr.grad
