"""Convolution-path ops on the HIP library, NHWC throughout: forward ops and their autograd forms, in two generations.

Direct kernels (csrc/conv.hip; compute_dtype "bf16x6" / "bf16", and maps too small for the planes GEMM):
    conv2d_nhwc          nn.Conv2d forward with the Bottleneck's eval-mode epilogue folded in
                         (reference: phase4_joined/Resnet.py:51-95, :112-118, :151-158; Model.py:66-69)
    maxpool3x3s2_nhwc    nn.MaxPool2d(3, 2, 1)                               (Resnet.py:119)
    deconv4x4s2_nhwc     nn.ConvTranspose2d(4, 2, 1, bias=False) + BN + ReLU (Model.py:47-63)
    nhwc_to_nchw         layout change for heads that want NCHW (Model_2D)
    *_autograd           their differentiable forms (dgrad / wgrad on the same kernels)
    to_ohwi / deconv_subkernels / fold_bn   weight-layout helpers (host side, once per set of weights)

Planes GEMM (csrc/gemm_planes16.h; compute_dtype "f16x3" / "bf16p"): every convolution of a training step and of eval
mode as a GEMM on 16-bit operand planes that the producer of each tensor writes (second half of this file):
    conv1x1[_bias]_planes, conv_planes, stem_planes, deconv4x4s2_planes     training, with autograd
    conv2d_planes_eval, deconv_planes_eval                                  eval, folded epilogue, planes in and out

Shared by both: batchnorm_relu_train[_planes] / bn_join_planes (training-mode BatchNorm, optionally reading a GEMM
epilogue's statistics, adding the residual and writing planes) and add_relu[_planes] (the residual join).

The reference model permutes its NHWC input to NCHW for cuDNN/MIOpen (Model.py:88); here activations stay NHWC
end to end: a feature map IS the [B*H*W][C] matrix the MFMA GEMM wants, a 1x1 convolution is a GEMM, a KxK
convolution is the same GEMM with a gathering A loader (implicit GEMM, no im2col buffer).
"""
import ctypes

import torch
from torch.autograd.graph import increment_version

from . import _lib


def to_ohwi(weight_oihw):
    """nn.Conv2d.weight [Cout][Cin][KH][KW] -> contiguous [Cout][KH][KW][Cin]."""
    return weight_oihw.permute(0, 2, 3, 1).contiguous()


def deconv_subkernels(weight_iohw):
    """nn.ConvTranspose2d(k=4, s=2, p=1).weight [Cin][Cout][4][4] -> [4 parities][Cout][2][2][Cin].
    Output row oh = 2*ih - 1 + kh: even rows (oh = 2a) take kh = 3 from input row a-1 and kh = 1 from row a;
    odd rows (oh = 2a+1) take kh = 2 from row a and kh = 0 from row a+1; columns alike."""
    w = weight_iohw
    if w.dim() != 4 or w.shape[2] != 4 or w.shape[3] != 4:
        raise ValueError("deconv_subkernels expects a [Cin][Cout][4][4] ConvTranspose2d weight")
    # tap a of parity ph is kh = 3 - (2a + ph): on the flipped filter the tap index IS 2a + ph, so a reshape of each 4 into
    # (a, ph) and one permuted copy build all four sub-kernels (no index tensors: nothing here touches the host, the whole
    # training step can be captured in a hipGraph)
    cin, cout = w.shape[0], w.shape[1]
    wf = w.flip(2, 3).reshape(cin, cout, 2, 2, 2, 2)           # [Cin][Cout][a][ph][b][pw]
    return wf.permute(3, 5, 1, 2, 4, 0).reshape(4, cout, 2, 2, cin).contiguous()


def fold_bn(bn):
    """(scale, shift) of an nn.BatchNorm2d in eval mode: y = x * scale + shift."""
    scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    return scale.contiguous(), (bn.bias - bn.running_mean * scale).contiguous()


def _pgrad(param, make):
    """The gradient of `param` from an autograd node's backward.  make(out) computes it: into `out` (a contiguous tensor of
    the parameter's shape) when given, else into a fresh tensor it returns.
    A parameter managed by arena.ModuleArena (`_pl_grad`: its view of the flat gradient arena) gets its gradient written
    straight into the arena -- the first backward of a step overwrites and attaches the view as .grad, a later one in the
    same step (a second forward pass: the phase5 Flip branch) accumulates -- and autograd is handed None; any other
    parameter's gradient goes to autograd as usual."""
    view = getattr(param, "_pl_grad", None)
    if view is None:
        return make(None)
    if param.grad is None:
        make(view)
        param.grad = view
    else:
        param.grad.add_(make(None).reshape(param.shape))
    return None


def _pgrad2(pa, pb, C, dev, run, need=(True, True)):
    """_pgrad for two parameters whose gradients ONE kernel writes (BatchNorm's dgamma, dbeta): run(out_a, out_b).
    need: the node's needs_input_grad of the two.  A frozen parameter's half lands in scratch and stays there: no .grad is
    attached (FlatAdam steps every arena range that holds a gradient) and autograd is handed None, as for any other
    parameter with requires_grad=False."""
    va, vb = getattr(pa, "_pl_grad", None), getattr(pb, "_pl_grad", None)
    if all(need) and va is not None and vb is not None and pa.grad is None and pb.grad is None:
        run(va, vb)
        pa.grad, pb.grad = va, vb
        return None, None
    a, b = torch.empty(C, device=dev), torch.empty(C, device=dev)
    run(a, b)
    out = []
    for p, v, t, n in ((pa, va, a, need[0]), (pb, vb, b, need[1])):
        if not n:
            out.append(None)
        elif v is None:
            out.append(t)
        else:
            if p.grad is None:
                v.copy_(t)
                p.grad = v
            else:
                p.grad.add_(t)
            out.append(None)
    return tuple(out)


def _oihw_from_ohwi(dw_ohwi, out):
    """[O][KH][KW][I] -> the parameter's [O][I][KH][KW] layout (pl_nhwc_to_nchw: rows O, pixels KH*KW, channels I)."""
    O, KH, KW, I = dw_ohwi.shape
    if out is None:
        out = torch.empty(O, I, KH, KW, device=dw_ohwi.device)
    with _lib.on_device(dw_ohwi.device):
        rc = _lib.lib().pl_nhwc_to_nchw(dw_ohwi.data_ptr(), O, KH * KW, I, out.data_ptr(), _lib.current_stream_ptr())
    _lib.check(rc, "pl_nhwc_to_nchw")
    return out


def _opt(t, name, n):
    if t is None:
        return None
    t = t.contiguous()
    _lib.require_device_tensor(t, name)
    if t.numel() != n:
        raise ValueError(f"{name} has {t.numel()} elements, expected {n}")
    return t


def _bits(rows, C, dev):
    """The ReLU bitmap of a [rows][C] map: one bit per element, four 64-bit words per row and 256-column strip."""
    return torch.empty(rows, 4 * ((C + 255) // 256), dtype=torch.int64, device=dev)


# The direct kernels' arithmetic per compute_dtype.  "f16x3" / "bf16p" run on the planes GEMM (second half of this file);
# what reaches a direct kernel under them -- maps too small for the planes path -- keeps the same grade: fp32-grade
# bf16x6 next to two fp16 planes, bf16 operands next to one bf16 plane.
ARITH = {"bf16x6": _lib.PL_BF16X6, "bf16": _lib.PL_BF16, "f16x3": _lib.PL_BF16X6, "bf16p": _lib.PL_BF16}


def conv2d_nhwc(x, w_ohwi, stride=1, padding=0, scale=None, shift=None, bias=None, relu=0, resid=None,
                arith="bf16x6"):
    """x [B,H,W,Cin] fp32 -> [B,Ho,Wo,Cout] fp32.  relu: 0 none, 1 ReLU then + resid, 2 + resid then ReLU.
    arith: "bf16x6" (fp32-grade) or "bf16" (operands rounded to bf16: the throughput mode)."""
    # (a contiguous view such as frames[1:] may start off 16 bytes: the implicit-GEMM kernels refuse that)
    x, w = _lib.aligned16(x.contiguous()), _lib.aligned16(w_ohwi.contiguous())
    _lib.require_device_tensor(x, "x")
    _lib.require_device_tensor(w, "weight")
    if x.dim() != 4 or w.dim() != 4 or w.shape[3] != x.shape[3]:
        raise ValueError(f"conv2d_nhwc: x {tuple(x.shape)} (NHWC) vs weight {tuple(w.shape)} (OHWI)")
    B, H, W, Cin = x.shape
    Cout, KH, KW, _ = w.shape
    Ho, Wo = (H + 2 * padding - KH) // stride + 1, (W + 2 * padding - KW) // stride + 1
    y = torch.empty(B, Ho, Wo, Cout, dtype=torch.float32, device=x.device)
    opt = [_opt(scale, "scale", Cout), _opt(shift, "shift", Cout), _opt(bias, "bias", Cout),
           _opt(resid, "resid", y.numel())]
    opt[3] = _lib.aligned16(opt[3]) if opt[3] is not None else None
    ptr = [t.data_ptr() if t is not None else None for t in opt]
    L = _lib.lib()
    nbytes = L.pl_conv2d_nhwc_scratch_bytes_ex(B, H, W, Cin, Cout, KH, KW, stride, padding, int(bias is not None),
                                               int(resid is not None), int(relu))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
    with _lib.on_device(x.device):
        rc = L.pl_conv2d_nhwc_fwd(x.data_ptr(), B, H, W, Cin, w.data_ptr(), Cout, KH, KW, stride, padding,
                                  ptr[0], ptr[1], ptr[2], relu, ptr[3], y.data_ptr(), ARITH[arith],
                                  scratch.data_ptr() if nbytes else None, nbytes, _lib.current_stream_ptr())
    _lib.check(rc, "pl_conv2d_nhwc_fwd")
    return y


def conv2d_nhwc_wgrad(x, dy, kernel_size, stride=1, padding=0, arith="bf16x6"):
    """Weight gradient of conv2d_nhwc: x [B,H,W,Cin], dy [B,Ho,Wo,Cout] -> dw [Cout,KH,KW,Cin] (OHWI)."""
    x, dy = _lib.aligned16(x.contiguous()), _lib.aligned16(dy.contiguous())
    _lib.require_device_tensor(x, "x")
    _lib.require_device_tensor(dy, "dy")
    B, H, W, Cin = x.shape
    KH = KW = int(kernel_size)
    Cout = dy.shape[3]
    Ho, Wo = (H + 2 * padding - KH) // stride + 1, (W + 2 * padding - KW) // stride + 1
    if tuple(dy.shape) != (B, Ho, Wo, Cout):
        raise ValueError(f"conv2d_nhwc_wgrad: dy {tuple(dy.shape)} does not match the forward output {(B, Ho, Wo, Cout)}")
    dw = torch.empty(Cout, KH, KW, Cin, dtype=torch.float32, device=x.device)
    L = _lib.lib()
    nbytes = L.pl_conv2d_nhwc_wgrad_scratch_bytes(B, H, W, Cin, Cout, KH, KW, stride, padding)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
    with _lib.on_device(x.device):
        rc = L.pl_conv2d_nhwc_wgrad(x.data_ptr(), B, H, W, Cin, dy.data_ptr(), Cout, KH, KW, stride, padding,
                                    dw.data_ptr(), ARITH[arith], scratch.data_ptr() if nbytes else None, nbytes,
                                    _lib.current_stream_ptr())
    _lib.check(rc, "pl_conv2d_nhwc_wgrad")
    return dw


def conv2d_nhwc_dgrad(dy, w_ohwi, in_hw, stride=1, padding=0, arith="bf16x6"):
    """Input gradient of conv2d_nhwc: dy [B,Ho,Wo,Cout], w [Cout,KH,KW,Cin] -> dx [B,H,W,Cin].  No kernel of its
    own: stride 1 is the forward convolution of dy with the flipped filter, channels swapped; stride 2 (3x3 pad 1
    and 1x1 pad 0, the backbone's two cases, any H and W) is the transposed convolution
    dx[2*oh - pad + kh] += dy[oh] * w[kh], i.e. deconv4x4s2_nhwc with the filter placed inside a 4x4 one -- computed on
    the 2 Ho x 2 Wo map and, where H or W is odd, cropped to H x W: the dropped last row / column is the padding position
    the forward read as zero, its gradient belongs to no input.  Other kernels and strides: NotImplementedError."""
    Cout, KH, KW, Cin = w_ohwi.shape
    H, W = (int(v) for v in in_hw)
    if stride == 1:
        wf = w_ohwi.flip(1, 2).permute(3, 1, 2, 0).contiguous()            # [Cin][KH][KW][Cout]
        dx = conv2d_nhwc(dy, wf, 1, KH - 1 - padding, arith=arith)
        if dx.shape[1:3] != (H, W):
            raise ValueError("conv2d_nhwc_dgrad: input size does not match")
        return dx
    if stride != 2 or KH != KW or (KH, padding) not in ((3, 1), (1, 0)):
        raise NotImplementedError(f"conv2d_nhwc_dgrad: stride {stride}, kernel {KH}x{KW}, padding {padding}, input {H}x{W} "
                                  "(stride 1, or stride 2 with 3x3 / pad 1 or 1x1 / pad 0)")
    B, Ho, Wo, _ = dy.shape
    if (Ho, Wo) != ((H - 1) // 2 + 1, (W - 1) // 2 + 1):
        raise ValueError(f"conv2d_nhwc_dgrad: dy {Ho}x{Wo} is not the stride-2 output of a {H}x{W} input")
    if KH == 1:
        # dy W on the even pixels: one GEMM ([M][Cout] x [Cout][Cin], the OHWI filter read as [Cin][1][1][Cout]^T)
        t = conv2d_nhwc(dy, w_ohwi.reshape(Cout, Cin).t().contiguous().reshape(Cin, 1, 1, Cout), 1, 0, arith=arith)
        dx = torch.empty(B, 2 * Ho, 2 * Wo, Cin, dtype=torch.float32, device=dy.device)
        with _lib.on_device(dy.device):
            rc = _lib.lib().pl_upsample2x_zero_nhwc(t.data_ptr(), B, Ho, Wo, Cin, dx.data_ptr(), _lib.current_stream_ptr())
        _lib.check(rc, "pl_upsample2x_zero_nhwc")
    else:
        # ConvTranspose2d weight [in = Cout][out = Cin][4][4] with the 3x3 filter at kh, kw = 0 .. 2 (padding 1)
        w4 = torch.zeros(Cout, Cin, 4, 4, dtype=torch.float32, device=w_ohwi.device)
        w4[:, :, :3, :3] = w_ohwi.permute(0, 3, 1, 2)
        dx = deconv4x4s2_nhwc(dy, deconv_subkernels(w4), arith=arith)
    if (2 * Ho, 2 * Wo) != (H, W):
        dx = dx[:, :H, :W].contiguous()
    return dx


def maxpool3x3s2_nhwc(x):
    x = _lib.aligned16(x.contiguous())
    _lib.require_device_tensor(x, "x")
    B, H, W, C = x.shape
    y = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, dtype=torch.float32, device=x.device)
    with _lib.on_device(x.device):
        rc = _lib.lib().pl_maxpool3x3s2_nhwc(x.data_ptr(), B, H, W, C, y.data_ptr(), _lib.current_stream_ptr())
    _lib.check(rc, "pl_maxpool3x3s2_nhwc")
    return y


def deconv4x4s2_nhwc(x, w_sub, scale=None, shift=None, relu=0, arith="bf16x6"):
    """x [B,Hi,Wi,Cin] -> [B,2Hi,2Wi,Cout]; w_sub from deconv_subkernels()."""
    x, w = _lib.aligned16(x.contiguous()), _lib.aligned16(w_sub.contiguous())
    _lib.require_device_tensor(x, "x")
    _lib.require_device_tensor(w, "w_sub")
    B, Hi, Wi, Cin = x.shape
    if w.dim() != 5 or w.shape[0] != 4 or w.shape[2:] != (2, 2, Cin):
        raise ValueError(f"deconv4x4s2_nhwc: w_sub {tuple(w.shape)} is not [4][Cout][2][2][{Cin}]")
    Cout = w.shape[1]
    y = torch.empty(B, 2 * Hi, 2 * Wi, Cout, dtype=torch.float32, device=x.device)
    scale, shift = _opt(scale, "scale", Cout), _opt(shift, "shift", Cout)
    L = _lib.lib()
    nbytes = L.pl_deconv4x4s2_nhwc_scratch_bytes(B, Hi, Wi, Cout)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    with _lib.on_device(x.device):
        rc = L.pl_deconv4x4s2_nhwc_fwd(x.data_ptr(), B, Hi, Wi, Cin, w.data_ptr(), Cout,
                                       scale.data_ptr() if scale is not None else None,
                                       shift.data_ptr() if shift is not None else None, relu, y.data_ptr(), ARITH[arith],
                                       scratch.data_ptr(), nbytes, _lib.current_stream_ptr())
    _lib.check(rc, "pl_deconv4x4s2_nhwc_fwd")
    return y


def nhwc_to_nchw(x):
    """[B,H,W,C] -> contiguous [B,C,H,W]."""
    x = x.contiguous()
    _lib.require_device_tensor(x, "x")
    B, H, W, C = x.shape
    y = torch.empty(B, C, H, W, dtype=torch.float32, device=x.device)
    with _lib.on_device(x.device):
        rc = _lib.lib().pl_nhwc_to_nchw(x.data_ptr(), B, H * W, C, y.data_ptr(), _lib.current_stream_ptr())
    _lib.check(rc, "pl_nhwc_to_nchw")
    return y


# ---------------------------------------------------------------------------------------------
# Training-mode building blocks (autograd), NHWC.  backbone.py assembles the trainable ResNet and head from them.
# The convolutions here run on the direct kernels; BatchNorm and the residual join serve the planes path as well
# (operand planes and PlaneLink: second half of this file).
# ---------------------------------------------------------------------------------------------
def _colsum(x, rows, C):
    """Column sums [C] of the fp32 map x [rows][C] (a bias gradient)."""
    L = _lib.lib()
    out = torch.empty(C, dtype=torch.float32, device=x.device)
    scratch = torch.empty(L.pl_colsum_scratch_bytes(rows, C), dtype=torch.uint8, device=x.device)
    with _lib.on_device(x.device):
        rc = L.pl_colsum(x.data_ptr(), rows, C, out.data_ptr(), scratch.data_ptr(), _lib.current_stream_ptr())
    _lib.check(rc, "pl_colsum")
    return out


class _Conv2dFn(torch.autograd.Function):
    """conv2d_nhwc (+ bias, or None) with autograd: dgrad and wgrad run on the library too (conv2d_nhwc_dgrad / _wgrad)."""

    @staticmethod
    def forward(ctx, x, w_ohwi, bias, stride, padding, arith):
        ctx.save_for_backward(x, w_ohwi)
        ctx.geom = (stride, padding, arith)
        return conv2d_nhwc(x, w_ohwi, stride, padding, bias=bias, arith=arith)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, padding, arith = ctx.geom
        dy = dy.contiguous()
        dx = conv2d_nhwc_dgrad(dy, w, x.shape[1:3], stride, padding, arith) if ctx.needs_input_grad[0] else None
        dw = conv2d_nhwc_wgrad(x, dy, w.shape[1], stride, padding, arith) if ctx.needs_input_grad[1] else None
        db = None
        if ctx.needs_input_grad[2]:
            C = dy.shape[-1]
            db = _colsum(dy, dy.numel() // C, C)
        return dx, dw, db, None, None, None


def conv2d_nhwc_autograd(x, w_ohwi, stride=1, padding=0, arith="bf16x6"):
    """Differentiable conv2d_nhwc (no folded epilogue: in training mode BatchNorm needs batch statistics).
    arith "bf16": forward, dgrad and wgrad round their operands to bf16 while staging (fp32 accumulate/storage)."""
    return _Conv2dFn.apply(x, w_ohwi, None, stride, padding, arith)


def conv2d_bias_nhwc_autograd(x, w_ohwi, bias, stride=1, padding=0, arith="bf16x6"):
    return _Conv2dFn.apply(x, w_ohwi, bias, stride, padding, arith)


def _bn_replicas(rows, C):
    """csrc/batchnorm.hip bn_replicas: the BatchNorm kernels work on a narrow map [rows][C] -- and lay out its ReLU bitmap --
    as [rows / R][R C]."""
    r = 4 if C <= 64 else (2 if C <= 128 else 1)
    while r > 1 and (rows % r != 0 or rows // r < 2):
        r >>= 1
    return r


def _bn_fwd(ctx, z, identity, gamma, beta, running_mean, running_var, batches, eps, momentum, *, relu, f32, planes, link, mode):
    """Training-mode BatchNorm of z [..., C] over every leading dimension (+ identity, when given) (+ ReLU): the output as
    fp32 (f32), as a carrier of its operand planes in `mode` (planes), or both -- returns (y, yp), [rows][C] or None.  With
    link, the planes convolution that produced z has left its epilogue statistics there (or None: one more pass over z).
    Saves what _bn_bwd needs on ctx.  (Here and in _bn_bwd the library is handed mode 0 next to a NULL planes pointer.)"""
    shape = z.shape
    C = shape[-1]
    # (the streaming kernels read z and the identity 16 bytes at a time: a contiguous view that starts off 16 bytes is copied)
    z2 = _lib.aligned16(z.contiguous()).reshape(-1, C)
    id2 = _lib.aligned16(identity.contiguous()).reshape(-1, C) if identity is not None else None
    rows = z2.shape[0]
    dev, L = z2.device, _lib.lib()
    y = torch.empty_like(z2) if f32 else None
    yp = torch.empty_like(z2) if planes else None
    bits = _bits(rows, C, dev)
    mean, rstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
    scratch = torch.empty(L.pl_bn_train_scratch_bytes(rows, C), dtype=torch.uint8, device=dev)
    gstat = None
    if link is not None:
        gstat, link.stat = link.stat, None
    with _lib.on_device(dev):
        rc = L.pl_bn_train_fwd_ex(z2.data_ptr(), rows, C, gamma.data_ptr(), beta.data_ptr(), eps, momentum,
                                  running_mean.data_ptr(), running_var.data_ptr(), batches.data_ptr(), int(relu),
                                  y.data_ptr() if f32 else None, bits.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                  scratch.data_ptr(), yp.data_ptr() if planes else None, mode if planes else 0,
                                  gstat.data_ptr() if gstat is not None else None,
                                  id2.data_ptr() if id2 is not None else None, _lib.current_stream_ptr())
    _lib.check(rc, "pl_bn_train_fwd_ex")
    ctx.save_for_backward(z2, bits, mean, rstd, gamma, beta)
    ctx.shape, ctx.link = shape, link
    return y, yp


def _bn_bwd(ctx, g2, need, gp2=None, join=False):
    """Backward of _bn_fwd from dy = g2 [rows][C] -- join: from dy = the sum of g2 and gp2 (or None) where the join's ReLU
    passed, which is also the identity's gradient dx.  dz is fp32 or, with a link, a carrier of its planes, range-scaled on
    the device (link.dz_scale).  need: needs_input_grad of (gamma, beta).  Returns (dz, dx or None, dgamma, dbeta), the last
    two as _pgrad2 hands them to autograd."""
    z2, bits, mean, rstd, gamma, beta = ctx.saved_tensors
    rows, C = z2.shape
    dev, L, link = z2.device, _lib.lib(), ctx.link
    dx = torch.empty_like(g2) if join else None
    dz = torch.empty_like(z2)
    scratch = torch.empty(L.pl_bn_train_scratch_bytes(rows, C), dtype=torch.uint8, device=dev)
    if link is not None:
        link.dz_scale = torch.empty(2, device=dev)
        dzf, dzp, mode, scale = None, dz.data_ptr(), link.mode, link.dz_scale.data_ptr()
    else:
        dzf, dzp, mode, scale = dz.data_ptr(), None, 0, None
    gp = gp2.data_ptr() if gp2 is not None else None

    def run(dgamma, dbeta):
        with _lib.on_device(dev):
            if join and C >= 256:
                # one pass writes the masked sum and takes BatchNorm-backward's column sums of it (pl_bn_join_bwd)
                rc = L.pl_bn_join_bwd(g2.data_ptr(), gp, bits.data_ptr(), z2.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                      gamma.data_ptr(), rows, C, dx.data_ptr(), dzf, dgamma.data_ptr(), dbeta.data_ptr(),
                                      scratch.data_ptr(), dzp, mode, scale, _lib.current_stream_ptr())
                _lib.check(rc, "pl_bn_join_bwd")
                return
            dy = g2
            if join:
                # (the bitmap is the forward's, in ITS view of a narrow map: the masked sum is elementwise, so it takes that view)
                R = _bn_replicas(rows, C)
                rc = L.pl_mask_add_by_bits(g2.data_ptr(), gp, bits.data_ptr(), rows // R, C * R, dx.data_ptr(),
                                           _lib.current_stream_ptr())
                _lib.check(rc, "pl_mask_add_by_bits")
                dy = dx     # (dy = dx where the join's bitmap is set: masking the masked sum again changes nothing)
            rc = L.pl_bn_train_bwd_ex(dy.data_ptr(), bits.data_ptr(), z2.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                      gamma.data_ptr(), rows, C, dzf, dgamma.data_ptr(), dbeta.data_ptr(), scratch.data_ptr(),
                                      dzp, mode, scale, _lib.current_stream_ptr())
            _lib.check(rc, "pl_bn_train_bwd_ex")
    dgamma, dbeta = _pgrad2(gamma, beta, C, dev, run, need)
    return dz, dx, dgamma, dbeta


class _BNFn(torch.autograd.Function):
    """BatchNorm (+ ReLU) with the output as fp32 (out_planes False) or ONLY as a carrier of its planes (True: the next op
    is a planes convolution), and -- link given: the convolution that produced z is a planes convolution -- dz returned as a
    carrier of its planes (PlaneLink)."""

    @staticmethod
    def forward(ctx, z, gamma, beta, running_mean, running_var, batches, eps, momentum, relu, out_planes, link, mode):
        z = z.contiguous()
        # (callers hand this node tensors of their own making; the join below only ever sees this file's outputs)
        for name, t in (("z", z), ("gamma", gamma), ("beta", beta), ("running_mean", running_mean), ("running_var", running_var)):
            _lib.require_device_tensor(t, name)
        _lib.require_device_tensor(batches, "num_batches_tracked", torch.int64)
        y, yp = _bn_fwd(ctx, z, None, gamma, beta, running_mean, running_var, batches, eps, momentum, relu=relu,
                        f32=not out_planes, planes=out_planes, link=link, mode=mode)
        return (yp if out_planes else y).reshape(z.shape)

    @staticmethod
    def backward(ctx, dy):
        dz, _, dgamma, dbeta = _bn_bwd(ctx, _lib.aligned16(dy.contiguous()).reshape(-1, ctx.shape[-1]), ctx.needs_input_grad[1:3])
        return dz.reshape(ctx.shape), dgamma, dbeta, None, None, None, None, None, None, None, None, None


class _BNJoinFn(torch.autograd.Function):
    """bn3 and the residual join of a Bottleneck in ONE pass: x = relu(bn(z) + identity) as fp32 (the next join's identity) AND
    as a carrier of its planes (the next block's convolutions) -- bn3's output is never materialised.  backward: the masked
    sum of the two incoming gradients IS both the identity's gradient and bn3's dy; dz leaves as a carrier of its planes
    (link).  Resnet.py:81-91."""

    @staticmethod
    def forward(ctx, z, identity, gamma, beta, running_mean, running_var, batches, eps, momentum, link):
        x, xp = _bn_fwd(ctx, z, identity, gamma, beta, running_mean, running_var, batches, eps, momentum, relu=True, f32=True,
                        planes=True, link=link, mode=link.mode)
        ctx.set_materialize_grads(False)
        return x.reshape(z.shape), xp.reshape(z.shape)

    @staticmethod
    def backward(ctx, g, gp):
        if g is None:
            g, gp = gp, None
        if g is None:
            return (None,) * 10
        C = ctx.shape[-1]
        dz, dx, dgamma, dbeta = _bn_bwd(ctx, _lib.aligned16(g.contiguous()).reshape(-1, C), ctx.needs_input_grad[2:4],
                                        _lib.aligned16(gp.contiguous()).reshape(-1, C) if gp is not None else None, join=True)
        return dz.reshape(ctx.shape), dx.reshape(ctx.shape), dgamma, dbeta, None, None, None, None, None, None


def _bn_state(bn):
    if bn.momentum is None:
        raise NotImplementedError("cumulative moving average (momentum=None)")
    return (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, float(bn.eps), float(bn.momentum))


def batchnorm_relu_train_planes(z, bn, relu=True, out_planes=False, link=None, mode=_lib.PL_F16X3):
    """Training-mode nn.BatchNorm2d `bn` (+ ReLU) applied to an NHWC feature map z [..., C] (batch statistics over
    every leading dimension); updates bn.running_mean / running_var / num_batches_tracked in place.  out_planes: the
    output is a carrier of its operand planes (`mode`, or the link's); link: z came from a planes convolution (PlaneLink)."""
    y = _BNFn.apply(z, *_bn_state(bn), bool(relu), bool(out_planes), link, link.mode if link is not None else mode)
    increment_version((bn.running_mean, bn.running_var, bn.num_batches_tracked))
    return y


def batchnorm_relu_train(z, bn, relu=True):
    """The same, fp32 in and out."""
    return batchnorm_relu_train_planes(z, bn, relu)


def bn_join_planes(z, identity, bn, link):
    """relu(bn(z) + identity) -> (fp32, carrier of its planes); z came from a planes convolution (link)."""
    x, xp = _BNJoinFn.apply(z, identity, *_bn_state(bn), link)
    increment_version((bn.running_mean, bn.running_var, bn.num_batches_tracked))
    return x, xp


class _AddReLUFn(torch.autograd.Function):
    """relu(a + b), the residual join of a Bottleneck (Resnet.py:90-91), as fp32 and -- mode given -- ALSO as a carrier of
    its planes (the next block's 1x1 convolutions); backward: one masked pass over the SUM of the two gradients (no
    separate add)."""

    @staticmethod
    def forward(ctx, a, b, mode):
        if a.shape != b.shape:
            raise ValueError("add_relu: shapes differ")
        C = a.shape[-1]
        a2, b2 = _lib.aligned16(a.contiguous()).reshape(-1, C), _lib.aligned16(b.contiguous()).reshape(-1, C)
        _lib.require_device_tensor(a2, "a")
        _lib.require_device_tensor(b2, "b")
        rows = a2.shape[0]
        out = torch.empty_like(a2)
        outp = torch.empty_like(a2) if mode is not None else None
        bits = _bits(rows, C, a2.device)
        with _lib.on_device(a2.device):
            rc = _lib.lib().pl_add_relu_fwd_ex(a2.data_ptr(), b2.data_ptr(), rows, C, out.data_ptr(), bits.data_ptr(),
                                               outp.data_ptr() if outp is not None else None, mode or 0,
                                               _lib.current_stream_ptr())
        _lib.check(rc, "pl_add_relu_fwd_ex")
        ctx.save_for_backward(bits)
        ctx.shape = a.shape
        ctx.set_materialize_grads(False)       # an unused output's gradient arrives as None, not as a zero map
        return out.reshape(a.shape), outp.reshape(a.shape) if outp is not None else None

    @staticmethod
    def backward(ctx, g, gp):
        (bits,) = ctx.saved_tensors
        C = ctx.shape[-1]
        if g is None:
            g, gp = gp, None
        if g is None:
            return None, None, None
        g2 = _lib.aligned16(g.contiguous()).reshape(-1, C)
        gp2 = _lib.aligned16(gp.contiguous()).reshape(-1, C) if gp is not None else None
        dx = torch.empty_like(g2)
        with _lib.on_device(g2.device):
            rc = _lib.lib().pl_mask_add_by_bits(g2.data_ptr(), gp2.data_ptr() if gp2 is not None else None, bits.data_ptr(),
                                                g2.shape[0], C, dx.data_ptr(), _lib.current_stream_ptr())
        _lib.check(rc, "pl_mask_add_by_bits")
        dx = dx.reshape(ctx.shape)
        return dx, dx, None


def add_relu(a, b):
    """relu(a + b), differentiable."""
    return _AddReLUFn.apply(a, b, None)[0]


def add_relu_planes(a, b, mode=_lib.PL_F16X3):
    """(relu(a + b), carrier of its planes)."""
    return _AddReLUFn.apply(a, b, mode)


class _MaxPoolFn(torch.autograd.Function):
    """Forward records the winning tap per output element (one byte); backward reads those and dy only."""

    @staticmethod
    def forward(ctx, x):
        _lib.require_device_tensor(x, "x")
        B, H, W, C = x.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty(B, Ho, Wo, C, dtype=torch.float32, device=x.device)
        idx = torch.empty(B, Ho, Wo, C, dtype=torch.uint8, device=x.device)
        with _lib.on_device(x.device):
            rc = _lib.lib().pl_maxpool3x3s2_nhwc_idx(x.data_ptr(), B, H, W, C, y.data_ptr(), idx.data_ptr(),
                                                     _lib.current_stream_ptr())
        _lib.check(rc, "pl_maxpool3x3s2_nhwc_idx")
        ctx.save_for_backward(idx)
        ctx.in_shape = tuple(x.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        dy = _lib.aligned16(dy.contiguous())
        B, H, W, C = ctx.in_shape
        dx = torch.empty(B, H, W, C, dtype=torch.float32, device=dy.device)
        with _lib.on_device(dy.device):
            rc = _lib.lib().pl_maxpool3x3s2_nhwc_bwd_idx(idx.data_ptr(), dy.data_ptr(), B, H, W, C, dx.data_ptr(),
                                                         _lib.current_stream_ptr())
        _lib.check(rc, "pl_maxpool3x3s2_nhwc_bwd_idx")
        return dx


def maxpool3x3s2_nhwc_autograd(x):
    return _MaxPoolFn.apply(_lib.aligned16(x.contiguous()))


class _DeconvFn(torch.autograd.Function):
    """nn.ConvTranspose2d(4, 2, 1, bias=False) on NHWC, weight in torch's [Cin][Cout][4][4] layout.  Its backward
    needs no kernel of its own: y = C^T x for the stride-2 convolution C with the same filter, so dx = C dy (the
    forward convolution kernel, stride 2) and dW = wgrad of C with input dy and output gradient x."""

    @staticmethod
    def forward(ctx, x, weight, arith):
        ctx.save_for_backward(x, weight)
        ctx.arith = arith
        return deconv4x4s2_nhwc(x, deconv_subkernels(weight.detach().float()), arith=arith)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:       # [Cin][4][4][Cout] as OHWI
            dx = conv2d_nhwc(dy, weight.detach().permute(0, 2, 3, 1).contiguous(), 2, 1, arith=ctx.arith)
        if ctx.needs_input_grad[1]:       # [Cin][4][4][Cout] -> [Cin][Cout][4][4]
            dw = conv2d_nhwc_wgrad(dy, x, 4, 2, 1, ctx.arith).permute(0, 3, 1, 2).contiguous()
        return dx, dw, None


def deconv4x4s2_nhwc_autograd(x, weight_iohw, arith="bf16x6"):
    return _DeconvFn.apply(x.contiguous(), weight_iohw, arith)


class _ToNCHWFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return nhwc_to_nchw(x)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        B, C, H, W = g.shape
        out = torch.empty(B, H, W, C, dtype=torch.float32, device=g.device)
        with _lib.on_device(g.device):   # [B][C][P] -> [B][P][C]: the same tiled transpose with the roles swapped
            rc = _lib.lib().pl_nhwc_to_nchw(g.data_ptr(), B, C, H * W, out.data_ptr(), _lib.current_stream_ptr())
        _lib.check(rc, "pl_nhwc_to_nchw")
        return out


def nhwc_to_nchw_autograd(x):
    return _ToNCHWFn.apply(x)


# ---------------------------------------------------------------------------------------------
# Convolutions on the planes GEMM (compute_dtype "f16x3" / "bf16p"): the lifter's round-2 design on the conv path.
#
# A 1x1 convolution over an NHWC map IS the GEMM [pixels][Cin] x [Cout][Cin]^T.  Its operands travel as 16-bit operand
# planes written by the kernel that produces the tensor (BatchNorm apply, the residual join, BatchNorm backward), and the
# GEMM stages them by LDS-DMA (csrc/gemm_planes16.h): three fp16 MFMAs per product instead of six bf16 ones and no split
# work in the loop.  Between autograd nodes a tensor that exists ONLY as planes travels in a float32-typed "carrier" of
# the logical shape: two fp16 planes are exactly four bytes per element, so the carrier has the size autograd expects of
# the tensor (or of its gradient) while its bytes are [2][n] fp16.  Carriers are only ever handed to the functions below
# (backbone.py wires producer to consumer directly); every gradient that reaches torch code is real fp32.
#   reference: phase4_joined/Resnet.py:56-63, 65-93 (the Bottleneck's conv1 / conv3 / downsample and their autograd)
# ---------------------------------------------------------------------------------------------
ACT_PLANE_SCALE = 1.0 / 64   # csrc/pl_internal.h kConvActPlaneScale (pl_conv_act_plane_scale(): checked by the host-logic test)
WEIGHT_PLANE_SCALE = 16.0    # kWeightPlaneScale


class PlaneLink:
    """Connects the BatchNorm behind a planes convolution to that convolution's backward: the BatchNorm backward writes
    dz as planes (fp16, scaled by a power of two chosen on the device) and leaves {S, 1/S} here for the two GEMMs."""
    __slots__ = ("dz_scale", "mode", "stat")

    def __init__(self, mode=_lib.PL_F16X3):
        self.dz_scale = None
        self.stat = None          # forward: the convolution's epilogue statistics [2][groups][C] for the BatchNorm behind it
        self.mode = mode          # PL_F16X3: two fp16 planes (fp32-grade); PL_BF16: one bf16 plane (bf16 STORAGE of the operands)


def _planes_of_strided(base, dims, strides, offset, scale, mode):
    """Planes of the strided view (dims, signed element strides, element offset) of `base` -- pl_planes_split_strided: the layout
    change and the split in one launch."""
    nd = len(dims)
    d4 = (ctypes.c_int64 * 4)(*((1,) * (4 - nd) + tuple(int(v) for v in dims)))
    s4 = (ctypes.c_int64 * 4)(*((0,) * (4 - nd) + tuple(int(v) for v in strides)))
    out = torch.empty(tuple(int(v) for v in dims), dtype=torch.float32, device=base.device)
    with _lib.on_device(base.device):
        rc = _lib.lib().pl_planes_split_strided(base.data_ptr() + 4 * int(offset), d4, s4, mode, float(scale), out.data_ptr(),
                                                _lib.current_stream_ptr())
    _lib.check(rc, "pl_planes_split_strided")
    return out


def _planes_of_flipped_t(w_ohwi, scale, mode):
    """Planes of w.flip(1, 2).permute(3, 1, 2, 0) -- [Cin][KH][KW][Cout], the stride-1 data gradient's kernel -- straight from
    the (possibly non-contiguous) OHWI view: the flip is a negative stride."""
    cout, kh, kw, cin = w_ohwi.shape
    S = w_ohwi.stride()
    if cout % 4 or w_ohwi.dtype != torch.float32:
        return _planes_of(w_ohwi.flip(1, 2).permute(3, 1, 2, 0), scale, mode)
    return _planes_of_strided(w_ohwi, (cin, kh, kw, cout), (S[3], -S[1], -S[2], S[0]), (kh - 1) * S[1] + (kw - 1) * S[2],
                              scale, mode)


def _planes_of(t, scale, mode=_lib.PL_F16X3):
    """fp32 tensor -> carrier holding its planes (weights: once per step and direction, they are small).  A PL_BF16
    carrier uses the first half of its bytes."""
    if not t.is_contiguous() and 1 <= t.dim() <= 4 and t.shape[-1] % 4 == 0 and t.dtype == torch.float32 and t.numel() > 0:
        return _planes_of_strided(t, t.shape, t.stride(), 0, scale, mode)       # (a permuted / transposed weight view)
    t = _lib.aligned16(t.contiguous())
    out = torch.empty_like(t)
    with _lib.on_device(t.device):
        rc = _lib.lib().pl_planes_split(t.data_ptr(), t.numel(), mode, float(scale), out.data_ptr(),
                                        _lib.current_stream_ptr())
    _lib.check(rc, "pl_planes_split")
    return out


def _stat_buffer(rows, cols, dev):
    """[2][groups][cols]: what a GEMM epilogue writes as training-mode BatchNorm partial statistics of its output."""
    return torch.empty(2, _lib.lib().pl_gemm_stat_groups(rows), cols, device=dev)


def _gemm_planes_raw(layout, a, a_rows_cols, b, b_rows_cols, M, N, K, out_scale, dyn_inv=None, mode=_lib.PL_F16X3, stat=None,
                     out=None, bias=None):
    """C [M][N] fp32 from two carriers (planes of row-major matrices a_rows_cols / b_rows_cols); out: where to put it.
    With a bias the launch is never split over K (no slabs: a problem the library would split is its error to report)."""
    L = _lib.lib()
    dev = a.device
    if out is not None:
        _lib.require_aligned16_out(out, "out")           # (the GEMM's staged epilogue writes C 16 bytes at a time)
    C = torch.empty(M, N, device=dev) if out is None else out
    splits = L.pl_gemm_planes_splits(M, N, K) if bias is None else 1
    slabs = torch.empty(splits * M * N, device=dev) if splits > 1 else None
    with _lib.on_device(dev):
        rc = L.pl_gemm_planes_raw(layout, mode, a.data_ptr(), a_rows_cols[0] * a_rows_cols[1], a_rows_cols[1],
                                  b.data_ptr(), b_rows_cols[0] * b_rows_cols[1], b_rows_cols[1], C.data_ptr(), M, N, K,
                                  bias.data_ptr() if bias is not None else None, float(out_scale),
                                  dyn_inv.data_ptr() if dyn_inv is not None else None,
                                  slabs.data_ptr() if slabs is not None else None,
                                  stat.data_ptr() if stat is not None else None, _lib.current_stream_ptr())
    _lib.check(rc, "pl_gemm_planes_raw")
    return C


def planes_conv_supported(rows, cin, cout):
    """Shapes the planes GEMMs of a 1x1 convolution take: whole 32-k tiles in every contraction (Cin forward, Cout for
    the data gradient, pixels for the weight gradient), 8-element rows, 32-bit byte offsets inside one operand."""
    return cin % 32 == 0 and cout % 32 == 0 and rows % 32 == 0 and rows * max(cin, cout) * 4 < (1 << 31)


class _Conv1x1PlanesFn(torch.autograd.Function):
    """z = x W^T (+ bias, or None) for a 1x1 convolution: xp = carrier of x's planes [rows][Cin], w [Cout][Cin] fp32 ->
    z [rows][Cout] fp32, and the epilogue's BatchNorm statistics of z or None.  backward takes dz as a carrier (PlaneLink:
    written by the BatchNorm behind this convolution or, for the head's final convolution with its bias -- Model.py:66-69 --
    by the soft-argmax backward, heads.py): data gradient NT on W^T, weight gradient TN over the pixels, bias gradient =
    column sums of the planes."""

    @staticmethod
    def forward(ctx, xp, wparam, bias, link):
        rows, cin = xp.shape
        cout = wparam.shape[0]
        w = wparam.float().reshape(cout, cin)
        wp = _planes_of(w, WEIGHT_PLANE_SCALE, link.mode)
        # the BatchNorm behind this convolution reads the epilogue's statistics (no pass over z) -- unless the GEMM is split over K
        stat = None
        if bias is None and _lib.lib().pl_gemm_planes_splits(rows, cout, cin) == 1:
            stat = _stat_buffer(rows, cout, xp.device)
            ctx.mark_non_differentiable(stat)
        z = _gemm_planes_raw(0, xp, (rows, cin), wp, (cout, cin), rows, cout, cin,
                             1.0 / (ACT_PLANE_SCALE * WEIGHT_PLANE_SCALE), None, link.mode, stat, bias=bias)
        ctx.save_for_backward(xp, wparam, bias)
        ctx.link = link
        ctx.set_materialize_grads(False)       # (no zero tensor the size of `stat` per backward)
        return z, stat

    @staticmethod
    def backward(ctx, dzp, _gstat):
        if dzp is None:
            return None, None, None, None
        xp, wparam, bparam = ctx.saved_tensors
        rows, cin = xp.shape
        cout = wparam.shape[0]
        w = wparam.detach().float().reshape(cout, cin)
        dzp = dzp.contiguous()
        inv, mode = ctx.link.dz_scale[1:], ctx.link.mode   # 1 / S of the dz planes (device scalar; fp16 planes only)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            wtp = _planes_of(w.t(), WEIGHT_PLANE_SCALE, mode)  # [Cin][Cout]: the data gradient is NT on W^T
            dx = _gemm_planes_raw(0, dzp, (rows, cout), wtp, (cin, cout), rows, cin, cout, 1.0 / WEIGHT_PLANE_SCALE, inv, mode)
        if ctx.needs_input_grad[1]:
            def make(out):
                o2 = out.reshape(cout, cin) if out is not None else None
                r = _gemm_planes_raw(2, dzp, (rows, cout), xp, (rows, cin), cout, cin, rows, 1.0 / ACT_PLANE_SCALE, inv, mode, out=o2)
                return r.reshape(wparam.shape)
            dw = _pgrad(wparam, make)
        if ctx.needs_input_grad[2]:
            L = _lib.lib()

            def make_b(out):
                b = torch.empty(cout, device=dzp.device) if out is None else out
                scratch = torch.empty(L.pl_colsum_scratch_bytes(rows, cout), dtype=torch.uint8, device=dzp.device)
                with _lib.on_device(dzp.device):
                    rc = L.pl_colsum_planes(dzp.data_ptr(), mode, rows, cout, inv.data_ptr(), b.data_ptr(), scratch.data_ptr(),
                                            _lib.current_stream_ptr())
                _lib.check(rc, "pl_colsum_planes")
                return b
            db = _pgrad(bparam, make_b)
        return dx, dw, db, None


def conv1x1_bias_planes(xp, weight_oihw, bias, link):
    """xp: carrier [B, H, W, Cin] of the input's planes; weight, bias: the nn.Conv2d parameters [Cout][Cin][1][1], [Cout]."""
    shape = xp.shape
    cout, cin = weight_oihw.shape[0], weight_oihw.shape[1]
    z, link.stat = _Conv1x1PlanesFn.apply(xp.reshape(-1, cin), weight_oihw, bias, link)
    return z.reshape(*shape[:-1], cout)


def conv1x1_planes(xp, weight_oihw, link):
    return conv1x1_bias_planes(xp, weight_oihw, None, link)


class _ToPlanesFn(torch.autograd.Function):
    """fp32 tensor -> carrier of its planes (the stem's max-pool output, read by layer1's first 1x1 convolutions)."""

    @staticmethod
    def forward(ctx, x, mode):
        return _planes_of(x, ACT_PLANE_SCALE, mode)

    @staticmethod
    def backward(ctx, g):
        return g, None


def to_planes(x, mode=_lib.PL_F16X3):
    return _ToPlanesFn.apply(x, mode)


def _conv_geom(H, W, kh, kw, stride, pad):
    """stride: s or (sh, sw); pad: p or (above = below, left, right) -> (sh, sw, ph, pw, pwr, Ho, Wo)."""
    sh, sw = stride if isinstance(stride, tuple) else (stride, stride)
    ph, pw, pwr = pad if isinstance(pad, tuple) else (pad, pad, pad)
    return sh, sw, ph, pw, pwr, (H + 2 * ph - kh) // sh + 1, (W + pw + pwr - kw) // sw + 1


def _conv_planes_fwd(xp, x_shape, wp, w_shape, stride, pad, out_scale, dyn_inv=None, mode=_lib.PL_F16X3, stat=None):
    """pl_conv2d_planes_fwd on carriers: xp planes of x [B][H][W][Cin], wp planes of the OHWI kernel w_shape."""
    B, H, W, cin = x_shape
    cout, kh, kw, _ = w_shape
    sh, sw, ph, pw, pwr, ho, wo = _conv_geom(H, W, kh, kw, stride, pad)
    y = torch.empty(B, ho, wo, cout, device=xp.device)
    with _lib.on_device(xp.device):
        rc = _lib.lib().pl_conv2d_planes_fwd_hw(mode, xp.data_ptr(), B * H * W * cin, B, H, W, cin, wp.data_ptr(),
                                                cout * kh * kw * cin, cout, kh, kw, sh, sw, ph, pw, pwr, y.data_ptr(), float(out_scale),
                                                dyn_inv.data_ptr() if dyn_inv is not None else None,
                                                stat.data_ptr() if stat is not None else None, _lib.current_stream_ptr())
    _lib.check(rc, "pl_conv2d_planes_fwd")
    return y


def _planes_wgrad(dzp, xp, x_shape, cout, kh, kw, stride, pad, inv, mode):
    """Weight gradient [cout][kh][kw][cin] (OHWI, fp32) of a planes convolution: the TN GEMM over the output pixels of the dz
    planes [B][Ho][Wo][cout] with the planes of x (x_shape) gathered; split over K into slabs where the library says so."""
    B, H, W, cin = x_shape
    sh, sw, ph, pw, pwr, ho, wo = _conv_geom(H, W, kh, kw, stride, pad)
    L = _lib.lib()
    splits = L.pl_gemm_planes_splits(cout, kh * kw * cin, B * ho * wo)
    slabs = torch.empty(splits * cout * kh * kw * cin, device=dzp.device) if splits > 1 else None
    dw = torch.empty(cout, kh, kw, cin, device=dzp.device)
    with _lib.on_device(dzp.device):
        rc = L.pl_conv2d_planes_wgrad_hw(mode, dzp.data_ptr(), B * ho * wo * cout, xp.data_ptr(), B * H * W * cin, B, H, W, cin,
                                         cout, kh, kw, sh, sw, ph, pw, pwr, dw.data_ptr(), 1.0 / ACT_PLANE_SCALE, inv.data_ptr(),
                                         slabs.data_ptr() if slabs is not None else None, _lib.current_stream_ptr())
    _lib.check(rc, "pl_conv2d_planes_wgrad_hw")
    return dw


class _PlanesTwinFn(torch.autograd.Function):
    """xp (the carrier of x's planes) presented as a function of x, the fp32 twin the same kernel wrote.  A block with a
    downsample branch reads its input's planes twice (conv1, downsample[0]) and its fp32 twin not at all: routing the
    downsample's input gradient to x instead of xp hands the producing join's backward its two gradients separately -- it
    adds them inside its masked pass (pl_mask_add_by_bits) -- where autograd would otherwise sum two maps for xp with a
    pass of its own (1 GB each at layer2.0, B = 256)."""

    @staticmethod
    def forward(ctx, x, xp):
        return xp.view_as(xp)

    @staticmethod
    def backward(ctx, g):
        return g, None


def planes_twin(x, xp):
    return _PlanesTwinFn.apply(x, xp.detach()) if x.requires_grad else xp


class _ConvKxKPlanesFn(torch.autograd.Function):
    """KxK convolution (the Bottleneck's conv2, the stride-2 downsample) on the planes GEMM with the input gathered by the
    loader waves: xp carrier of x's planes [B][H][W][Cin], w OHWI fp32 -> z [B][Ho][Wo][Cout] fp32.  backward takes dz as a
    carrier (PlaneLink): the data gradient is the same kernel on dz with the kernel flipped and transposed (a stride-2
    convolution's dz is first spread over the even pixels of a zero map), the weight gradient the TN GEMM over the output
    pixels with the gathered x."""

    @staticmethod
    def forward(ctx, xp, wparam, stride, pad, link):
        w = wparam.float().permute(0, 2, 3, 1)         # the OHWI kernel as a VIEW of the [Cout][Cin][KH][KW] parameter
        wp = _planes_of(w, WEIGHT_PLANE_SCALE, link.mode)
        B, H, W, _ = xp.shape
        cout, kh, kw, _ = w.shape
        ho, wo = _conv_geom(H, W, kh, kw, stride, pad)[5:]
        stat = _stat_buffer(B * ho * wo, cout, xp.device)
        z = _conv_planes_fwd(xp, xp.shape, wp, w.shape, stride, pad, 1.0 / (ACT_PLANE_SCALE * WEIGHT_PLANE_SCALE), None, link.mode,
                             stat)
        ctx.save_for_backward(xp, wparam)
        ctx.geom, ctx.link = (stride, pad), link
        ctx.mark_non_differentiable(stat)
        ctx.set_materialize_grads(False)
        return z, stat

    @staticmethod
    def backward(ctx, dzp, _gstat):
        if dzp is None:
            return None, None, None, None, None
        xp, wparam = ctx.saved_tensors
        w = wparam.detach().float().permute(0, 2, 3, 1)
        stride, pad = ctx.geom
        B, H, W, cin = xp.shape
        cout, kh, kw, _ = w.shape
        _, ho, wo, _ = dzp.shape
        dzp = dzp.contiguous()
        inv, mode = ctx.link.dz_scale[1:], ctx.link.mode
        npl = 2 if mode == _lib.PL_F16X3 else 1
        dx = dw = None
        if ctx.needs_input_grad[0]:
            even = stride == 2 and H % 2 == 0 and W % 2 == 0 and 2 * ho == H and 2 * wo == W
            if even and kh == 1 and kw == 1 and pad == 0 and planes_conv_supported(B * ho * wo, cin, cout):
                # 1x1 stride 2 (the downsample): dz W at the output resolution, placed on the even pixels of a zero map
                wtp = _planes_of(w.reshape(cout, cin).t(), WEIGHT_PLANE_SCALE, mode)
                low = _gemm_planes_raw(0, dzp, (B * ho * wo, cout), wtp, (cin, cout), B * ho * wo, cin, cout,
                                       1.0 / WEIGHT_PLANE_SCALE, inv, mode)
                dx = torch.empty(B, H, W, cin, device=dzp.device)
                with _lib.on_device(dzp.device):
                    rc = _lib.lib().pl_upsample2x_zero_nhwc(low.data_ptr(), B, ho, wo, cin, dx.data_ptr(), _lib.current_stream_ptr())
                _lib.check(rc, "pl_upsample2x_zero_nhwc")
            elif even and kh == 3 and kw == 3 and pad == 1 and planes_deconv_supported(B, ho, wo, cout, cin):
                # 3x3 stride 2 pad 1: its transpose is ConvTranspose2d(4, 2, 1) with this filter in the top-left 3x3 of a
                # zero 4x4 one (ih = 2 oh - 1 + kh) -- four 2x2-tap gathers at the OUTPUT resolution, 4 taps per input
                # pixel instead of the 9 of the stride-1 gather over a zero-spread map (and no map to fill)
                w4 = torch.zeros(cout, cin, 4, 4, device=w.device)
                w4[:, :, :3, :3] = w.permute(0, 3, 1, 2)
                wsub = _planes_of(deconv_subkernels(w4), WEIGHT_PLANE_SCALE, mode)
                dx = torch.empty(B, H, W, cin, device=dzp.device)
                with _lib.on_device(dzp.device):
                    rc = _lib.lib().pl_deconv4x4s2_planes_fwd(mode, dzp.data_ptr(), B * ho * wo * cout, B, ho, wo, cout,
                                                              wsub.data_ptr(), wsub.numel(), cin, dx.data_ptr(),
                                                              1.0 / WEIGHT_PLANE_SCALE, inv.data_ptr(), _lib.current_stream_ptr())
                _lib.check(rc, "pl_deconv4x4s2_planes_fwd")
            elif stride == 1:
                wf = _planes_of_flipped_t(w, WEIGHT_PLANE_SCALE, mode)                          # [Cin][KH][KW][Cout]
                dx = _conv_planes_fwd(dzp, (B, ho, wo, cout), wf, (cin, kh, kw, cout), 1, kh - 1 - pad, 1.0 / WEIGHT_PLANE_SCALE, inv, mode)
            else:
                wf = _planes_of_flipped_t(w, WEIGHT_PLANE_SCALE, mode)
                # dz at the even pixels of a zero map the size the stride-1 gradient expects (planes are 16-bit: as int16)
                hu, wu = H + 2 * pad - kh + 1, W + 2 * pad - kw + 1
                up = torch.zeros(2, B, hu, wu, cout, dtype=torch.int16, device=dzp.device)
                up[:npl, :, ::stride, ::stride][:, :, :ho, :wo] = \
                    dzp.reshape(-1).view(torch.int16)[:npl * B * ho * wo * cout].reshape(npl, B, ho, wo, cout)
                src, shape = up.reshape(-1).view(torch.float32).reshape(B, hu, wu, cout), (B, hu, wu, cout)
                dx = _conv_planes_fwd(src, shape, wf, (cin, kh, kw, cout), 1, kh - 1 - pad, 1.0 / WEIGHT_PLANE_SCALE, inv, mode)
        if ctx.needs_input_grad[1]:
            dw_ohwi = _planes_wgrad(dzp, xp, xp.shape, cout, kh, kw, stride, pad, inv, mode)
            dw = _pgrad(wparam, lambda out: _oihw_from_ohwi(dw_ohwi, out))
        return dx, dw, None, None, None


# ---------------------------------------------------------------------------------------------------------------------
# The stem (phase4_joined/Resnet.py:112-113,137: Conv2d(3, 64, 7, stride 2, padding 3, bias=False)) on the planes GEMM.
# K = 7*7*3 = 147 fits nothing the matrix pipeline stages, so the frame is padded to 4 channels and read as pixel PAIRS
# [B][H][W/2][8]; the window of output (oh, ow) in kernel row kh is then the four pairs ow - 2 .. ow + 1 of input row
# 2 oh - 3 + kh: 32 contiguous values = one k-tile, of which the first pixel (kw = -1) and every fourth channel meet zero
# weights.  A convolution with 7 x 4 taps of 8 channels, stride (2, 1), padding 3 / 3 / 2 left / 1 right: K = 224 (pl_conv2d_planes_fwd_hw;
# the weight gradient is the gathered TN GEMM with the same geometry, its 224 columns folded back to the 147 real ones).
# Round 3; before: a direct fp32 kernel on the vector unit (1.45 ms forward, 1.28 ms weight gradient at B = 256).
# ---------------------------------------------------------------------------------------------------------------------
def stem_planes_supported(B, H, W, cin, cout, kh, kw, stride, pad):
    return (cin == 3 and cout == 64 and kh == 7 and kw == 7 and stride == 2 and pad == 3 and H % 2 == 0 and W % 4 == 0 and
            (B * (H // 2) * (W // 2)) % 256 == 0 and B * H * W * 4 * 2 < (1 << 31))


def stem_input_planes(frames_nhwc, mode=_lib.PL_F16X3):
    """[B, H, W, 3] fp32 frames -> carrier of the planes of the 4-channel pixel-pair view [B, H, W/2, 8]."""
    B, H, W, _ = frames_nhwc.shape
    x4 = torch.nn.functional.pad(frames_nhwc.float(), (0, 1))
    return _planes_of(x4.reshape(B, H, W // 2, 8), ACT_PLANE_SCALE, mode)


def _stem_weight_pairs(w_oihw, ohwi=False):
    """[64][3][7][7] (or, ohwi: [64][7][7][3]) -> the 7 x 4-tap kernel on pixel pairs [64][7][4][8]: pixel p of the 8-pixel
    window is kw = p - 1."""
    cout = w_oihw.shape[0]
    wv = torch.zeros(cout, 7, 8, 4, device=w_oihw.device, dtype=torch.float32)
    wv[:, :, 1:, :3] = w_oihw.float() if ohwi else w_oihw.float().permute(0, 2, 3, 1)
    return wv.reshape(cout, 7, 4, 8)


class _StemPlanesFn(torch.autograd.Function):
    """z [B][H/2][W/2][64] fp32 (+ the epilogue's BatchNorm statistics) from the frame's pair-view planes and the conv1
    parameter; backward: the weight gradient only (frames need none)."""

    @staticmethod
    def forward(ctx, xp, wparam, link):
        B, H, W2, _ = xp.shape
        wp = _planes_of(_stem_weight_pairs(wparam.detach()), WEIGHT_PLANE_SCALE, link.mode)
        rows = B * (H // 2) * W2
        stat = _stat_buffer(rows, 64, xp.device)
        z = _conv_planes_fwd(xp, xp.shape, wp, (64, 7, 4, 8), (2, 1), (3, 2, 1), 1.0 / (ACT_PLANE_SCALE * WEIGHT_PLANE_SCALE), None,
                             link.mode, stat)
        ctx.save_for_backward(xp, wparam)
        ctx.link = link
        ctx.mark_non_differentiable(stat)
        ctx.set_materialize_grads(False)
        return z, stat

    @staticmethod
    def backward(ctx, dzp, _gstat):
        if dzp is None or not ctx.needs_input_grad[1]:
            return None, None, None
        xp, wparam = ctx.saved_tensors
        cout = dzp.shape[3]
        dzp = dzp.contiguous()
        inv, mode = ctx.link.dz_scale[1:], ctx.link.mode
        dwp = _planes_wgrad(dzp, xp, xp.shape, cout, 7, 4, (2, 1), (3, 2, 1), inv, mode).reshape(cout, 7, 8, 4)

        def make(out):
            g = dwp[:, :, 1:, :3].permute(0, 3, 1, 2)              # the 147 real taps, as OIHW
            if out is None:
                return g.contiguous()
            out.copy_(g)
            return out
        return None, _pgrad(wparam, make), None


def stem_planes(xp, weight_oihw, link):
    """xp: stem_input_planes(frames); weight: the conv1 parameter [64][3][7][7]; z fp32 [B][H/2][W/2][64]."""
    z, stat = _StemPlanesFn.apply(xp, weight_oihw, link)
    link.stat = stat
    return z


def conv_planes(xp, weight_oihw, stride, pad, link):
    """xp: carrier [B, H, W, Cin]; weight: the nn.Conv2d parameter [Cout][Cin][KH][KW]."""
    # (the OHWI kernel as a VIEW of the parameter: its planes -- and the flipped / transposed ones of the backward -- are
    #  gathered by pl_planes_split_strided, no layout copy)
    z, stat = _ConvKxKPlanesFn.apply(xp, weight_oihw, stride, pad, link)
    link.stat = stat
    return z


def planes_convk_supported(B, H, W, cin, cout, k, stride, pad):
    """Whole 32-k tiles in every contraction (Cin per tap forward, Cout per tap for the data gradient, output pixels for the
    weight gradient) and gathered tensors -- x, and the (zero-spread, for stride 2) dz map of the data gradient -- whose
    planes stay below the DMA descriptor's 2 GiB."""
    ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    hu, wu = (ho, wo) if stride == 1 else (H + 2 * pad - k + 1, W + 2 * pad - k + 1)
    big = max(B * H * W * cin, B * hu * wu * cout)
    return cin % 32 == 0 and cout % 32 == 0 and (B * ho * wo) % 32 == 0 and big * 2 < (1 << 31) - 64


class _DeconvPlanesFn(torch.autograd.Function):
    """nn.ConvTranspose2d(4, 2, 1, bias=False) on the planes GEMM: xp carrier of x's planes [B][H][W][Cin], weight in torch's
    [Cin][Cout][4][4] layout -> y [B][2H][2W][Cout] fp32 (four 2x2-tap gathers, one per output parity).  y = C^T x for the
    stride-2 convolution C with the same filter, so the backward (dy as a carrier, PlaneLink) is dx = C dy -- the gathered
    forward kernel, 4x4 stride 2 -- and dW = the weight gradient of C with the roles of x and dy exchanged."""

    @staticmethod
    def forward(ctx, xp, weight, link):
        B, H, W, cin = xp.shape
        cout = weight.shape[1]
        wsub = _planes_of(deconv_subkernels(weight.float()), WEIGHT_PLANE_SCALE, link.mode)
        y = torch.empty(B, 2 * H, 2 * W, cout, device=xp.device)
        with _lib.on_device(xp.device):
            rc = _lib.lib().pl_deconv4x4s2_planes_fwd(link.mode, xp.data_ptr(), xp.numel(), B, H, W, cin, wsub.data_ptr(),
                                                      wsub.numel(), cout, y.data_ptr(),
                                                      1.0 / (ACT_PLANE_SCALE * WEIGHT_PLANE_SCALE), None,
                                                      _lib.current_stream_ptr())
        _lib.check(rc, "pl_deconv4x4s2_planes_fwd")
        ctx.save_for_backward(xp, weight)
        ctx.link = link
        return y

    @staticmethod
    def backward(ctx, dyp):
        xp, weight = ctx.saved_tensors
        B, H, W, cin = xp.shape
        cout = weight.shape[1]
        dyp = dyp.contiguous()
        inv, mode = ctx.link.dz_scale[1:], ctx.link.mode
        dx = dw = None
        if ctx.needs_input_grad[0]:       # C dy: OHWI kernel [Cin][4][4][Cout]
            wc = _planes_of(weight.float().permute(0, 2, 3, 1), WEIGHT_PLANE_SCALE, mode)
            dx = _conv_planes_fwd(dyp, (B, 2 * H, 2 * W, cout), wc, (cin, 4, 4, cout), 2, 1, 1.0 / WEIGHT_PLANE_SCALE, inv, mode)
        if ctx.needs_input_grad[1]:       # wgrad of C: "output gradient" x [B][H][W][Cin], gathered input dy -> [Cin][4][4][Cout]
            dwc = _planes_wgrad(xp, dyp, (B, 2 * H, 2 * W, cout), cin, 4, 4, 2, 1, inv, mode)
            dw = _pgrad(weight, lambda out: _oihw_from_ohwi(dwc, out))      # [Cin][4][4][Cout] -> [Cin][Cout][4][4]
        return dx, dw, None


def deconv4x4s2_planes(xp, weight_iohw, link):
    return _DeconvPlanesFn.apply(xp, weight_iohw, link)


def planes_deconv_supported(B, H, W, cin, cout):
    return (cin % 32 == 0 and cout % 32 == 0 and (B * H * W) % 32 == 0 and
            max(B * H * W * cin, B * 4 * H * W * cout) * 4 < (1 << 31))


# ---------------------------------------------------------------------------------------------
# Eval mode on the planes GEMM: conv2d_nhwc / deconv4x4s2_nhwc with planes in (and, optionally, out)
# ---------------------------------------------------------------------------------------------
def _epilogue(scale, shift, bias, relu, resid, y_planes):
    ep = _lib.PLPlanesEpilogue()
    ep.bias = bias.data_ptr() if bias is not None else None
    ep.scale = scale.data_ptr() if scale is not None else None
    ep.shift = shift.data_ptr() if shift is not None else None
    ep.resid = resid.data_ptr() if resid is not None else None
    ep.relu = int(relu)
    ep.y_planes = y_planes.data_ptr() if y_planes is not None else None
    return ep


def conv2d_planes_eval(xp, wp, w_shape, stride=1, padding=0, scale=None, shift=None, bias=None, relu=0, resid=None,
                       want_f32=True, want_planes=False, mode=_lib.PL_F16X3):
    """conv2d_nhwc with the input as a carrier of its planes [B,H,W,Cin] and the OHWI kernel's planes wp (w_shape):
    returns (y fp32 or None, carrier of y's planes or None)."""
    B, H, W, cin = xp.shape
    cout, kh, kw, _ = w_shape
    sh, sw, ph, pw, pwr, ho, wo = _conv_geom(H, W, kh, kw, stride, padding)
    y = torch.empty(B, ho, wo, cout, device=xp.device) if want_f32 else None
    yp = torch.empty(B, ho, wo, cout, device=xp.device) if want_planes else None
    opt = [_opt(scale, "scale", cout), _opt(shift, "shift", cout), _opt(bias, "bias", cout),
           _opt(resid, "resid", B * ho * wo * cout)]
    ep = _epilogue(opt[0], opt[1], opt[2], relu, opt[3], yp)
    with _lib.on_device(xp.device):
        rc = _lib.lib().pl_conv2d_planes_fwd_ep_hw(mode, xp.data_ptr(), B * H * W * cin, B, H, W, cin, wp.data_ptr(),
                                                   cout * kh * kw * cin, cout, kh, kw, sh, sw, ph, pw, pwr,
                                                   y.data_ptr() if y is not None else None,
                                                   1.0 / (ACT_PLANE_SCALE * WEIGHT_PLANE_SCALE), ctypes.byref(ep),
                                                   _lib.current_stream_ptr())
    _lib.check(rc, "pl_conv2d_planes_fwd_ep")
    return y, yp


def deconv_planes_eval(xp, wsubp, cout, scale=None, shift=None, relu=0, want_f32=True, want_planes=False, mode=_lib.PL_F16X3):
    """deconv4x4s2_nhwc the same way: wsubp = planes of deconv_subkernels(weight)."""
    B, H, W, cin = xp.shape
    y = torch.empty(B, 2 * H, 2 * W, cout, device=xp.device) if want_f32 else None
    yp = torch.empty(B, 2 * H, 2 * W, cout, device=xp.device) if want_planes else None
    ep = _epilogue(_opt(scale, "scale", cout), _opt(shift, "shift", cout), None, relu, None, yp)
    with _lib.on_device(xp.device):
        rc = _lib.lib().pl_deconv4x4s2_planes_fwd_ep(mode, xp.data_ptr(), B * H * W * cin, B, H, W, cin, wsubp.data_ptr(),
                                                     16 * cout * cin, cout, y.data_ptr() if y is not None else None,
                                                     1.0 / (ACT_PLANE_SCALE * WEIGHT_PLANE_SCALE), ctypes.byref(ep),
                                                     _lib.current_stream_ptr())
    _lib.check(rc, "pl_deconv4x4s2_planes_fwd_ep")
    return y, yp
