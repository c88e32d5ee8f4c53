"""MyViT, the transformer lifter of phase1_lifting/baselineModel.py:220-362 (the model train_1.py:35 trains; phase5's
3D->2D projector is MyViT(chw=(1,17,3), out_d=2)), on the HIP library.

Per token (T = seq * B rows of H = hidden_d features):
    x = x2d Wm^T + bm + pos_embed                       pl_vit_embed_fwd
    per block:  x += to_out(attn(mhsa.norm(norm1(x))))  pl_vit_ln_fwd (both LayerNorms, one pass), GEMM, pl_vit_attn_fwd, GEMM
                x += mlp.2(GELU(mlp.0(norm2(x))))       pl_vit_ln_fwd (the residual add in front), GEMM, pl_vit_gelu_fwd, GEMM
    head:       mlp.2(ReLU(mlp.0(x)))                   pl_vit_ln_fwd (the last residual add), GEMM, pl_vit_head_fwd
The whole forward is ONE autograd node (_ViTFn); its backward runs the same kernels' backward forms and returns every
parameter gradient (pos_embed's only when it requires one).  No dropout, no BatchNorm: train and eval forward are one path.

compute_dtype
  "fp32"   every Linear on the fp32 MFMA GEMM (pl_gemm_f32).
  "f16x3"  the block Linears (qkv, to_out, mlp.0, mlp.2: forward, data and weight gradients) on the planes GEMM
           (pl_gemm_planes_raw: two fp16 planes per operand, three MFMAs per product).  Activations and gradients are
           split with a power-of-two scale chosen on the device from their max |x| (pl_vit_planes_dyn) -- never a fixed
           scale; the weights with the static weight-plane scale, cached until the parameter's _version moves (an
           in-place change or a FlatAdam step).  The token head's Linears stay fp32 (the residual stream they read is not
           normalised).
  "bf16p"  the same four block Linears with bf16 operands: one bf16 plane per operand, one MFMA per product, fp32
           accumulate (pl_gemm_planes_raw, PL_BF16).  No scale and no max |x| pass: each operand is written once, as a
           bf16 carrier [pad32(T)][cols] with zero padding rows, by the kernel that produces it (the LayerNorm forward /
           backward, attention forward / backward, GELU forward / backward; the last block's output gradient, which the
           head's fp32 GEMM produces, by pl_vit_bf16_pack), rounded once from the fp32 value the fp32 mode computes.  The
           backward keeps those carriers instead of fp32 copies of a, o, n2 and GELU(h).  The weights are unscaled bf16
           carriers of W and W^T, cached like the f16x3 planes.  Everything else is the fp32 mode's arithmetic: the
           residual stream, the LayerNorm statistics, attention (scores, softmax, P V and their backward), the embedding,
           the token head's Linears and every parameter-gradient reduction (biases, gamma / beta, embedding).  Accuracy
           is bf16-storage grade, not fp32 grade: DESIGN.md 3b has the measured error against the fp64 twin.
"""
import numpy as np
import torch
from torch import nn

from . import _lib, conv

DIM_HEAD = 64
_DTYPES = ("f16x3", "fp32", "bf16p")


def positional_embeddings(seq, d):
    """pos[i][j] = sin(i / 10000^(j/d)) for even j, cos(i / 10000^((j-1)/d)) for odd j: evaluated per element in float64
    (numpy's sin / cos of the double quotient) and rounded to float32, as the reference builds it."""
    out = torch.ones(seq, d)
    for i in range(seq):
        for j in range(d):
            e = j if j % 2 == 0 else j - 1
            arg = i / ((1e4) ** (e / d))
            out[i][j] = np.sin(arg) if j % 2 == 0 else np.cos(arg)
    return out


class Attention(nn.Module):
    """Parameter holder with the reference's names: norm, attend (no parameters), to_qkv, to_out."""

    def __init__(self, dim, heads, dim_head):
        super().__init__()
        self.heads, self.scale = heads, dim_head ** -0.5
        self.norm = nn.LayerNorm(dim)
        self.attend = nn.Softmax(dim=-1)
        self.to_qkv = nn.Linear(dim, dim_head * heads * 3, bias=False)
        self.to_out = nn.Linear(dim_head * heads, dim, bias=False)


class MyViTBlock(nn.Module):
    def __init__(self, hidden_d, n_heads, mlp_ratio=4):
        super().__init__()
        self.hidden_d, self.n_heads = hidden_d, n_heads
        self.norm1 = nn.LayerNorm(hidden_d)
        self.mhsa = Attention(hidden_d, n_heads, int(hidden_d / n_heads))
        self.norm2 = nn.LayerNorm(hidden_d)
        self.mlp = nn.Sequential(nn.Linear(hidden_d, mlp_ratio * hidden_d), nn.GELU(), nn.Linear(mlp_ratio * hidden_d, hidden_d))


def _check_shape(chw, n_blocks, hidden_d, n_heads, out_d):
    seq, in_d = int(chw[1]), int(chw[2])
    if n_heads < 1 or hidden_d % n_heads or hidden_d // n_heads != DIM_HEAD:
        raise _lib.PoseliftError(f"MyViT: dim_head = hidden_d / n_heads must be {DIM_HEAD} (hidden_d={hidden_d}, n_heads={n_heads})")
    if not 1 <= seq <= 32:
        raise _lib.PoseliftError(f"MyViT: the attention kernels take sequences of 1 .. 32 tokens, not {seq}")
    if not 1 <= in_d <= 8:
        raise _lib.PoseliftError(f"MyViT: token input width {in_d} (1 .. 8 supported)")
    # pl_vit_attn_bwd stages a sample's q, k, v, dO and two [heads][seq][32] score tiles in LDS (160 KB)
    lds = 4 * (seq * (3 * hidden_d + 1) + seq * (hidden_d + 1) + 2 * n_heads * seq * 32)
    if hidden_d > 512 or lds > 160 * 1024:
        raise _lib.PoseliftError(f"MyViT: hidden_d {hidden_d} with {seq} tokens does not fit the attention kernels")
    if not 1 <= out_d <= 4:
        raise _lib.PoseliftError(f"MyViT: out_d {out_d} unsupported (1 .. 4)")
    if n_blocks < 1:
        raise _lib.PoseliftError("MyViT: at least one block")


class MyViT(nn.Module):
    """baselineModel.MyViT with the same submodules, names, creation order (a seeded construction draws the reference's
    initial weights) and state_dict; compute_dtype selects the GEMM arithmetic (module docstring)."""

    def __init__(self, chw=(1, 17, 2), n_blocks=2, hidden_d=256, n_heads=4, out_d=3, compute_dtype="f16x3"):
        super().__init__()
        if compute_dtype not in _DTYPES:
            raise _lib.PoseliftError(f"MyViT: compute_dtype {compute_dtype!r} (one of {_DTYPES})")
        _check_shape(chw, n_blocks, hidden_d, n_heads, out_d)
        self.chw, self.n_block, self.n_heads, self.hidden_d, self.out_d = tuple(chw), n_blocks, n_heads, hidden_d, out_d
        self.compute_dtype = compute_dtype
        self.input_d = chw[2]
        self.linear_mapper = nn.Linear(self.input_d, self.hidden_d)
        self.pos_embed = nn.Parameter(positional_embeddings(chw[1], self.hidden_d))
        self.pos_embed.requires_grad = False
        self.blocks = nn.ModuleList([MyViTBlock(hidden_d, n_heads) for _ in range(n_blocks)])
        self.mlp = nn.Sequential(nn.Linear(self.hidden_d, int(self.hidden_d / 2)), nn.ReLU(), nn.Linear(int(self.hidden_d / 2), out_d))
        self._wcache = {}

    def _params(self):
        ps = [self.linear_mapper.weight, self.linear_mapper.bias, self.pos_embed]
        for b in self.blocks:
            ps += [b.norm1.weight, b.norm1.bias, b.mhsa.norm.weight, b.mhsa.norm.bias, b.mhsa.to_qkv.weight, b.mhsa.to_out.weight,
                   b.norm2.weight, b.norm2.bias, b.mlp[0].weight, b.mlp[0].bias, b.mlp[2].weight, b.mlp[2].bias]
        ps += [self.mlp[0].weight, self.mlp[0].bias, self.mlp[2].weight, self.mlp[2].bias]
        return ps

    def _wplanes(self, w):
        """(planes of W [N][K], planes of W^T [K][N]) with the weight-plane scale ("bf16p": unscaled bf16 carriers);
        rebuilt after a FlatAdam step or any in-place change of the parameter."""
        key = (w._version, w.data_ptr(), self.compute_dtype)
        hit = self._wcache.get(id(w))
        if hit is not None and hit[0] == key:
            return hit[1]
        wd = w.detach()
        if self.compute_dtype == "bf16p":
            planes = (conv._planes_of(wd, 1.0, _lib.PL_BF16), conv._planes_of(wd.t(), 1.0, _lib.PL_BF16))
        else:
            planes = (conv._planes_of(wd, conv.WEIGHT_PLANE_SCALE), conv._planes_of(wd.t(), conv.WEIGHT_PLANE_SCALE))
        self._wcache[id(w)] = (key, planes)
        return planes

    def forward(self, images):
        if images.dim() != 3 or images.shape[1] != self.chw[1] or images.shape[2] != self.input_d:
            raise ValueError(f"MyViT expects (B, {self.chw[1]}, {self.input_d}) input, got {tuple(images.shape)}")
        x = images.float().contiguous()
        _lib.require_device_tensor(x, "input")
        ps = self._params()
        for p in ps:
            _lib.require_device_tensor(p.data, "parameter")
        need = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in ps))
        return _ViTFn.apply(self, need, x, *ps)


# ------------------------------------------------------------------------------------------------ host-side launch helpers
def _ptr(t):
    return t.data_ptr() if t is not None else None


def _run(name, *args):
    _lib.check(getattr(_lib.lib(), name)(*args, _lib.current_stream_ptr()), name)


def _gemm_f32(layout, A, B, M, N, K, bias=None, out=None):
    """C [M][N] = op(A) op(B) (+ bias) on the fp32 MFMA GEMM; weight gradients (TN) split over the token rows."""
    C = torch.empty(M, N, device=A.device) if out is None else out
    split, slabs = 1, None
    if layout == 2:
        tiles = ((M + 127) // 128) * ((N + 127) // 128)
        split = max(1, min(32, 256 // tiles, K // 512))
        if split > 1:
            slabs = torch.empty(split * M * N, device=A.device)
    _run("pl_gemm_f32", layout, A.data_ptr(), B.data_ptr(), C.data_ptr(), M, N, K, _ptr(bias), split, _ptr(slabs))
    return C


def _pad32(n):
    return (n + 31) // 32 * 32


# ------------------------------------------------------------------------------------------------ the operand layer
# An OPERAND is what a block GEMM reads: the fp32 tensor itself ("fp32") or a _Planes ("f16x3", "bf16p").  A mode object
# says where a producing kernel writes (dest, carrier), how what it wrote becomes an operand, and computes the three
# products; the block below is written once against it and never looks at compute_dtype.
class _Planes:
    """A planes-GEMM operand [rows][cols] in the carrier p [rows_pad][cols] (padding rows zero): two fp16 planes and the
    device scale {S, 1/S, 1/(S S_other)} ("f16x3"), or one bf16 plane and no scale ("bf16p")."""
    __slots__ = ("p", "scale", "rows", "cols", "rows_pad")

    def __init__(self, p, scale, rows):
        self.p, self.scale, self.rows = p, scale, rows
        self.rows_pad, self.cols = p.shape

    def inv(self, i):
        """scale[i] as the GEMM's device-side factor (None: no scale)."""
        return self.scale[i:i + 1] if self.scale is not None else None


class _Fp32:
    """Every block Linear on pl_gemm_f32."""

    def __init__(self, model, T, dev):
        self.model, self.T, self.Tp, self.dev = model, T, _pad32(T), dev

    def carrier(self, cols):
        """The bf16 carrier [Tp][cols] a producing kernel writes next to its fp32 output ("bf16p"; the others: None)."""
        return None

    def dest(self, cols):
        """(fp32 output or None, carrier or None) for a value [T][cols] that only GEMMs read."""
        return torch.empty(self.T, cols, device=self.dev), None

    def operand(self, x, carrier, partner=None):
        """The operand of x as its producer left it (x fp32 or None, carrier or None); partner: the operand x meets in the
        weight gradient."""
        return x

    def linear(self, a, w, bias=None):
        """y [T][N] = a W^T (+ bias), W [N][K]."""
        return _gemm_f32(0, a, w, self.T, w.shape[0], w.shape[1], bias)

    def wgrad(self, g, a):
        """dW [g cols][a cols] = g^T a."""
        return _gemm_f32(2, g, a, g.shape[1], a.shape[1], self.T)

    def dgrad(self, g, w):
        """dx [T][K] = g W."""
        return _gemm_f32(1, g, w, self.T, w.shape[1], w.shape[0])


class _F16x3(_Fp32):
    """pl_gemm_planes_raw on fp16 planes: every operand split from its fp32 value by pl_vit_planes_dyn."""
    mode, w_inv = _lib.PL_F16X3, 1.0 / conv.WEIGHT_PLANE_SCALE

    def operand(self, x, carrier, partner=None):
        p, scale = torch.empty(self.Tp, x.shape[1], device=self.dev), torch.empty(4, device=self.dev)
        scratch = torch.empty(_lib.lib().pl_vit_planes_scratch_bytes(), dtype=torch.uint8, device=self.dev)
        _run("pl_vit_planes_dyn", x.data_ptr(), self.T, x.shape[1], self.Tp, _ptr(partner.scale if partner is not None else None),
             scale.data_ptr(), p.data_ptr(), scratch.data_ptr())
        return _Planes(p, scale, self.T)

    def linear(self, a, w, bias=None):
        (N, K), M, wp = w.shape, a.rows, self.model._wplanes(w)[0]
        C = torch.empty(M, N, device=self.dev)
        splits = _lib.lib().pl_gemm_planes_splits(M, N, K)
        slabs = torch.empty(splits * M * N, device=self.dev) if splits > 1 else None
        _run("pl_gemm_planes_raw", 0, self.mode, a.p.data_ptr(), a.rows_pad * K, K, wp.data_ptr(), N * K, K, C.data_ptr(), M, N, K,
             _ptr(bias if splits == 1 else None), self.w_inv, a.scale.data_ptr() + 4 if a.scale is not None else None,
             _ptr(slabs), None)
        if bias is not None and splits > 1:
            C.add_(bias)
        return C

    def wgrad(self, g, a):
        """Over the zero-padded rows; g was split with partner=a, so g.scale[2] = 1 / (S_g S_a)."""
        return conv._gemm_planes_raw(2, g.p, (g.rows_pad, g.cols), a.p, (a.rows_pad, a.cols), g.cols, a.cols, g.rows_pad, 1.0,
                                     g.inv(2), self.mode)

    def dgrad(self, g, w):
        """NT on the planes of W^T [K][N]."""
        return conv._gemm_planes_raw(0, g.p, (g.rows_pad, g.cols), self.model._wplanes(w)[1], (w.shape[1], g.cols), g.rows,
                                     w.shape[1], g.cols, self.w_inv, g.inv(1), self.mode)


class _Bf16p(_F16x3):
    """pl_gemm_planes_raw on bf16 carriers the producers write themselves: no fp32 copy of a GEMM-only value, no scale."""
    mode, w_inv = _lib.PL_BF16, 1.0

    def carrier(self, cols):
        return torch.empty(self.Tp, cols, dtype=torch.bfloat16, device=self.dev)

    def dest(self, cols):
        return None, self.carrier(cols)

    def operand(self, x, carrier, partner=None):
        if carrier is None:                 # no producer wrote one: the head's fp32 GEMM made x
            carrier = self.carrier(x.shape[1])
            _run("pl_vit_bf16_pack", x.data_ptr(), self.T, x.shape[1], self.Tp, carrier.data_ptr())
        return _Planes(carrier, None, self.T)


_MODES = {"fp32": _Fp32, "f16x3": _F16x3, "bf16p": _Bf16p}


def _block_fwd(ops, blk, x, add, B, seq, eps):
    """One block: x (+ add: the previous block's mlp output) is the residual stream.  Returns (xa, m, what the backward
    keeps): the next block's x and add."""
    (g1, b1, g2, b2, wqkv, wout, g3, b3, w0, b0, w2, b2m) = blk
    T, Tp, dev, H, heads = ops.T, ops.Tp, ops.dev, ops.model.hidden_d, ops.model.n_heads
    xb = torch.empty(T, H, device=dev) if add is not None else x
    a, a_c = ops.dest(H)
    st12 = torch.empty(4, T, device=dev)
    _run("pl_vit_ln_fwd_bf16", x.data_ptr(), _ptr(add), T, H, 2, g1.data_ptr(), b1.data_ptr(), g2.data_ptr(), b2.data_ptr(),
         eps, _ptr(xb if add is not None else None), _ptr(a), _ptr(a_c), Tp, st12.data_ptr())
    a = ops.operand(a, a_c)
    qkv = ops.linear(a, wqkv)
    o, o_c = ops.dest(H)
    lse = torch.empty(B, heads, seq, device=dev)
    _run("pl_vit_attn_fwd_bf16", qkv.data_ptr(), B, seq, heads, DIM_HEAD, DIM_HEAD ** -0.5, _ptr(o), _ptr(o_c), Tp,
         lse.data_ptr())
    o = ops.operand(o, o_c)
    u = ops.linear(o, wout)
    xa = torch.empty(T, H, device=dev)
    n2, n2_c = ops.dest(H)
    st3 = torch.empty(2, T, device=dev)
    _run("pl_vit_ln_fwd_bf16", xb.data_ptr(), u.data_ptr(), T, H, 1, g3.data_ptr(), b3.data_ptr(), None, None, eps,
         xa.data_ptr(), _ptr(n2), _ptr(n2_c), Tp, st3.data_ptr())
    n2 = ops.operand(n2, n2_c)
    h = ops.linear(n2, w0, b0)
    g, g_c = ops.dest(4 * H)
    _run("pl_vit_gelu_fwd_bf16", h.data_ptr(), T, 4 * H, Tp, _ptr(g), _ptr(g_c))
    g = ops.operand(g, g_c)
    m = ops.linear(g, w2, b2m)
    return xa, m, dict(xb=xb, st12=st12, a=a, qkv=qkv, lse=lse, o=o, xa=xa, st3=st3, n2=n2, h=h, g=g)


def _block_bwd(ops, s, blk, grads, base, dx, dx_c, B, seq, lnscratch, want_carrier):
    """The backward of one block: dx is the gradient of its output (the residual stream), dx_c its carrier if a producer
    wrote one.  Fills grads[base:base + 12]; returns (dx of the block input, its carrier when want_carrier)."""
    (g1, b1, g2, b2, wqkv, wout, g3, b3, w0, b0, w2, b2m) = blk
    T, Tp, dev, H, heads = ops.T, ops.Tp, ops.dev, ops.model.hidden_d, ops.model.n_heads
    # mlp: m = mlp.2(GELU(mlp.0(n2)));  dm = dx
    dm = ops.operand(dx, dx_c, s["g"])
    grads[base + 10] = ops.wgrad(dm, s["g"])
    dg = ops.dgrad(dm, w2)
    grads[base + 11] = _colsum(dx)
    dh_c = ops.carrier(4 * H)
    _run("pl_vit_gelu_bwd_bf16", s["h"].data_ptr(), dg.data_ptr(), T, 4 * H, Tp, dg.data_ptr(), _ptr(dh_c))
    dh = ops.operand(dg, dh_c, s["n2"])                    # (dg now holds dh in fp32)
    grads[base + 8] = ops.wgrad(dh, s["n2"])
    dn2 = ops.dgrad(dh, w0)
    grads[base + 9] = _colsum(dg)
    del dg, dh, dh_c
    # norm2 with the residual: dxa = dx + LN3'(dn2)
    dxa = torch.empty(T, H, device=dev)
    dxa_c = ops.carrier(H)
    dgb3 = torch.empty(2 * H, device=dev)
    _run("pl_vit_ln_bwd_bf16", dn2.data_ptr(), dx.data_ptr(), s["xa"].data_ptr(), s["st3"].data_ptr(), T, H, 1, g3.data_ptr(),
         None, None, dxa.data_ptr(), _ptr(dxa_c), Tp, dgb3.data_ptr(), lnscratch.data_ptr())
    grads[base + 6], grads[base + 7] = dgb3[:H], dgb3[H:]
    # attention: u = to_out(o)
    du = ops.operand(dxa, dxa_c, s["o"])
    grads[base + 5] = ops.wgrad(du, s["o"])
    do = ops.dgrad(du, wout)
    dqkv, dq_c = ops.dest(3 * H)
    _run("pl_vit_attn_bwd_bf16", s["qkv"].data_ptr(), s["lse"].data_ptr(), do.data_ptr(), B, seq, heads, DIM_HEAD,
         DIM_HEAD ** -0.5, _ptr(dqkv), _ptr(dq_c), Tp)
    dq = ops.operand(dqkv, dq_c, s["a"])
    grads[base + 4] = ops.wgrad(dq, s["a"])
    da = ops.dgrad(dq, wqkv)
    # norm1 -> mhsa.norm with the residual: dx = dxa + LN1'(LN2'(da))
    dxb = torch.empty(T, H, device=dev)
    dxb_c = ops.carrier(H) if want_carrier else None
    dgb12 = torch.empty(4 * H, device=dev)
    _run("pl_vit_ln_bwd_bf16", da.data_ptr(), dxa.data_ptr(), s["xb"].data_ptr(), s["st12"].data_ptr(), T, H, 2,
         g1.data_ptr(), b1.data_ptr(), g2.data_ptr(), dxb.data_ptr(), _ptr(dxb_c), Tp, dgb12.data_ptr(), lnscratch.data_ptr())
    grads[base + 0], grads[base + 1] = dgb12[:H], dgb12[H:2 * H]
    grads[base + 2], grads[base + 3] = dgb12[2 * H:3 * H], dgb12[3 * H:]
    return dxb, dxb_c


def _colsum(x):
    rows, cols = x.shape
    out = torch.empty(cols, device=x.device)
    scratch = torch.empty(_lib.lib().pl_colsum_scratch_bytes(rows, cols), dtype=torch.uint8, device=x.device)
    _run("pl_colsum", x.data_ptr(), rows, cols, out.data_ptr(), scratch.data_ptr())
    return out


def _check_versions(model, ps, vers):
    """Eager torch's rule for tensors saved for backward: the backward reads the parameters as they are now (the GEMMs,
    the weight planes), so a parameter changed since the forward would mix two versions of the weights."""
    for i, (p, v) in enumerate(zip(ps, vers)):
        if p._version != v:
            name = next((n for n, q in model.named_parameters() if q is p), f"#{i}")
            raise RuntimeError(f"MyViT backward: parameter {name} was modified by an inplace operation or a FlatAdam step "
                               f"after the forward (version {v} -> {p._version})")


class _ViTFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, want, x2d, *ps):
        B, seq, in_d = x2d.shape
        H, out_d = model.hidden_d, model.out_d
        T, dev = B * seq, x2d.device
        ops = _MODES[model.compute_dtype](model, T, dev)
        eps = 1e-5
        Wm, bm, pos = ps[0], ps[1], ps[2]
        saved = []
        with _lib.on_device(dev):
            x = torch.empty(T, H, device=dev)
            _run("pl_vit_embed_fwd", x2d.data_ptr(), T, in_d, seq, Wm.data_ptr(), bm.data_ptr(), pos.data_ptr(), H, x.data_ptr())
            add = None
            for bi in range(model.n_block):
                x, add, s = _block_fwd(ops, ps[3 + 12 * bi: 15 + 12 * bi], x, add, B, seq, eps)
                if want:
                    saved.append(s)
            xf = torch.empty(T, H, device=dev)
            _run("pl_vit_ln_fwd_bf16", x.data_ptr(), add.data_ptr(), T, H, 0, None, None, None, None, eps, xf.data_ptr(), None,
                 None, 0, None)
            wh, bh, wl, bl = ps[-4:]
            z = _gemm_f32(0, xf, wh, T, H // 2, H, bh)
            y = torch.empty(B, seq, out_d, device=dev)
            _run("pl_vit_head_fwd", z.data_ptr(), T, H // 2, wl.data_ptr(), bl.data_ptr(), out_d, y.data_ptr())
        if want:
            ctx.model, ctx.saved, ctx.x2d, ctx.xf, ctx.z, ctx.ps = model, saved, x2d, xf, z, ps
            ctx.ops, ctx.dims = ops, (B, seq, in_d, T)
            ctx.versions = tuple(p._version for p in ps)     # (a FlatAdam step bumps them too)
        return y

    @staticmethod
    def backward(ctx, dy):
        model, saved, ps, ops = ctx.model, ctx.saved, ctx.ps, ctx.ops
        _check_versions(model, ps, ctx.versions)
        B, seq, in_d, T = ctx.dims
        H, out_d = model.hidden_d, model.out_d
        dev = dy.device
        dy = dy.float().contiguous()
        grads = [None] * len(ps)
        L = _lib.lib()
        with _lib.on_device(dev):
            wh, bh, wl, bl = ps[-4:]
            dz = torch.empty(T, H // 2, device=dev)
            dwbl = torch.empty(out_d * (H // 2) + out_d, device=dev)
            scratch = torch.empty(L.pl_vit_head_bwd_scratch_bytes(T, H // 2, out_d), dtype=torch.uint8, device=dev)
            _run("pl_vit_head_bwd", dy.data_ptr(), ctx.z.data_ptr(), T, H // 2, wl.data_ptr(), out_d, dz.data_ptr(),
                 dwbl.data_ptr(), scratch.data_ptr())
            grads[-2], grads[-1] = dwbl[:out_d * (H // 2)].view(out_d, H // 2), dwbl[out_d * (H // 2):]
            grads[-4] = _gemm_f32(2, dz, ctx.xf, H // 2, H, T)
            grads[-3] = _colsum(dz)
            dx = _gemm_f32(1, dz, wh, T, H, H // 2)              # d(block output) = d(x_final)
            dx_c = None                                         # (the head's fp32 GEMM writes no carrier)
            lnscratch = torch.empty(max(L.pl_vit_ln_bwd_scratch_bytes(T, H, 2), 4), dtype=torch.uint8, device=dev)
            for bi in reversed(range(model.n_block)):
                base = 3 + 12 * bi                              # (block 0's input gradient meets no GEMM: no carrier)
                dx, dx_c = _block_bwd(ops, saved[bi], ps[base: base + 12], grads, base, dx, dx_c, B, seq, lnscratch, bi > 0)
            Wm, pos = ps[0], ps[2]
            dwb = torch.empty(H * in_d + H, device=dev)
            dpos = torch.empty(seq, H, device=dev) if ctx.needs_input_grad[5] else None
            need_x = ctx.needs_input_grad[2]
            dx2d = torch.empty(B, seq, in_d, device=dev) if need_x else None
            scratch = torch.empty(L.pl_vit_embed_bwd_scratch_bytes(T, in_d, H), dtype=torch.uint8, device=dev)
            _run("pl_vit_embed_bwd", dx.data_ptr(), ctx.x2d.data_ptr(), T, in_d, seq, H, Wm.data_ptr(), dwb.data_ptr(),
                 _ptr(dpos), _ptr(dx2d), scratch.data_ptr())
            grads[0], grads[1], grads[2] = dwb[:H * in_d].view(H, in_d), dwb[H * in_d:], dpos
        ctx.saved = ctx.ps = ctx.xf = ctx.z = ctx.x2d = None
        out = []
        for i, (p, gr) in enumerate(zip(ps, grads)):
            out.append(gr.view(p.shape) if (gr is not None and ctx.needs_input_grad[3 + i]) else None)
        return (None, None, dx2d) + tuple(out)


def supported(seq, hidden_d, n_heads):
    """Shapes the kernels take (the constructor raises PoseliftError on the others)."""
    try:
        _check_shape((1, seq, 2), 1, hidden_d, n_heads, 3)
    except _lib.PoseliftError:
        return False
    return True


__all__ = ["MyViT", "positional_embeddings", "supported"]
