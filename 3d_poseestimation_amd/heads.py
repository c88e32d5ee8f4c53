"""Fused softmax + integral soft-argmax heads, computed by libposelift.so.

soft_argmax_3d  = the tail of Model_3D.forward   /root/reference/phase4_joined/Model.py:94-133
soft_argmax_2d  = the tail of Model_2D.forward   /root/reference/phase5_loop/Model_2d.py:96-134
Both take the final 1x1-conv output of the reference model and are differentiable; the normalised
heat-map (17.8 MB per frame in 3-D) is never materialised.
"""
import ctypes

import torch

from . import _lib


class _SoftArgmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, BJ, D, H, W, ncoord, centred):
        _lib.require_device_tensor(logits, "heat-map logits")
        coords = torch.empty(BJ, ncoord, dtype=torch.float32, device=logits.device)
        stats = torch.empty(BJ, 5, dtype=torch.float32, device=logits.device)
        with _lib.on_device(logits.device):
            rc = _lib.lib().pl_softargmax_fwd(logits.data_ptr(), BJ, D, H, W, ncoord, centred, coords.data_ptr(),
                                              stats.data_ptr(), _lib.current_stream_ptr())
        _lib.check(rc, "pl_softargmax_fwd")
        ctx.save_for_backward(logits, stats)
        ctx.dims = (BJ, D, H, W, ncoord, centred)
        return coords

    @staticmethod
    def backward(ctx, g):
        logits, stats = ctx.saved_tensors
        BJ, D, H, W, ncoord, centred = ctx.dims
        g = g.contiguous()
        dl = torch.empty_like(logits)
        with _lib.on_device(logits.device):
            rc = _lib.lib().pl_softargmax_bwd(logits.data_ptr(), stats.data_ptr(), g.data_ptr(), BJ, D, H, W, ncoord,
                                              centred, dl.data_ptr(), _lib.current_stream_ptr())
        _lib.check(rc, "pl_softargmax_bwd")
        return dl, None, None, None, None, None, None


def soft_argmax_3d(out, num_joints=17, depth_dim=64):
    """(B, num_joints*depth_dim, H, W) logits -> (B, num_joints*3) coordinates in (-1, 1), (x, y, z) per joint."""
    B, C, H, W = out.shape
    if C != num_joints * depth_dim:
        raise ValueError(f"expected {num_joints * depth_dim} channels, got {C}")
    x = out.contiguous().float()
    return _SoftArgmaxFn.apply(x, B * num_joints, depth_dim, H, W, 3, 1).reshape(B, num_joints * 3)


def soft_argmax_2d(out, num_joints=17):
    """(B, num_joints, H, W) logits -> (B, num_joints*2) coordinates in (0, 1), (x, y) per joint."""
    B, C, H, W = out.shape
    if C != num_joints:
        raise ValueError(f"expected {num_joints} channels, got {C}")
    x = out.contiguous().float()
    return _SoftArgmaxFn.apply(x, B * num_joints, 1, H, W, 2, 0).reshape(B, num_joints * 2)


def _pow2_scale_for_bound(bound):
    """{S, 1/S} on the device: S the power of two that maps `bound` (a 0-d device tensor >= max |value|) into [2^13, 2^14)
    -- the range scale of fp16 operand planes (conv.py PlaneLink); bound 0 / inf / nan -> 1."""
    ok = torch.isfinite(bound) & (bound > 0)
    e = torch.frexp(torch.where(ok, bound, torch.ones_like(bound))).exponent
    S = torch.ldexp(torch.ones_like(bound), 14 - e)
    S = torch.where(ok, S, torch.ones_like(bound))
    return torch.stack([S, 1.0 / S]).float().contiguous()


class _SoftArgmax3dNHWCFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, num_joints, link=None):
        ctx.link = link
        B, H, W, _ = x.shape
        coords = torch.empty(B * num_joints, 3, dtype=torch.float32, device=x.device)
        stats = torch.empty(B * num_joints, 5, dtype=torch.float32, device=x.device)
        with _lib.on_device(x.device):
            rc = _lib.lib().pl_softargmax3d_nhwc_fwd(x.data_ptr(), B, num_joints, H, W, coords.data_ptr(),
                                                     stats.data_ptr(), _lib.current_stream_ptr())
        _lib.check(rc, "pl_softargmax3d_nhwc_fwd")
        ctx.save_for_backward(x, stats)
        ctx.num_joints = num_joints
        return coords

    @staticmethod
    def backward(ctx, g):
        x, stats = ctx.saved_tensors
        B, H, W, _ = x.shape
        g = g.contiguous()
        dl = torch.empty_like(x)
        link = ctx.link
        if link is not None:
            # the final convolution runs on the planes GEMM (conv.py): dlogits leave as a carrier of their planes, fp16 ones
            # scaled by a power of two from the bound |dlogit| <= 2 max_(b,j) sum_c |g_c| (softmax weights <= 1)
            link.dz_scale = torch.empty(2, dtype=torch.float32, device=x.device)
            with _lib.on_device(x.device):
                _lib.check(_lib.lib().pl_softargmax_dl_scale(g.data_ptr(), g.numel() // 3, 3, link.dz_scale.data_ptr(),
                                                             _lib.current_stream_ptr()), "pl_softargmax_dl_scale")
                rc = _lib.lib().pl_softargmax3d_nhwc_bwd_ex(x.data_ptr(), stats.data_ptr(), g.data_ptr(), B, ctx.num_joints, H, W,
                                                            None, dl.data_ptr(), link.mode, link.dz_scale.data_ptr(),
                                                            _lib.current_stream_ptr())
            _lib.check(rc, "pl_softargmax3d_nhwc_bwd_ex")
            return dl, None, None
        with _lib.on_device(x.device):
            rc = _lib.lib().pl_softargmax3d_nhwc_bwd(x.data_ptr(), stats.data_ptr(), g.data_ptr(), B, ctx.num_joints,
                                                     H, W, dl.data_ptr(), _lib.current_stream_ptr())
        _lib.check(rc, "pl_softargmax3d_nhwc_bwd")
        return dl, None, None


def soft_argmax_3d_nhwc(out, num_joints=17, link=None):
    """(B, H, W, num_joints*64) NHWC logits (depth_dim 64) -> (B, num_joints*3), differentiable: what Model_3D's
    final 1x1 convolution writes, read in place -- no NHWC <-> NCHW pass in either direction."""
    x = out.contiguous()
    _lib.require_device_tensor(x, "heat-map logits")
    B, H, W, C = x.shape
    if C != num_joints * 64:
        raise ValueError(f"expected {num_joints * 64} channels (depth 64), got {C}")
    return _SoftArgmax3dNHWCFn.apply(x, num_joints, link).reshape(B, num_joints * 3)


# ---- heat-map supervision: sq[b, j] = sum over voxels (softmax(logits) - Gaussian target)^2, neither tensor stored -------
# csrc/heatmap_target.h has the target's definition; the law that places its centre is chosen here.

def heatmap_law(width, height, depth=1, centred=True, centre="head"):
    """Public (exported by the package): the `law[6]` argument of the pl_*_hm_* and pl_heatmap_gaussian* entry points, for
    callers of the C ABI and for tests.  [alpha_x, alpha_y, alpha_z, gamma_x, gamma_y, gamma_z]: the centre index of a target coordinate t on axis a is
    mu_a = alpha_a * (t_a + gamma_a); axes (x, y, z) <-> (W, H, D), the order the heads emit.
      centre="head"       the inverse of the head's own coordinate law, so the coordinate loss and the heat-map loss have
                          the same minimiser: mu = (t/2 + 0.5) dim for the centred 3-D head, mu = t dim for the 2-D head
      centre="reference"  the dataset's law 31.5 (1 + t) (H36_dataset.py:163), i.e. (dim - 1)/2 (1 + t); centred heads only"""
    dims = (float(width), float(height), float(depth))
    if centre == "head":
        if centred:
            return [d / 2.0 for d in dims] + [1.0, 1.0, 1.0]
        return list(dims) + [0.0, 0.0, 0.0]
    if centre == "reference":
        if not centred:
            raise ValueError('centre="reference" is the dataset\'s law for coordinates in (-1, 1): centred heads only, '
                             'not the 2-D head')
        return [(d - 1.0) / 2.0 for d in dims] + [1.0, 1.0, 1.0]
    raise ValueError(f'centre is "head" or "reference", got {centre!r}')


def _law_array(law):
    return (ctypes.c_float * 6)(*law)


def _hm_target(target, BJ, ncoord, device):
    """The target coordinates as a contiguous fp32 (BJ, ncoord) device tensor; takes no gradient."""
    t = target.detach()
    if t.numel() != BJ * ncoord:
        raise ValueError(f"heat-map target has {t.numel()} values, expected {BJ} x {ncoord} (one coordinate set per joint)")
    t = t.to(device=device, dtype=torch.float32).reshape(BJ, ncoord).contiguous()
    return t


def gaussian_heatmap(target, dims, sigma=0.5, centre="head"):
    """The dense Gaussian target the fused loss is defined against, for visualisation and tests.
    target: (..., ncoord) device tensor of coordinates, ncoord = len(dims); dims = (D, H, W) for the centred 3-D head or
    (H, W) for the 2-D head.  Returns (BJ, D, H, W) fp32 (D = 1 for two dims), BJ the number of coordinate sets."""
    dims = tuple(int(d) for d in dims)
    if len(dims) == 3:
        D, H, W = dims
        ncoord, centred = 3, True
    elif len(dims) == 2:
        (H, W), D = dims, 1
        ncoord, centred = 2, False
    else:
        raise ValueError("dims is (D, H, W) or (H, W)")
    law = heatmap_law(W, H, D, centred, centre)
    if not target.is_cuda:
        raise _lib.PoseliftError(f"heat-map target is on {target.device}: the library computes on the device only")
    if target.numel() == 0 or target.numel() % ncoord:
        raise ValueError(f"target holds {target.numel()} values: not a whole number of {ncoord}-coordinate sets")
    BJ = target.numel() // ncoord
    t = _hm_target(target, BJ, ncoord, target.device)
    out = torch.empty(BJ, D, H, W, dtype=torch.float32, device=t.device)
    with _lib.on_device(t.device):
        rc = _lib.lib().pl_heatmap_gaussian(t.data_ptr(), BJ, D, H, W, ncoord, float(sigma), _law_array(law), out.data_ptr(),
                                            _lib.current_stream_ptr())
    _lib.check(rc, "pl_heatmap_gaussian")
    return out


class _SoftArgmaxHmFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, BJ, D, H, W, ncoord, centred, sigma, law):
        _lib.require_device_tensor(logits, "heat-map logits")
        coords = torch.empty(BJ, ncoord, dtype=torch.float32, device=logits.device)
        sq = torch.empty(BJ, dtype=torch.float32, device=logits.device)
        stats = torch.empty(BJ, 8, dtype=torch.float32, device=logits.device)
        with _lib.on_device(logits.device):
            rc = _lib.lib().pl_softargmax_hm_fwd(logits.data_ptr(), target.data_ptr(), BJ, D, H, W, ncoord, centred, sigma,
                                                 _law_array(law), coords.data_ptr(), sq.data_ptr(), stats.data_ptr(),
                                                 _lib.current_stream_ptr())
        _lib.check(rc, "pl_softargmax_hm_fwd")
        ctx.save_for_backward(logits, target, stats)
        ctx.dims = (BJ, D, H, W, ncoord, centred, sigma, law)
        return coords, sq

    @staticmethod
    def backward(ctx, g, gsq):
        logits, target, stats = ctx.saved_tensors
        BJ, D, H, W, ncoord, centred, sigma, law = ctx.dims
        g, gsq = g.contiguous(), gsq.contiguous()
        dl = torch.empty_like(logits)
        with _lib.on_device(logits.device):
            rc = _lib.lib().pl_softargmax_hm_bwd(logits.data_ptr(), target.data_ptr(), stats.data_ptr(), g.data_ptr(),
                                                 gsq.data_ptr(), BJ, D, H, W, ncoord, centred, sigma, _law_array(law),
                                                 dl.data_ptr(), _lib.current_stream_ptr())
        _lib.check(rc, "pl_softargmax_hm_bwd")
        return (dl,) + (None,) * 9


def soft_argmax_3d_hm(out, target, sigma=0.5, centre="head", num_joints=17, depth_dim=64):
    """soft_argmax_3d + heat-map supervision: (B, num_joints*depth_dim, H, W) logits and target coordinates (B, num_joints*3)
    in the head's own (x, y, z) order and range -> (coords (B, num_joints*3), sq (B, num_joints)); sq[b, j] is the squared
    error of joint j's normalised heat-map against the Gaussian target centred at its coordinate (gaussian_heatmap), summed
    over the voxels.  Both are differentiable in the logits; the target takes no gradient."""
    B, C, H, W = out.shape
    if C != num_joints * depth_dim:
        raise ValueError(f"expected {num_joints * depth_dim} channels, got {C}")
    x = out.contiguous().float()
    law = heatmap_law(W, H, depth_dim, True, centre)
    t = _hm_target(target, B * num_joints, 3, x.device)
    coords, sq = _SoftArgmaxHmFn.apply(x, t, B * num_joints, depth_dim, H, W, 3, 1, float(sigma), law)
    return coords.reshape(B, num_joints * 3), sq.reshape(B, num_joints)


def soft_argmax_2d_hm(out, target, sigma=0.5, centre="head", num_joints=17):
    """soft_argmax_2d + heat-map supervision: (B, num_joints, H, W) logits, target (B, num_joints*2) in (0, 1) ->
    (coords (B, num_joints*2), sq (B, num_joints)).  centre="reference" is not defined for this head."""
    B, C, H, W = out.shape
    if C != num_joints:
        raise ValueError(f"expected {num_joints} channels, got {C}")
    x = out.contiguous().float()
    law = heatmap_law(W, H, 1, False, centre)
    t = _hm_target(target, B * num_joints, 2, x.device)
    coords, sq = _SoftArgmaxHmFn.apply(x, t, B * num_joints, 1, H, W, 2, 0, float(sigma), law)
    return coords.reshape(B, num_joints * 2), sq.reshape(B, num_joints)


class _SoftArgmax3dNHWCHmFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target, num_joints, sigma, law, link=None):
        ctx.link = link
        B, H, W, _ = x.shape
        coords = torch.empty(B * num_joints, 3, dtype=torch.float32, device=x.device)
        sq = torch.empty(B * num_joints, dtype=torch.float32, device=x.device)
        stats = torch.empty(B * num_joints, 8, dtype=torch.float32, device=x.device)
        with _lib.on_device(x.device):
            rc = _lib.lib().pl_softargmax3d_nhwc_hm_fwd(x.data_ptr(), target.data_ptr(), B, num_joints, H, W, sigma,
                                                        _law_array(law), coords.data_ptr(), sq.data_ptr(), stats.data_ptr(),
                                                        _lib.current_stream_ptr())
        _lib.check(rc, "pl_softargmax3d_nhwc_hm_fwd")
        ctx.save_for_backward(x, target, stats)
        ctx.args = (num_joints, sigma, law)
        return coords, sq

    @staticmethod
    def backward(ctx, g, gsq):
        x, target, stats = ctx.saved_tensors
        num_joints, sigma, law = ctx.args
        B, H, W, _ = x.shape
        g, gsq = g.contiguous(), gsq.contiguous()
        dl = torch.empty_like(x)
        link = ctx.link
        scale, planes_mode, f32 = None, 0, dl.data_ptr()
        with _lib.on_device(x.device):
            if link is not None:
                # as _SoftArgmax3dNHWCFn: dlogits leave as a carrier of their planes; the fp16 scale's bound grows by 4 |gsq|
                link.dz_scale = torch.empty(2, dtype=torch.float32, device=x.device)
                _lib.check(_lib.lib().pl_softargmax_hm_dl_scale(g.data_ptr(), gsq.data_ptr(), g.numel() // 3, 3,
                                                                link.dz_scale.data_ptr(), _lib.current_stream_ptr()),
                           "pl_softargmax_hm_dl_scale")
                scale, planes_mode, f32 = link.dz_scale.data_ptr(), link.mode, None
            rc = _lib.lib().pl_softargmax3d_nhwc_hm_bwd_ex(x.data_ptr(), target.data_ptr(), stats.data_ptr(), g.data_ptr(),
                                                           gsq.data_ptr(), B, num_joints, H, W, sigma, _law_array(law), f32,
                                                           dl.data_ptr() if link is not None else None, planes_mode, scale,
                                                           _lib.current_stream_ptr())
        _lib.check(rc, "pl_softargmax3d_nhwc_hm_bwd_ex")
        return dl, None, None, None, None, None


def soft_argmax_3d_nhwc_hm(out, target, sigma=0.5, centre="head", num_joints=17, link=None):
    """soft_argmax_3d_nhwc + heat-map supervision on the NHWC logits (B, H, W, num_joints*64), read in place:
    -> (coords (B, num_joints*3), sq (B, num_joints)); see soft_argmax_3d_hm."""
    x = out.contiguous()
    _lib.require_device_tensor(x, "heat-map logits")
    B, H, W, C = x.shape
    if C != num_joints * 64:
        raise ValueError(f"expected {num_joints * 64} channels (depth 64), got {C}")
    law = heatmap_law(W, H, 64, True, centre)
    t = _hm_target(target, B * num_joints, 3, x.device)
    coords, sq = _SoftArgmax3dNHWCHmFn.apply(x, t, num_joints, float(sigma), law, link)
    return coords.reshape(B, num_joints * 3), sq.reshape(B, num_joints)
