"""Fused softmax + integral soft-argmax heads, computed by libposelift.so.

soft_argmax_3d  = the tail of Model_3D.forward   /root/reference/phase4_joined/Model.py:94-133
soft_argmax_2d  = the tail of Model_2D.forward   /root/reference/phase5_loop/Model_2d.py:96-134
Both take the final 1x1-conv output of the reference model and are differentiable; the normalised
heat-map (17.8 MB per frame in 3-D) is never materialised.
"""
import ctypes

import torch

from . import _lib


def _call(name, dev, *args):
    """One launching entry point of the library on dev's current stream."""
    with _lib.on_device(dev):
        rc = getattr(_lib.lib(), name)(*args, _lib.current_stream_ptr())
    _lib.check(rc, name)


# The two autograd nodes, one per layout.  target: None, or the (BJ, ncoord) fp32 heat-map target with sigma and the law array
# beside it -- then the _hm entry points run, the statistics are 8 wide instead of 5 and the node returns (coords, sq).
# backward(ctx, *grads) takes either form; an output the loss does not use arrives as zeros.

class _SoftArgmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, dims, target, sigma, law):
        BJ, D, H, W, ncoord, centred = dims
        dev = logits.device
        coords = torch.empty(BJ, ncoord, dtype=torch.float32, device=dev)
        if target is None:
            out, stats = coords, torch.empty(BJ, 5, dtype=torch.float32, device=dev)
            _call("pl_softargmax_fwd", dev, logits.data_ptr(), BJ, D, H, W, ncoord, centred, coords.data_ptr(), stats.data_ptr())
        else:
            sq = torch.empty(BJ, dtype=torch.float32, device=dev)
            out, stats = (coords, sq), torch.empty(BJ, 8, dtype=torch.float32, device=dev)
            _call("pl_softargmax_hm_fwd", dev, logits.data_ptr(), target.data_ptr(), BJ, D, H, W, ncoord, centred, sigma, law,
                  coords.data_ptr(), sq.data_ptr(), stats.data_ptr())
        ctx.save_for_backward(logits, stats, target)
        ctx.args = (dims, sigma, law)
        return out

    @staticmethod
    def backward(ctx, *grads):
        logits, stats, target = ctx.saved_tensors
        (BJ, D, H, W, ncoord, centred), sigma, law = ctx.args
        g = grads[0].contiguous()
        if target is None:
            dl = torch.empty_like(logits)
            _call("pl_softargmax_bwd", logits.device, logits.data_ptr(), stats.data_ptr(), g.data_ptr(), BJ, D, H, W, ncoord,
                  centred, dl.data_ptr())
        else:
            gsq = grads[1].contiguous()
            dl = torch.empty_like(logits)
            _call("pl_softargmax_hm_bwd", logits.device, logits.data_ptr(), target.data_ptr(), stats.data_ptr(), g.data_ptr(),
                  gsq.data_ptr(), BJ, D, H, W, ncoord, centred, sigma, law, dl.data_ptr())
        return dl, None, None, None, None


class _SoftArgmax3dNHWCFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, num_joints, target, sigma, law, link):
        B, H, W, _ = x.shape
        BJ, dev = B * num_joints, x.device
        coords = torch.empty(BJ, 3, dtype=torch.float32, device=dev)
        if target is None:
            out, stats = coords, torch.empty(BJ, 5, dtype=torch.float32, device=dev)
            _call("pl_softargmax3d_nhwc_fwd", dev, x.data_ptr(), B, num_joints, H, W, coords.data_ptr(), stats.data_ptr())
        else:
            sq = torch.empty(BJ, dtype=torch.float32, device=dev)
            out, stats = (coords, sq), torch.empty(BJ, 8, dtype=torch.float32, device=dev)
            _call("pl_softargmax3d_nhwc_hm_fwd", dev, x.data_ptr(), target.data_ptr(), B, num_joints, H, W, sigma, law,
                  coords.data_ptr(), sq.data_ptr(), stats.data_ptr())
        ctx.save_for_backward(x, stats, target)
        ctx.args = (num_joints, sigma, law, link)
        return out

    @staticmethod
    def backward(ctx, *grads):
        x, stats, target = ctx.saved_tensors
        num_joints, sigma, law, link = ctx.args
        B, H, W, _ = x.shape
        dev = x.device
        g = grads[0].contiguous()
        gsq = None if target is None else grads[1].contiguous()
        dl = torch.empty_like(x)
        f32, planes, mode, scale = dl.data_ptr(), None, 0, None
        if link is not None:
            # the final convolution runs on the planes GEMM (conv.py): dlogits leave as a carrier of their planes only, fp16
            # ones scaled by a power of two from the bound |dlogit| <= 2 max_(b,j) (sum_c |g_c| + 2 |gsq|) (softmax weights <= 1)
            link.dz_scale = torch.empty(2, dtype=torch.float32, device=dev)
            f32, planes, mode, scale = None, f32, link.mode, link.dz_scale.data_ptr()
            if target is None:
                _call("pl_softargmax_dl_scale", dev, g.data_ptr(), g.numel() // 3, 3, scale)
            else:
                _call("pl_softargmax_hm_dl_scale", dev, g.data_ptr(), gsq.data_ptr(), g.numel() // 3, 3, scale)
        if target is not None:
            _call("pl_softargmax3d_nhwc_hm_bwd_ex", dev, x.data_ptr(), target.data_ptr(), stats.data_ptr(), g.data_ptr(),
                  gsq.data_ptr(), B, num_joints, H, W, sigma, law, f32, planes, mode, scale)
        elif link is not None:
            _call("pl_softargmax3d_nhwc_bwd_ex", dev, x.data_ptr(), stats.data_ptr(), g.data_ptr(), B, num_joints, H, W, f32,
                  planes, mode, scale)
        else:
            _call("pl_softargmax3d_nhwc_bwd", dev, x.data_ptr(), stats.data_ptr(), g.data_ptr(), B, num_joints, H, W, f32)
        return dl, None, None, None, None, None


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
    return t.to(device=device, dtype=torch.float32).reshape(BJ, ncoord).contiguous()


def _node_args(hm, dims, centred, BJ, ncoord, device):
    """hm = None or (target, sigma, centre) -> the nodes' (target, sigma, law) for a map of dims = (W, H, D)."""
    if hm is None:
        return None, 0.0, None
    target, sigma, centre = hm
    law = _law_array(heatmap_law(*dims, centred, centre))
    return _hm_target(target, BJ, ncoord, device), float(sigma), law


def _shaped(out, B, num_joints, ncoord):
    if isinstance(out, tuple):
        return out[0].reshape(B, num_joints * ncoord), out[1].reshape(B, num_joints)
    return out.reshape(B, num_joints * ncoord)


def head_nchw(logits, num_joints, depth_dim, hm=None, centred=None):
    """What the four NCHW functions below do.  hm: None, or (target, sigma, centre) -> (coords, sq).  centred: the 3-D
    head's three coordinates in (-1, 1), or the 2-D head's two in (0, 1); None: by depth_dim (depth 1 is the 2-D head)."""
    centred = depth_dim > 1 if centred is None else centred
    ncoord = 3 if centred else 2
    B, C, H, W = logits.shape
    if C != num_joints * depth_dim:
        raise ValueError(f"expected {num_joints * depth_dim} channels, got {C}")
    x = _lib.aligned16(logits.contiguous().float())     # (both passes read the logits 16 bytes at a time)
    _lib.require_device_tensor(x, "heat-map logits")
    BJ = B * num_joints
    node_args = _node_args(hm, (W, H, depth_dim), centred, BJ, ncoord, x.device)
    return _shaped(_SoftArgmaxFn.apply(x, (BJ, depth_dim, H, W, ncoord, int(centred)), *node_args), B, num_joints, ncoord)


def head_nhwc(logits, num_joints, hm=None, link=None):
    """What the two NHWC functions below do; hm as in head_nchw, link: conv.PlaneLink of the final convolution or None."""
    x = _lib.aligned16(logits.contiguous())             # (the backward reads the logits 16 bytes at a time)
    _lib.require_device_tensor(x, "heat-map logits")
    B, H, W, C = x.shape
    if C != num_joints * 64:
        raise ValueError(f"expected {num_joints * 64} channels (depth 64), got {C}")
    node_args = _node_args(hm, (W, H, 64), True, B * num_joints, 3, x.device)
    return _shaped(_SoftArgmax3dNHWCFn.apply(x, num_joints, *node_args, link), B, num_joints, 3)


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


def soft_argmax_3d(out, num_joints=17, depth_dim=64):
    """(B, num_joints*depth_dim, H, W) logits -> (B, num_joints*3) coordinates in (-1, 1), (x, y, z) per joint."""
    return head_nchw(out, num_joints, depth_dim, None, True)


def soft_argmax_2d(out, num_joints=17):
    """(B, num_joints, H, W) logits -> (B, num_joints*2) coordinates in (0, 1), (x, y) per joint."""
    return head_nchw(out, num_joints, 1)


def soft_argmax_3d_nhwc(out, num_joints=17, link=None):
    """(B, H, W, num_joints*64) NHWC logits (depth_dim 64) -> (B, num_joints*3), differentiable: what Model_3D's
    final 1x1 convolution writes, read in place -- no NHWC <-> NCHW pass in either direction."""
    return head_nhwc(out, num_joints, None, link)


def soft_argmax_3d_hm(out, target, sigma=0.5, centre="head", num_joints=17, depth_dim=64):
    """soft_argmax_3d + heat-map supervision: (B, num_joints*depth_dim, H, W) logits and target coordinates (B, num_joints*3)
    in the head's own (x, y, z) order and range -> (coords (B, num_joints*3), sq (B, num_joints)); sq[b, j] is the squared
    error of joint j's normalised heat-map against the Gaussian target centred at its coordinate (gaussian_heatmap), summed
    over the voxels.  Both are differentiable in the logits; the target takes no gradient."""
    return head_nchw(out, num_joints, depth_dim, (target, sigma, centre), True)


def soft_argmax_2d_hm(out, target, sigma=0.5, centre="head", num_joints=17):
    """soft_argmax_2d + heat-map supervision: (B, num_joints, H, W) logits, target (B, num_joints*2) in (0, 1) ->
    (coords (B, num_joints*2), sq (B, num_joints)).  centre="reference" is not defined for this head."""
    return head_nchw(out, num_joints, 1, (target, sigma, centre))


def soft_argmax_3d_nhwc_hm(out, target, sigma=0.5, centre="head", num_joints=17, link=None):
    """soft_argmax_3d_nhwc + heat-map supervision on the NHWC logits (B, H, W, num_joints*64), read in place:
    -> (coords (B, num_joints*3), sq (B, num_joints)); see soft_argmax_3d_hm."""
    return head_nhwc(out, num_joints, (target, sigma, centre), link)
