"""Planes-convolution entry points, host-side contract (no GPU): the exported names that share a launcher in csrc/api.hip
refuse the same bad calls with the same return code, each under its own name in pl_last_error(), before any HIP call.

EVERY call in this file must fail in argument validation.  The pointers are made-up addresses (16 and 24): a call with
nothing wrong would launch a kernel on them where there is a GPU.  _call() therefore asserts, for each call, a non-zero
return AND a message that starts with the entry point's own name (a launch that got as far as the runtime reports under
the kernel's name); when adding a case, check it by hand against the checks in api.hip first."""
import ctypes

import pytest

EINVAL, ESHAPE, EDTYPE, EWORKSPACE = -1, -2, -3, -6          # include/poselift.h


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()


one, odd = ctypes.c_void_p(16), ctypes.c_void_p(24)           # non-null, never dereferenced on these paths; `odd`: 8-byte aligned only


def _call(L, name, *args):
    """(return code, message) of a call that must fail under `name` (the _hw forms report under the name without _hw)."""
    rc, msg = getattr(L, name)(*args, None), L.pl_last_error()
    assert rc != 0 and msg.startswith(name.replace("_hw", "").encode() + b":"), (name, rc, msg)
    return rc, msg


def test_conv_planes_forward_names_share_their_checks(pkg):
    L, F16, BF = pkg.lib(), pkg._lib.PL_F16X3, pkg._lib.PL_BF16
    Ep = pkg._lib.PLPlanesEpilogue

    def four(mode=F16, x=one, w=one, y=one, B=2, H=8, W=8, cin=32, cout=32, k=3, stride=1, pad=1, ep=None):
        """The same bad convolution through the names that share the launcher: (square | per-axis geometry) x (training |
        eval-epilogue form).  With an epilogue only the two eval names are called: the training names take none, and a
        call with nothing wrong must not be made with these pointers."""
        head = (mode, x, B * H * W * cin, B, H, W, cin, w, cout * k * k * cin, cout, k, k)
        sq, hw = (stride, pad), (stride, stride, pad, pad, pad)
        if ep is not None:
            return [_call(L, "pl_conv2d_planes_fwd_ep", *head, *sq, y, 1.0, ctypes.byref(ep)),
                    _call(L, "pl_conv2d_planes_fwd_ep_hw", *head, *hw, y, 1.0, ctypes.byref(ep))]
        return [_call(L, "pl_conv2d_planes_fwd", *head, *sq, y, 1.0, None, None),
                _call(L, "pl_conv2d_planes_fwd_hw", *head, *hw, y, 1.0, None, None),
                _call(L, "pl_conv2d_planes_fwd_ep", *head, *sq, y, 1.0, None),
                _call(L, "pl_conv2d_planes_fwd_ep_hw", *head, *hw, y, 1.0, None)]

    for bad, code, word in ((dict(mode=7), EDTYPE, b"mode"), (dict(mode=pkg._lib.PL_BF16X6), EDTYPE, b"mode"),
                            (dict(x=None), EINVAL, b"null"), (dict(w=None), EINVAL, b"null"), (dict(y=None), EINVAL, b"null"),
                            (dict(cout=0), EINVAL, b"null"), (dict(B=0), ESHAPE, b"geometry"), (dict(stride=0), ESHAPE, b"geometry"),
                            (dict(pad=-1, mode=BF), ESHAPE, b"geometry"), (dict(H=1, W=1, k=5, pad=0), ESHAPE, b"geometry"),
                            (dict(B=1 << 20, H=64, W=64), ESHAPE, b"geometry")):
        for rc, msg in four(**bad):
            assert rc == code and word in msg, (bad, rc, msg)

    # what only an epilogue can get wrong: the two eval names agree (the training names take no epilogue)
    def ep(**kw):
        e = Ep()
        for k, v in kw.items():
            setattr(e, k, v.value if isinstance(v, ctypes.c_void_p) else v)
        return e
    for e, word in ((ep(relu=3), b"relu"), (ep(relu=-1), b"relu"), (ep(scale=one), b"scale without shift"),
                    (ep(shift=one, relu=1), b"scale without shift"), (ep(y_planes=odd), b"y_planes misaligned")):
        for rc, msg in four(ep=e):
            assert rc == EINVAL and word in msg, (word, rc, msg)
    for rc, msg in four(ep=ep(y_planes=one), cout=4, cin=32, B=1, H=1, W=1, k=1, pad=0):     # 4 outputs: not whole 8s
        assert rc == EINVAL and b"y_planes misaligned" in msg
    # y may be NULL only when the epilogue has planes to write instead
    for rc, msg in four(y=None, ep=ep(relu=1)):
        assert rc == EINVAL and b"null" in msg


def test_deconv_planes_forward_names_share_their_checks(pkg):
    L, F16 = pkg.lib(), pkg._lib.PL_F16X3
    Ep = pkg._lib.PLPlanesEpilogue

    def two(mode=F16, x=one, w=one, y=one, B=2, H=8, W=8, cin=32, cout=32, ep=None):
        head = (mode, x, B * H * W * cin, B, H, W, cin, w, 16 * cout * cin, cout, y, 1.0)
        if ep is not None:               # (only the eval name takes one)
            return [_call(L, "pl_deconv4x4s2_planes_fwd_ep", *head, ctypes.byref(ep))]
        return [_call(L, "pl_deconv4x4s2_planes_fwd", *head, None), _call(L, "pl_deconv4x4s2_planes_fwd_ep", *head, None)]

    for bad, code, word in ((dict(mode=0), EDTYPE, b"mode"), (dict(x=None), EINVAL, b"null"), (dict(w=None), EINVAL, b"null"),
                            (dict(y=None), EINVAL, b"null"), (dict(cout=0), EINVAL, b"null"), (dict(H=0), ESHAPE, b"geometry"),
                            (dict(cin=0), ESHAPE, b"geometry"), (dict(B=1 << 20, H=64, W=64), ESHAPE, b"geometry")):
        for rc, msg in two(**bad):
            assert rc == code and word in msg, (bad, rc, msg)
    e = Ep()
    e.resid = one.value
    rc, msg = two(ep=e)[0]
    assert rc == EINVAL and b"no residual on a transposed convolution" in msg
    for e, word in ((Ep(relu=5), b"relu"), (Ep(scale=one.value), b"scale without shift"), (Ep(y_planes=odd.value), b"y_planes misaligned")):
        rc, msg = two(ep=e)[0]
        assert rc == EINVAL and word in msg, (word, rc, msg)


def test_direct_conv_scratch_queries_answer_for_the_route_of_each_rectangular_case(pkg):
    """pl_conv2d_nhwc_scratch_bytes_ex / pl_conv2d_nhwc_wgrad_scratch_bytes on the shapes tests/test_gpu_conv_shapes.py runs
    (tests/conv_shape_cases.py): the bytes of the route each row names -- none, splits x M x Cout floats of split-K slabs,
    the im2col buffer (forward: pixels and weight rows padded to whole K tiles; weight gradient: pixels x taps, unpadded),
    or the stem weight gradient's one partial per workgroup -- so a wrapper that sizes its scratch by the query hands the
    kernels of that route exactly what they index."""
    import conv_shape_cases as cs
    L = pkg.lib()
    for name, geom, bn, relu, res, bias, kernels, scratch in cs.FWD_CASES:
        B, H, W, Cin, Cout, k, stride, pad = geom
        got = L.pl_conv2d_nhwc_scratch_bytes_ex(B, H, W, Cin, Cout, k, k, stride, pad, int(bias), int(res), relu)
        assert got == cs.fwd_scratch_bytes(geom, scratch), (name, got)
        assert (got > 0) == (scratch[0] != "none"), name
    for name, geom, kernels, scratch, _ in cs.WGRAD_CASES:
        B, H, W, Cin, Cout, k, stride, pad = geom
        got = L.pl_conv2d_nhwc_wgrad_scratch_bytes(B, H, W, Cin, Cout, k, k, stride, pad)
        assert got == cs.wgrad_scratch_bytes(geom, scratch), (name, got)
    # the two sides of the stem weight gradient's LDS limit, as the cases assume them
    wo = {name: cs.out_hw(geom)[1] for name, geom, *_ in cs.WGRAD_CASES}
    assert wo["stem widest row"] == cs.STEM_WGRAD_MAX_WO and wo["stem past the widest row"] == cs.STEM_WGRAD_MAX_WO + 1
    assert (cs.STEM_WGRAD_MAX_WO * 64 + 7 * (2 * cs.STEM_WGRAD_MAX_WO + 5) * 3) * 4 == 64868 <= 65536
    # the stride-1 data gradient is the forward convolution of dy (Cout channels in, Cin out): no scratch on these shapes
    for name, geom, _, _, dgrad in cs.WGRAD_CASES:
        B, H, W, Cin, Cout, k, stride, pad = geom
        if dgrad is not None and stride == 1:
            Ho, Wo = cs.out_hw(geom)
            assert L.pl_conv2d_nhwc_scratch_bytes_ex(B, Ho, Wo, Cout, Cin, k, k, 1, k - 1 - pad, 0, 0, 0) == 0, name


def test_split_k_tail_of_gemm_and_weight_gradient(pkg):
    """pl_gemm_planes_raw and pl_conv2d_planes_wgrad[_hw] share the split-K launch: a problem the library splits over K
    needs slabs (and, for the GEMM, takes no bias or statistics)."""
    L, F16 = pkg.lib(), pkg._lib.PL_F16X3
    M, N, K = 64, 64, 1 << 16
    assert L.pl_gemm_planes_splits(M, N, K) > 1 and L.pl_gemm_planes_splits(4096, 4096, 64) == 1

    def gemm(layout=2, mode=F16, a=one, b=one, c=one, M=M, K=K, bias=None, slabs=None, stat=None):
        return _call(L, "pl_gemm_planes_raw", layout, mode, a, M * K, M, b, N * K, N, c, M, N, K, bias, 1.0, None, slabs, stat)
    rc, msg = gemm()
    assert rc == EWORKSPACE and b"K slices need slabs" in msg
    assert gemm(bias=one)[0] == EWORKSPACE                          # (the slabs are asked for first)
    for kw in (dict(bias=one), dict(stat=one)):
        rc, msg = gemm(slabs=one, **kw)
        assert rc == EINVAL and b"no bias / statistics on a split-K problem" in msg
    assert gemm(layout=3)[0] == EINVAL and gemm(mode=2)[0] == EDTYPE and gemm(a=None)[0] == EINVAL and gemm(M=0)[0] == ESHAPE

    def wgrad(mode=F16, dz=one, x=one, dw=one, B=64, H=32, W=32, cin=32, cout=64, k=3, stride=1, pad=1):
        head = (mode, dz, B * H * W * cout, x, B * H * W * cin, B, H, W, cin, cout, k, k)
        return [_call(L, "pl_conv2d_planes_wgrad", *head, stride, pad, dw, 1.0, None, None),
                _call(L, "pl_conv2d_planes_wgrad_hw", *head, stride, stride, pad, pad, pad, dw, 1.0, None, None)]
    assert L.pl_gemm_planes_splits(64, 9 * 32, 64 * 32 * 32) > 1
    for bad, code, word in ((dict(), EWORKSPACE, b"K slices need slabs"), (dict(mode=0), EDTYPE, b"mode"),
                            (dict(dz=None), EINVAL, b"null"), (dict(dw=None), EINVAL, b"null"), (dict(cout=0), EINVAL, b"null"),
                            (dict(stride=0), ESHAPE, b"geometry"), (dict(H=1, W=1, k=5, pad=0), ESHAPE, b"geometry")):
        for rc, msg in wgrad(**bad):
            assert rc == code and word in msg, (bad, rc, msg)


def test_bn_replicas_of_conv_py_is_the_rule_of_the_batchnorm_kernels(pkg):
    """conv._bn_replicas is a copy of csrc/batchnorm.hip bn_replicas (the view [rows / R][R C] the BatchNorm kernels take of a
    narrow map, and lay its ReLU bitmap out in): the join's masked sum reads the bitmap in that view.  The C rule is static,
    so the copy is tied to it twice: the function's text is the text the copy was made from -- whoever changes the rule
    changes both -- and pl_bn_join_bwd, which refuses exactly the maps with R != 1, refuses every map the copy folds."""
    import os
    import re
    import __graft_entry__ as ge
    with open(os.path.join(ge.CSRC, "batchnorm.hip")) as f:
        m = re.search(r"static int bn_replicas\(int64_t rows, int64_t C\) \{(.*?)\n\}", f.read(), re.S)
    assert m and " ".join(m.group(1).split()) == ("int r = C <= 64 ? 4 : (C <= 128 ? 2 : 1); "
                                                  "while (r > 1 && (rows % r != 0 || rows / r < 2)) r >>= 1; return r;")
    R = pkg.conv._bn_replicas
    want = {(120, 64): 4, (122, 64): 2, (65, 64): 1, (65, 24): 1, (4, 64): 2, (6, 32): 2, (2, 64): 1, (3, 8): 1, (8, 64): 4,
            (66, 128): 2, (67, 128): 1, (2, 128): 1, (4, 128): 2, (120, 132): 1, (65, 256): 1, (4096, 2048): 1, (33792, 64): 4}
    assert {k: R(*k) for k in want} == want
    L = pkg.lib()
    for (rows, C), r in want.items():
        if r != 1:                                 # (R == 1 would pass validation and launch on these pointers: never called)
            rc, msg = _call(L, "pl_bn_join_bwd", one, one, one, one, one, one, one, rows, C, one, one, one, one, one, None, 0, None)
            assert rc == ESHAPE and b"narrower than one 256-column strip" in msg, (rows, C, msg)
