"""The alignment contract of caller pointers, host side (no GPU).

  * every entry point and pointer the audit marks "C check": an 8-byte and a 4-byte aligned made-up address are refused with
    PL_EINVAL and a message that names the argument and says "16-byte aligned"; the 16-byte aligned address gets past that
    check and the call fails on something checked after it.  The checks that existed before the audit (metrics, heads, ViT)
    are pinned the same way; pointers the audit marks gate / scalar are NOT refused.
  * _lib.aligned16, and the wrappers that apply it: no misaligned pointer reaches an entry point that refuses.
  * tests/alignment_cases.py: its views sit where they claim, its sentinel check fires.
  * the DESIGN.md table names every pl_* symbol of include/poselift.h that has a pointer parameter.

EVERY library call in this file must fail in argument validation: the pointers are made-up addresses, a call with nothing
wrong would launch a kernel on them where there is a GPU (as tests/test_grad_clip_host.py, tests/test_conv_planes_host.py)."""
import ctypes
import os
import re

import pytest
import torch

import alignment_cases as ac
from conftest import ROOT

EINVAL = -1
one, odd, word = ctypes.c_void_p(16), ctypes.c_void_p(24), ctypes.c_void_p(20)   # 16-, 8- and 4-byte aligned made-up addresses
off4 = ctypes.c_void_p(18)                                                        # not even 4-byte aligned


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()


def _desc(lib):
    d = lib.PLDesc(in_dim=34, hidden=128, out_dim=51, num_stage=1, bn=1, dtype=lib.PL_F32, p_dropout=0.5, bn_eps=1e-5,
                   bn_momentum=0.1)
    d.params, d.bn_running = 16, 16
    return d


def _specs(lib):
    """(entry point, arguments with every pointer 16-byte aligned and ONE thing wrong that is checked after the alignment,
    {argument index: the name the message must carry}, indices of pointers the contract leaves free).  The one wrong thing:
    an empty batch / map, an unknown arithmetic, a carrier too short."""
    d = ctypes.byref(_desc(lib))
    st = lib.PLAdamWStep(m=16, v=16, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, t=1)
    opt = ctypes.byref(st)
    o = one
    X6 = lib.PL_BF16X6
    S = []
    # ---- the lifter: x where a forward stages it as float4 (the saved-activation forwards and the fused steps), dy on the
    # backward ones; x of the plain eval forward and of the backward, y, dx, target, loss are free
    S += [("pl_lifter_fwd_eval", [d, o, o, 0, o, 0, None], {}, [1, 2]),
          ("pl_lifter_fwd_train", [d, o, o, 0, o, 0, 0, 0, None, None], {1: "x"}, [2]),
          ("pl_lifter_fwd_eval_saved", [d, o, o, 0, o, 0, None], {1: "x"}, [2]),
          ("pl_lifter_bwd", [d, o, o, 0, o, 0, o, o, None], {2: "dy"}, [1, 6]),
          ("pl_lifter_bwd_eval", [d, o, o, 0, o, 0, o, o, None], {2: "dy"}, [1, 6]),
          ("pl_lifter_bwd_layers", [d, o, o, 0, o, 0, o, o, 3, 0, None], {2: "dy"}, [1, 6]),
          ("pl_lifter_train_fwd_bwd", [d, o, o, 0, o, 0, 0, 0, o, o, o, 3, 0, None], {1: "x"}, [2, 8, 9]),
          ("pl_lifter_train_fwd_bwd_crit", [d, o, o, 0, o, 0, 0, 0, None, o, o, o, 3, 0, None], {1: "x"}, [2, 9, 10]),
          ("pl_lifter_train_step", [d, o, o, 0, o, 0, 0, 0, o, o, o, opt, None], {1: "x"}, [2, 8, 9]),
          ("pl_lifter_train_step_crit", [d, o, o, 0, o, 0, 0, 0, None, o, o, o, opt, None], {1: "x"}, [2, 9, 10])]
    # ---- GEMM building blocks on operand planes (M = 0)
    S += [("pl_gemm_planes", [0, lib.PL_F16X3, o, o, o, 0, 128, 128, o, 1.0, 1.0, o, None], {2: "A", 3: "Bm", 4: "C", 8: "bias"}, []),
          ("pl_gemm_planes_raw", [0, lib.PL_F16X3, o, 0, 128, o, 0, 128, o, 0, 128, 128, o, 1.0, None, o, o, None],
           {2: "A", 5: "Bm", 8: "C", 12: "bias", 16: "stat"}, []),
          ("pl_planes_split", [o, 8, 99, 1.0, o, None], {0: "x"}, [])]
    # ---- direct convolution family (an unknown arithmetic, an empty batch)
    S += [("pl_conv2d_nhwc_fwd", [o, 1, 8, 8, 32, o, 32, 1, 1, 1, 0, o, o, o, 0, o, o, 99, o, 0, None], {16: "y", 15: "resid"},
           [11, 12, 13]),
          ("pl_conv2d_nhwc_wgrad", [o, 0, 8, 8, 3, o, 64, 7, 7, 2, 3, o, X6, o, 0, None], {5: "dy"}, []),
          ("pl_deconv4x4s2_nhwc_fwd", [o, 1, 4, 4, 32, o, 32, o, o, 0, o, 99, o, 0, None], {10: "y"}, [7, 8]),
          ("pl_maxpool3x3s2_nhwc", [o, 0, 8, 8, 8, o, None], {0: "x", 5: "y"}, []),
          ("pl_maxpool3x3s2_nhwc_idx", [o, 0, 8, 8, 8, o, o, None], {0: "x", 5: "y"}, []),
          ("pl_maxpool3x3s2_nhwc_bwd", [o, o, 0, 8, 8, 8, o, None], {0: "x", 1: "dy", 6: "dx"}, []),
          ("pl_maxpool3x3s2_nhwc_bwd_idx", [o, o, 0, 8, 8, 8, o, None], {1: "dy", 6: "dx"}, []),
          ("pl_upsample2x_zero_nhwc", [o, 0, 4, 4, 8, o, None], {0: "x", 5: "y"}, [])]
    # ---- conv-path BatchNorm, join and mask (rows = 0)
    S += [("pl_bn_train_fwd", [o, 0, 8, o, o, 1e-5, 0.1, o, o, o, 1, o, o, o, o, o, None], {0: "z", 11: "y", 12: "bits"},
           [3, 4, 7, 8, 13, 14]),
          ("pl_bn_train_fwd_ex", [o, 0, 8, o, o, 1e-5, 0.1, o, o, o, 1, o, o, o, o, o, None, 0, o, o, None],
           {0: "z", 11: "y", 12: "bits", 19: "join"}, [3, 4, 13, 14, 18]),
          ("pl_bn_train_bwd", [o, o, o, o, o, o, 0, 8, o, o, o, o, None],
           {0: "dy", 1: "bits", 2: "z", 3: "mean", 4: "rstd", 8: "dz"}, [5, 9, 10]),
          ("pl_bn_train_bwd_ex", [o, o, o, o, o, o, 0, 8, o, o, o, o, None, 0, None, None],
           {0: "dy", 1: "bits", 2: "z", 3: "mean", 4: "rstd", 8: "dz"}, [5, 9, 10]),
          ("pl_bn_join_bwd", [o, o, o, o, o, o, o, 0, 256, o, o, o, o, o, None, 0, None, None],
           {0: "g", 1: "g2", 2: "bits", 3: "z", 4: "mean", 5: "rstd", 9: "dx", 10: "dz"}, [6, 11, 12]),
          ("pl_add_relu_fwd", [o, o, 0, 8, o, o, None], {0: "a", 1: "b", 4: "out", 5: "bits"}, []),
          ("pl_add_relu_fwd_ex", [o, o, 0, 8, o, o, None, 0, None], {0: "a", 1: "b", 4: "out", 5: "bits"}, []),
          ("pl_mask_by_bits", [o, o, 0, 8, o, None], {0: "g", 1: "bits", 4: "dx"}, []),
          ("pl_mask_add_by_bits", [o, o, o, 0, 8, o, None], {0: "g", 1: "g2", 2: "bits", 5: "dx"}, [])]
    # ---- checks that existed before the audit.  metrics: err at an address that is not 4-byte aligned is what fails next
    S += [("pl_pose_errors", [o, o, 1, 17, off4, o, None], {0: "pred", 1: "tgt", 5: "aligned"}, []),
          ("pl_pose_errors_t", [o, o, 1, 17, o, o, off4, o, None], {0: "pred", 1: "tgt", 7: "aligned"}, [4, 5]),
          ("pl_pose_errors_host", [o, o, 1, 17, off4, o], {0: "pred", 1: "tgt", 5: "aligned"}, [])]
    # heads (BJ = 0 / B = 0 fails next)
    law = (ctypes.c_float * 6)(1, 1, 1, 0, 0, 0)
    S += [("pl_softargmax_fwd", [o, 0, 2, 2, 4, 3, 1, o, o, None], {0: "logits"}, [7, 8]),
          ("pl_softargmax_hm_fwd", [o, o, 0, 2, 2, 4, 3, 1, 0.5, law, o, o, o, None], {0: "logits"}, [1, 10, 11, 12]),
          ("pl_softargmax_bwd", [o, o, o, 0, 2, 2, 4, 3, 1, o, None], {0: "logits", 9: "dlogits"}, [1, 2]),
          ("pl_softargmax_hm_bwd", [o, o, o, o, o, 0, 2, 2, 4, 3, 1, 0.5, law, o, None], {0: "logits", 13: "dlogits"}, [1, 2, 3, 4]),
          ("pl_softargmax3d_nhwc_bwd", [o, o, o, 0, 17, 3, 5, o, None], {0: "logits", 7: "dlogits"}, [1, 2]),
          ("pl_softargmax3d_nhwc_bwd_ex", [o, o, o, 0, 17, 3, 5, o, None, 0, None, None], {0: "logits", 7: "dlogits"}, [1, 2]),
          ("pl_softargmax3d_nhwc_hm_bwd_ex", [o, o, o, o, o, 0, 17, 3, 5, 0.5, law, o, None, 0, None, None],
           {0: "logits", 11: "dlogits"}, [1, 2, 3, 4])]
    # ViT, through the carrier forms (the plain forms are the same function without a carrier): a carrier of 1 row fails next
    S += [("pl_vit_ln_fwd_bf16", [o, o, 32, 64, 2, o, o, o, o, 1e-5, o, o, o, 1, o, None],
           {0: "x", 1: "add", 5: "g1", 6: "b1", 7: "g2", 8: "b2", 10: "x_out", 11: "y"}, [14]),
          ("pl_vit_ln_bwd_bf16", [o, o, o, o, 32, 64, 2, o, o, o, o, o, 1, o, o, None],
           {0: "dy", 1: "dres", 2: "x", 7: "g1", 8: "b1", 9: "g2", 10: "dx"}, [3, 13]),
          ("pl_vit_attn_fwd_bf16", [o, 1, 17, 4, 64, 0.125, o, o, 1, o, None], {0: "qkv"}, [6, 9]),
          ("pl_vit_attn_bwd_bf16", [o, o, o, 1, 17, 4, 64, 0.125, o, o, 1, None], {0: "qkv", 2: "dout"}, [1, 8])]
    return S


def _call(L, name, args):
    rc, msg = getattr(L, name)(*args), L.pl_last_error()
    return rc, msg


def test_every_c_check_refuses_8_and_4_byte_aligned_pointers_and_lets_16_through(pkg):
    L, lib = pkg.lib(), pkg._lib
    specs = _specs(lib)
    seen = set()
    for name, args, checked, free in specs:
        rc, msg = _call(L, name, args)
        # the base call: every pointer aligned, rejected by the check that comes AFTER the alignment (never a launch)
        assert rc != 0 and b"aligned" not in msg.replace(b"4-byte aligned", b"") and b"launch failed" not in msg, (name, rc, msg)
        base_msg = msg
        for idx, arg in checked.items():
            for bad in (odd, word):
                a = list(args)
                a[idx] = bad
                rc, msg = _call(L, name, a)
                assert rc == EINVAL, (name, arg, bad.value, rc, msg)
                assert b"16-byte aligned" in msg and re.search(rb"\b" + arg.encode() + rb"\b", msg), (name, arg, bad.value, msg)
            seen.add((name, arg))
        for idx in free:                      # element code or a gate behind it: a 4-byte aligned pointer is the caller's right
            a = list(args)
            a[idx] = word
            rc, msg = _call(L, name, a)
            assert rc != 0 and msg == base_msg, (name, idx, rc, msg)
    assert len(seen) >= 110


def test_refusals_whose_check_is_the_last_one_before_the_launch(pkg):
    """pl_vit_bf16_pack and pl_vit_planes_dyn check x last: only the refusal can be shown without a launch."""
    L = pkg.lib()
    for bad in (odd, word):
        rc, msg = _call(L, "pl_vit_bf16_pack", [bad, 32, 64, 32, one, None])
        assert rc == EINVAL and b"x must be 16-byte aligned" in msg, msg
        rc, msg = _call(L, "pl_vit_planes_dyn", [bad, 32, 64, 32, None, one, one, one, None])
        assert rc == EINVAL and b"x must be 16-byte aligned" in msg, msg
        rc, msg = _call(L, "pl_vit_bf16_pack", [one, 32, 64, 32, bad, None])
        assert rc == EINVAL and b"carrier must be 16-byte aligned" in msg, msg


# ------------------------------------------------------------------------------------------------ the Python helper
def _cpu_view(shape, k, seed=0):
    g = torch.Generator().manual_seed(seed)
    return ac.OffViews().off_view(torch.randn(*shape, generator=g), k)


def test_aligned16_returns_the_tensor_itself_or_an_aligned_equal_copy(pkg):
    a16 = pkg._lib.aligned16
    t = torch.randn(5, 7)
    assert t.data_ptr() % 16 == 0 and a16(t) is t
    for k in ac.OFFSETS:
        v = _cpu_view((5, 7), k)
        assert v.data_ptr() % 16 == 4 * k and v.is_contiguous()
        c = a16(v)
        assert c is not v and c.data_ptr() % 16 == 0 and torch.equal(c, v) and c.is_contiguous() and not c.requires_grad
        v.requires_grad_(True)
        c = a16(v)
        assert c.requires_grad and c.data_ptr() % 16 == 0
        w = torch.arange(35.0).reshape(5, 7)
        (c * w).sum().backward()              # the gradient arrives at the misaligned leaf
        assert v.grad is not None and torch.equal(v.grad, w)


def test_an_out_tensor_is_refused_by_name_never_copied(pkg):
    lib = pkg._lib
    lib.require_aligned16_out(torch.zeros(8), "out")
    with pytest.raises(lib.PoseliftError, match="out must be 16-byte aligned"):          # (conv._gemm_planes_raw(out=), its one user)
        lib.require_aligned16_out(_cpu_view((8,), 1), "out")


class _Recorder:
    """Stands in for the loaded library: records every call's pointer-sized arguments and answers 0 (a size query: 64)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 64 if name.endswith("_bytes") else 0
        return fn


@pytest.fixture
def recorder(pkg, monkeypatch):
    """The wrappers run on CPU tensors: device / dtype checks and the stream lookup are stubbed, the library is a recorder.
    What is under test is which ADDRESSES the wrappers pass."""
    rec = _Recorder()
    lib = pkg._lib
    monkeypatch.setattr(lib, "lib", lambda: rec)
    monkeypatch.setattr(lib, "current_stream_ptr", lambda: 0)
    monkeypatch.setattr(lib, "on_device", lambda dev: lib._NO_SWITCH)
    real = lib.require_device_tensor

    def on_cpu(t, name, dtype=torch.float32):
        if t.dtype != dtype or not t.is_contiguous():
            real(t, name, dtype)
    monkeypatch.setattr(lib, "require_device_tensor", on_cpu)
    return rec


def _ptrs(rec, name, idx):
    calls = [a for n, a in rec.calls if n == name]
    assert calls, (name, [n for n, _ in rec.calls])
    return [a[i] for a in calls for i in idx]


@pytest.mark.parametrize("k", ac.OFFSETS)
def test_no_wrapper_hands_a_misaligned_pointer_to_an_entry_point_that_refuses(pkg, recorder, k):
    pred, tgt = _cpu_view((3, 17, 3), k, 1), _cpu_view((3, 17, 3), k, 2)
    pkg.pose_errors(pred, tgt)
    pkg.procrustes_align(pred, tgt)
    assert all(p % 16 == 0 for p in _ptrs(recorder, "pl_pose_errors", (0, 1)))
    logits = _cpu_view((2, 17 * 2, 2, 4), k, 3).requires_grad_(True)
    out = pkg.soft_argmax_3d(logits, 17, 2)
    out.sum().backward()
    assert logits.grad is not None and logits.grad.shape == logits.shape
    assert all(p % 16 == 0 for p in _ptrs(recorder, "pl_softargmax_fwd", (0,)) + _ptrs(recorder, "pl_softargmax_bwd", (0, 9)))
    nhwc = _cpu_view((2, 3, 5, 17 * 64), k, 4).requires_grad_(True)
    pkg.soft_argmax_3d_nhwc(nhwc, 17).sum().backward()
    assert all(p % 16 == 0 for p in _ptrs(recorder, "pl_softargmax3d_nhwc_bwd", (0, 7)))
    frames = _cpu_view((2, 15, 21, 3), k, 5)
    w = _cpu_view((64, 7, 7, 3), k, 6)
    resid = _cpu_view((2, 8, 11, 64), k, 7)
    pkg.conv.conv2d_nhwc(frames, w, 2, 3, resid=resid, relu=2)
    assert all(p % 16 == 0 for p in _ptrs(recorder, "pl_conv2d_nhwc_fwd", (0, 5, 15, 16)))
    pkg.conv.conv2d_nhwc_wgrad(frames, resid, 7, 2, 3)
    assert all(p % 16 == 0 for p in _ptrs(recorder, "pl_conv2d_nhwc_wgrad", (0, 5)))
    pkg.conv.maxpool3x3s2_nhwc(resid)
    assert all(p % 16 == 0 for p in _ptrs(recorder, "pl_maxpool3x3s2_nhwc", (0, 5)))
    # the autograd building blocks, forward and the incoming gradients of their backward
    xa = _cpu_view((2, 9, 13, 8), k, 8).requires_grad_(True)
    pkg.conv.maxpool3x3s2_nhwc_autograd(xa).backward(_cpu_view((2, 5, 7, 8), k, 9))
    assert all(p % 16 == 0 for p in _ptrs(recorder, "pl_maxpool3x3s2_nhwc_idx", (0, 5)) +
               _ptrs(recorder, "pl_maxpool3x3s2_nhwc_bwd_idx", (1, 6)))
    a, b = _cpu_view((2, 5, 7, 8), k, 10).requires_grad_(True), _cpu_view((2, 5, 7, 8), k, 11)
    pkg.conv.add_relu(a, b).backward(_cpu_view((2, 5, 7, 8), k, 12))
    assert all(p % 16 == 0 for p in _ptrs(recorder, "pl_add_relu_fwd_ex", (0, 1, 4, 5)) +
               _ptrs(recorder, "pl_mask_add_by_bits", (0, 2, 5)))
    bn = torch.nn.BatchNorm2d(8).train()
    z = _cpu_view((2, 5, 7, 8), k, 13).requires_grad_(True)
    pkg.conv.batchnorm_relu_train(z, bn).backward(_cpu_view((2, 5, 7, 8), k, 14))
    assert all(p % 16 == 0 for p in _ptrs(recorder, "pl_bn_train_fwd_ex", (0, 11, 12)) +
               _ptrs(recorder, "pl_bn_train_bwd_ex", (0, 1, 2, 3, 4, 8)))
    pkg.conv.to_planes(_cpu_view((2, 5, 7, 8), k, 15))
    assert all(p % 16 == 0 for p in _ptrs(recorder, "pl_planes_split", (0, 4)))


# ------------------------------------------------------------------------------------------------ the test helper of the GPU file
def test_off_views_sit_where_they_claim_and_the_sentinel_check_fires():
    for dtype, unit in ((torch.float32, 4), (torch.int32, 4), (torch.uint8, 1)):
        for k in ac.OFFSETS:
            ov = ac.OffViews()
            t = (torch.arange(3 * 5) % 251).to(dtype).reshape(3, 5)
            v = ov.off_view(t, k)
            assert torch.equal(v, t) and v.shape == t.shape and v.is_contiguous()
            assert v.data_ptr() % 16 == ((4 + k) * unit) % 16
            if unit == 4:
                assert v.data_ptr() % 16 == 4 * k
            assert ov.guards_intact() == 1
            base = torch.empty(0, dtype=dtype).set_(v.untyped_storage(), 0, (15 + 8,), (1,))
            assert base.data_ptr() % 16 == 0 and torch.equal(base[4 + k:4 + k + 15].view(3, 5), t)
            saved = base[4 + k + 15].clone()
            base[4 + k + 15] = 1                                    # one element behind the values: a float4 tail store
            with pytest.raises(AssertionError, match=r"guard element 15 \(behind"):
                ov.guards_intact()
            base[4 + k + 15] = saved
            assert ov.guards_intact() == 1
            base[4 + k - 1] = 1                                     # one element in front
            with pytest.raises(AssertionError, match=r"guard element -1 \(in front"):
                ov.guards_intact()
            ov = ac.OffViews()
            v = ov.off_view(t, k, "poses")
            v[1, 2] += 1                                            # the call modified its input
            with pytest.raises(AssertionError, match="poses: input element 7 was modified"):
                ov.guards_intact()
    x = torch.full((4,), float("nan"))
    assert ac.same_bits(x, x.clone()) and not ac.same_bits(torch.zeros(1), -torch.zeros(1))


def test_run_aligned_and_off_compares_bits_gradients_and_guards():
    w = torch.arange(12.0).reshape(3, 4)
    def op(st, a, b):
        loss = (a * b * w).sum()
        loss.backward()                                                  # (the call runs its own backward)
        return [loss, a + b]
    ref = ac.run_aligned_and_off(lambda: None, op, [torch.randn(3, 4), torch.randn(3, 4)], grad_idx=(0,))
    assert len(ref) == 3 and ref[2].shape == (3, 4)

    def depends_on_the_address(st, a):
        return [a + float(a.data_ptr() % 16)]
    with pytest.raises(AssertionError, match="offset 1: result 0 of 1 differs"):
        ac.run_aligned_and_off(lambda: None, depends_on_the_address, [torch.randn(5)])

    def writes_past_its_input(st, a):
        torch.empty(0).set_(a.untyped_storage(), a.storage_offset(), (a.numel() + 1,), (1,))[-1] = 0.0
        return [a * 2]
    with pytest.raises(AssertionError, match="guard element 5"):
        ac.run_aligned_and_off(lambda: None, writes_past_its_input, [torch.randn(5)])


# ------------------------------------------------------------------------------------------------ the audit table
def _header_symbols_with_pointers():
    h = open(os.path.join(ROOT, "include", "poselift.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    h = re.sub(r"//[^\n]*", "", h)
    return {m.group(1) for m in re.finditer(r"\b(pl_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", h, flags=re.S) if "*" in m.group(2)}


def _design_table():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^## 3h\. Alignment contract of caller pointers.*?(?=^## )", text, flags=re.S | re.M)
    assert m, "DESIGN.md has no section 'Alignment contract of caller pointers'"
    rows = [ln for ln in m.group(0).splitlines() if ln.startswith("|")]
    assert rows[0].startswith("| Entry point") and set(rows[1]) <= set("|- ")
    return [[c.strip() for c in ln.strip().strip("|").split("|")] for ln in rows[2:]]


def test_design_table_names_every_entry_point_that_takes_a_pointer(pkg):
    rows = _design_table()
    assert all(len(r) == 4 for r in rows), [r for r in rows if len(r) != 4][:1]
    named, owner = set(), None
    for entry, ptrs, widest, guarantee in rows:
        names = set(re.findall(r"`(pl_[a-z0-9_]+)`", entry))
        assert names or owner, "a continuation row before any entry point"
        owner = names or owner
        named |= names
        assert ptrs and widest and guarantee, (entry, ptrs)
        assert re.search(r"C check|gate|scalar|not applicable", guarantee), (sorted(owner)[0], guarantee)
    syms = _header_symbols_with_pointers()
    assert len(syms) > 130
    assert syms - named == set(), sorted(syms - named)
    assert named - set(pkg._lib.SIGNATURES) == set(), sorted(named - set(pkg._lib.SIGNATURES))
    # every (entry point, pointer) the host test above refuses is a "C check" row of the table that names that pointer
    by_entry = {}
    owner = None
    for entry, ptrs, widest, guarantee in rows:
        owner = set(re.findall(r"`(pl_[a-z0-9_]+)`", entry)) or owner
        for n in owner:
            by_entry.setdefault(n, []).append((ptrs, guarantee))
    for name, _args, checked, _free in _specs(pkg._lib):
        for arg in checked.values():
            arg = {"Bm": "B"}.get(arg, arg)
            hits = [g for p, g in by_entry[name] if re.search(r"`" + re.escape(arg) + r"[`_]", p) or f"`{arg}`" in p]
            assert hits and any("C check" in g for g in hits), (name, arg, by_entry[name])
