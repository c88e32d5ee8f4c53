"""MyViT "bf16p" host-side contract (no GPU): the mode constructs with the fp32 mode's state_dict and seeded weights, "bf16"
still raises, and the bf16-carrier entry points reject bad arguments before any HIP call."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()


@pytest.mark.parametrize("kw", [dict(), dict(chw=(1, 17, 3), out_d=2)])
def test_bf16p_constructs_with_the_fp32_state_dict_and_seeded_weights(pkg, kw):
    torch.manual_seed(7)
    a = pkg.MyViT(compute_dtype="bf16p", **kw)
    torch.manual_seed(7)
    b = pkg.MyViT(compute_dtype="fp32", **kw)
    assert a.compute_dtype == "bf16p"
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k]), k
    assert [k for k, p in a.named_parameters() if p.requires_grad] == [k for k, p in b.named_parameters() if p.requires_grad]


def test_bf16_is_still_not_a_mode(pkg):
    with pytest.raises(pkg.PoseliftError):
        pkg.MyViT(compute_dtype="bf16")


def test_bf16p_cpu_forward_raises_no_fallback(pkg):
    with pytest.raises(pkg.PoseliftError):
        pkg.MyViT(compute_dtype="bf16p")(torch.zeros(2, 17, 2))


def test_carrier_entry_points_reject_bad_arguments(pkg):
    L = pkg.lib()
    one = ctypes.c_void_p(16)           # non-null, 16-byte aligned: never dereferenced on these paths
    odd = ctypes.c_void_p(24)           # 8-byte aligned only
    T = 17 * 3
    # LayerNorm forward: rows_pad < T, rows_pad % 32, H % 4, misaligned carrier, no output at all, a carrier with nnorm 0
    ln = lambda H, nn, y, c, rp: L.pl_vit_ln_fwd_bf16(one, None, T, H, nn, one, one, one, one, 1e-5, None, y, c, rp, one, None)
    assert ln(256, 2, None, one, 32) != 0 and b"rows_pad" in L.pl_last_error()
    assert ln(256, 2, None, one, 80) != 0 and b"rows_pad" in L.pl_last_error()
    assert ln(258, 2, None, one, 64) != 0
    assert ln(256, 2, None, odd, 64) != 0 and b"aligned" in L.pl_last_error()
    assert ln(256, 2, None, None, 64) != 0 and b"null" in L.pl_last_error()
    assert L.pl_vit_ln_fwd_bf16(one, one, T, 256, 0, None, None, None, None, 1e-5, one, None, one, 64, None, None) != 0
    # LayerNorm backward
    lb = lambda dx, c, rp: L.pl_vit_ln_bwd_bf16(one, None, one, one, T, 256, 1, one, None, None, dx, c, rp, one, one, None)
    assert lb(None, None, 64) != 0 and b"null" in L.pl_last_error()
    assert lb(None, one, 48) != 0 and b"rows_pad" in L.pl_last_error()
    assert lb(one, odd, 64) != 0 and b"aligned" in L.pl_last_error()
    # attention
    assert L.pl_vit_attn_fwd_bf16(one, 3, 17, 4, 64, 0.125, None, None, 64, one, None) != 0
    assert b"null" in L.pl_last_error()
    assert L.pl_vit_attn_fwd_bf16(one, 3, 17, 4, 64, 0.125, None, one, 32, one, None) != 0
    assert b"rows_pad" in L.pl_last_error()
    assert L.pl_vit_attn_fwd_bf16(one, 3, 33, 4, 64, 0.125, None, one, 128, one, None) != 0      # seq > 32
    assert L.pl_vit_attn_bwd_bf16(one, one, one, 3, 17, 4, 64, 0.125, None, one, 60, None) != 0
    assert b"rows_pad" in L.pl_last_error()
    assert L.pl_vit_attn_bwd_bf16(one, one, None, 3, 17, 4, 64, 0.125, None, one, 64, None) != 0
    assert b"null" in L.pl_last_error()
    # GELU and the pack: cols % 4, rows_pad, null
    assert L.pl_vit_gelu_fwd_bf16(one, T, 1026, 64, None, one, None) != 0
    assert L.pl_vit_gelu_fwd_bf16(one, T, 1024, 50, None, one, None) != 0 and b"rows_pad" in L.pl_last_error()
    assert L.pl_vit_gelu_fwd_bf16(one, T, 1024, 64, None, None, None) != 0 and b"null" in L.pl_last_error()
    assert L.pl_vit_gelu_bwd_bf16(one, None, T, 1024, 64, one, one, None) != 0 and b"null" in L.pl_last_error()
    assert L.pl_vit_gelu_bwd_bf16(one, one, T, 1024, 64, None, odd, None) != 0 and b"aligned" in L.pl_last_error()
    assert L.pl_vit_bf16_pack(one, T, 256, 32, one, None) != 0 and b"rows_pad" in L.pl_last_error()
    assert L.pl_vit_bf16_pack(one, T, 254, 64, one, None) != 0
    assert L.pl_vit_bf16_pack(None, T, 256, 64, one, None) != 0 and b"null" in L.pl_last_error()
    assert L.pl_vit_bf16_pack(odd, T, 256, 64, one, None) != 0 and b"aligned" in L.pl_last_error()
