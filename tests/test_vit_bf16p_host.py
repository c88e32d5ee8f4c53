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


def test_plain_and_null_carrier_forms_refuse_the_same_calls_with_the_same_code(pkg):
    """Each of the six carrier kernels has one checked launcher behind both of its names: a bad call is refused with the same
    return code through the plain form and through the _bf16 form with a NULL carrier, and neither accepts a NULL fp32
    output when there is no carrier to write instead."""
    L = pkg.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(24)
    T, H, Tp = 17 * 3, 256, 64

    def both(name, plain_args, carrier_args):          # (return codes; each message names the entry point that was called)
        rp, mp = getattr(L, name)(*plain_args, None), L.pl_last_error()
        rc, mc = getattr(L, name + "_bf16")(*carrier_args, None), L.pl_last_error()
        assert mp.startswith(name.encode() + b":") and mc.startswith(name.encode() + b"_bf16:"), (mp, mc)
        return rp, rc

    def ln_fwd(x=one, add=None, T=T, H=H, nn=2, g1=one, b1=one, g2=one, b2=one, x_out=None, y=one, stats=one):
        return both("pl_vit_ln_fwd", (x, add, T, H, nn, g1, b1, g2, b2, 1e-5, x_out, y, stats),
                    (x, add, T, H, nn, g1, b1, g2, b2, 1e-5, x_out, y, None, Tp, stats))

    def ln_bwd(dy=one, dres=None, x=one, stats=one, T=T, H=H, nn=2, g1=one, b1=one, g2=one, dx=one, dgb=one, scratch=one):
        return both("pl_vit_ln_bwd", (dy, dres, x, stats, T, H, nn, g1, b1, g2, dx, dgb, scratch),
                    (dy, dres, x, stats, T, H, nn, g1, b1, g2, dx, None, Tp, dgb, scratch))

    def attn_fwd(qkv=one, B=3, seq=17, heads=4, dh=64, o=one, lse=one):
        return both("pl_vit_attn_fwd", (qkv, B, seq, heads, dh, 0.125, o, lse), (qkv, B, seq, heads, dh, 0.125, o, None, Tp, lse))

    def attn_bwd(qkv=one, lse=one, dout=one, B=3, seq=17, heads=4, dh=64, dqkv=one):
        return both("pl_vit_attn_bwd", (qkv, lse, dout, B, seq, heads, dh, 0.125, dqkv),
                    (qkv, lse, dout, B, seq, heads, dh, 0.125, dqkv, None, Tp))

    def gelu_fwd(u=one, rows=T, y=one):          # the plain form takes the element count
        return both("pl_vit_gelu_fwd", (u, rows * 1024, y), (u, rows, 1024, Tp, y, None))

    def gelu_bwd(u=one, dy=one, rows=T, du=one):
        return both("pl_vit_gelu_bwd", (u, dy, rows * 1024, du), (u, dy, rows, 1024, Tp, du, None))

    bad = {
        "ln_fwd": [ln_fwd(y=None), ln_fwd(x=None), ln_fwd(T=0), ln_fwd(H=1028), ln_fwd(H=258), ln_fwd(nn=3), ln_fwd(g2=None),
                   ln_fwd(stats=None), ln_fwd(add=one), ln_fwd(nn=0), ln_fwd(x=odd), ln_fwd(y=odd), ln_fwd(b1=odd),
                   ln_fwd(add=odd, x_out=one)],
        "ln_bwd": [ln_bwd(dx=None), ln_bwd(dy=None), ln_bwd(nn=0), ln_bwd(H=1028), ln_bwd(T=-1), ln_bwd(b1=None), ln_bwd(g2=None),
                   ln_bwd(dgb=None), ln_bwd(scratch=None), ln_bwd(dx=odd), ln_bwd(dres=odd), ln_bwd(g1=odd)],
        "attn_fwd": [attn_fwd(o=None), attn_fwd(qkv=None), attn_fwd(lse=None), attn_fwd(seq=33), attn_fwd(dh=32), attn_fwd(B=0),
                     attn_fwd(heads=0), attn_fwd(qkv=odd)],
        "attn_bwd": [attn_bwd(dqkv=None), attn_bwd(qkv=None), attn_bwd(lse=None), attn_bwd(dout=None), attn_bwd(seq=33),
                     attn_bwd(seq=32, heads=4), attn_bwd(dh=32), attn_bwd(dout=odd)],
        "gelu_fwd": [gelu_fwd(y=None), gelu_fwd(u=None), gelu_fwd(rows=0), gelu_fwd(rows=-3)],
        "gelu_bwd": [gelu_bwd(du=None), gelu_bwd(u=None), gelu_bwd(dy=None), gelu_bwd(rows=0)],
    }
    for kernel, calls in bad.items():
        for i, (plain, null_carrier) in enumerate(calls):       # (the first of each list: no fp32 output and no carrier)
            assert plain != 0 and null_carrier == plain, (kernel, i, plain, null_carrier)
