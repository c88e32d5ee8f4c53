"""No GPU: the reference that tests/test_gpu_bf16_exact.py holds the bf16 kernels to (tests/bf16_oracle.py).
bf16_round is pinned against an integer-bit restatement of round-to-nearest-even; on the very inputs of the GPU GEMM
cases, simulated kernel defects exceed the rounded-operand bound while the "bf16-sized" 2e-2 bound lets them through;
and an fp32 evaluation of the rounded operands -- the arithmetic the kernels are documented to perform -- stays under
half of that bound, so the bound asks nothing the reference arithmetic cannot meet."""
import numpy as np
import pytest
import torch

import bf16_oracle as bo


def _bits(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32)


def _rne_bits(v):
    """(u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000 on the fp32 bit pattern (finite values and infinities)."""
    u = _bits(v).astype(np.uint64)
    r = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return r.astype(np.uint32).view(np.float32)


def _f(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


EDGES = {
    "tie, even kept": _f(0x3F808000, 0xBF808000, 0x40008000),              # low half 0x8000, bf16 lsb 0: rounds down
    "tie, odd rounds up": _f(0x3F818000, 0xBF818000, 0x40018000),          # low half 0x8000, bf16 lsb 1: rounds up
    "just off a tie": _f(0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001),
    "largest finite": _f(0x7F7F0000, 0xFF7F0000, 0x7F7F7FFF, 0xFF7F7FFF),
    "rounds up to inf": _f(0x7F7F8000, 0xFF7F8000, 0x7F7FFFFF, 0xFF7FFFFF),
    "zeros": _f(0x00000000, 0x80000000),
    "subnormals": _f(0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x807F8000, 0x00800000),
    "infinities": _f(0x7F800000, 0xFF800000),
}


@pytest.mark.parametrize("name", sorted(EDGES))
def test_bf16_round_is_round_to_nearest_even_bit_for_bit(name):
    v = EDGES[name]
    want = _rne_bits(v)
    got_np, got_t = bo.bf16_round(v), bo.bf16_round(torch.from_numpy(v.copy())).numpy()
    assert got_np.dtype == np.float32
    np.testing.assert_array_equal(_bits(got_np), _bits(want))           # bits: -0 stays -0
    np.testing.assert_array_equal(_bits(got_t), _bits(want))
    assert np.all(_bits(got_np) & np.uint32(0xFFFF) == 0)
    if name == "tie, even kept":
        np.testing.assert_array_equal(_bits(got_np), _bits(v) & np.uint32(0xFFFF0000))
    if name == "tie, odd rounds up":
        np.testing.assert_array_equal(_bits(got_np), (_bits(v) & np.uint32(0xFFFF0000)) + np.uint32(0x10000))
    if name == "rounds up to inf":
        assert np.all(np.isinf(got_np)) and np.array_equal(np.signbit(got_np), np.signbit(v))
    if name == "largest finite":
        assert np.all(np.abs(got_np) == np.float32(3.3895313892515355e38))


def test_bf16_round_random_bits_and_nan():
    rng = np.random.default_rng(0)
    u = rng.integers(0, 1 << 32, size=200000, dtype=np.uint64).astype(np.uint32)
    v = u.view(np.float32)
    fin = ~np.isnan(v)
    got = bo.bf16_round(v)
    np.testing.assert_array_equal(_bits(got[fin]), _bits(_rne_bits(v[fin])))
    assert np.all(np.isnan(got[~fin])) and (~fin).sum() > 100
    nan = _f(0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0x7F80FFFF)      # the last three would carry out of the
    assert np.all(np.isnan(bo.bf16_round(nan)))                               # mantissa under the integer formula
    assert bool(torch.isnan(bo.bf16_round(torch.from_numpy(nan.copy()))).all())
    x = rng.standard_normal((3, 5)).astype(np.float32)                        # shape kept, idempotent
    assert bo.bf16_round(x).shape == (3, 5)
    np.testing.assert_array_equal(bo.bf16_round(bo.bf16_round(x)), bo.bf16_round(x))


def test_ambiguous_marks_the_neighbourhood_of_rounding_midpoints():
    lo, hi = 1.0, 1.0 + 2.0 ** -7                                 # adjacent bf16 values
    mid = 0.5 * (lo + hi)
    v = np.array([mid, mid + 1e-9, mid - 1e-9, mid + 1e-5, lo, hi, -mid, 3.0 * mid])
    got = bo.ambiguous(v, 1e-8)
    np.testing.assert_array_equal(got[:7], [True, True, True, False, False, False, True])
    assert not got[7]                                             # 3 mid = 3.01171875 is a bf16 value's neighbour, no midpoint
    assert bo.ambiguous(np.array([4.5 * 2.0 ** -133]), 0.0)[0]    # subnormal range: spacing 2^-133, midpoints exist
    np.testing.assert_array_equal(bo.ulp_bf16(np.array([1.0, 1.99, 2.0, 0.75, 2.0 ** -126, 2.0 ** -130])),
                                  [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -133, 2.0 ** -133])
    # what it is for: a value perturbed by less than delta rounds differently only where ambiguous() says so
    rng = np.random.default_rng(1)
    x = rng.standard_normal(100000)
    d = 1e-5 * rng.uniform(-1, 1, x.size)
    flips = bo.bf16_round(x.astype(np.float32)) != bo.bf16_round((x + d).astype(np.float32))
    amb = bo.ambiguous(x, 1e-5 + 2.0 ** -24 * np.abs(x))          # (+ the fp32 rounding of both arguments)
    assert flips.sum() > 100 and not np.any(flips & ~amb)
    assert amb.mean() < 0.03


def _trunc(v):
    return (_bits(v) & np.uint32(0xFFFF0000)).view(np.float32)


@pytest.mark.parametrize("layout,M,N,K", bo.PLANES_GEMM_CASES)
def test_simulated_defects_exceed_the_rounded_operand_bound(layout, M, N, K):
    """One 32-k tile dropped, truncation instead of RNE, one output element taken from its neighbour: each is many
    times outside 2e-6 (|a_r| @ |b_r| + |bias|) + 1e-7 around the rounded-operand result.  Truncation moves an operand
    by under 2^-7 of itself, a product by under 1.6e-2 of |a| |b|: the 2e-2 bound around the unrounded result, which the
    bf16 rows had until now, passes it on every input; at K = 4096 it passes a dropped tile too."""
    a, b, bias = bo.gemm_inputs(layout, M, N, K)
    emu, tight = bo.gemm_reference(a, b, bias)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    want = a64 @ b64 + bias
    loose = 2e-2 * (np.abs(a64) @ np.abs(b64) + np.abs(bias)) + 1e-7
    assert np.all(np.abs(emu - want) <= loose)                    # (a correct kernel passes the old bound)
    ar, br = bo.bf16_round(a).astype(np.float64), bo.bf16_round(b).astype(np.float64)
    drop = ar[:, :-32] @ br[:-32] + bias
    trunc = _trunc(a).astype(np.float64) @ _trunc(b).astype(np.float64) + bias
    swap = emu.copy()
    swap[5, 7] = emu[5, 8]
    for name, bad in (("tile dropped", drop), ("truncation", trunc), ("neighbour's element", swap)):
        assert (np.abs(bad - emu) / tight).max() > 100.0, name
    assert (np.abs(trunc - want) / loose).max() < 1.0
    assert (np.abs(swap - want) / loose).max() > 1.0              # (the old bound does see a foreign element)
    if K == 4096:
        assert (np.abs(drop - want) / loose).max() < 1.0


@pytest.mark.parametrize("layout,M,N,K", bo.PLANES_GEMM_CASES)
def test_fp32_evaluations_of_the_rounded_operands_use_under_half_the_bound(layout, M, N, K):
    """The arithmetic the kernels are documented to perform, on the CPU: fp32 BLAS, and fp32 sums of 32-k chunks (the
    kernels' k tile).  Both stay under half of the bound: the reference alone leaves the kernel room."""
    a, b, bias = bo.gemm_inputs(layout, M, N, K)
    emu, tight = bo.gemm_reference(a, b, bias)
    ar, br = bo.bf16_round(a), bo.bf16_round(b)
    blas = ar @ br + bias
    acc = np.zeros((M, N), np.float32)
    for k0 in range(0, K, 32):
        acc = acc + ar[:, k0:k0 + 32] @ br[k0:k0 + 32]
    acc = acc + bias
    assert blas.dtype == np.float32 and acc.dtype == np.float32
    assert (np.abs(blas.astype(np.float64) - emu) / tight).max() < 0.5
    assert (np.abs(acc.astype(np.float64) - emu) / tight).max() < 0.5


@pytest.mark.parametrize("reference", [bo.planes_eval_conv_reference, bo.planes_eval_deconv_reference],
                         ids=["conv", "deconv"])
def test_stored_plane_inputs_leave_few_ambiguous_elements(reference):
    """The inputs of the stored-bf16-plane cases of the GPU test: under 0.5 % of the reference outputs lie so close to a
    rounding midpoint that the fp32 result may legitimately round to the neighbour (the GPU test allows 1 %), and the
    ReLU clips some but not most of them."""
    want, delta = reference()
    amb = bo.ambiguous(want.numpy(), delta.numpy())
    assert amb.mean() < 0.005, float(amb.mean())
    assert 0.02 < float((want == 0).double().mean()) < 0.5


# ---------------------------------------------------------------------------- the lifter's emulated oracle
def test_operand_round_none_is_the_reference_arithmetic_and_bf16_is_not():
    """oracle.lifter_oracle with operand_round=None computes what it computed before the hook existed (the goldens of
    tests/test_oracle_golden.py regenerate bit for bit); with the bf16 rounding the first and the output Linear still see
    unrounded operands: rounding the first layer's weight as well changes the result, so the hook did not."""
    from oracle import lifter_oracle as orc
    st, x, t = bo.lifter_inputs(64, 128, True)
    masks = [np.ones((64, 128), bool)] * 5
    kw = dict(num_stage=2, train=True, p_dropout=0.5, keep_masks=masks, update_running=False)
    y0, c0 = orc.forward(st, x, **kw)
    y1, c1 = orc.forward(st, x, operand_round=None, **kw)
    assert np.array_equal(y0, y1)
    yq, cq = orc.forward(st, x, operand_round=bo.operand_round, **kw)
    assert not np.array_equal(y0, yq)
    assert np.array_equal(c0["layers"][0]["z"], cq["layers"][0]["z"])              # the first Linear: untouched
    zq = bo.bf16_round(cq["layers"][0]["a_out"]) @ bo.bf16_round(st["linear_stages.0.w1.weight"]).T + st["linear_stages.0.w1.bias"]
    assert np.allclose(cq["layers"][1]["z"], zq, rtol=0, atol=1e-5) and not np.allclose(c0["layers"][1]["z"], zq, rtol=0, atol=1e-5)
    g0, dx0 = orc.backward(st, c0, y0 * np.float32(1e-2))
    g1, dx1 = orc.backward(st, c1, y0 * np.float32(1e-2), operand_round=None)
    assert all(np.array_equal(g0[k], g1[k]) for k in g0) and np.array_equal(dx0, dx1)
    gq, _ = orc.backward(st, cq, y0 * np.float32(1e-2))
    assert not np.array_equal(g0["linear_stages.1.w2.weight"], gq["linear_stages.1.w2.weight"])


@pytest.mark.parametrize("name,B,H,bn", bo.LIFTER_CASES, ids=[c[0] for c in bo.LIFTER_CASES])
def test_lifter_reference_alone_meets_the_gates_of_the_gpu_test(name, B, H, bn):
    """Rounding ties: the emulated oracle in fp32 against the same in fp64 (decisions forced).  bo.LIFTER_MEASURED records
    what this measured when the gates were set; the gates of the GPU test are twice that or the fp32-grade bound."""
    mm, loss, rel, worst = bo.lifter_reference_alone(B, H, bn)
    print(f"{name}: MPJPE {mm:.3e} mm, loss {loss:.3e}, worst relative L2 {rel:.3e} ({worst})")
    g_mm, g_loss, g_rel = bo.lifter_gates(name)
    assert mm <= g_mm and loss <= g_loss and rel <= g_rel, (mm, loss, rel)


def test_eval_backward_reference_alone_meets_the_emulated_gate():
    """The fp32 emulated oracle as "the device" through eval_backward_oracle.compare(kind="bf16-emulated")."""
    import eval_backward_oracle as ebo
    case = next(c for c in ebo.CASES if c.id == "bf16-256x256-dual")
    st, xa, ta, xb, tb = ebo.make_inputs(case)
    q = bo.operand_round
    r32 = ebo.reference(st, xa, ta, xb, tb, case.S, case.bn, dtype=np.float32, operand_round=q)
    got = ebo.as_device(r32)
    ref = ebo.reference(st, xa, ta, xb, tb, case.S, case.bn, got["masks_a"], got["masks_b"], operand_round=q)
    rep = ebo.compare(got, ref, "bf16-emulated")
    print(ebo.summary(rep), {k: f"{rep['errors'][k]:.2e}" for k in ("y", "yb", "dx_max", "dx")})
