"""Contiguous tensors that do NOT start on a 16-byte boundary, for tests/test_gpu_alignment.py (and, on the CPU,
tests/test_alignment_host.py): what `table[n:]`, a dropped first row or `table[i * B:(i + 1) * B]` hand the library.

    ov = OffViews()
    x = ov.off_view(t, k)        # t's values at byte offset 4 k mod 16 (fp32 / int32; k in their own units for other types)
    ...                          # the call under test
    ov.guards_intact()           # nothing wrote the floats around any view, and no view's own values changed

Every view sits inside its own block of `numel + 8` elements: 4 + k guard elements in front, the values, 4 - k behind; the
guards hold a sentinel whose bits no computed value has (a NaN payload for fp32: a kernel that READS a guard into a sum
poisons its result as well).  Comparison is on the bits, so the NaN sentinels compare equal to themselves.

The shapes the GPU cases use are listed here too, each with the reason it is in the list."""
import torch

_SENTINEL_BITS = {torch.float32: (torch.int32, 0x7FA11CE5), torch.int32: (torch.int32, 0x2AAAAAAA),
                  torch.int64: (torch.int64, 0x2AAAAAAA2AAAAAAA), torch.uint8: (torch.uint8, 0xA5)}
OFFSETS = (1, 2, 3)             # elements past a 16-byte boundary: 4, 8 and 12 bytes for fp32


def _bits(t):
    return t.view(_SENTINEL_BITS[t.dtype][0])


class OffViews:
    def __init__(self):
        self._blocks = []       # (flat block, first value index, numel, bit-copy of the values, name)

    def off_view(self, t, k, name=None):
        """A contiguous tensor equal to `t` (same shape, dtype, device) whose data_ptr() is (4 + k) elements past a 16-byte
        boundary: for fp32 and int32 that is 4 k bytes mod 16."""
        if t.dtype not in _SENTINEL_BITS:
            raise TypeError(f"off_view: no sentinel for {t.dtype}")
        if not 0 <= k <= 4:
            raise ValueError("off_view: k in 0..4")
        t = t.detach()
        n = t.numel()
        flat = torch.empty(n + 8, dtype=t.dtype, device=t.device)
        assert flat.data_ptr() % 16 == 0, "a fresh allocation is 16-byte aligned"
        _bits(flat).fill_(_SENTINEL_BITS[t.dtype][1])
        lo = 4 + k
        flat[lo:lo + n] = t.reshape(-1)
        view = flat[lo:lo + n].view(t.shape)
        assert view.is_contiguous() and view.data_ptr() == flat.data_ptr() + lo * t.element_size()
        assert view.data_ptr() % 16 == (lo * t.element_size()) % 16
        if t.element_size() == 4:
            assert view.data_ptr() % 16 == (4 * k) % 16
        self._blocks.append((flat, lo, n, _bits(flat[lo:lo + n]).clone(), name or f"view {len(self._blocks)}"))
        return view

    def guards_intact(self, values_too=True):
        """AssertionError naming the view and the element if a guard element changed (or, values_too, one of the values)."""
        for flat, lo, n, saved, name in self._blocks:
            dt, want = _SENTINEL_BITS[flat.dtype]
            b = _bits(flat)
            for what, seg, base in (("in front of", b[:lo], 0), ("behind", b[lo + n:], lo + n)):
                bad = (seg != want).nonzero()
                assert bad.numel() == 0, (f"{name}: guard element {int(bad[0]) + base - lo} ({what} the values, counted from the "
                                          f"first value) was overwritten: bits {int(seg[int(bad[0])]):#x}")
            if values_too:
                bad = (b[lo:lo + n] != saved).nonzero()
                assert bad.numel() == 0, f"{name}: input element {int(bad[0])} was modified by the call"
        return len(self._blocks)


def same_bits(a, b):
    """torch.equal on the bit patterns (NaN == NaN, -0.0 != 0.0): a copy runs the same kernel on the same values."""
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype in (torch.float32, torch.float64):
        return torch.equal(a.contiguous().view(torch.int32 if a.dtype == torch.float32 else torch.int64),
                           b.contiguous().view(torch.int32 if b.dtype == torch.float32 else torch.int64))
    return torch.equal(a, b)


def run_aligned_and_off(build, call, tensors, grad_idx=(), offsets=OFFSETS, seed=20240):
    """The criterion of every Python-level case.  build() -> state (models, optimizers; built afresh from `seed` for every
    run); call(state, *tensors) -> list of tensors (outputs, gradients, every piece of state the call updates).  The call on
    aligned clones is the reference; for every k the call on off_view(t, k) of every tensor must give the same bits, the
    .grad of the misaligned leaves (grad_idx) included, with every guard element and every input value intact."""
    def run(ts):
        torch.manual_seed(seed)
        state = build()
        ts = [t.requires_grad_(True) if i in grad_idx else t for i, t in enumerate(ts)]
        out = list(call(state, *ts))
        out += [ts[i].grad for i in grad_idx]
        if ts and ts[0].is_cuda:
            torch.cuda.synchronize()
        return [o.detach().clone() if o is not None else None for o in out]

    ref = run([t.detach().clone() for t in tensors])
    for i in grad_idx:
        assert ref[len(ref) - len(grad_idx) + list(grad_idx).index(i)] is not None, f"the aligned call left no .grad on input {i}"
    for k in offsets:
        ov = OffViews()
        views = [ov.off_view(t, k, f"input {i} at offset {k}") for i, t in enumerate(tensors)]
        for v in views:
            assert v.data_ptr() % 16 == (4 + k) * v.element_size() % 16
            assert v.element_size() > 4 or v.data_ptr() % 16 != 0
        got = run(views)
        assert ov.guards_intact() == len(tensors)
        assert len(got) == len(ref)
        for j, (g, r) in enumerate(zip(got, ref)):
            assert same_bits(g, r), f"offset {k}: result {j} of {len(ref)} differs from the aligned call"
    return ref


# ---- shapes -------------------------------------------------------------------------------------------------------------------
# the lifter: (B, H, num_stage, compute_dtype, in_dim, out_dim)
LIFTER = [
    (65, 128, 1, "fp32", 34, 51),       # one whole 64-row group on the float4 staging of skinny.hip, plus one ragged row
    (128, 128, 1, "f16x3", 34, 51),     # operand-planes path, two fp16 planes
    (128, 128, 1, "bf16", 34, 51),      # operand-planes path, one bf16 plane
    (37, 256, 1, "fp32", 34, 51),       # small_layer.hip; the fused step carries AdamW
    (200, 36, 0, "fp32", 20, 7),        # generic GEMMs and their vec_ok gates (no skinny kernel: in 20, out 7, H 36)
]
LIFTER_IDS = [f"B{b}-H{h}-S{s}-{dt}-{i}to{o}" for b, h, s, dt, i, o in LIFTER]

# soft-argmax heads, NCHW: (B, D, H, W) with 17 joints; NHWC: (B, H, W) with depth 64
HEADS_NCHW = [(2, 2, 2, 4), (2, 1, 3, 4)]
HEADS_NHWC = [(2, 3, 5)]

# pl_gemm_f32 behind its gates: (M, N, K) -- ragged everything; whole tiles of the thin-GEMM size; > one tile with K > 512
GEMM_SHAPES = [(130, 51, 34), (64, 128, 32), (257, 129, 1030)]
# pl_gemm_arith, as tests/test_gpu_parity.py::test_gemm_bf16_arithmetic_modes: (layout, M, N, K)
GEMM_ARITH = [(0, 256, 128, 96), (2, 128, 256, 512)]
