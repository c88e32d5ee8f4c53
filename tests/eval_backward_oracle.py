"""fp64 reference and flip-accounted comparison of the lifter's eval-mode backward.  TEST INFRASTRUCTURE ONLY.

model.eval() inside an autograd graph (the phase-5 cycle step: pl_lifter_fwd_eval_saved / pl_lifter_bwd_eval) on the graph
of test_eval_mode_backward_vs_torch_twin:

    ya = f(xa)  with the input gradient,   yb = f(xb)  without it,
    loss = mean((ya - ta)^2) + 0.5 mean((yb - tb)^2)

  reference   that graph on oracle/lifter_oracle.py (BatchNorm on the running statistics, Dropout the identity), in any
              dtype, optionally with the ReLU decisions of each call forced to the implementation's own
  compare     decision accounting per layer and call, then every error against the fp64 reference with the decisions forced,
              and each error as a multiple of the fp32 oracle's under the same decisions (reported, never asserted)
  CASES       one case per branch the eval-mode backward can take (api.hip plan(), pair_route, f32_pair_route), shared by
              tests/test_eval_backward_host.py (the fp32 oracle as "the device") and tests/test_gpu_eval_backward.py
"""
from collections import namedtuple

import numpy as np

from oracle import lifter_oracle as orc

# the reference alone on "bf16-256x256-dual" (see BOUNDS["bf16-emulated"]): output error of max (the second call's), dx max-abs
# of max, largest relative L2 (dx)
EMULATED_MEASURED = dict(y=7.0e-4, dx_max=5.9e-4, rel_l2=9.1e-5)

# kind -> the project's own bounds.  Decisions: _assert_decisions_consistent (test_gpu_parity.py) made relative to the
# layer's largest pre-ReLU value; bf16: the flip rule of the bf16 gates.  Errors: the eval forward's 2e-5 of max, the
# existing dx bound of test_eval_mode_backward_vs_torch_twin, the 2e-4 / 8e-2 relative-L2 bounds of the gradient gates.
BOUNDS = {
    "fp32-grade": dict(flip_frac=1e-4, flip_abs=None, flip_rel=1e-4, y=2e-5, dx_max=5e-4, rel_l2=2e-4),
    "bf16": dict(flip_frac=0.02, flip_abs=0.2, flip_rel=None, y=3e-2, dx_max=None, rel_l2=8e-2),
    # bf16 against the EMULATED oracle (reference(..., operand_round=bf16_oracle.operand_round): the hidden x hidden GEMMs on
    # bf16-rounded operands, as the library's): the fp32-grade error bounds, widened only where rounding ties ask for it.
    # An fp32-perturbed activation or dz may round to the neighbouring bf16 value; what that costs was measured on the CPU
    # from the reference alone -- the emulated oracle in fp32 against the same in fp64, on the inputs of
    # "bf16-256x256-dual": EMULATED_MEASURED -- y 7.0e-4 of max, dx max-abs 5.9e-4 of max, relative L2 at most 9.1e-5 -- and
    # each gate is twice that or the fp32-grade bound, whichever is larger: y 1.4e-3, dx max-abs 1.18e-3, relative L2 2e-4
    # (tests/test_bf16_oracle_host.py re-measures and holds the reference alone to these gates).  Decisions: the flip rule
    # of the bf16 gates.
    "bf16-emulated": dict(flip_frac=0.02, flip_abs=0.2, flip_rel=None, y=max(2 * EMULATED_MEASURED["y"], 2e-5),
                          dx_max=max(2 * EMULATED_MEASURED["dx_max"], 5e-4), rel_l2=max(2 * EMULATED_MEASURED["rel_l2"], 2e-4)),
}

PLANES_CHAIN, PLANES_DUAL = "planes_gemm_chain_kernel", "planes_gemm_dual_kernel"
F32_DUAL, X6_DUAL = "gemm_f32_dual_kernel", "gemm_x6_planes_dual_kernel"
PAIR_KERNELS = (PLANES_CHAIN, PLANES_DUAL, F32_DUAL, X6_DUAL)

# pair: the one-launch pair kernels the backward must run (none: two launches per hidden layer, or no hidden pair at all);
# thin: does a dX GEMM of the backward run on the thin GEMM; fwd: "planes" = the hidden Linears of the saved forward are planes
# tile GEMMs (Lin::Planes), "mid" = none of them is (Lin::PlanesMid), None = off the planes path
Case = namedtuple("Case", "id dtype B H S bn dims pair thin fwd seed")


def _case(id, dtype, B, H, pair=(), thin=False, fwd=None, S=2, bn=True, dims=(34, 51), seed=17):
    return Case(id, dtype, B, H, S, bn, dims, frozenset(pair), thin, fwd, seed)


CASES = [
    # on the planes path (whole 128-row tiles, BatchNorm, f16x3 / bf16)
    _case("f16x3-128x128-chain", "f16x3", 128, 128, {PLANES_CHAIN}, fwd="planes"),
    _case("f16x3-256x256-dual-mid", "f16x3", 256, 256, {PLANES_DUAL}, fwd="mid"),
    _case("f16x3-640x128-chain", "f16x3", 640, 128, {PLANES_CHAIN}, fwd="planes"),
    _case("f16x3-640x256-dual", "f16x3", 640, 256, {PLANES_DUAL}, fwd="planes"),
    _case("f16x3-128x1024-cycle", "f16x3", 128, 1024, {PLANES_DUAL}, fwd="mid"),
    _case("f16x3-384x256-S1", "f16x3", 384, 256, {PLANES_DUAL}, fwd="mid", S=1),
    _case("f16x3-256x128-S3", "f16x3", 256, 128, {PLANES_CHAIN}, fwd="planes", S=3),
    _case("bf16-256x256-dual", "bf16", 256, 256, {PLANES_DUAL}, fwd="planes"),
    # off it
    _case("fp32-512x256-tile-dual", "fp32", 512, 256, {F32_DUAL}),
    _case("bf16x6-512x256-x6-dual", "bf16x6", 512, 256, {X6_DUAL}),
    _case("f16x3-100x256-ragged", "f16x3", 100, 256, thin=True),
    _case("fp32-520x128-ragged", "fp32", 520, 128),
    _case("fp32-100x64-projector", "fp32", 100, 64, thin=True, dims=(51, 34)),
    _case("fp32-64x128-noBN", "fp32", 64, 128, thin=True, bn=False),
    _case("fp32-96x128-S0", "fp32", 96, 128, S=0),
    _case("fp32-2x128", "fp32", 2, 128, thin=True),
    _case("fp32-1x128", "fp32", 1, 128, thin=True),
]


def kind_of(case):
    return "bf16" if case.dtype == "bf16" else "fp32-grade"


def make_inputs(case):
    """(st, xa, ta, xb, tb): the weights and input distributions of test_eval_mode_backward_vs_torch_twin."""
    i_dim, o_dim = case.dims
    st = orc.init_state(i_dim, o_dim, case.H, case.S, rng=np.random.default_rng(5), nontrivial_bn=True)
    rng = np.random.default_rng(case.seed)
    xa, xb = rng.random((case.B, i_dim), dtype=np.float32), rng.random((case.B, i_dim), dtype=np.float32)
    ta = rng.random((case.B, o_dim), dtype=np.float32) - np.float32(0.5)
    tb = rng.random((case.B, o_dim), dtype=np.float32) - np.float32(0.5)
    return st, xa, ta, xb, tb


def loss_grads(ya, ta, yb, tb, dtype):
    """d loss / d ya and d loss / d yb of  mean((ya - ta)^2) + 0.5 mean((yb - tb)^2)."""
    dya = (ya - ta.astype(dtype)) * dtype(2.0 / ya.size)
    dyb = (yb - tb.astype(dtype)) * dtype(0.5 * 2.0 / yb.size)
    return dya, dyb


def reference(st, xa, ta, xb, tb, S, bn, masks_a=None, masks_b=None, dtype=np.float64, operand_round=None):
    """The two-call graph on the oracle.  masks_*: per hidden layer the (B, H) boolean ReLU decisions to force in that call
    (cache['layers'][l]['on_disagree'] then holds |pre-ReLU| wherever they differ from the oracle's own).
    Returns outputs, dx (of the first call alone), parameter gradients summed over the two calls, both caches and the
    arguments (compare() replays them in fp32)."""
    kw = dict(num_stage=S, train=False, use_bn=bn, dtype=dtype, operand_round=operand_round)
    ya, ca = orc.forward(st, xa, on_masks=masks_a, **kw)
    yb, cb = orc.forward(st, xb, on_masks=masks_b, **kw)
    dya, dyb = loss_grads(ya, ta, yb, tb, dtype)
    ga, dx = orc.backward(st, ca, dya)
    gb, _ = orc.backward(st, cb, dyb)
    return dict(ya=ya, yb=yb, dx=dx, grads={k: ga[k] + gb[k] for k in ga}, cache_a=ca, cache_b=cb,
                inputs=dict(st=st, xa=xa, ta=ta, xb=xb, tb=tb, S=S, bn=bn, masks_a=masks_a, masks_b=masks_b,
                            operand_round=operand_round))


def decisions_of(cache):
    return [c["rmask"] for c in cache["layers"]]


def as_device(res):
    """A reference() result in the form compare() takes from an implementation: outputs, dx, gradients, the decisions of
    each call and the running statistics after the step."""
    st = res["inputs"]["st"]
    return dict(ya=res["ya"], yb=res["yb"], dx=res["dx"], grads=dict(res["grads"]),
                masks_a=decisions_of(res["cache_a"]), masks_b=decisions_of(res["cache_b"]),
                running={k: np.array(v) for k, v in st.items() if "running" in k or "num_batches" in k})


def _pre_relu(st, lin, bnp, c, bn):
    if not bn:
        return c["z"]
    return c["zhat"] * st[bnp + ".weight"].astype(np.float64) + st[bnp + ".bias"].astype(np.float64)


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def _errors(res, ref):
    """Every compared quantity of `res` as an error against the fp64 `ref`."""
    ymax = max(np.abs(ref["ya"]).max(), 1e-300)
    e = {"y": float(np.abs(res["ya"] - ref["ya"]).max() / ymax),
         "dx_max": float(np.abs(res["dx"] - ref["dx"]).max() / max(np.abs(ref["dx"]).max(), 1e-300)),
         "dx": _rel_l2(res["dx"], ref["dx"])}
    if res.get("yb") is not None:
        e["yb"] = float(np.abs(res["yb"] - ref["yb"]).max() / max(np.abs(ref["yb"]).max(), 1e-300))
    for k, v in res["grads"].items():
        e[k] = _rel_l2(v, ref["grads"][k])
    return e


def compare(got, ref, kind):
    """got: as_device()'s keys from the implementation under test; ref: reference(...) in fp64 with got's decisions forced.
    Asserts the decision accounting, the bounds of BOUNDS[kind] and that the running statistics did not move.  Returns
    {"flips": {call: [per layer]}, "worst_flip": largest |pre-ReLU| at a disagreeing decision, "errors": {...},
    "ratios": {...: error / the fp32 oracle's error under the same decisions}}."""
    b = BOUNDS[kind]
    inp = ref["inputs"]
    st, S, bn = inp["st"], inp["S"], inp["bn"]
    assert ref["cache_a"]["dtype"] is np.float64
    for call in ("a", "b"):
        forced, own = inp["masks_" + call], got["masks_" + call]
        assert forced is not None and len(forced) == len(own) == 1 + 2 * S
        assert all(np.array_equal(f, o) for f, o in zip(forced, own)), "the reference was not forced to these decisions"
    # ---- decisions: few disagree with fp64, each on a round-off-sized pre-activation
    report = {"flips": {}, "worst_flip": 0.0}
    for call in ("a", "b"):
        counts = []
        for (lin, bnp), c in zip(orc.hidden_layer_names(S), ref["cache_" + call]["layers"]):
            d = c["on_disagree"]
            counts.append(int(d.size))
            assert d.size <= b["flip_frac"] * c["z"].size + 2, (call, lin, d.size, c["z"].size)
            if d.size:
                lim = b["flip_abs"] if b["flip_abs"] is not None else \
                    b["flip_rel"] * max(1.0, float(np.abs(_pre_relu(st, lin, bnp, c, bn)).max()))
                assert d.max() < lim, (call, lin, float(d.max()), lim)
                report["worst_flip"] = max(report["worst_flip"], float(d.max()))
        report["flips"][call] = counts
    # ---- the running statistics are constants of this graph
    for k, v in st.items():
        if "running" in k or "num_batches" in k:
            assert np.array_equal(np.asarray(got["running"][k]), v), k
    # ---- errors against fp64 with the decisions forced
    want = set(orc.param_names(S, bn_params=bn))
    assert set(got["grads"]) == want, sorted(set(got["grads"]) ^ want)
    err = _errors(got, ref)
    r32 = reference(st, inp["xa"], inp["ta"], inp["xb"], inp["tb"], S, bn, inp["masks_a"], inp["masks_b"], dtype=np.float32,
                    operand_round=inp.get("operand_round"))
    e32 = _errors(r32, ref)
    report["errors"] = err
    report["ratios"] = {k: (v / e32[k] if e32[k] > 0 else (0.0 if v == 0 else float("inf"))) for k, v in err.items()}
    assert err["y"] <= b["y"], ("ya", err["y"])
    if "yb" in err:
        assert err["yb"] <= b["y"], ("yb", err["yb"])
    if b["dx_max"] is not None:
        assert err["dx_max"] <= b["dx_max"], ("dx max-abs", err["dx_max"])
    assert err["dx"] < b["rel_l2"], ("dx", err["dx"])
    for k in sorted(want):
        assert err[k] < b["rel_l2"], (k, err[k])
    return report


def summary(report):
    """One line for a log or a table: flips per call and layer, the worst flip, the largest error ratios."""
    r = report["ratios"]
    grads = [v for k, v in r.items() if k not in ("y", "yb", "dx", "dx_max")]
    return (f"flips a {report['flips']['a']} b {report['flips']['b']} worst |pre-ReLU| {report['worst_flip']:.2e}; "
            f"error / fp32 oracle's: y {r['y']:.2f} dx max {r['dx_max']:.2f} dx L2 {r['dx']:.2f} "
            f"grads worst {max(grads):.2f}; dx max-abs {report['errors']['dx_max']:.2e}")
