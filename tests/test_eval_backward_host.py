"""tests/eval_backward_oracle.py discriminates (no GPU): compare() is fed the fp32 oracle's result as "the device" at
every shape of the GPU case table -- it must pass, with no disagreeing ReLU decision -- and then that result with one
defect of the eval-mode backward at a time: each must fail."""
import numpy as np
import pytest

import eval_backward_oracle as ebo
from oracle import lifter_oracle as orc

IDS = [c.id for c in ebo.CASES]


def _fp32_device(case):
    st, xa, ta, xb, tb = ebo.make_inputs(case)
    r32 = ebo.reference(st, xa, ta, xb, tb, case.S, case.bn, dtype=np.float32)
    return (st, xa, ta, xb, tb), r32, ebo.as_device(r32)


def _ref_for(case, inputs, got):
    return ebo.reference(*inputs, case.S, case.bn, got["masks_a"], got["masks_b"])


@pytest.mark.parametrize("case", ebo.CASES, ids=IDS)
def test_fp32_oracle_passes_with_no_disagreeing_decision(case):
    inputs, _, got = _fp32_device(case)
    rep = ebo.compare(got, _ref_for(case, inputs, got), "fp32-grade")
    assert rep["flips"] == {"a": [0] * (1 + 2 * case.S), "b": [0] * (1 + 2 * case.S)}, rep["flips"]
    assert all(abs(v - 1.0) < 1e-12 or v == 0.0 for v in rep["ratios"].values())     # the fp32 oracle against itself
    assert set(rep["errors"]) >= {"y", "yb", "dx", "dx_max", "w2.weight", "w1.bias"}
    assert (("batch_norm1.weight" in rep["errors"]) == case.bn)
    print(case.id, ebo.summary(rep))


def test_bf16_bounds_accept_what_the_fp32_grade_bounds_accept():
    case = ebo.CASES[1]
    inputs, _, got = _fp32_device(case)
    ebo.compare(got, _ref_for(case, inputs, got), "bf16")


# ---------------------------------------------------------------------------------------------- mutations
def _backward(st, cache, dout, dtype, batch_mean_terms=False, drop_skip=None, batch_zhat_dgamma=False):
    """orc.backward written out, with three defects of an eval-mode backward behind switches: the training-mode dz
    (batch-mean terms, as if the eval flag were ignored), the skip gradient of residual block `drop_skip` missing, dgamma
    on a zhat formed from the batch's own statistics."""
    S, bn = cache["num_stage"], cache["use_bn"]
    names, L = orc.hidden_layer_names(S), cache["layers"]
    grads = {}

    def hidden(l, g):
        lin, bnp = names[l]
        c = L[l]
        dy = np.where(c["rmask"], g, dtype(0))
        if bn:
            gamma, B = st[bnp + ".weight"].astype(dtype), dtype(dy.shape[0])
            dgamma, dbeta = (dy * c["zhat"]).sum(axis=0, dtype=dtype), dy.sum(axis=0, dtype=dtype)
            dz = dy * (gamma * c["rstd"])
            if batch_mean_terms:
                dz = gamma * c["rstd"] * (dy - dbeta / B - c["zhat"] * (dgamma / B))
            if batch_zhat_dgamma:
                z = c["z"]
                zb = (z - z.mean(axis=0)) / np.sqrt(z.var(axis=0) + dtype(orc.BN_EPS))
                dgamma = (dy * zb).sum(axis=0, dtype=dtype)
            grads[bnp + ".weight"], grads[bnp + ".bias"] = dgamma, dbeta
        else:
            dz = dy
        grads[lin + ".weight"] = dz.T @ c["a_in"]
        grads[lin + ".bias"] = dz.sum(axis=0, dtype=dtype)
        return dz @ st[lin + ".weight"].astype(dtype)

    dout = np.asarray(dout).astype(dtype)
    grads["w2.weight"] = dout.T @ cache["h_last"]
    grads["w2.bias"] = dout.sum(axis=0, dtype=dtype)
    g = dout @ st["w2.weight"].astype(dtype)
    for s in reversed(range(S)):
        gh = hidden(1 + 2 * s, hidden(2 + 2 * s, g))
        g = gh if drop_skip == s else g + gh
    dx = hidden(0, g)
    return grads, dx


def _device_with(case, inputs, r32, w_b=0.5, dx_both=False, **defect):
    """The fp32 oracle's step recomputed from its caches with one defect."""
    st, xa, ta, xb, tb = inputs
    f = np.float32
    dya, dyb = ebo.loss_grads(r32["ya"], ta, r32["yb"], tb, f)
    ga, dxa = _backward(st, r32["cache_a"], dya, f, **defect)
    gb, dxb = _backward(st, r32["cache_b"], dyb * f(w_b / 0.5), f, **defect)
    got = ebo.as_device(r32)
    got["grads"] = {k: ga[k] + gb[k] for k in ga}
    got["dx"] = dxa + dxb if dx_both else dxa
    return got


def _flip_one_unforced(case, inputs, r32):
    """One decision of the first call differs from what the device reports: the smallest pre-activation of the top layer."""
    st, xa, ta, xb, tb = inputs
    masks = ebo.decisions_of(r32["cache_a"])
    top = r32["cache_a"]["layers"][-1]
    lin, bnp = orc.hidden_layer_names(case.S)[-1]
    y = np.abs(ebo._pre_relu(st, lin, bnp, top, case.bn))
    flipped = [m.copy() for m in masks]
    i = np.unravel_index(np.argmin(y), y.shape)
    flipped[-1][i] = ~flipped[-1][i]
    run = ebo.reference(st, xa, ta, xb, tb, case.S, case.bn, flipped, ebo.decisions_of(r32["cache_b"]), dtype=np.float32)
    got = ebo.as_device(run)
    got["masks_a"] = masks                       # ... and the report says nothing of it
    return got


def _moved_running(case, inputs, r32):
    got = ebo.as_device(r32)
    k = "batch_norm1.running_var"
    got["running"][k] = got["running"][k].copy()
    got["running"][k][3] = np.nextafter(got["running"][k][3], np.float32(2))
    return got


MUTATIONS = {
    "decision-flipped-not-forced": _flip_one_unforced,
    "dz-with-batch-mean-terms": lambda c, i, r: _device_with(c, i, r, batch_mean_terms=True),
    "skip-gradient-dropped": lambda c, i, r: _device_with(c, i, r, drop_skip=c.S - 1),
    "dgamma-on-batch-zhat": lambda c, i, r: _device_with(c, i, r, batch_zhat_dgamma=True),
    "second-call-weighted-1": lambda c, i, r: _device_with(c, i, r, w_b=1.0),
    "dx-includes-second-call": lambda c, i, r: _device_with(c, i, r, dx_both=True),
    "running-statistics-moved": _moved_running,
}
# the reported shape, the smallest planes shape, three stages, the 64-wide projector, two rows
MUTATION_CASES = [c for c in ebo.CASES if c.id in ("f16x3-640x256-dual", "f16x3-128x128-chain", "f16x3-256x128-S3",
                                                   "fp32-100x64-projector", "fp32-2x128")]


@pytest.fixture(scope="module")
def fp32_runs():
    return {c.id: _fp32_device(c) for c in MUTATION_CASES}


@pytest.mark.parametrize("case", MUTATION_CASES, ids=[c.id for c in MUTATION_CASES])
def test_the_written_out_backward_is_the_oracles(case, fp32_runs):
    """Without a defect switched on, _device_with reproduces the fp32 oracle bit for bit -- so each mutation below differs
    from a passing result by its defect alone."""
    inputs, r32, got = fp32_runs[case.id]
    same = _device_with(case, inputs, r32)
    assert np.array_equal(same["dx"], got["dx"])
    assert all(np.array_equal(same["grads"][k], v) for k, v in got["grads"].items())


@pytest.mark.parametrize("name", list(MUTATIONS))
@pytest.mark.parametrize("case", MUTATION_CASES, ids=[c.id for c in MUTATION_CASES])
def test_compare_fails_on(case, name, fp32_runs):
    inputs, r32, _ = fp32_runs[case.id]
    bad = MUTATIONS[name](case, inputs, r32)
    ref = _ref_for(case, inputs, bad)
    with pytest.raises(AssertionError):
        ebo.compare(bad, ref, "fp32-grade")
