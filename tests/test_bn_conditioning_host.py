"""The gate of tests/test_gpu_bn_conditioning.py has margin and teeth, shown without a GPU: on the ill-conditioned columns
of oracle/bn_cases.py an fp32-step emulation of the kernels' scheme (sums per 64 rows, M2 about the group mean, Chan merge)
stays inside 16 u_c, and the scheme the kernels promise not to use (sum z^2, sum z) leaves 64 u_c -- the GPU tests' bound --
on some column of kinds 1 - 3 at every batch size.  So do the other faults the columns are there for, each on the kind of
column meant for it: a dropped or halved between-group term n d^2 (kind 4, more than one group), a ragged last group counted
as full (kind 3), a pre-folded shift that lost the mean's low bits (kinds 1 - 3; the fp32 fold itself stays inside 16 u_c).
Without that second half the GPU tests could pass vacuously."""
import numpy as np
import pytest

from oracle import bn_cases

EPS = 1e-5
C = 40
BATCHES = [37, 64, 65, 105, 256, 1000, 4096]


@pytest.fixture(scope="module", params=BATCHES)
def case(request):
    B = request.param
    return B, bn_cases.columns(B, C, seed=B)


def test_columns_are_what_the_table_says():
    z = bn_cases.columns(129, 20, seed=1)
    assert z.dtype == np.float32 and z.shape == (129, 20)
    mu, var, _ = bn_cases.stats64(z, EPS)
    assert abs(mu[0] - 0.5) < 1 and 2 < var[0] < 7
    assert 100 <= mu[1] < 200.5 and -200.5 < mu[6] <= -100 and var[1] < 0.03            # alternating sign
    assert [float(z[0, c]) for c in (2, 7, 12, 17)] == [np.float32(v) for v in bn_cases.CONSTANTS]
    assert all(var[c] == 0 for c in (2, 7, 12, 17))
    assert (z[:-1, 3] == np.float32(7.3)).all() and z[-1, 3] == np.float32(7.3 + 1e-2)
    assert var[4] > 20 and np.abs(z[64:128, 4] - 10).max() < 0.5                        # the between-group term dominates
    # the unit: fp32 resolution of zhat -- 2^-24 on a centred column, 2^-24 |mu| / s on a shifted one
    u = bn_cases.bound(z, EPS)
    assert u[0] < 3 * bn_cases.EPS24 and 500 * bn_cases.EPS24 < u[1] < 3000 * bn_cases.EPS24
    assert np.isclose(u[7], bn_cases.EPS24 * (100 + np.sqrt(EPS)) / np.sqrt(EPS))


def test_group_chan_scheme_stays_inside_16_units(case):
    B, z = case
    e = bn_cases.errors_in_units(z, EPS, *bn_cases.chan_stats_f32(z, EPS))
    print(f"B = {B}: worst error of the group / Chan scheme per kind, in u_c:",
          [round(float(e[k::5].max()), 2) for k in range(5)])
    assert np.isfinite(e).all() and e.max() <= 16, (B, e.max(), int(e.argmax()))


def test_naive_sums_of_squares_leave_the_gpu_gate(case):
    B, z = case
    e = bn_cases.errors_in_units(z, EPS, *bn_cases.naive_stats_f32(z, EPS))
    bad = [c for c in range(C) if c % 5 in (1, 2, 3) and not e[c] <= bn_cases.K]
    print(f"B = {B}: naive scheme, worst finite error per kind, in u_c:",
          [round(float(np.nanmax(np.where(np.isfinite(e[k::5]), e[k::5], 0))), 1) for k in range(5)],
          "non-finite columns:", [c for c in range(C) if not np.isfinite(e[c])])
    assert bad, (B, e)


def _outside(e, kinds):
    return [c for c in range(C) if c % 5 in kinds and not e[c] <= bn_cases.K]


@pytest.mark.parametrize("between", [0.0, 0.5])
def test_dropped_or_halved_between_group_term_leaves_the_gpu_gate(case, between):
    B, z = case
    e = bn_cases.errors_in_units(z, EPS, *bn_cases.chan_stats_f32(z, EPS, between=between))
    print(f"B = {B}, between-group term x {between}: worst error on the group-shifted columns, in u_c: {float(e[4::5].max()):.3g}")
    if B > 64:        # (one group: there is no such term, and the scheme is the honest one)
        assert len(_outside(e, (4,))) == C // 5, (B, e[4::5])
    else:
        assert e.max() <= 16


def test_last_group_counted_as_full_leaves_the_gpu_gate(case):
    B, z = case
    e = bn_cases.errors_in_units(z, EPS, *bn_cases.chan_stats_f32(z, EPS, last_full=True))
    print(f"B = {B}, last group counted as 64 rows: worst error on the one-row-outlier columns, in u_c: {float(e[3::5].max()):.3g}")
    if B % 64:        # (whole groups: the count is right)
        assert len(_outside(e, (3,))) == C // 5, (B, e[3::5])
    else:
        assert e.max() <= 16


def test_shift_that_loses_the_mean_leaves_the_gpu_gate(case):
    B, z = case
    mean, rstd, _ = bn_cases.chan_stats_f32(z, EPS)
    e32 = bn_cases.errors_in_units(z, EPS, mean, rstd, bn_cases.folded_zhat_f32(z, mean, rstd))
    e16 = bn_cases.errors_in_units(z, EPS, mean, rstd, bn_cases.folded_zhat_f32(z, mean, rstd, np.float16))
    print(f"B = {B}, folded shift: fp32 worst {float(e32.max()):.3g} u_c; 16-bit shift, worst per kind:",
          [float(f"{e16[k::5].max():.3g}") for k in range(5)])
    assert e32.max() <= 16, (B, e32.max(), int(e32.argmax()))
    assert _outside(e16, (1,)) and _outside(e16, (2,)) and _outside(e16, (3,)), (B, e16)
