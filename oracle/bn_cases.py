"""Ill-conditioned BatchNorm columns and the accuracy unit they are judged in.  TEST INFRASTRUCTURE ONLY (numpy).

columns(B, C, seed)   an fp32 [B][C] matrix whose column c has kind c % 5 (KINDS below): what training really feeds a
                      BatchNorm -- grown biases (|mean| / sigma ~ 1e3), dead units (constant columns: var = 0,
                      rstd = 1 / sqrt(eps)), a one-row outlier, a mean that drifts from one 64-row group to the next.
bound(z64, eps)       the per-column unit u_c = 2^-24 (|mu_c| + s_c) / s_c, s = sqrt(var + eps): the fp32 resolution of
                      zhat = (z - mu) / s at that column (the fp32 rounding of z itself is inside it).  Every assertion of
                      tests/test_gpu_bn_conditioning.py is K * u_c with K = 64 and nothing else is a free number.
chan_stats_f32 / naive_stats_f32   fp32-step emulations of the kernels' scheme (sequential sums per 64 rows, M2 about the
                      group mean, Chan merge against the total mean with the true row count of the last group) and of
                      the scheme the kernels promise NOT to use (sum z^2, sum z): tests/test_bn_conditioning_host.py
                      shows the first inside 16 u_c and the second outside 64 u_c: the GPU gate has margin and teeth.
                      chan_stats_f32's `between` and `last_full` and folded_zhat_f32's `shift_dtype` emulate the other
                      faults the columns are there for: a dropped or mis-weighted between-group term, a ragged last
                      group counted as full, a shift beta - mean scale that lost the mean's low bits.
"""
import numpy as np

K = 64
EPS24 = 2.0 ** -24
KINDS = ("control", "large mean", "constant", "one-row outlier", "group-shifted")
CONSTANTS = (0.1, 100.0, 0.0, -3.7)


def columns(B, C, seed):
    rng = np.random.default_rng(seed)
    z = np.empty((B, C), np.float64)
    rows = np.arange(B)
    for c in range(C):
        kind, n = c % 5, c // 5
        if kind == 0:
            z[:, c] = 0.5 + 2.0 * rng.standard_normal(B)
        elif kind == 1:
            z[:, c] = (1 - 2 * (n % 2)) * 100.0 * (1.0 + rng.random()) + 0.1 * rng.standard_normal(B)
        elif kind == 2:
            z[:, c] = CONSTANTS[n % 4]
        elif kind == 3:
            z[:, c] = 7.3
            z[B - 1, c] = 7.3 + 1e-2
        else:
            z[:, c] = 10.0 * (rows // 64) + 0.05 * rng.standard_normal(B)
    return z.astype(np.float32)


def stats64(z, eps):
    """(mu, biased var, s = sqrt(var + eps)) per column, in fp64, of the given z."""
    z64 = np.asarray(z, np.float64)
    mu = z64.mean(0)
    var = ((z64 - mu) ** 2).mean(0)
    return mu, var, np.sqrt(var + eps)


def bound(z64, eps):
    mu, _, s = stats64(z64, eps)
    return EPS24 * (np.abs(mu) + s) / s


def _finish(z, mean, var, eps):
    f = np.float32
    rstd = f(1) / np.sqrt(var + f(eps), dtype=f)
    return mean, rstd, ((z - mean) * rstd).astype(f)


def chan_stats_f32(z, eps, gs=64, between=1.0, last_full=False):
    """(mean, rstd, zhat), every step in fp32, as the finalize kernels do it: per gs-row group a sequential sum and a
    sequential sum of squares about the group's own mean; mean = (sum of the group sums) / B; M2 = the sum over the groups, in
    order, of M2_g + n_g (sum_g / n_g - mean)^2 (Chan et al., all groups against the total) with n_g the true row count of
    the ragged last group.  The faults: `between` weighs the between-group term n_g d^2 (0: dropped, 0.5: halved);
    `last_full` counts the ragged last group as gs rows."""
    f = np.float32
    z = np.asarray(z, f)
    B, C = z.shape
    groups = []
    for r0 in range(0, B, gs):
        blk = z[r0:r0 + gs]
        n = f(gs if last_full else len(blk))
        s = np.zeros(C, f)
        for row in blk:
            s = s + row
        mean_g = s / n
        m2 = np.zeros(C, f)
        for row in blk:
            d = row - mean_g
            m2 = m2 + d * d
        groups.append((n, s, m2))
    total = np.zeros(C, f)
    for _, s, _ in groups:
        total = total + s
    mean = total / f(B)
    M2 = np.zeros(C, f)
    for n, s, m2 in groups:
        d = s / n - mean
        M2 = M2 + (m2 + f(between) * n * d * d)
    return _finish(z, mean, M2 / f(B), eps)


def folded_zhat_f32(z, mean, rstd, shift_dtype=np.float32):
    """zhat as an apply pass with a pre-folded shift computes it (gamma = 1, beta = 0): fl(fl(z rstd) + shift),
    shift = fl(-mean rstd) kept as shift_dtype.  fp32 keeps the mean's bits to within the unit; a 16-bit shift does not."""
    f = np.float32
    shift = (-(mean * rstd)).astype(f).astype(shift_dtype).astype(f)
    return (np.asarray(z, f) * rstd).astype(f) + shift


def naive_stats_f32(z, eps):
    """(mean, rstd, zhat) from sequential fp32 sums of z and z^2: var = E[z^2] - E[z]^2 (may be negative: rstd NaN)."""
    f = np.float32
    z = np.asarray(z, f)
    B, C = z.shape
    s, q = np.zeros(C, f), np.zeros(C, f)
    for row in z:
        s = s + row
        q = q + row * row
    mean = s / f(B)
    with np.errstate(invalid="ignore"):
        return _finish(z, mean, q / f(B) - mean * mean, eps)


def errors_in_units(z, eps, mean, rstd, zhat):
    """Per column: the worst of |zhat - ref|, |rstd s - 1| and |mean - mu| / s, in units of u_c (NaN where non-finite)."""
    mu, _, s = stats64(z, eps)
    u = bound(z, eps)
    z64 = np.asarray(z, np.float64)
    e = np.maximum(np.abs(zhat.astype(np.float64) - (z64 - mu) / s).max(0),
                   np.maximum(np.abs(rstd.astype(np.float64) * s - 1), np.abs(mean.astype(np.float64) - mu) / s))
    return e / u
