"""The flat AdamW step in fp64, the bounds a fp32 implementation is held to, and the cases both are run on (numpy only).

One step of torch.optim.AdamW's single-tensor update, in the order csrc/adamw.h adamw_one takes it:

    g' = g * gscale * coef          p <- p * (1 - lr * wd)
    m' = m + (g' - m) * (1 - b1)    v' = v * b2 + (1 - b2) * g' * g'
    den = sqrt(v') / sqrt(bc2) + eps,   bc1 = 1 - b1^t,   bc2 = 1 - b2^t
    p' = p - (lr / bc1) * m' / den

THE REFERENCE STARTS FROM THE IMPLEMENTATION'S OWN fp32 STATE of the step before (p, m, v as the GPU left them, g as the GPU
read it): nothing accumulates from step to step, so every step of a run is held to rounding alone.

Hyper-parameters are ROUNDED TO fp32 FIRST: the C ABI takes floats, and 1 - beta is formed from the rounded beta, as
adamw_consts does.  t is exact and the bias corrections are fp64.

Bounds, with K = 16, u = 2^-24, tau = 2^-126 (the smallest normal fp32):

    |m' - m^| <= K u (|m| + |g'|) + tau
    |v' - v^| <= K u v^ + tau
    |p' - p^| <= K u (|p| + (lr / bc1) (|m| + |g'|) / den) + tau
    |e' - e^| <= 4 u (|e| + |p'|) + tau         (averaged weights; e^ formed from the implementation's own p')

The update is about ten fp32 roundings: g', the decay constant and its product, (g' - m), its product and sum, the two products
and the sum of v', the square root, its quotient by sqrt(bc2) (itself rounded once), the sum with eps, m' / den, the product
with lr / bc1 (rounded once), the difference.  Each is at most u relative to a quantity the right-hand sides majorise: m' is a
convex combination of m and g' (so |m'| <= |m| + |g'|, and the cancellation in it is paid for in those terms, not in |m'|);
v' is a sum of non-negative terms; den is a sum of positive terms, so its relative error is that of its parts.  K = 16 leaves
the factor the emulation below measures (tests/test_adamw_edges_host.py prints it).  tau: a denormal v or m has no relative
accuracy (absolute 2^-149), and such a v cannot move p past eps.  Fused multiply-adds only remove roundings.
The average is two roundings (the difference, one fused multiply-add): 4 u on |e| + |p'| covers both with a factor two.
"""
from collections import namedtuple

import numpy as np

K = 16
U = 2.0 ** -24
TAU = 2.0 ** -126

Ref = namedtuple("Ref", "p m v gp den step")
Case = namedtuple("Case", "id cls hp t")          # hp = (lr, beta1, beta2, eps, wd, gscale)


def f32(x):
    """x rounded to fp32, as a Python float (what the C ABI's float arguments hold)."""
    return float(np.float32(x))


def round_hp(hp):
    return tuple(f32(x) for x in hp)


def _a64(x):
    return np.asarray(x, dtype=np.float64)


def step64(p, g, m, v, hp, t, coef=1.0):
    """One step in fp64 from the caller's fp32 state.  hp = (lr, beta1, beta2, eps, wd, gscale) is first rounded to fp32 (the C
    ABI takes floats; 1 - beta is formed from the ROUNDED beta, as adamw.h does), so is coef (a float of the clip record); t is
    an exact integer and the bias corrections are fp64.  Returns Ref(p, m, v, gp, den, step): the new state, the gradient
    as it entered the moments, the denominator and lr / bc1 (what bounds() needs)."""
    lr, b1, b2, eps, wd, gs = round_hp(hp)
    t = int(t)
    assert t >= 1
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    p, g, m, v = _a64(p), _a64(g), _a64(m), _a64(v)
    gp = g * gs * f32(coef)
    pd = p * (1.0 - lr * wd)
    mn = m + (gp - m) * (1.0 - b1)
    vn = v * b2 + (1.0 - b2) * gp * gp
    den = np.sqrt(vn) / np.sqrt(bc2) + eps
    step = lr / bc1
    return Ref(pd - step * mn / den, mn, vn, gp, den, step)


def bounds(p, m, ref):
    """(bound on p', on m', on v') for a step from (p, m) whose reference is ref."""
    gm = np.abs(_a64(m)) + np.abs(ref.gp)
    return (K * U * (np.abs(_a64(p)) + ref.step * gm / ref.den) + TAU, K * U * gm + TAU, K * U * ref.v + TAU)


def ratios(got_p, got_m, got_v, p, m, ref, k=K):
    """Worst |got - ref| / bound per quantity, in units of the bounds at K = k: {'p':, 'm':, 'v':}.  Non-finite -> inf."""
    out = {}
    bp, bm, bv = bounds(p, m, ref)
    for name, got, want, b in (("p", got_p, ref.p, bp), ("m", got_m, ref.m, bm), ("v", got_v, ref.v, bv)):
        got = _a64(got)
        b = (b - TAU) * (k / K) + TAU
        if not np.isfinite(got).all():
            out[name] = float("inf")
        else:
            out[name] = float((np.abs(got - want) / b).max())
    return out


def ema_omd(decay, warmup, n):
    """(float)(1 - d_n), d_n = decay or min(decay, (1 + n) / (10 + n)): csrc/adamw.h ema_omd, n the 1-based update count."""
    d = f32(decay)
    if warmup:
        d = min(d, (1.0 + n) / (10.0 + n))
    return f32(1.0 - d)


def ema64(e, p_new, decay, warmup, n):
    """(e^, bound): the average after update n, in fp64 from the implementation's own e and p'."""
    e, p_new = _a64(e), _a64(p_new)
    return e + (p_new - e) * ema_omd(decay, warmup, n), 4 * U * (np.abs(e) + np.abs(p_new)) + TAU


# ---- the fp32 emulation of the kernel's order, and the faults the gate has to see -----------------------------------------
FAULTS = ("pow32", "eps_fixed", "beta_swap", "t_off_by_one", "gscale_m_only", "wd_after", "eps_scaled", "coef_dropped")


def emulate32(p, g, m, v, hp, t, coef=1.0, fault=None):
    """The step in numpy fp32 in the order of adamw_consts / adamw_one (constants in double, each rounded once; every element
    operation rounded to fp32; no fused multiply-add).  fault: one of FAULTS --
      pow32          bias corrections formed with an fp32 pow
      eps_fixed      eps hard-coded to 1e-8
      beta_swap      beta1 and beta2 exchanged
      t_off_by_one   t + 1 in the bias corrections
      gscale_m_only  the gradient scale reaches m but not v
      wd_after       weight decay applied after the update instead of before
      eps_scaled     1 / sqrt(bc2) applied to eps too
      coef_dropped   the clip coefficient ignored
    Returns (p', m', v') as fp32 arrays."""
    assert fault is None or fault in FAULTS
    F = np.float32
    lr, b1, b2, eps, wd, gs = round_hp(hp)
    t = int(t)
    if fault == "beta_swap":
        b1, b2 = b2, b1
    if fault == "t_off_by_one":
        t += 1
    if fault == "eps_fixed":
        eps = f32(1e-8)
    with np.errstate(all="ignore"):
        if fault == "pow32":
            bc1 = float(F(1) - np.power(F(b1), F(t)))
            bc2 = float(F(1) - np.power(F(b2), F(t)))
        else:
            bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        decay, omb1, omb2 = F(1.0 - lr * wd), F(1.0 - b1), F(1.0 - b2)
        step, bc2s = F(lr / bc1), F(np.sqrt(bc2))
        gsc = F(gs) if fault == "coef_dropped" else F(gs) * F(coef)
        p, g, m, v = (np.asarray(a, F) for a in (p, g, m, v))
        gm = g * gsc
        gv = g if fault == "gscale_m_only" else gm
        pd = p if fault == "wd_after" else p * decay
        mn = m + (gm - m) * omb1
        vn = v * F(b2) + (omb2 * gv) * gv
        if fault == "eps_scaled":
            den = (np.sqrt(vn) + F(eps)) / bc2s
        else:
            den = np.sqrt(vn) / bc2s + F(eps)
        pn = pd - step * (mn / den)
        if fault == "wd_after":
            pn = pn * decay
    return pn.astype(F), mn.astype(F), vn.astype(F)


# ---- the cases ----------------------------------------------------------------------------------------------------------
HP_TUPLES = (                                   # (lr, beta1, beta2, eps, wd)
    (1e-3, 0.9, 0.999, 1e-8, 0.01),
    (1e-3, 0.0, 0.999, 1e-8, 0.01),
    (1e-3, 0.5, 0.9, 1e-3, 0.0),
    (1e-1, 0.9, 0.99999, 1e-12, 0.3),
    (1e-3, 0.99, 0.5, 1e-8, 0.01),
    (0.0, 0.9, 0.999, 1e-8, 0.0),                # p comes back bitwise; m and v still move
)
GSCALES = (1.0, 0.125, 3.7)
TS = (1, 2, 7, 1000, 10 ** 6, 10 ** 9)
CLASSES = ("normal", "tiny", "huge", "zero", "mixed")
N_GRID = 1027


def cases(classes=CLASSES):
    """Every (class, tuple, gscale, t) of the grid, with an id that names it."""
    out = []
    for cls in classes:
        for i, hp in enumerate(HP_TUPLES):
            for gs in GSCALES:
                for t in TS:
                    out.append(Case(f"{cls}/hp{i}/gs{gs:g}/t{t}", cls, hp + (gs,), t))
    return out


def values(cls, n, t, seed=0):
    """(p, g, m, v) fp32 of one value class; at t = 1 the moments are zero (a first step).
      normal  g, m ~ 1e-2, v ~ 1e-4
      tiny    |g|, |m| ~ 1e-20 (g^2 below the fp32 normal range), v ~ 1e-40 (denormal)
      huge    |g|, |m| ~ 1e15, v ~ 1e30 (g'^2 <= (2 * 3.7e15)^2 < fp32 max)
      zero    g = m = v = 0: the denominator is eps
      mixed   per element, independently, |g|, |m| = 10^k and v = 10^2k', k, k' in -12 .. 5
    p ~ N(0, 1) with every seventh element zero."""
    rng = np.random.default_rng([seed, CLASSES.index(cls), n, t % 1009])
    F = np.float32
    p = rng.standard_normal(n)
    p[::7] = 0.0
    sign = lambda: rng.choice([-1.0, 1.0], n)
    spread = lambda: rng.uniform(0.5, 2.0, n)
    if cls == "normal":
        g, m, v = rng.standard_normal(n) * 1e-2, rng.standard_normal(n) * 1e-2, rng.uniform(0.5, 1.5, n) * 1e-4
    elif cls == "tiny":
        g, m, v = sign() * spread() * 1e-20, sign() * spread() * 1e-20, spread() * 1e-40
    elif cls == "huge":
        g, m, v = sign() * spread() * 1e15, sign() * spread() * 1e15, spread() * 1e30
    elif cls == "zero":
        g, m, v = np.zeros(n), np.zeros(n), np.zeros(n)
    elif cls == "mixed":
        g = sign() * 10.0 ** rng.integers(-12, 6, n)
        m = sign() * 10.0 ** rng.integers(-12, 6, n)
        v = 10.0 ** (2 * rng.integers(-12, 6, n))
    else:
        raise ValueError(cls)
    if t == 1:
        m, v = np.zeros(n), np.zeros(n)
    with np.errstate(all="ignore"):
        return p.astype(F), g.astype(F), m.astype(F), v.astype(F)
