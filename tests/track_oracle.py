"""numpy restatement of csrc/track.h in plain loops, written from the issue's definitions and the text of the reference
(phase1_lifting/video2keypoints.py:14-57 coco2h36m, :83-98 the all-zero row of a frame without a detection).

remap and prepare take a dtype: np.float32 restates the library's arithmetic operation by operation (numpy float32 scalars
round after every operation and never fuse), so bits can be compared; np.float64 is the yardstick for figures.  filter and
velocity_errors are fp64 only and come with the error bounds the tests hold the fp32 library to."""
import numpy as np

COCO17, H36M17 = 0, 1
VALID, INTERPOLATED, HELD, LOST = 0, 1, 2, 3
U = 2.0 ** -24                     # unit round-off of fp32


def _min(a, b):
    """minimum, a NaN winning"""
    if a != a:
        return a
    if b != b:
        return b
    return b if b < a else a


def remap(det, layout=COCO17, dtype=np.float32):
    """det (T, 17, 3) -> (T, 17, 3) in the H36M-17 layout, confidences following their joints (a derived joint: the minimum)."""
    f = dtype
    x = np.asarray(det, np.float32).astype(f)
    if layout == H36M17:
        return x.copy()
    y = np.zeros_like(x)
    half = f(0.5)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(x.shape[0]):
            r = x[t]

            def mid(a, b):
                return [(a[0] + b[0]) * half, (a[1] + b[1]) * half, _min(a[2], b[2])]
            y[t, 0] = mid(r[11], r[12])
            y[t, 1] = r[12]
            y[t, 2] = r[14]
            y[t, 3] = r[16]
            y[t, 4] = r[11]
            y[t, 5] = r[13]
            y[t, 6] = r[15]
            y[t, 8] = mid(r[5], r[6])
            y[t, 7] = mid(y[t, 0], y[t, 8])
            y[t, 9] = r[0]
            y[t, 10] = mid(r[1], r[2])
            y[t, 11] = r[5]
            y[t, 12] = r[7]
            y[t, 13] = r[9]
            y[t, 14] = r[6]
            y[t, 15] = r[8]
            y[t, 16] = r[10]
    return y


def _same_seq(seq, t, s):
    return seq is None or seq[s] == seq[t]


def prepare(det, layout=COCO17, div=(1.0, 1.0), conf_thr=0.1, max_gap=8, fill_conf=0.5, seq_ids=None, dtype=np.float32):
    """-> xy (T, 17, 2), w (T, 17) of `dtype`, state (T, 17) uint8.  The parameters are rounded to float32 first, as the C
    interface takes them."""
    f = dtype
    h = remap(det, layout, f)
    T = h.shape[0]
    dw, dh, thr, fc = (f(np.float32(v)) for v in (div[0], div[1], conf_thr, fill_conf))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        sx, sy, conf = h[..., 0] / dw, h[..., 1] / dh, h[..., 2]
        valid = (conf >= thr) & np.isfinite(sx) & np.isfinite(sy)
    s = np.stack([sx, sy], axis=-1)
    xy, w, state = np.zeros((T, 17, 2), f), np.zeros((T, 17), f), np.zeros((T, 17), np.uint8)

    def search(t, j, step):
        """(distance of the nearest valid sample or 0, whether the search left the sequence)"""
        for i in range(1, max_gap + 1):
            u = t + step * i
            if u < 0 or u >= T or not _same_seq(seq_ids, t, u):
                return 0, True
            if valid[u, j]:
                return i, False
        return 0, False

    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            for j in range(17):
                if valid[t, j]:
                    xy[t, j], w[t, j], state[t, j] = s[t, j], conf[t, j], VALID
                    continue
                da, left_a = search(t, j, -1)
                db, left_b = search(t, j, +1)
                if da and db and da + db - 1 <= max_gap:
                    a, b = t - da, t + db
                    frac = f(da) / f(da + db)
                    for d in range(2):
                        xy[t, j, d] = s[a, j, d] + (s[b, j, d] - s[a, j, d]) * frac
                    w[t, j], state[t, j] = fc * _min(conf[a, j], conf[b, j]), INTERPOLATED
                elif bool(da) != bool(db) and (left_b if da else left_a):
                    u = t - da if da else t + db
                    xy[t, j], w[t, j], state[t, j] = s[u, j], fc * conf[u, j], HELD
                else:
                    for d in range(2):
                        xy[t, j, d] = s[t, j, d] if np.isfinite(s[t, j, d]) else f(0)
                    w[t, j], state[t, j] = f(0), LOST
    return xy, w, state


def window(seq_ids, T, t, h):
    """the frames of t's sequence within h of t: (lo, hi) as offsets"""
    lo = hi = 0
    while lo > -h and t + lo - 1 >= 0 and _same_seq(seq_ids, t, t + lo - 1):
        lo -= 1
    while hi < h and t + hi + 1 < T and _same_seq(seq_ids, t, t + hi + 1):
        hi += 1
    return lo, hi


def filter(x, taps, w=None, seq_ids=None):  # noqa: A001
    """fp64: y (T, J, D) and xmax (T, J, D) = max |x| over the samples of each window (what the bound scales with).
    A window without a positive denominator passes x[t] through; there xmax = 0 (the result is a copy: no error allowed)."""
    x32 = np.asarray(x, np.float32)
    x64 = x32.astype(np.float64)
    taps = np.asarray(taps, np.float32).astype(np.float64)
    w64 = None if w is None else np.asarray(w, np.float32).astype(np.float64)
    T, J, D = x64.shape
    K, h = len(taps), len(taps) // 2
    y, xmax = np.zeros_like(x64), np.zeros_like(x64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):                                   # the joints of a frame share the window: arrays over (J, D)
            lo, hi = window(seq_ids, T, t, h)
            num, den, big, used = np.zeros((J, D)), np.zeros(J), np.zeros((J, D)), np.zeros(J, bool)
            for k in range(K):
                o = k - h
                if o < lo or o > hi:
                    continue
                ws = np.ones(J) if w64 is None else w64[t + o]
                take = ws != 0.0                             # a sample with w == 0 is skipped, whatever x holds there
                c = taps[k] * ws
                num = np.where(take[:, None], num + c[:, None] * x64[t + o], num)
                den = np.where(take, den + c, den)
                big = np.where(take[:, None], np.fmax(big, np.abs(x64[t + o])), big)
                used |= take
            ok = used & (den > 0)
            y[t] = np.where(ok[:, None], num / np.where(ok, den, 1.0)[:, None], x64[t])
            xmax[t] = np.where(ok[:, None], big, 0.0)
    return y, xmax


def filter_bound(xmax, K):
    """|fp32 result - fp64 result| allowed per element: (K + 3) 2^-24 X, X = max |x| over the window.
    With c_k = taps[k] w_k >= 0 the result is the convex combination sum c_k x_k / sum c_k of values |x_k| <= X.  A first-order
    worst-case count of the fp32 form -- per term one product and at most K - 1 additions in the numerator, each at most
    u X sum c_k; K - 1 additions in the denominator; the rounding of c_k, a relative perturbation of the weights, worth 2 u X;
    one division -- gives (2 K + 2) u X.  The tests hold the library to the tighter figure the specification sets, the running
    error of the K-term combination plus the three single roundings (weight, product, division): (K + 3) u X."""
    return (K + 3) * U * xmax


def has_stencil(seq_ids, T, t, order):
    if t < 1 or not _same_seq(seq_ids, t, t - 1):
        return False
    if order == 2 and (t + 1 >= T or not _same_seq(seq_ids, t, t + 1)):
        return False
    return True


def velocity_errors(pred, target, seq_ids=None, order=1, sub=None, div=None):
    """fp64: err (T, J), count (T,) uint8 and bound (T, J), the fp32 library's allowed distance from err.
    Bound: with A_d the sum of the magnitudes a stencil element combines (|p[t]| + |p[t-1]| + |g[t]| + |g[t-1]|; order 2:
    |q[t+1]| + 2 |q[t]| + |q[t-1]| for both tracks), every rounded subtraction or addition errs by at most u A_d and there
    are r = 3 (order 1) or 5 (order 2; 2 q[t] is exact) of them: delta_d <= r u A_d.  A load through (sub, div) is two more
    roundings, each at most u (|v div| + |sub|), entering with the stencil's coefficients.  The norm moves by at most
    ||delta||; squares, two additions and a correctly rounded square root add a relative 2.5 u, taken as 4 u to cover the
    second-order terms."""
    p = np.asarray(pred, np.float32).astype(np.float64)
    g = np.asarray(target, np.float32).astype(np.float64)
    T, J, _ = p.shape
    load = np.zeros_like(p)
    if sub is not None:
        s64, d64 = np.asarray(sub, np.float32).astype(np.float64), np.asarray(div, np.float32).astype(np.float64)
        zero = np.broadcast_to(d64 == 0, p.shape)

        def back(v):
            return np.where(zero, np.broadcast_to(s64, v.shape), v * d64 + s64), np.where(zero, 0.0, 2 * U * (np.abs(v * d64) + np.abs(s64)))
        (p, lp), (g, lg) = back(p), back(g)
    else:
        lp = lg = load
    err, count, bound = np.zeros((T, J)), np.zeros(T, np.uint8), np.zeros((T, J))
    for t in range(T):
        if not has_stencil(seq_ids, T, t, order):
            continue
        count[t] = 1
        if order == 1:
            e = (p[t] - p[t - 1]) - (g[t] - g[t - 1])
            A = np.abs(p[t]) + np.abs(p[t - 1]) + np.abs(g[t]) + np.abs(g[t - 1])
            ld = lp[t] + lp[t - 1] + lg[t] + lg[t - 1]
            r = 3
        else:
            e = (p[t + 1] - 2 * p[t] + p[t - 1]) - (g[t + 1] - 2 * g[t] + g[t - 1])
            A = (np.abs(p[t + 1]) + 2 * np.abs(p[t]) + np.abs(p[t - 1]) + np.abs(g[t + 1]) + 2 * np.abs(g[t]) + np.abs(g[t - 1]))
            ld = lp[t + 1] + 2 * lp[t] + lp[t - 1] + lg[t + 1] + 2 * lg[t] + lg[t - 1]
            r = 5
        delta = np.linalg.norm(r * U * (A + ld) + ld, axis=-1)
        err[t] = np.linalg.norm(e, axis=-1)
        bound[t] = delta + 4 * U * (err[t] + delta)
    return err, count, bound
