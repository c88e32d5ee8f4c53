"""CPU tests of the video-track definitions: csrc/track.h through the _host entry points (the same inline text the kernels
run, compiled for the CPU) against the numpy restatement of track_oracle.py.

remap and prepare are exact: state equal, xy and w bit for bit against the float32 restatement.  The filter is held to
(K + 3) 2^-24 max|x| of its window against the fp64 oracle (track_oracle.filter_bound), the velocity errors to the bound
track_oracle.velocity_errors derives beside its values.  The recorded track g15_video_tracks.npz supplies the figures."""
import json
import os

import numpy as np
import pytest

import track_oracle as orc
from conftest import load_golden

EINVAL, ESHAPE = -1, -2
F = np.float32


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()


@pytest.fixture(scope="module")
def g15():
    return load_golden("g15_video_tracks.npz")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _p(a):
    return None if a is None else a.ctypes.data


def _seq(seq):
    return None if seq is None else np.ascontiguousarray(seq, np.int32)


# ---- host entry points (the GPU tests import these) ---------------------------------------------------------------------------
def host_remap(pkg, det, layout=orc.COCO17, expect=0):
    det = np.ascontiguousarray(det, F)
    out = np.full(det.shape, -7.0, F)
    assert pkg.lib().pl_track_remap_host(det.ctypes.data, det.shape[0], layout, out.ctypes.data) == expect, pkg.lib().pl_last_error()
    return out


def host_prepare(pkg, det, layout=orc.COCO17, div=(1.0, 1.0), conf_thr=0.1, max_gap=8, fill_conf=0.5, seq=None, expect=0):
    det, seq = np.ascontiguousarray(det, F), _seq(seq)
    T = det.shape[0]
    xy, w, st = np.full((T, 17, 2), -7.0, F), np.full((T, 17), -7.0, F), np.full((T, 17), 77, np.uint8)
    rc = pkg.lib().pl_track_prepare_host(det.ctypes.data, T, layout, div[0], div[1], conf_thr, max_gap, fill_conf, _p(seq),
                                         xy.ctypes.data, w.ctypes.data, st.ctypes.data)
    assert rc == expect, pkg.lib().pl_last_error()
    return xy, w, st


def host_filter(pkg, x, taps, w=None, seq=None, expect=0):
    x, taps, seq = np.ascontiguousarray(x, F), np.ascontiguousarray(taps, F), _seq(seq)
    w = None if w is None else np.ascontiguousarray(w, F)
    T, J, D = x.shape
    y = np.full(x.shape, -7.0, F)
    rc = pkg.lib().pl_track_filter_host(x.ctypes.data, T, J, D, _p(w), _p(seq), taps.ctypes.data, len(taps), y.ctypes.data)
    assert rc == expect, pkg.lib().pl_last_error()
    return y


def host_velocity(pkg, pred, tgt, seq=None, order=1, sub=None, div=None, expect=0):
    pred, tgt, seq = np.ascontiguousarray(pred, F), np.ascontiguousarray(tgt, F), _seq(seq)
    sub = None if sub is None else np.ascontiguousarray(sub, F)
    div = None if div is None else np.ascontiguousarray(div, F)
    T, J, _ = pred.shape
    err, cnt = np.full((T, J), -7.0, F), np.full(T, 77, np.uint8)
    rc = pkg.lib().pl_track_velocity_errors_host(pred.ctypes.data, tgt.ctypes.data, T, J, _p(seq), order, _p(sub), _p(div),
                                                 err.ctypes.data, cnt.ctypes.data)
    assert rc == expect, pkg.lib().pl_last_error()
    return err, cnt


# ---- shared makers -------------------------------------------------------------------------------------------------------------
def make_seq(T, kind, seed=0):
    """None, two halves, an id per frame, or random runs that include runs of one and two frames"""
    if kind == "none":
        return None
    if kind == "halves":
        return np.where(np.arange(T) < (T + 1) // 2, 5, 2).astype(np.int32)
    if kind == "each":
        return (np.arange(T) * 3 - 7).astype(np.int32)
    rs = np.random.RandomState(seed + T)
    ids, t = np.zeros(T, np.int32), 0
    while t < T:
        n = int(rs.choice([1, 1, 2, 3, 9, 40]))
        ids[t:t + n] = rs.randint(-5, 1000)
        t += n
    return ids


def make_det(T, seed, low=0.25, missing=0.08):
    """A random detector track in pixels: confidences in (0.2, 1), a share `low` of the joints in runs below the threshold
    0.1, a share `missing` of the frames all zeros."""
    rs = np.random.RandomState(seed + 7 * T)
    det = np.empty((T, 17, 3), F)
    det[..., 0], det[..., 1] = rs.uniform(0, 1000, (T, 17)), rs.uniform(0, 1002, (T, 17))
    det[..., 2] = rs.uniform(0.2, 1.0, (T, 17))
    bad = rs.rand(T, 17) < low / 2
    for n in (1, 2, 7):                                                # grow some of them into runs
        grow = bad & (rs.rand(T, 17) < 0.3)
        for k in range(1, n + 1):
            bad[k:] |= grow[:-k] if k < T else False
    det[..., 2][bad] = rs.uniform(0.0, 0.0999, int(bad.sum()))
    det[rs.rand(T) < missing] = 0.0
    return det


PREP_T, PREP_G = (1, 2, 9, 64, 65, 130), (0, 1, 8, 64)
SEQ_KINDS = ("none", "halves", "each", "runs")


def prepare_cases():
    """(det, layout, div, conf_thr, G, fill_conf, seq) over every T, G and sequence shape, both layouts"""
    out = []
    for ti, T in enumerate(PREP_T):
        for gi, G in enumerate(PREP_G):
            for si, kind in enumerate(SEQ_KINDS):
                layout = (ti + gi + si) % 2
                out.append((make_det(T, 100 * gi + si), layout, (1000.0, 1002.0), 0.1, G, 0.5 if si % 2 else 0.3, make_seq(T, kind, gi)))
    return out


def gap_track(G):
    """H36M-17 rows with hand-placed gaps of joint j (confidence 0 inside a gap): (det, T, expected state (T, 17))
       j 0  a gap of exactly G after frame 0                      -> interpolated
       j 1  a gap of G + 1 after frame 0                          -> lost
       j 2  the first min(G, 3) frames                            -> held from the right
       j 3  the last min(G, 3) frames                             -> held from the left
       j 4  every frame                                           -> lost
       j 5  the first G + 1 frames                                -> frame 0 lost (its sample is G + 1 away), frame G lost (its
                                                                     G steps to the left all stay inside the sequence), the rest held
       j 6  a gap of G in the middle whose far end lies G + 1 from its first frame: all interpolated"""
    T = 130 if G == 64 else 3 * G + 10
    rs = np.random.RandomState(G)
    det = np.empty((T, 17, 3), F)
    det[..., :2], det[..., 2] = rs.uniform(0, 1000, (T, 17, 2)), rs.uniform(0.2, 1.0, (T, 17))
    want = np.zeros((T, 17), np.uint8)
    g3 = min(G, 3)
    for j, (a, b, st) in enumerate([(1, 1 + G, orc.INTERPOLATED), (1, 2 + G, orc.LOST), (0, g3, orc.HELD), (T - g3, T, orc.HELD),
                                    (0, T, orc.LOST), (0, G + 1, orc.HELD), (T - G - 3, T - 3, orc.INTERPOLATED)]):
        det[a:b, j, 2] = 0.0
        want[a:b, j] = st
    want[0, 5] = want[G, 5] = orc.LOST
    return det, T, want


def filter_taps(pkg, K, seed):
    if seed % 2:
        return pkg.TemporalFilter.gaussian(K / 6.0 + 0.3, radius=K // 2).taps
    return np.random.RandomState(seed + K).uniform(0.0, 1.0, K).astype(F)


def make_x(T, J, D, seed):
    rs = np.random.RandomState(seed + 3 * T + J)
    return (rs.randn(T, J, D) * 0.4 + rs.uniform(-2, 2, (1, J, D))).astype(F)


def make_w(T, J, seed, zeros=0.2):
    rs = np.random.RandomState(seed + 5 * T + J)
    w = rs.uniform(0.05, 1.0, (T, J)).astype(F)
    w[rs.rand(T, J) < zeros] = 0.0
    return w


FILT_K, FILT_T = (1, 3, 7, 65), (1, 2, 31, 33, 64, 65, 129)


def filter_cases(pkg):
    """(x, taps, w, seq): every K with every T at J = 17 and both D; every (J, D) at two sizes; a sequence boundary in the
    middle of a window, on the edge of a workgroup's tile and one frame to either side of it."""
    out = []
    for ki, K in enumerate(FILT_K):
        for ti, T in enumerate(FILT_T):
            for D in (2, 3):
                n = ki + ti + D
                out.append((make_x(T, 17, D, n), filter_taps(pkg, K, n), make_w(T, 17, n) if n % 3 else None,
                            make_seq(T, SEQ_KINDS[n % 4], n)))
    for K, T in ((7, 65), (65, 129)):
        for J in (1, 17, 32):
            for D in (2, 3):
                out.append((make_x(T, J, D, K), filter_taps(pkg, K, J), make_w(T, J, K), make_seq(T, "runs", K + J)))
    for K in (7, 65):
        tile = pkg.lib().pl_track_filter_tile_frames(17, 3, K)
        assert tile == 64
        for b in (tile - 1, tile, tile + 1, tile + K // 2, 2 * tile):
            seq = (np.arange(129) >= b).astype(np.int32)
            out.append((make_x(129, 17, 3, b), filter_taps(pkg, K, 1), make_w(129, 17, b), seq))
    K = 65
    assert pkg.lib().pl_track_filter_tile_frames(32, 3, K) == 32            # the halved tile of the widest rows
    for b in (31, 32, 33):
        out.append((make_x(129, 32, 3, b), filter_taps(pkg, K, 1), make_w(129, 32, b), (np.arange(129) >= b).astype(np.int32)))
    return out


def velocity_cases():
    """(pred, tgt, seq, order, sub, div)"""
    out = []
    for T in (1, 2, 3, 9, 65):
        for J in (1, 17, 32):
            for order in (1, 2):
                for kind in ("none", "runs", "each", "halves"):
                    g = make_x(T, J, 3, order)
                    p = (g + np.random.RandomState(T + J).randn(T, J, 3) * 0.05).astype(F)
                    sub = div = None
                    if kind in ("runs", "halves"):
                        rs = np.random.RandomState(J)
                        sub, div = rs.uniform(-0.3, 0.3, (J, 3)).astype(F), rs.uniform(0.05, 0.6, (J, 3)).astype(F)
                        sub[0], div[0] = 0.0, 0.0
                    out.append((p, g, make_seq(T, kind, order), order, sub, div))
    return out


# ---- remap ------------------------------------------------------------------------------------------------------------------
def test_remap_is_coco2h36m_in_float32(pkg):
    rs = np.random.RandomState(1)
    det = np.concatenate([rs.uniform(0, 1000, (67, 17, 2)), rs.uniform(0, 1, (67, 17, 1))], axis=-1).astype(F)
    got = host_remap(pkg, det)
    assert same_bits(got, orc.remap(det))
    # the reference's function, restated on whole arrays: numpy float32 rounds after every operation
    x = det[..., :2]
    y = np.zeros_like(x)
    y[:, 0] = (x[:, 11] + x[:, 12]) * F(0.5)
    for j, s in ((1, 12), (2, 14), (3, 16), (4, 11), (5, 13), (6, 15), (9, 0), (11, 5), (12, 7), (13, 9), (14, 6), (15, 8), (16, 10)):
        y[:, j] = x[:, s]
    y[:, 8] = (x[:, 5] + x[:, 6]) * F(0.5)
    y[:, 7] = (y[:, 0] + y[:, 8]) * F(0.5)
    y[:, 10] = (x[:, 1] + x[:, 2]) * F(0.5)
    assert same_bits(got[..., :2], y)
    c = det[..., 2]
    assert same_bits(got[:, 0, 2], np.minimum(c[:, 11], c[:, 12])) and same_bits(got[:, 8, 2], np.minimum(c[:, 5], c[:, 6]))
    assert same_bits(got[:, 10, 2], np.minimum(c[:, 1], c[:, 2]))
    assert same_bits(got[:, 7, 2], np.minimum(np.minimum(c[:, 11], c[:, 12]), np.minimum(c[:, 5], c[:, 6])))
    assert same_bits(got[:, 3, 2], c[:, 16]) and same_bits(got[:, 9, 2], c[:, 0])
    assert same_bits(host_remap(pkg, det, orc.H36M17), det)
    host_remap(pkg, det, 2, expect=EINVAL)


# ---- prepare ----------------------------------------------------------------------------------------------------------------
def check_prepare(pkg, det, layout, div, thr, G, fc, seq):
    xy, w, st = host_prepare(pkg, det, layout, div, thr, G, fc, seq)
    oxy, ow, ost = orc.prepare(det, layout, div, thr, G, fc, seq)
    tag = (det.shape[0], layout, G, None if seq is None else seq[:4])
    assert np.array_equal(st, ost), tag
    assert same_bits(xy, oxy) and same_bits(w, ow), tag
    assert np.isfinite(xy).all() and np.isfinite(w).all()
    return xy, w, st


def test_prepare_matches_the_restatement_bit_for_bit(pkg):
    seen = np.zeros(4, np.int64)
    for case in prepare_cases():
        seen += np.bincount(check_prepare(pkg, *case)[2].reshape(-1), minlength=4)
    assert (seen > 100).all(), seen                                   # every state is exercised


@pytest.mark.parametrize("G", [0, 1, 8, 64])
def test_prepare_gaps_of_exactly_g_and_g_plus_one(pkg, G):
    det, T, want = gap_track(G)
    if G == 0:
        want = np.where(det[..., 2] == 0, orc.LOST, 0).astype(np.uint8)
    xy, w, st = check_prepare(pkg, det, orc.H36M17, (1.0, 1.0), 0.1, G, 0.5, None)
    assert np.array_equal(st, want)
    lost = st == orc.LOST
    assert np.all(w[lost].view(np.uint32) == 0) and same_bits(xy[lost], det[..., :2][lost])      # own value, weight +0
    if G:
        g3 = min(G, 3)
        assert same_bits(xy[:g3, 2], np.broadcast_to(det[g3, 2, :2], (g3, 2)))                  # held from the right
        assert same_bits(w[:g3, 2], np.full(g3, F(0.5) * det[g3, 2, 2]))
        assert same_bits(xy[T - g3:, 3], np.broadcast_to(det[T - g3 - 1, 3, :2], (g3, 2)))
        t = 1 + G // 2                                                                          # one interpolated sample by hand
        a, b = det[0, 0], det[G + 1, 0]
        frac = F(t) / F(G + 1)
        assert same_bits(xy[t, 0], a[:2] + (b[:2] - a[:2]) * frac) and w[t, 0] == F(0.5) * min(a[2], b[2])


def test_prepare_gaps_at_sequence_starts_and_ends(pkg):
    T, G = 40, 8
    rs = np.random.RandomState(3)
    det = np.empty((T, 17, 3), F)
    det[..., :2], det[..., 2] = rs.uniform(0, 1000, (T, 17, 2)), rs.uniform(0.2, 1.0, (T, 17))
    seq = np.repeat(np.array([4, 4, 9, 1, 7], np.int32), [10, 0, 12, 1, 17])           # 10 + 12 + 1 + 17 frames
    det[10:13, 0, 2] = 0            # touches the start of the second sequence
    det[19:22, 1, 2] = 0            # touches its end
    det[10:22, 2, 2] = 0            # both: the joint has no valid sample in that sequence
    det[22, 3, 2] = 0               # the sequence of length 1
    det[8:12, 4, 2] = 0             # a gap that straddles a boundary: two held halves, nothing interpolated across
    xy, w, st = check_prepare(pkg, det, orc.H36M17, (1.0, 1.0), 0.1, G, 0.5, seq)
    assert (st[10:13, 0] == orc.HELD).all() and same_bits(xy[10:13, 0], np.broadcast_to(det[13, 0, :2], (3, 2)))
    assert (st[19:22, 1] == orc.HELD).all() and same_bits(xy[19:22, 1], np.broadcast_to(det[18, 1, :2], (3, 2)))
    assert (st[10:22, 2] == orc.LOST).all() and st[22, 3] == orc.LOST
    assert (st[8:12, 4] == orc.HELD).all() and same_bits(xy[8:10, 4], np.broadcast_to(det[7, 4, :2], (2, 2)))
    assert same_bits(xy[10:12, 4], np.broadcast_to(det[12, 4, :2], (2, 2)))
    one = host_prepare(pkg, det[10:22], orc.H36M17, (1.0, 1.0), 0.1, G, 0.5, None)                  # a sequence alone
    assert same_bits(one[0], xy[10:22]) and same_bits(one[1], w[10:22]) and np.array_equal(one[2], st[10:22])


def test_prepare_non_finite_values_reach_no_output(pkg):
    for layout in (orc.COCO17, orc.H36M17):
        for T, G in ((9, 1), (65, 8), (130, 64)):
            det = make_det(T, 50 + G)
            clean = host_prepare(pkg, det, layout, (1000.0, 1002.0), 0.1, G)
            rs = np.random.RandomState(T)
            bad = det.copy()
            low = det[..., 2] < 0.1
            vals = np.array([np.nan, np.inf, -np.inf], F)
            hit = low & (rs.rand(T, 17) < 0.5)                          # non-finite coordinates in invalid samples
            bad[..., 0][hit] = vals[rs.randint(0, 3, int(hit.sum()))]
            bad[..., 1][hit & (rs.rand(T, 17) < 0.5)] = np.nan
            xy, w, st = check_prepare(pkg, bad, layout, (1000.0, 1002.0), 0.1, G, 0.5, None)
            assert np.array_equal(st, clean[2]) and same_bits(w, clean[1])
            keep = st != orc.LOST                                       # a lost sample shows its own value: 0 where not finite
            assert same_bits(xy[keep], clean[0][keep])
            hit2 = ~low & (rs.rand(T, 17) < 0.2)                        # ... and in samples whose confidence is valid
            bad2 = det.copy()
            bad2[..., 1][hit2] = vals[rs.randint(0, 3, int(hit2.sum()))]
            bad2[..., 2][~low & ~hit2 & (rs.rand(T, 17) < 0.05)] = np.nan      # and NaN confidences
            xy2, w2, st2 = check_prepare(pkg, bad2, layout, (1000.0, 1002.0), 0.1, G, 0.5, make_seq(T, "halves"))
            if layout == orc.H36M17:
                assert (st2[hit2] != orc.VALID).all()


def test_prepare_rejects_bad_arguments(pkg):
    det = make_det(9, 1)
    for kw in (dict(max_gap=-1), dict(max_gap=65), dict(div=(0.0, 1.0)), dict(div=(1.0, float("inf"))), dict(div=(-2.0, 1.0)),
               dict(conf_thr=float("nan")), dict(fill_conf=-0.5), dict(fill_conf=float("nan")), dict(layout=7)):
        host_prepare(pkg, det, expect=EINVAL, **kw)
    L = pkg.lib()
    assert L.pl_track_prepare_host(det.ctypes.data, 0, 0, 1.0, 1.0, 0.1, 8, 0.5, None, det.ctypes.data, det.ctypes.data, det.ctypes.data) == ESHAPE
    assert L.pl_track_prepare_host(det.ctypes.data, 9, 0, 1.0, 1.0, 0.1, 8, 0.5, None, det.ctypes.data, None, None) == EINVAL
    buf = np.zeros(9 * 17 * 3, F)
    assert L.pl_track_prepare_host(det.ctypes.data, 9, 0, 1.0, 1.0, 0.1, 8, 0.5, None, det.ctypes.data, buf.ctypes.data,
                                   buf.ctypes.data) == EINVAL         # outputs on the input and on each other


# ---- filter -----------------------------------------------------------------------------------------------------------------
def check_filter(got, x, taps, w, seq):
    want, xmax = orc.filter(x, taps, w, seq)
    bound = orc.filter_bound(xmax, len(taps))
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    err = np.abs(got.astype(np.float64) - want)
    ok = ~nan
    assert np.all(err[ok] <= bound[ok]), (x.shape, len(taps), float(np.max(err[ok] - bound[ok])))
    passed = ok & (xmax == 0) & (want != 0)
    assert same_bits(got[passed], x[passed])
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(ok & (bound > 0), err / bound, 0.0))) if ok.any() else 0.0


def test_filter_within_the_derived_bound_of_the_fp64_oracle(pkg):
    worst = {}
    for x, taps, w, seq in filter_cases(pkg):
        r = check_filter(host_filter(pkg, x, taps, w, seq), x, taps, w, seq)
        worst[len(taps)] = max(worst.get(len(taps), 0.0), r)
    print("worst |error| / ((K + 3) 2^-24 max|x|) per K:", {k: f"{v:.3f}" for k, v in sorted(worst.items())})


def test_filter_single_unit_tap_is_the_identity(pkg):
    for T, J, D in ((1, 17, 2), (65, 17, 3), (129, 32, 3)):
        x = make_x(T, J, D, 9)
        x[0, 0, 0] = -0.0
        assert same_bits(host_filter(pkg, x, [1.0]), x)
        w01 = (make_w(T, J, 1, zeros=0.3) > 0).astype(F)               # weights 0 (passed through) and 1 (x * 1 / 1)
        assert same_bits(host_filter(pkg, x, [1.0], w01, make_seq(T, "runs")), x)


def test_filter_zero_weights_and_nans(pkg):
    T, J, D, K = 129, 17, 3, 7
    x, w, taps = make_x(T, J, D, 2), make_w(T, J, 2, zeros=0.0), filter_taps(pkg, K, 1)
    seq = make_seq(T, "halves")
    w[40:50, 3] = 0.0                                  # frames 43..46 of joint 3 have nothing but zero weights in their window
    w[:, 5] = 0.0
    y = host_filter(pkg, x, taps, w, seq)
    check_filter(y, x, taps, w, seq)
    assert same_bits(y[43:47, 3], x[43:47, 3]) and same_bits(y[:, 5], x[:, 5])
    assert not same_bits(y[42, 3], x[42, 3])
    xn = x.copy()                                      # a NaN under zero weight changes nothing
    xn[44, 3, 1], xn[10, 5, :] = np.nan, np.inf
    w[70, 8] = 0.0
    xn[70, 8, 0] = np.nan
    yn = host_filter(pkg, xn, taps, w, seq)
    y2 = host_filter(pkg, x, taps, w, seq)
    mask = np.ones(x.shape, bool)
    mask[44, 3, 1], mask[10, 5, :] = False, False      # passed through: the input's own bits
    assert same_bits(yn[mask], y2[mask]) and np.isnan(yn[44, 3, 1]) and np.isinf(yn[10, 5]).all()
    assert np.isfinite(yn[70, 8]).all()
    # no weights: exactly the windows that contain the NaN become NaN
    xm = x.copy()
    xm[64, 2, 1] = np.nan                              # frame 64 is the last of the first sequence (65 frames)
    ym = host_filter(pkg, xm, taps, None, seq)
    want = np.zeros(x.shape, bool)
    want[61:65, 2, 1] = True
    assert np.array_equal(np.isnan(ym), want)
    check_filter(ym, xm, taps, None, seq)
    # a NaN weight: no positive denominator, the frame keeps its value
    wn = w.copy()
    wn[20, 1] = np.nan
    yw = host_filter(pkg, x, taps, wn, seq)
    assert same_bits(yw[17:24, 1], x[17:24, 1])


def test_filter_rejects_bad_taps_and_shapes(pkg):
    x = make_x(9, 17, 3, 0)
    for taps in ([0.5, 0.5], [0.2, -0.1, 0.9], [0.2, float("nan"), 0.2], [float("inf")], [1.0] * 67, [0.25] * 4):
        host_filter(pkg, x, taps, expect=EINVAL)
    host_filter(pkg, make_x(9, 33, 3, 0), [1.0], expect=ESHAPE)
    host_filter(pkg, np.zeros((9, 17, 4), F), [1.0], expect=ESHAPE)
    L = pkg.lib()
    t = np.ones(1, F)
    assert L.pl_track_filter_host(x.ctypes.data, 9, 17, 3, None, None, t.ctypes.data, 1, x.ctypes.data) == EINVAL   # in place
    for bad in ([0.5, 0.5], [-1.0], [1.0] * 66):
        with pytest.raises(ValueError):
            pkg.TemporalFilter(bad)
    g = pkg.TemporalFilter.gaussian(1.0)
    assert len(g) == 7 and g.taps.dtype == F and abs(float(g.taps.astype(np.float64).sum()) - 1) < 1e-6
    k = np.arange(-3, 4, dtype=np.float64)
    e = np.exp(-k * k / 2)
    assert np.array_equal(g.taps, (e / e.sum()).astype(F))
    assert len(pkg.TemporalFilter.gaussian(2.5)) == 17 and len(pkg.TemporalFilter.gaussian(2.0, radius=2)) == 5
    assert np.array_equal(pkg.TemporalFilter.box(5).taps, np.full(5, 0.2, F))


# ---- velocity -----------------------------------------------------------------------------------------------------------------
def check_velocity(got, p, g, seq, order, sub, div):
    err, cnt = got
    oerr, ocnt, bound = orc.velocity_errors(p, g, seq, order, sub, div)
    assert np.array_equal(cnt, ocnt)
    assert np.all(err[cnt == 0].view(np.uint32) == 0)
    d = np.abs(err.astype(np.float64) - oerr)
    assert np.all(d <= bound), (p.shape, order, float((d - bound).max()))
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(bound > 0, d / bound, 0.0)))


def test_velocity_errors_within_the_derived_bounds(pkg):
    worst = 0.0
    for p, g, seq, order, sub, div in velocity_cases():
        worst = max(worst, check_velocity(host_velocity(pkg, p, g, seq, order, sub, div), p, g, seq, order, sub, div))
    print(f"worst |error| / bound: {worst:.3f}")


def test_velocity_counts_of_short_sequences(pkg):
    p, g = make_x(9, 17, 3, 1), make_x(9, 17, 3, 2)
    seq = np.array([3, 8, 8, 1, 1, 1, 2, 5, 5], np.int32)              # lengths 1, 2, 3, 1, 2
    _, c1 = host_velocity(pkg, p, g, seq, 1)
    _, c2 = host_velocity(pkg, p, g, seq, 2)
    assert c1.tolist() == [0, 0, 1, 0, 1, 1, 0, 0, 1] and c2.tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    e, c = host_velocity(pkg, p, p, None, 1)
    assert c.tolist() == [0] + [1] * 8 and not e.any()
    host_velocity(pkg, p, g, None, 3, expect=EINVAL)
    host_velocity(pkg, p, g, None, 1, sub=np.zeros((17, 3), F), expect=EINVAL)
    host_velocity(pkg, make_x(4, 33, 3, 0), make_x(4, 33, 3, 0), expect=ESHAPE)


# ---- the recorded track -------------------------------------------------------------------------------------------------------
def px_error(xy, gt):
    return np.linalg.norm(xy.astype(np.float64) - gt.astype(np.float64), axis=-1)


def test_fixture_figures_on_the_oracle(g15):
    det, gt = g15["det"], g15["gt2d"]
    assert det.shape == (256, 17, 3) and det.dtype == F and not det[216].any()
    raw = px_error(det[..., :2], gt)
    xy, w, st = orc.prepare(det, orc.H36M17, (1.0, 1.0), 0.1, 8, 0.5, None, dtype=np.float64)
    filled = px_error(xy, gt)
    interp = st == orc.INTERPOLATED
    taps = np.exp(-np.arange(-3, 4, dtype=np.float64) ** 2 / 2)
    filt, _ = orc.filter(xy.astype(F), (taps / taps.sum()).astype(F), w.astype(F), None)
    filtered = px_error(filt, gt)
    invalid = float((st != orc.VALID).mean())
    print(f"g15: invalid {100 * invalid:.1f} %, interpolated {int(interp.sum())}, held {int((st == orc.HELD).sum())}, "
          f"lost {int((st == orc.LOST).sum())}; interpolated joints raw {raw[interp].mean():.2f} px -> filled "
          f"{filled[interp].mean():.2f} px; all joints raw {raw.mean():.2f} px, filled {filled.mean():.2f} px, "
          f"filtered {filtered.mean():.2f} px")
    assert abs(invalid - 0.104) < 0.001 and int(interp.sum()) == 205
    assert filled.mean() < raw.mean()
    assert filled[interp].mean() < raw[interp].mean()
    assert filtered.mean() < filled.mean()
    assert abs(raw[interp].mean() - 55.4) < 0.1 and abs(filled[interp].mean() - 17.4) < 0.1 and abs(raw.mean() - 14.9) < 0.1


def test_fixture_host_results_sit_inside_the_bounds(pkg, g15):
    det = g15["det"]
    xy, w, st = check_prepare(pkg, det, orc.H36M17, (1.0, 1.0), 0.1, 8, 0.5, None)
    taps = pkg.TemporalFilter.gaussian(1.0).taps
    r = check_filter(host_filter(pkg, xy, taps, w), xy, taps, w, None)
    mb = g15["mb3d"]
    f3 = host_filter(pkg, mb, taps)
    r3 = check_filter(f3, mb, taps, None, None)
    for order in (1, 2):
        check_velocity(host_velocity(pkg, f3, mb, None, order), f3, mb, None, order, None, None)
    print(f"g15: filter error / bound 2-D {r:.3f}, 3-D {r3:.3f}")


def test_velocity_sign_on_the_recorded_track(g15):
    """Filtering a jittered track brings its velocity back towards the recorded track's: on the oracle alone."""
    mb = g15["mb3d"]
    taps = np.exp(-np.arange(-3, 4, dtype=np.float64) ** 2 / 2)
    taps = (taps / taps.sum()).astype(F)
    jit = (mb + np.random.RandomState(15).randn(*mb.shape).astype(F) * F(0.01)).astype(F)
    smooth, _ = orc.filter(mb, taps)
    jit_f, _ = orc.filter(jit, taps)

    def mpjve(a):
        e, c, _ = orc.velocity_errors(a, mb)
        return e.sum() / (c.sum() * 17)
    v_smooth, v_jit, v_jit_f = mpjve(smooth.astype(F)), mpjve(jit), mpjve(jit_f.astype(F))
    print(f"g15 MPJVE against mb3d: filtered mb3d {v_smooth:.5f}, jittered {v_jit:.5f}, jittered then filtered {v_jit_f:.5f}")
    assert np.isfinite(v_smooth) and v_smooth < v_jit_f < v_jit


def test_load_keypoints_json(pkg, g15, tmp_path):
    det = g15["det"][:5]
    for nested in (True, False):
        path = os.path.join(tmp_path, f"k{int(nested)}.json")
        with open(path, "w") as f:
            json.dump([{"image_id": f"{t:04d}.jpg", "category_id": 1, "score": 0.5,
                        "keypoints": det[t].tolist() if nested else det[t].reshape(-1).tolist()} for t in range(5)], f)
        back = pkg.load_keypoints_json(path)
        assert back.dtype == F and same_bits(back, det)
    with open(path, "w") as f:
        json.dump([{"keypoints": [0.0] * 50}], f)
    with pytest.raises(ValueError):
        pkg.load_keypoints_json(path)


def test_sequence_lifter_needs_a_device_and_eval_mode(pkg):
    import torch
    with pytest.raises(pkg.PoseliftError):
        pkg.prepare_tracks(torch.zeros(4, 17, 3))                       # no CPU path
    with pytest.raises(ValueError):
        pkg.SequenceLifter(None, layout="coco18")
    with pytest.raises(TypeError):
        pkg.SequenceLifter(None, filter_2d=[0.25, 0.5, 0.25])
