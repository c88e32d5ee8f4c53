"""CPU tests of the pose-table definitions: csrc/pose_table.h through the _host entry points (the same inline text the
kernels run, compiled for the CPU) against the numpy restatement of pose_table_oracle.py.

Everything is exact except the statistics' mean and std, whose bounds are the textbook ones of an fp64 sum of N terms in
any order: |d mean| <= N 2^-52 max|x|, |d std| <= N 2^-52 max|x - mean| + 2^-52 std."""
import ctypes
import os

import numpy as np
import pytest

import pose_augment_oracle as aorc
import pose_table_oracle as orc
from test_pose_augment_host import ALL_ON, N_CASE, aug_struct, host_augment, make_table, same_bits

EINVAL, ESHAPE = -1, -2
U = 2.0 ** -52
H36M_17 = (0, 1, 2, 3, 6, 7, 8, 12, 13, 14, 15, 17, 18, 19, 25, 26, 27)
# the configurations of test_gpu_pose_augment.py (copied)
EXACT = [dict(), dict(p_flip=1.0), dict(p_flip=0.5, seed=7), dict(p_flip=1.0, flip_offset=0.0),
         dict(scale_range=0.25, max_shift=0.1, seed=99), dict(scale_range=0.5, p_flip=0.5, cx=0.25, cy=0.75, seed=5),
         dict(max_shift=0.03, seed=2 ** 63 + 9)]
TRANSCENDENTAL = [ALL_ON, dict(max_rot=np.pi, seed=3), dict(jitter_sigma=0.05, seed=3),
                  dict(p_flip=0.5, max_rot=0.3, jitter_sigma=0.01, flip_offset=0.0, cx=0.0, cy=0.0, seed=8)]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()


@pytest.fixture(scope="module")
def table(pkg):
    return make_table(pkg)


def bits64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---- shared makers (the GPU tests import these) ---------------------------------------------------------------------------
def make_cameras(seed=3):
    """4 random unit quaternions and one non-unit one, translations of a few metres: (5, 7) float64."""
    rs = np.random.RandomState(seed)
    q = rs.randn(5, 4)
    q[:4] /= np.linalg.norm(q[:4], axis=1, keepdims=True)
    q[4] *= 1.7
    return np.ascontiguousarray(np.concatenate([rs.uniform(-5, 5, (5, 3)), q], axis=1))


def make_raw(n, jsrc, d, seed=0):
    rs = np.random.RandomState(seed + 31 * n + jsrc)
    return np.ascontiguousarray((rs.randn(n, jsrc, d) * 0.6 + rs.uniform(-2, 2, (1, 1, d))).astype(np.float32))


def host_prepare(pkg, raw, joints=None, cams=None, cam_id=None, zero_centre=False, expect=0, J=None):
    n, jsrc, d = raw.shape
    J = (len(joints) if joints is not None else jsrc) if J is None else J
    pick = None if joints is None else (ctypes.c_int32 * len(joints))(*joints)
    ids = None if cam_id is None else np.ascontiguousarray(cam_id, np.int32)
    out = np.full((n, J, d), -7.0, np.float32)
    rc = pkg.lib().pl_pose_prepare_host(raw.ctypes.data, n, jsrc, d, pick, J, None if ids is None else ids.ctypes.data,
                                        None if cams is None else cams.ctypes.data, 0 if cams is None else len(cams),
                                        int(zero_centre), out.ctypes.data)
    assert rc == expect, pkg.lib().pl_last_error()
    return out


PREPARE_SHAPES = [(32, H36M_17), (1, None), (32, None), (40, tuple(range(39, 7, -1)))]   # (Jsrc, joints): J = 17, 1, 32, 32


def prepare_cases(n):
    """(raw, joints, cams, cam_id, zero_centre) over the shapes, D in {2, 3}, every stage on and off."""
    cams = make_cameras()
    out = []
    for jsrc, joints in PREPARE_SHAPES:
        for d in (2, 3):
            raw = make_raw(n, jsrc, d)
            cid = (np.arange(n) * 7 % 5).astype(np.int32)
            for use_cam in ((False, True) if d == 3 else (False,)):
                for zc in (False, True):
                    out.append((raw, joints, cams if use_cam else None, cid if use_cam else None, zc))
    return out


def stat_sizes(pkg):
    R = pkg.lib().pl_pose_stats_chunk_rows()
    return [1, 2, R - 1, R, R + 1, 2 * R + 1, 100003]


STAT_WIDTHS = (2, 34, 51, 96)


def make_columns(n, w, seed=0):
    """Columns with offsets up to 1000 and spreads from 1e-3 to 50: pixel coordinates next to root-relative metres."""
    rs = np.random.RandomState(seed + 13 * w + n % 9973)
    off = rs.uniform(-1000, 1000, w)
    spread = 10.0 ** rs.uniform(-3, np.log10(50), w)
    off[0], spread[0] = 1000.0, 1e-3
    off[-1], spread[-1] = 0.0, 50.0
    return np.ascontiguousarray((rs.randn(n, w) * spread + off).astype(np.float32))


def host_stats(pkg, x, expect=0):
    n, w = x.shape
    out = np.full((4, w), -7.0, np.float64)
    assert pkg.lib().pl_pose_stats_host(x.ctypes.data, n, w, out.ctypes.data) == expect, pkg.lib().pl_last_error()
    return out


def host_affine(pkg, x, sub, div, invert, inplace=False):
    x = np.ascontiguousarray(x, np.float32)
    sub, div = np.ascontiguousarray(sub, np.float32).reshape(-1), np.ascontiguousarray(div, np.float32).reshape(-1)
    w = sub.size
    y = x.copy() if inplace else np.full(x.shape, -7.0, np.float32)
    src = y if inplace else x
    rc = pkg.lib().pl_pose_affine_host(src.ctypes.data, x.size // w, w, sub.ctypes.data, div.ctypes.data, int(invert),
                                       y.ctypes.data)
    assert rc == 0, pkg.lib().pl_last_error()
    return y


def make_transforms(seed=1):
    """Left/right ASYMMETRIC (sub, div) pairs over (17, 2) and (17, 3); the 3-D root column has div = 0."""
    rs = np.random.RandomState(seed)
    s2, d2 = rs.uniform(0.2, 0.8, (17, 2)).astype(np.float32), rs.uniform(0.05, 0.4, (17, 2)).astype(np.float32)
    s3, d3 = rs.uniform(-0.3, 0.3, (17, 3)).astype(np.float32), rs.uniform(0.05, 0.6, (17, 3)).astype(np.float32)
    s3[0], d3[0] = 0.0, 0.0
    return (s2, d2), (s3, d3)


def host_augment_t(pkg, a, b, src_idx, row_id, cfg, t2, t3, epoch=0):
    row_id = np.ascontiguousarray(row_id, dtype=np.uint64).view(np.int64)
    n = len(row_id)
    src = None if src_idx is None else np.ascontiguousarray(src_idx, dtype=np.int64)
    oa, ob = np.full((n, 17, 2), -7.0, np.float32), np.full((n, 17, 3), -7.0, np.float32)
    p = lambda t, k: None if t is None else t[k].ctypes.data
    rc = pkg.lib().pl_pose_augment_host_t(a.ctypes.data, b.ctypes.data, None if src is None else src.ctypes.data,
                                          row_id.ctypes.data, n, a.shape[0], oa.ctypes.data, ob.ctypes.data,
                                          ctypes.byref(aug_struct(pkg, cfg)), int(epoch), p(t2, 0), p(t2, 1), p(t3, 0), p(t3, 1))
    assert rc == 0, pkg.lib().pl_last_error()
    return oa, ob


# ---- prepare --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 67])
def test_prepare(pkg, n):
    for raw, joints, cams, cid, zc in prepare_cases(n):
        got = host_prepare(pkg, raw, joints, cams, cid, zc)
        want = orc.prepare(raw, joints, cams, cid, zc)
        assert same_bits(got, want), (raw.shape, joints, cams is not None, zc)
        if cams is None and not zc:                                   # the pick alone is a bit copy
            assert same_bits(got, raw if joints is None else raw[:, list(joints)])
        if zc:
            assert np.all(got[:, 0].view(np.uint32) == 0)             # +0, not -0
        if cams is None and zc:                                       # root-centring is numpy float32
            p = raw if joints is None else raw[:, list(joints)]
            assert same_bits(got[:, 1:], p[:, 1:] - p[:, :1])


def test_prepare_camera_view_is_a_rotation_for_unit_quaternions(pkg):
    cams = make_cameras()
    raw = make_raw(67, 17, 3)
    for c in range(4):
        cid = np.full(67, c, np.int32)
        got = host_prepare(pkg, raw, None, cams, cid).astype(np.float64)
        d_in = np.linalg.norm((raw[:, 1:] - raw[:, :1]).astype(np.float64), axis=-1)
        d_out = np.linalg.norm(got[:, 1:] - got[:, :1], axis=-1)
        assert np.allclose(d_in, d_out, rtol=0, atol=1e-5)             # bone lengths survive; fp32 inputs of size ~10
    got = host_prepare(pkg, raw, None, cams, np.full(67, 4, np.int32)).astype(np.float64)
    d_out = np.linalg.norm(got[:, 1:] - got[:, :1], axis=-1)
    assert np.allclose(d_out, d_in * (cams[4, 3:] ** 2).sum(), rtol=1e-5)      # the non-unit quaternion scales by |q|^2


def test_prepare_bad_camera_ids_and_arguments(pkg):
    cams = make_cameras()
    raw = make_raw(67, 32, 3)
    cid = (np.arange(67) % 5).astype(np.int32)
    good = host_prepare(pkg, raw, H36M_17, cams, cid, True)
    cid2 = cid.copy()
    cid2[[5, 40]] = [-1, len(cams)]
    got = host_prepare(pkg, raw, H36M_17, cams, cid2, True)
    bad = np.zeros(67, bool)
    bad[[5, 40]] = True
    assert np.isnan(got[bad]).all() and same_bits(got[~bad], good[~bad])
    assert same_bits(got, orc.prepare(raw, H36M_17, cams, cid2, True))
    host_prepare(pkg, raw, (0, 1, 32), expect=ESHAPE)                                    # pick index == Jsrc
    host_prepare(pkg, raw, (0, -1), expect=ESHAPE)
    host_prepare(pkg, make_raw(4, 32, 2), H36M_17, cams, np.zeros(4, np.int32), expect=ESHAPE)   # D = 2 with cameras
    host_prepare(pkg, raw, None, J=17, expect=ESHAPE)                                    # no list, J != Jsrc
    host_prepare(pkg, make_raw(2, 65, 3), expect=ESHAPE)
    host_prepare(pkg, raw, None, cams, None, expect=EINVAL)                              # cameras without cam_id


# ---- statistics -----------------------------------------------------------------------------------------------------------
def check_stats(got, x):
    """The derived bounds against the oracle; prints the worst ratios."""
    n = x.shape[0]
    want = orc.stats(x)
    x64 = x.astype(np.float64)
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    b_mean = n * U * np.abs(x64).max(axis=0)
    b_std = n * U * np.abs(x64 - want[0]).max(axis=0) + U * want[1]
    e_mean, e_std = np.abs(got[0] - want[0]), np.abs(got[1] - want[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        r_mean, r_std = np.nanmax(np.where(b_mean > 0, e_mean / b_mean, 0)), np.nanmax(np.where(b_std > 0, e_std / b_std, 0))
    print(f"N = {n}, W = {x.shape[1]}: worst |d mean| / bound {r_mean:.2e}, worst |d std| / bound {r_std:.2e}")
    assert np.all(e_mean <= b_mean) and np.all(e_std <= b_std)


def test_stats_against_the_oracle(pkg):
    for n in stat_sizes(pkg):
        for w in STAT_WIDTHS:
            x = make_columns(n, w)
            got = host_stats(pkg, x)
            check_stats(got, x)
            assert np.array_equal(bits64(got), bits64(host_stats(pkg, x)))          # two calls, the same bits
            if n == 1:
                assert np.array_equal(got[0], x[0].astype(np.float64)) and np.all(bits64(got[1]) == 0)


def test_stats_catch_an_fp32_accumulator(pkg):
    """The yardstick is worth something: a float32 running sum misses the mean bound by orders of magnitude."""
    x = make_columns(100003, 34)
    want = orc.stats(x)
    bad = np.cumsum(x, axis=0, dtype=np.float32)[-1].astype(np.float64) / x.shape[0]
    bound = x.shape[0] * U * np.abs(x.astype(np.float64)).max(axis=0)
    assert (np.abs(bad - want[0]) > 1e3 * bound).any()


def test_stats_nan_inf_and_constant_columns(pkg):
    R = pkg.lib().pl_pose_stats_chunk_rows()
    for n in (2, R + 1, 2 * R + 1):
        x = make_columns(n, 51)
        clean = host_stats(pkg, x)
        y = x.copy()
        y[n - 1, 3] = np.nan                     # a NaN in the last (short) chunk
        y[0, 7] = np.nan
        y[n // 2, 11] = np.inf
        y[:, 20] = np.float32(0.1)               # a constant that no fp64 sum reproduces exactly
        y[:, 0] = 0.0                            # the zeroed root
        got = host_stats(pkg, y)
        assert np.isnan(got[:, 3]).all() and np.isnan(got[:, 7]).all()
        assert got[0, 11] == np.inf and got[3, 11] == np.inf and np.isnan(got[1, 11]) and np.isfinite(got[2, 11])
        assert got[0, 20] == float(np.float32(0.1)) and got[1, 20] == 0 and got[2, 20] == got[3, 20] == got[0, 20]
        assert np.all(bits64(got[:, 0]) == 0)
        rest = [c for c in range(51) if c not in (0, 3, 7, 11, 20)]
        assert np.array_equal(bits64(got[:, rest]), bits64(clean[:, rest]))          # no other column is touched
        with np.errstate(invalid="ignore"):
            want = orc.stats(y)
        assert np.array_equal(np.isnan(got), np.isnan(want))
    assert pkg.lib().pl_pose_stats_host(x.ctypes.data, 4, 97, got.ctypes.data) == ESHAPE


# ---- transform ------------------------------------------------------------------------------------------------------------
def test_affine(pkg):
    rs = np.random.RandomState(2)
    for n, (j, d) in ((1, (17, 3)), (67, (17, 2)), (67, (32, 3)), (5, (1, 2))):
        x = (rs.randn(n, j, d) * 3 + 1).astype(np.float32)
        sub, div = rs.randn(j, d).astype(np.float32), rs.uniform(-2, 2, (j, d)).astype(np.float32)
        div[0, 0] = 0.0
        x[0, -1, -1] = np.nan
        if n > 1:
            x[1, 0, 0] = np.inf
        y = host_affine(pkg, x, sub, div, False)
        assert same_bits(y, orc.apply(x, sub, div))
        assert np.all(y[:, 0, 0].view(np.uint32) == 0)                               # div == 0 applies to +0, NaN / inf included
        back = host_affine(pkg, y, sub, div, True)
        assert same_bits(back, orc.invert(y, sub, div))
        assert same_bits(back[:, 0, 0], np.full(n, sub[0, 0]))                       # ... and inverts to sub
        assert same_bits(host_affine(pkg, x, sub, div, False, inplace=True), y)
        assert same_bits(host_affine(pkg, y, sub, div, True, inplace=True), back)
        ok = np.isfinite(x) & (np.broadcast_to(div, x.shape) != 0)
        assert np.allclose(back[ok], x[ok], rtol=1e-5, atol=1e-5)


def test_normalize_constructors(pkg):
    x = np.random.RandomState(4).uniform(0, 1, (67, 17, 2)).astype(np.float32)
    x[0, 0], x[1, 0] = (0.0, 1.0), (2.0 ** -30, 1 - 2.0 ** -24)
    t = pkg.PoseTransform.normalize_2d()
    assert same_bits(host_affine(pkg, x, t.sub.numpy(), t.div.numpy(), False), np.float32(2) * x - np.float32(1))
    z = np.random.RandomState(5).uniform(-1, 1, (67, 17, 3)).astype(np.float32)
    t3 = pkg.PoseTransform.normalize_3d()
    y = host_affine(pkg, z, t3.sub.numpy(), t3.div.numpy(), False)
    assert np.allclose(y, (z + 1) / 2 - 0.5, rtol=0, atol=2e-7) and np.abs(y).max() <= 0.5
    t3 = pkg.PoseTransform.normalize_3d(lo=-2.0, hi=6.0)
    assert np.allclose(host_affine(pkg, z, t3.sub.numpy(), t3.div.numpy(), False), (z + 2) / 8 - 0.5, rtol=0, atol=2e-7)
    with pytest.raises(ValueError):
        pkg.PoseTransform(np.zeros((17, 3)), np.zeros((17, 2)))
    with pytest.raises(ValueError):
        pkg.PoseTransform(np.full((17, 3), np.nan), np.ones((17, 3)))
    with pytest.raises(ValueError):
        pkg.PoseTransform(np.zeros((17, 3)), np.full((17, 3), 1e300))               # inf in fp32


# ---- the transform inside the augmented gather -----------------------------------------------------------------------------
def test_augment_host_t_is_the_transform_of_the_augmentation(pkg, table):
    a, b, idx = table
    t2, t3 = make_transforms()
    for kw in EXACT + TRANSCENDENTAL:
        cfg = aorc.config(**kw)
        for epoch in (0, 2 ** 32 + 3):
            pa, pb = host_augment(pkg, a, b, idx, idx, cfg, epoch=epoch)
            oa, ob = host_augment_t(pkg, a, b, idx, idx, cfg, t2, t3, epoch=epoch)
            assert same_bits(oa, orc.apply(pa, *t2)) and same_bits(ob, orc.apply(pb, *t3)), (kw, epoch)
            assert np.all(ob[:, 0].view(np.uint32) == 0)
    cfg = aorc.config(**ALL_ON)
    pa, pb = host_augment(pkg, a, b, idx, idx, cfg, epoch=1)
    na, nb = host_augment_t(pkg, a, b, idx, idx, cfg, None, None, epoch=1)            # both NULL: pl_pose_augment_host
    assert same_bits(na, pa) and same_bits(nb, pb)
    oa, ob = host_augment_t(pkg, a, b, idx, idx, cfg, t2, None, epoch=1)              # one of the two
    assert same_bits(oa, orc.apply(pa, *t2)) and same_bits(ob, pb)
    oa, ob = host_augment_t(pkg, a, b, idx, idx, cfg, None, t3, epoch=1)
    assert same_bits(oa, pa) and same_bits(ob, orc.apply(pb, *t3))
    rc = pkg.lib().pl_pose_augment_host_t(a.ctypes.data, b.ctypes.data, None, idx.ctypes.data, N_CASE, a.shape[0],
                                          oa.ctypes.data, ob.ctypes.data, ctypes.byref(aug_struct(pkg, cfg)), 0,
                                          t2[0].ctypes.data, None, None, None)
    assert rc == EINVAL                                                                # a transform is a pair


def test_transform_after_augment_is_not_augment_after_transform(pkg, table):
    """The motivating case: with left/right asymmetric statistics a flip of standardised poses is no mirror image."""
    a, b, idx = table
    t2, t3 = make_transforms()
    cfg = aorc.config(p_flip=1.0)
    oa, ob = host_augment_t(pkg, a, b, idx, idx, cfg, t2, t3)
    assert same_bits(oa, orc.apply(aorc.flip_pose(a[idx], np.float32(1)), *t2))      # T(flip_pose(raw))
    assert same_bits(ob, orc.apply(aorc._neg_flip(b[idx]), *t3))
    # the advice this replaces: standardise the table, then flip about 0
    sa, sb = orc.apply(a, *t2), orc.apply(b, *t3)
    wa, wb = host_augment(pkg, sa, sb, idx, idx, aorc.config(p_flip=1.0, flip_offset=0.0))
    assert np.abs(wa - oa).max() > 0.1 and np.abs(wb - ob).max() > 0.1


# ---- PoseStats ------------------------------------------------------------------------------------------------------------
def test_pose_stats_files(pkg, tmp_path):
    import torch
    x = make_columns(500, 51).reshape(500, 17, 3)
    rec = host_stats(pkg, x.reshape(500, 51)).reshape(4, 17, 3)
    st = pkg.PoseStats(*rec)
    path = os.path.join(tmp_path, "stats3d.npz")
    st.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["max_train_3d", "mean_train_3d", "min_train_3d", "std_train_3d"]
    back = pkg.PoseStats.load(path)
    for u, v in zip((st.mean, st.std, st.min, st.max), (back.mean, back.std, back.min, back.max)):
        assert u.dtype == torch.float64 and tuple(u.shape) == (17, 3) and np.array_equal(bits64(u.numpy()), bits64(v.numpy()))
    packaged = os.path.join(os.path.dirname(pkg.__file__), "data", "h36m_stats.npz")
    with np.load(packaged) as z:
        for dim in (2, 3):
            s = pkg.PoseStats.from_npz(packaged, dim)
            assert tuple(s.mean.shape) == (17, dim)
            assert np.array_equal(s.mean.numpy(), z[f"mean_train_{dim}d"].astype(np.float64))
            assert np.array_equal(s.std.numpy(), z[f"std_train_{dim}d"].astype(np.float64))
            t = pkg.PoseTransform.standardize(s)
            assert t.shape == (17, dim) and np.array_equal(t.div.numpy(), z[f"std_train_{dim}d"].astype(np.float32))
    with pytest.raises(ValueError):
        pkg.PoseStats.load(packaged)                                   # holds both dimensions: say which
    with pytest.raises(ValueError):
        pkg.PoseStats(rec[0], rec[1], rec[2], rec[3][:5])
