"""CPU tests of the pose augmentation: csrc/pose_augment.h through pl_pose_augment_host (the same inline text the kernel runs,
compiled for the CPU) against the fp64 restatement and the fp32 twin of pose_augment_oracle.py, and on structural properties.

Gate of the transcendental configurations: 8x the worst absolute error of the fp32 numpy twin against fp64 on the same
cases (computed and printed by the test, never typed in).  The factor covers sincosf / logf implementations that differ by a
few ulp and their amplification through Box-Muller."""
import ctypes

import numpy as np
import pytest

import pose_augment_oracle as orc
from oracle.philox import dropout_keep_mask, dropout_threshold, philox4x32_10

EINVAL, ESHAPE = -1, -2
GATE_FACTOR = 8.0
TABLE_ROWS, N_CASE = 1000, 67
ALL_ON = dict(p_flip=0.5, max_rot=np.pi, scale_range=0.25, max_shift=0.1, jitter_sigma=0.05, seed=0x123456789ABCDEF)
# p_flip = 0.5 over rows 0..4095 at epoch 0: this seed flips 2016 of 4096 (|k - 2048| = 32 <= 160 = 5 binomial sigmas)
FLIP_SEED = 7
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()


@pytest.fixture(scope="module")
def table(pkg):
    return make_table(pkg)


def make_table(pkg):
    """1000 synthetic poses (x2d in [0,1], y3d root-relative with a zero root row) and the 67 non-monotone rows of the cases."""
    x, y = pkg.synth.synthetic_batch(TABLE_ROWS, 4242)
    a = np.ascontiguousarray(x.numpy(), dtype=np.float32)
    b = np.ascontiguousarray(y.numpy(), dtype=np.float32)
    idx = np.random.RandomState(5).permutation(TABLE_ROWS)[:N_CASE].astype(np.int64)
    assert (np.diff(idx) < 0).any() and (np.diff(idx) > 0).any()
    a.setflags(write=False), b.setflags(write=False), idx.setflags(write=False)
    return a, b, idx


def aug_struct(pkg, cfg):
    return pkg._lib.PLPoseAug(cfg["p_flip"], cfg["flip_offset"], cfg["max_rot"], cfg["scale_range"], cfg["max_shift"],
                              cfg["jitter_sigma"], cfg["cx"], cfg["cy"], cfg["seed"])


def host_augment(pkg, a, b, src_idx, row_id, cfg, epoch=0, expect=0):
    """pl_pose_augment_host on numpy arrays: a (rows,17,2), b (rows,17,3); src_idx None = rows in order."""
    row_id = np.ascontiguousarray(row_id, dtype=np.uint64).view(np.int64)
    n = len(row_id)
    src = None if src_idx is None else np.ascontiguousarray(src_idx, dtype=np.int64)
    oa, ob = np.full((n, 17, 2), -7.0, np.float32), np.full((n, 17, 3), -7.0, np.float32)
    rc = pkg.lib().pl_pose_augment_host(a.ctypes.data, b.ctypes.data, None if src is None else src.ctypes.data,
                                        row_id.ctypes.data, n, a.shape[0], oa.ctypes.data, ob.ctypes.data,
                                        ctypes.byref(aug_struct(pkg, cfg)), int(epoch))
    assert rc == expect, pkg.lib().pl_last_error()
    return oa, ob


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same_bits(x, y):
    return np.array_equal(bits(x), bits(y))


def yardstick(cfg, epoch, rows, a, b):
    """(fp64 oracle outputs, worst absolute error of the fp32 twin against them)."""
    a64, b64, _ = orc.augment(cfg, epoch, rows, a, b, np.float64)
    a32, b32, _ = orc.augment(cfg, epoch, rows, a, b, np.float32)
    ea, eb = float(np.abs(a32.astype(np.float64) - a64).max()), float(np.abs(b32.astype(np.float64) - b64).max())
    return a64, b64, max(ea, eb), (ea, eb)


def check_against_fp64(oa, ob, cfg, epoch, rows, a, b, what):
    """The 8x-twin gate; prints both numbers.  Returns (error, gate)."""
    a64, b64, twin, (ta, tb) = yardstick(cfg, epoch, rows, a, b)
    ea, eb = float(np.abs(oa.astype(np.float64) - a64).max()), float(np.abs(ob.astype(np.float64) - b64).max())
    err, gate = max(ea, eb), GATE_FACTOR * twin
    print(f"{what}: worst |error| vs fp64 {err:.3e} (2-D {ea:.3e}, 3-D {eb:.3e}); fp32 twin {twin:.3e} "
          f"(2-D {ta:.3e}, 3-D {tb:.3e}); gate {gate:.3e}")
    assert twin > 0.0
    assert err <= gate
    return err, gate


def test_identity_copies_bits(pkg, table):
    a, b, idx = table
    cfg = orc.config()
    oa, ob = host_augment(pkg, a, b, idx, idx, cfg)
    assert same_bits(oa, a[idx]) and same_bits(ob, b[idx])
    oa, ob = host_augment(pkg, a, b, None, idx, cfg)
    assert same_bits(oa, a[:N_CASE]) and same_bits(ob, b[:N_CASE])


def test_flip_only(pkg, table):
    a, b, idx = table
    oa, ob = host_augment(pkg, a, b, idx, idx, orc.config(p_flip=1.0))
    assert same_bits(oa, orc.flip_pose(a[idx], np.float32(1))) and same_bits(ob, orc._neg_flip(b[idx]))
    oa0, ob0 = host_augment(pkg, a, b, idx, idx, orc.config(p_flip=1.0, flip_offset=0.0))
    assert same_bits(oa0, orc.flip_pose(a[idx], np.float32(0))) and same_bits(ob0, ob)
    assert np.array_equal(oa0[:, orc.SWAP, 0], -a[idx][:, :, 0]) and same_bits(oa0[:, orc.SWAP, 1], a[idx][:, :, 1])


def test_flip_half_matches_the_oracle_word_for_word(pkg, table):
    a, b, _ = table
    rows = np.arange(4096, dtype=np.int64)
    src = rows % TABLE_ROWS
    cfg = orc.config(p_flip=0.5, seed=FLIP_SEED)
    oa, ob = host_augment(pkg, a, b, src, rows, cfg)
    flipped = ~np.all(bits(oa) == bits(a[src]), axis=(1, 2))
    want = orc.decisions(cfg, 0, rows, np.float64)["flip"]
    assert np.array_equal(flipped, want)
    assert np.array_equal(flipped, ~np.all(bits(ob) == bits(b[src]), axis=(1, 2)))
    assert same_bits(oa, np.where(want[:, None, None], orc.flip_pose(a[src], np.float32(1)), a[src]))
    k = int(flipped.sum())
    print(f"p_flip 0.5, seed {FLIP_SEED}: {k} of 4096 rows flipped")
    assert abs(k - 2048) <= 160


def test_scale_and_shift_equal_the_fp32_twin_bit_for_bit(pkg, table):
    a, b, idx = table
    for kw in (dict(scale_range=0.25, max_shift=0.1), dict(scale_range=0.5), dict(max_shift=0.03, cx=0.25, cy=0.75),
               dict(scale_range=0.25, max_shift=0.1, p_flip=0.5)):
        cfg = orc.config(seed=99, **kw)
        oa, ob = host_augment(pkg, a, b, idx, idx, cfg, epoch=3)
        ta, tb, _ = orc.augment(cfg, 3, idx, a[idx], b[idx], np.float32)
        assert same_bits(oa, ta) and same_bits(ob, tb), kw
        assert not same_bits(oa, a[idx])
        if "p_flip" not in kw:
            assert same_bits(ob, b[idx])                 # weak perspective: the 3-D target is left alone


def test_rotation_and_jitter_against_fp64(pkg, table):
    a, b, idx = table
    cfg = orc.config(**ALL_ON)
    oa, ob = host_augment(pkg, a, b, idx, idx, cfg, epoch=1)
    check_against_fp64(oa, ob, cfg, 1, idx, a[idx], b[idx], "host, all stages on, n = 67 of 1000")
    for kw in (dict(max_rot=np.pi), dict(jitter_sigma=0.05)):
        c1 = orc.config(seed=3, **kw)
        o1a, o1b = host_augment(pkg, a, b, idx, idx, c1)
        check_against_fp64(o1a, o1b, c1, 0, idx, a[idx], b[idx], f"host, {kw}")


def test_structure(pkg, table):
    a, b, idx = table
    cfg = orc.config(**ALL_ON)
    oa, ob = host_augment(pkg, a, b, idx, idx, cfg, epoch=2)
    d = orc.decisions(cfg, 2, idx, np.float64)
    assert d["flip"].any() and not d["flip"].all()
    src = b[idx].astype(np.float64)
    src = np.where(d["flip"][:, None, None], src[:, orc.SWAP], src)      # the source joint of every output joint
    out = ob.astype(np.float64)
    # each rotated coordinate carries three fp32 roundings of values bounded by the pose's extent, and c^2 + s^2 = 1 to
    # 2^-23: lengths move by a few ulp of that extent
    tol = 16 * EPS32 * max(1.0, float(np.abs(b).max()))
    assert np.abs(np.linalg.norm(out, axis=2) - np.linalg.norm(src, axis=2)).max() <= tol
    par = np.array(orc.PARENT[1:])
    bone = lambda p: np.linalg.norm(p[:, 1:] - p[:, par], axis=2)
    assert np.abs(bone(out) - bone(src)).max() <= 2 * tol
    assert same_bits(ob[:, :, 2], np.where(d["flip"][:, None], b[idx][:, orc.SWAP, 2], b[idx][:, :, 2]))
    assert np.all(b[idx][:, 0] == 0) and np.all(ob[:, 0] == 0)
    # the noise of a pose does not depend on p_flip, max_rot or scale_range
    quiet = host_augment(pkg, a, b, idx, idx, orc.config(**dict(ALL_ON, jitter_sigma=0.0)), epoch=2)[0]
    other = dict(ALL_ON, p_flip=0.0, max_rot=0.3, scale_range=0.0)
    oa2 = host_augment(pkg, a, b, idx, idx, orc.config(**other), epoch=2)[0]
    quiet2 = host_augment(pkg, a, b, idx, idx, orc.config(**dict(other, jitter_sigma=0.0)), epoch=2)[0]
    n1, n2 = oa.astype(np.float64) - quiet, oa2.astype(np.float64) - quiet2
    # one rounding of the sum on each side, at |value| <= max |output|
    ntol = 2 * EPS32 * max(1.0, float(np.abs(oa).max()), float(np.abs(oa2).max()))
    assert np.abs(n1 - n2).max() <= ntol
    assert np.abs(n1 - d["noise"]).max() <= ntol + 8 * EPS32 * 0.05 * 6     # + the fp32 Box-Muller value itself (|z| < 6)
    assert 0.04 < n1.std() < 0.06


def test_stream_identity(pkg, table):
    a, b, idx = table
    cfg = orc.config(**ALL_ON)
    ref_a, ref_b = host_augment(pkg, a, b, idx, idx, cfg, epoch=5)
    # other n, other places in the batch, and the ungathered mode: the same (seed, epoch, row) -> the same pose
    order = np.random.RandomState(9).permutation(N_CASE)[:23]
    ga, gb = np.ascontiguousarray(a[idx[order]]), np.ascontiguousarray(b[idx[order]])
    oa, ob = host_augment(pkg, ga, gb, None, idx[order], cfg, epoch=5)
    assert same_bits(oa, ref_a[order]) and same_bits(ob, ref_b[order])
    oa, ob = host_augment(pkg, a, b, idx[order][:1], idx[order][:1], cfg, epoch=5)
    assert same_bits(oa, ref_a[order][:1]) and same_bits(ob, ref_b[order][:1])
    # seed, epoch, row: each changes the draws of the same source pose
    one_a, one_b = np.ascontiguousarray(a[:1]), np.ascontiguousarray(b[:1])
    base = host_augment(pkg, one_a, one_b, None, [17], cfg, epoch=5)[0]
    assert not same_bits(base, host_augment(pkg, one_a, one_b, None, [18], cfg, epoch=5)[0])
    assert not same_bits(base, host_augment(pkg, one_a, one_b, None, [17], cfg, epoch=6)[0])
    assert not same_bits(base, host_augment(pkg, one_a, one_b, None, [17], orc.config(**dict(ALL_ON, seed=1)), epoch=5)[0])
    assert not same_bits(base, host_augment(pkg, one_a, one_b, None, [17],
                                            orc.config(**dict(ALL_ON, seed=ALL_ON["seed"] ^ (1 << 40))), epoch=5)[0])
    # the high words of the epoch (key) and of the row (counter), held to the twin bit for bit on the exact stages
    exact = orc.config(scale_range=0.25, max_shift=0.1, p_flip=0.5, seed=ALL_ON["seed"])
    for epoch, rows in ((2 ** 32 + 3, idx), (3, idx), (0, idx.astype(np.uint64) + np.uint64(2 ** 32)), (0, idx),
                        (2 ** 63 + 5, idx.astype(np.uint64) + np.uint64(2 ** 63))):
        oa, ob = host_augment(pkg, ga[:1].repeat(N_CASE, 0), gb[:1].repeat(N_CASE, 0), None, rows, exact, epoch=epoch)
        ta, tb, _ = orc.augment(exact, epoch, rows, ga[:1].repeat(N_CASE, 0), gb[:1].repeat(N_CASE, 0), np.float32)
        assert same_bits(oa, ta) and same_bits(ob, tb), (epoch, rows[:2])
    hi = host_augment(pkg, one_a, one_b, None, [2 ** 32 + 17], exact)[0]
    lo = host_augment(pkg, one_a, one_b, None, [17], exact)[0]
    assert not same_bits(hi, lo)
    assert not same_bits(host_augment(pkg, one_a, one_b, None, [17], exact, epoch=2 ** 32 + 3)[0],
                         host_augment(pkg, one_a, one_b, None, [17], exact, epoch=3)[0])


def test_no_draw_collides_with_the_dropout_stream(pkg, table):
    a, b, _ = table
    seed, step, rows = 0xDEADBEEF12345678, 11, np.arange(1024, dtype=np.uint64)
    thr = np.uint32(dropout_threshold(0.5))
    agree = []
    for c2 in range(11):
        ours = np.stack(orc.words(seed, step, rows, c2), axis=1)
        # the dropout stream of hidden layer c2 with 4 columns: element group g = row
        theirs = np.stack(philox4x32_10(rows & np.uint64(0xFFFFFFFF), rows >> np.uint64(32), c2, step, seed & 0xFFFFFFFF,
                                        (seed >> 32) ^ (step >> 32)), axis=1)
        keep = dropout_keep_mask(seed, step, c2, 1024, 4, 0.5)
        assert np.array_equal(keep, theirs >= thr)                  # `theirs` IS the dropout stream's words
        assert not (ours == theirs).all(axis=1).any()
        assert (ours == theirs).sum() <= 2                          # 4096 word pairs, each equal with probability 2^-32
        agree.append(((ours >= thr) == keep).mean())
    assert abs(np.mean(agree) - 0.5) <= 5 * 0.5 / np.sqrt(11 * 4096)
    # and the library's flip bits are the tagged stream's, not the dropout stream's
    cfg = orc.config(p_flip=0.5, seed=seed)
    src = rows.astype(np.int64) % TABLE_ROWS
    oa, _ = host_augment(pkg, a, b, src, rows, cfg, epoch=step)
    flipped = ~np.all(bits(oa) == bits(a[src]), axis=(1, 2))
    assert np.array_equal(flipped, orc.words(seed, step, rows, 0)[0] < thr)
    assert not np.array_equal(flipped, ~dropout_keep_mask(seed, step, 0, 1024, 4, 0.5)[:, 0])


def test_errors(pkg, table):
    a, b, idx = table
    L = pkg.lib()
    n = len(idx)
    oa, ob = np.zeros((n, 17, 2), np.float32), np.zeros((n, 17, 3), np.float32)
    A, B, I, OA, OB = a.ctypes.data, b.ctypes.data, idx.ctypes.data, oa.ctypes.data, ob.ctypes.data

    def call(a_=A, b_=B, src=I, rid=I, n_=n, rows=TABLE_ROWS, oa_=OA, ob_=OB, cfg=None, null_aug=False):
        s = aug_struct(pkg, cfg or orc.config())
        return L.pl_pose_augment_host(a_, b_, src, rid, n_, rows, oa_, ob_, None if null_aug else ctypes.byref(s), 0)

    assert call() == 0
    for kw in (dict(a_=None), dict(b_=None), dict(rid=None), dict(oa_=None), dict(ob_=None), dict(null_aug=True)):
        assert call(**kw) == EINVAL and b"null" in L.pl_last_error(), kw
    for kw in (dict(oa_=A), dict(ob_=B), dict(oa_=OB), dict(ob_=A + 4 * 34 * 10), dict(ob_=OA)):
        assert call(**kw) == EINVAL and b"aliased" in L.pl_last_error(), kw
    for kw in (dict(n_=0), dict(n_=-3), dict(rows=0), dict(src=None, rows=n - 1)):
        assert call(**kw) == ESHAPE and b"pl_pose_augment_host" in L.pl_last_error(), kw
    bad_idx = idx.copy()
    bad_idx[5] = TABLE_ROWS
    assert call(src=bad_idx.ctypes.data) == EINVAL and b"outside the table" in L.pl_last_error()
    raw = lambda **kw: dict(orc.config(), **kw)                      # past config()'s own rounding: NaN, negatives
    for kw, text in ((dict(scale_range=1.0), b"scale_range"), (dict(scale_range=1.5), b"scale_range"),
                     (dict(jitter_sigma=-0.05), b"jitter_sigma"), (dict(max_rot=float("nan")), b"max_rot"),
                     (dict(p_flip=-0.1), b"p_flip"), (dict(max_shift=float("inf")), b"max_shift"),
                     (dict(cx=float("nan")), b"cx"), (dict(flip_offset=float("-inf")), b"flip_offset")):
        assert call(cfg=raw(**kw)) == EINVAL and text in L.pl_last_error(), kw
    # the device entry point runs the same checks before it touches a device
    s = aug_struct(pkg, raw(scale_range=1.0))
    assert L.pl_pose_augment_gather(A, B, I, I, n, TABLE_ROWS, OA, OB, ctypes.byref(s), 0, None) == EINVAL
    assert L.pl_pose_augment_gather(A, B, I, I, n, TABLE_ROWS, OA, OA, ctypes.byref(aug_struct(pkg, orc.config())), 0, None) == EINVAL
    assert L.pl_pose_augment_gather(A, B, I, None, n, TABLE_ROWS, OA, OB, ctypes.byref(aug_struct(pkg, orc.config())), 0, None) == EINVAL
    assert L.pl_pose_augment_gather(A, B, I, I, 0, TABLE_ROWS, OA, OB, ctypes.byref(aug_struct(pkg, orc.config())), 0, None) == ESHAPE


def test_pose_augment_value_object(pkg):
    aug = pkg.PoseAugment(p_flip=0.5, max_rot=0.2, centre=(0.25, 0.75), seed=2 ** 63 + 1)
    s = aug.struct()
    assert (s.p_flip, s.flip_offset, s.cx, s.cy, s.seed) == (0.5, 1.0, 0.25, 0.75, 2 ** 63 + 1)
    assert abs(s.max_rot - 0.2) < 1e-7 and s.scale_range == s.max_shift == s.jitter_sigma == 0.0
    assert aug == pkg.PoseAugment(p_flip=0.5, max_rot=0.2, centre=[0.25, 0.75], seed=2 ** 63 + 1) and hash(aug) is not None
    with pytest.raises(Exception):
        aug.p_flip = 0.1                                             # frozen
    for kw in (dict(scale_range=1.0), dict(jitter_sigma=-1.0), dict(max_rot=float("nan")), dict(p_flip=-0.5),
               dict(centre=(0.5,)), dict(seed=-1), dict(seed=2 ** 64), dict(flip_offset=float("inf"))):
        with pytest.raises(ValueError):
            pkg.PoseAugment(**kw)
    assert ctypes.sizeof(pkg._lib.PLPoseAug) == 40
