"""Restatement of the pose-augmentation definition (csrc/pose_augment.h, include/poselift.h PLPoseAug) in numpy, written from
the definition and built on oracle.philox.philox4x32_10: in fp64 (the oracle) and, same formulas, in fp32 (the twin, whose
own error against fp64 is the yardstick for the code under test).  Shared by test_pose_augment_host.py and
test_gpu_pose_augment.py.

Definition.  A pose is a (17,2) 2-D and a (17,3) 3-D array.  Per pose, from (seed, epoch, row):
  key     = (seed & M, (seed >> 32) ^ (epoch >> 32) ^ 0x41554721),  counter = (row & M, row >> 32, c2, epoch & M)
  f(w) = (w >> 8) 2^-24,  g(w) = ((w >> 8) + 1) 2^-24
  c2 = 0: flip iff w0 < thr(p_flip) (>= 1: always, <= 0: never); theta = (2 f(w1) - 1) max_rot; s = 1 + (2 f(w2) - 1) scale_range
  c2 = 1: tx = (2 f(w0) - 1) max_shift, ty = (2 f(w1) - 1) max_shift
  c2 = 2 + (k >> 2), k = joint * 2 + coord: word pairs (v0, v1), (v2, v3) -> Box-Muller r = sqrt(-2 log g(v_even)),
          phi = 2 pi f(v_odd), z_even = r cos phi, z_odd = r sin phi; noise_k = jitter_sigma z_(k & 3)
  2-D: flip_pose (x -> flip_offset - x, joints [4,5,6,11,12,13] <-> [1,2,3,14,15,16]), rotate about (cx, cy) by
       [[c, -s], [s, c]], scale about (cx, cy), translate, add noise.   3-D: flip_pose (x -> -x), rotate (x, y); z stays.
  A stage whose parameter is 0 is skipped.
"""
import numpy as np

from oracle.philox import dropout_threshold, philox4x32_10

M32 = 0xFFFFFFFF
TAG = 0x41554721
LEFT, RIGHT = [4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]
# Human3.6M 17-joint skeleton (parent of each joint); the flip maps bones to bones
PARENT = [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15]
SWAP = list(range(17))
for _l, _r in zip(LEFT, RIGHT):
    SWAP[_l], SWAP[_r] = _r, _l

DEFAULTS = dict(p_flip=0.0, flip_offset=1.0, max_rot=0.0, scale_range=0.0, max_shift=0.0, jitter_sigma=0.0, cx=0.5, cy=0.5,
                seed=0)


def config(**kw):
    """A full parameter dict; the float parameters are rounded to fp32, which is what the library is handed."""
    c = dict(DEFAULTS)
    assert set(kw) <= set(c), kw
    c.update(kw)
    return {k: (int(v) if k == "seed" else float(np.float32(v))) for k, v in c.items()}


def words(seed, epoch, rows, c2):
    """The four uint32 words of call c2 for every row (uint64 array)."""
    rows = np.asarray(rows, dtype=np.uint64)
    seed, epoch = int(seed) & (2 ** 64 - 1), int(epoch) & (2 ** 64 - 1)
    k1 = ((seed >> 32) ^ (epoch >> 32) ^ TAG) & M32
    return philox4x32_10(rows & np.uint64(M32), rows >> np.uint64(32), c2, epoch & M32, seed & M32, k1)


def flip_pose(p, offset):
    """flip_pose of the reference (utils.py:372-396) on (n,17,D): x -> offset - x, then the left/right swap."""
    q = p.copy()
    q[:, :, 0] = offset - q[:, :, 0]
    out = q.copy()
    out[:, LEFT], out[:, RIGHT] = q[:, RIGHT], q[:, LEFT]
    return out


def decisions(cfg, epoch, rows, dtype):
    """flip (bool), theta, s, tx, ty (n,) and noise (n,17,2) of the rows, arithmetic in dtype."""
    T = dtype
    n = len(rows)
    f = lambda w: (w >> np.uint32(8)).astype(T) * T(2.0 ** -24)
    g = lambda w: ((w >> np.uint32(8)).astype(np.uint64) + np.uint64(1)).astype(T) * T(2.0 ** -24)
    sym = lambda w: T(2) * f(w) - T(1)
    w0 = words(cfg["seed"], epoch, rows, 0)
    if cfg["p_flip"] >= 1.0:
        flip = np.ones(n, bool)
    elif cfg["p_flip"] <= 0.0:
        flip = np.zeros(n, bool)
    else:
        flip = w0[0] < np.uint32(dropout_threshold(cfg["p_flip"]))
    theta = sym(w0[1]) * T(cfg["max_rot"])
    s = T(1) + sym(w0[2]) * T(cfg["scale_range"])
    w1 = words(cfg["seed"], epoch, rows, 1)
    tx, ty = sym(w1[0]) * T(cfg["max_shift"]), sym(w1[1]) * T(cfg["max_shift"])
    two_pi = T(2) * T(np.pi)
    z = np.zeros((n, 9, 4), T)
    for q in range(9):
        v = words(cfg["seed"], epoch, rows, 2 + q)
        for h in (0, 1):
            r = np.sqrt(T(-2) * np.log(g(v[2 * h])))
            phi = two_pi * f(v[2 * h + 1])
            z[:, q, 2 * h], z[:, q, 2 * h + 1] = r * np.cos(phi), r * np.sin(phi)
    noise = (T(cfg["jitter_sigma"]) * z).reshape(n, 36)[:, :34].reshape(n, 17, 2)
    return dict(flip=flip, theta=theta, s=s, tx=tx, ty=ty, noise=noise)


def augment(cfg, epoch, rows, a, b, dtype=np.float64):
    """a (n,17,2), b (n,17,3): the SOURCE poses of the rows (already gathered) -> (oa, ob, decisions) in dtype."""
    T = dtype
    rows = np.asarray(rows, dtype=np.uint64)
    A, B = np.asarray(a).astype(T).reshape(-1, 17, 2), np.asarray(b).astype(T).reshape(-1, 17, 3)
    d = decisions(cfg, epoch, rows, T)
    cx, cy = T(cfg["cx"]), T(cfg["cy"])
    if cfg["p_flip"] > 0.0:
        fl = d["flip"][:, None, None]
        A = np.where(fl, flip_pose(A, T(cfg["flip_offset"])), A)
        B = np.where(fl, _neg_flip(B), B)
    if cfg["max_rot"] != 0.0:
        c, s = np.cos(d["theta"])[:, None], np.sin(d["theta"])[:, None]
        dx, dy = A[:, :, 0] - cx, A[:, :, 1] - cy
        A = np.stack([(c * dx - s * dy) + cx, (s * dx + c * dy) + cy], axis=2)
        x, y = B[:, :, 0], B[:, :, 1]
        B = np.stack([c * x - s * y, s * x + c * y, B[:, :, 2]], axis=2)
    if cfg["scale_range"] != 0.0:
        C = np.array([cx, cy], T)
        A = d["s"][:, None, None] * (A - C) + C
    if cfg["max_shift"] != 0.0:
        A = A + np.stack([d["tx"], d["ty"]], axis=1)[:, None, :]
    if cfg["jitter_sigma"] != 0.0:
        A = A + d["noise"]
    assert A.dtype == T and B.dtype == T
    return A, B, d


def _neg_flip(B):
    """flip_pose with x -> -x written as a negation (0 - 0 is +0, -(0) is -0: the sign of a zero is not part of any
    comparison below, but the twin keeps the library's form)."""
    q = B.copy()
    q[:, :, 0] = -q[:, :, 0]
    out = q.copy()
    out[:, LEFT], out[:, RIGHT] = q[:, RIGHT], q[:, LEFT]
    return out
