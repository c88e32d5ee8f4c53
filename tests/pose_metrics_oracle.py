"""numpy fp64 oracle of the evaluation metrics (MPJPE, N-MPJPE, P-MPJPE per pose and joint; per-group sums and PCK counts)
and the inputs the host and GPU tests share.

P-MPJPE is computed by the SVD route with the determinant fix (Martinez et al. / VideoPose3D `p_mpjpe`), deliberately a
different algorithm from the library's quaternion eigenvector.  The degenerate rules are written out: a prediction with
||P0||^2 == 0 gets scale 0 (it is scored against the target's centroid), and so does a collapsed target (M == 0), whose
error is then 0; sum P.P == 0 gives N-MPJPE scale 0."""
import os

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
AUC_THRESHOLDS = np.arange(31, dtype=np.float64) * 0.005
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_pose_metrics.npz")


def pose_errors(pred, tgt):
    """pred, tgt (B, J, 3) -> err (3, B, J), aligned (B, J, 3), gap (B,) in fp64.
    gap = (l1 - l2) / l1 of the two largest eigenvalues of Horn's 4x4 matrix, from the singular values of M and the sign of
    det M (l1 = s1 + s2 + d s3, l2 = s1 - s2 - d s3); inf for a degenerate pose (collapsed prediction or target)."""
    P, T = np.asarray(pred, np.float64), np.asarray(tgt, np.float64)
    B, J, _ = P.shape
    err = np.empty((3, B, J))
    aligned = np.empty((B, J, 3))
    gap = np.empty(B)
    for b in range(B):
        p, t = P[b], T[b]
        err[0, b] = np.linalg.norm(p - t, axis=1)
        pp = (p * p).sum()
        s = (p * t).sum() / pp if pp != 0 else 0.0
        err[1, b] = np.linalg.norm(s * p - t, axis=1)
        mu_p, mu_t = p.mean(axis=0), t.mean(axis=0)
        p0, t0 = p - mu_p, t - mu_t
        n0 = (p0 * p0).sum()
        if not (np.isfinite(p).all() and np.isfinite(t).all()):
            err[:, b], aligned[b], gap[b] = np.nan, np.nan, np.inf
            continue
        if n0 == 0 or (t0 * t0).sum() == 0:           # collapsed prediction / collapsed target: scale 0
            aligned[b] = mu_t
            gap[b] = np.inf
        else:
            M = p0.T @ t0                              # M_ab = sum_j P0_ja T0_jb
            U, S, Vt = np.linalg.svd(M)
            d = np.sign(np.linalg.det(Vt.T @ U.T))
            d = 1.0 if d == 0 else d
            D = np.diag([1.0, 1.0, d])
            R = Vt.T @ D @ U.T                         # y = R x maximises tr(R M) over proper rotations
            a = (S[0] + S[1] + d * S[2]) / n0
            aligned[b] = a * p0 @ R.T + mu_t
            l1, l2 = S[0] + S[1] + d * S[2], S[0] - S[1] - d * S[2]
            gap[b] = (l1 - l2) / l1
        err[2, b] = np.linalg.norm(aligned[b] - t, axis=1)
    return err, aligned, gap


def coord_scale(pred, tgt):
    """S of the gate: the largest absolute coordinate of each pose pair, (B,)."""
    B = pred.shape[0]
    return np.maximum(np.abs(np.asarray(pred, np.float64)).reshape(B, -1).max(axis=1),
                      np.abs(np.asarray(tgt, np.float64)).reshape(B, -1).max(axis=1))


def gate(ref, S):
    """|got - ref| <= 1e-5 |ref| + 64 eps32 S; S (B,) broadcast over a (3, B, J) or (B, J, 3) array."""
    S = S[None, :, None] if ref.shape[0] == 3 and ref.ndim == 3 and ref.shape[1] == S.shape[0] else S[:, None, None]
    return 1e-5 * np.abs(ref) + 64 * EPS32 * S


def excess_in_eps(got, ref, S):
    """max |got - ref| in units of eps32 S (what DESIGN.md records)."""
    Sb = S[None, :, None] if ref.shape[0] == 3 and ref.ndim == 3 and ref.shape[1] == S.shape[0] else S[:, None, None]
    return float((np.abs(np.asarray(got, np.float64) - ref) / (EPS32 * Sb)).max())


def accumulate(err, groups, G, thresholds):
    """One pass over err (3, B, J): sums (G, 3, J), counts (G, 3, T, J), n_poses (G + 1,) -- ids outside [0, G) only count
    in n_poses[G]."""
    _, B, J = err.shape
    thr = np.asarray(thresholds, np.float32).astype(np.float64)
    sums = np.zeros((G, 3, J))
    counts = np.zeros((G, 3, len(thr), J), np.int64)
    n = np.zeros(G + 1, np.int64)
    groups = np.zeros(B, np.int64) if groups is None else np.asarray(groups, np.int64)
    for g in range(G):
        sel = groups == g
        n[g] = sel.sum()
        sums[g] = err[:, sel].sum(axis=1)
        counts[g] = (err[:, sel, None, :] <= thr[None, None, :, None]).sum(axis=1)
    n[G] = ((groups < 0) | (groups >= G)).sum()
    return sums, counts, n


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def random_poses(B=512, J=17, seed=13):
    """H36M-shaped: per-joint std from 0.03 to 0.58 m, joint 0 at the origin, prediction = target + N(0, 0.04)."""
    rng = np.random.default_rng(seed)
    std = np.linspace(0.03, 0.58, J)
    tgt = rng.standard_normal((B, J, 3)) * std[None, :, None]
    tgt[:, 0] = 0
    pred = tgt + rng.standard_normal((B, J, 3)) * 0.04
    return pred.astype(np.float32), tgt.astype(np.float32)


def well_conditioned_poses(B, J, seed, min_gap=0.1):
    """The first B of 4 B random poses whose eigenvalue gap (the oracle's, nothing else looked at) is at least min_gap: at
    J = 3 every pose is a triangle, and a near-collinear one leaves the rotation about its long side undetermined."""
    pred, tgt = random_poses(4 * B, J, seed)
    keep = np.flatnonzero(pose_errors(pred, tgt)[2] >= min_gap)[:B]
    assert keep.size == B
    return np.ascontiguousarray(pred[keep]), np.ascontiguousarray(tgt[keep])


def golden_poses():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return z["pred"], z["tgt"]


def special_poses():
    """name -> (pred, tgt), (1, J, 3) fp32 each."""
    rng = np.random.default_rng(5)
    _, base = random_poses(1, 17, seed=21)
    base = base[0].astype(np.float64)
    noise = rng.standard_normal((17, 3)) * 0.04
    out = {}
    out["identical"] = (base, base)
    out["mirrored_x"] = (base * np.array([-1.0, 1.0, 1.0]), base)
    out["similarity"] = (1.7 * base @ _rot([1, 2, 3], 0.7).T + np.array([120.0, -75.0, 40.0]), base)
    flat = base * np.array([1.0, 1.0, 0.0])
    out["planar"] = (flat + noise * np.array([1.0, 1.0, 0.0]), flat)
    out["near_180"] = (base @ _rot([0.3, -1, 0.5], np.pi - 1e-3).T + noise, base)
    out["offset_1000m"] = (base + noise + 1000.0, base)
    out["collapsed_pred"] = (np.tile([0.3, 0.2, 0.1], (17, 1)), base)
    out["collapsed_tgt"] = (base + noise, np.tile([0.3, 0.2, 0.1], (17, 1)))
    for J in (3, 16, 32):
        p, t = random_poses(1, J, seed=100 + J)
        out[f"J{J}"] = (p[0], t[0])
    return {k: (np.ascontiguousarray(p, np.float32)[None], np.ascontiguousarray(t, np.float32)[None]) for k, (p, t) in out.items()}


def all_cases():
    """name -> (pred, tgt): g13, the 512 random poses and every special pose."""
    cases = {"g13": golden_poses(), "random512": random_poses()}
    cases.update(special_poses())
    return cases
