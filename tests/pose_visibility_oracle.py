"""numpy fp64 oracle of the evaluation metrics with per-pose joint weights (include/poselift.h pl_pose_errors_w):
visibility-weighted N-MPJPE and P-MPJPE per pose and joint, and the masked per-group sums, PCK counts and visible counts.

As tests/pose_metrics_oracle.py, P-MPJPE goes by the SVD route with the determinant fix -- here of the WEIGHTED covariance of
the visible joints -- deliberately not the library's quaternion eigenvector.  V = {j : w_j > 0}; a weight that is not > 0
(zero, negative, NaN) is "not visible".  Sums over V are taken over the selected rows only, so whatever an invisible joint
holds (a NaN-coded missing target) reaches its own errors and aligned coordinates and nothing else.  Degenerate rules: no
visible joint -> s = 0, a = 0, both centroids 0; a collapsed visible prediction or target (one visible joint is both) -> a = 0.

The gate, its scale S and the pose generators are pose_metrics_oracle's; the weights are row_weights_oracle.weights (about
a quarter zeros, one all-zero row, one all-zero joint column)."""
import os

import numpy as np

from pose_metrics_oracle import (AUC_THRESHOLDS, EPS32, coord_scale, excess_in_eps, gate, golden_poses,  # noqa: F401
                                 random_poses, special_poses, well_conditioned_poses)
from row_weights_oracle import weights  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_pose_visibility.npz")
MIN_GAP = 0.05          # rotation-dependent outputs are compared for poses whose oracle gap is at least this (as the unweighted tests)


def gate_err(ref, S):
    """pose_metrics_oracle.gate, |got - ref| <= 1e-5 |ref| + 64 eps32 S, for any slice (..., B, J) of the errors; S (B,)."""
    return 1e-5 * np.abs(ref) + 64 * EPS32 * np.asarray(S)[:, None]


def gate_aligned(ref, S):
    """The same gate for (B, J, 3) aligned poses."""
    assert ref.ndim == 3 and ref.shape[2] == 3
    return gate(ref, S) if ref.shape[0] != 3 else 1e-5 * np.abs(ref) + 64 * EPS32 * np.asarray(S)[:, None, None]


def excess(got, ref, S):
    """max |got - ref| in units of eps32 S (excess_in_eps for any slice): errors (..., B, J) or aligned (B, J, 3) by ndim of S."""
    Sb = np.asarray(S)[:, None, None] if (ref.ndim == 3 and ref.shape[-1] == 3 and ref.shape[0] == len(S)) else np.asarray(S)[:, None]
    d = np.abs(np.asarray(got, np.float64) - ref) / (EPS32 * Sb)
    return float(d.max()) if d.size else 0.0


def visible(w):
    with np.errstate(invalid="ignore"):
        return np.asarray(w) > 0                      # False for NaN


def pose_errors(pred, tgt, w):
    """pred, tgt (B, J, 3), w (B, J) -> err (3, B, J), aligned (B, J, 3), gap (B,) in fp64.
    gap: (l1 - l2) / l1 of the two largest eigenvalues of Horn's matrix of the weighted covariance, as in the unweighted
    oracle; inf for a degenerate pose (no or one visible joint, collapsed visible prediction or target)."""
    P, T, Wt = np.asarray(pred, np.float64), np.asarray(tgt, np.float64), np.asarray(w, np.float64)
    B, J, _ = P.shape
    assert Wt.shape == (B, J)
    err = np.empty((3, B, J))
    aligned = np.empty((B, J, 3))
    gap = np.empty(B)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            p, t = P[b], T[b]
            v = visible(Wt[b])
            wv, pv, tv = Wt[b][v], p[v], t[v]
            err[0, b] = np.linalg.norm(p - t, axis=1)
            if not (np.isfinite(pv).all() and np.isfinite(tv).all()):          # a NaN at a VISIBLE joint: as the unweighted route
                err[1:, b], aligned[b], gap[b] = np.nan, np.nan, np.inf
                continue
            pp = (wv[:, None] * pv * pv).sum()
            s = (wv[:, None] * pv * tv).sum() / pp if pp != 0 else 0.0
            err[1, b] = np.linalg.norm(s * p - t, axis=1)
            gap[b] = np.inf
            if not v.any():
                a, R, mu_p, mu_t = 0.0, np.eye(3), np.zeros(3), np.zeros(3)
            else:
                Wsum = wv.sum()
                # a collapsed visible subset is decided on the coordinates themselves, and its centroid is the point: the
                # weighted mean of equal values would leave round-off where the definition has an exact 0
                flat_p, flat_t = bool((pv == pv[0]).all()), bool((tv == tv[0]).all())
                mu_p = pv[0].copy() if flat_p else (wv[:, None] * pv).sum(axis=0) / Wsum
                mu_t = tv[0].copy() if flat_t else (wv[:, None] * tv).sum(axis=0) / Wsum
                p0v, t0v = pv - mu_p, tv - mu_t
                n0 = (wv[:, None] * p0v * p0v).sum()
                if flat_p or flat_t:
                    a, R = 0.0, np.eye(3)
                else:
                    M = (wv[:, None] * p0v).T @ t0v                            # M_ab = sum_V w_j P0_ja T0_jb
                    U, S, Vt = np.linalg.svd(M)
                    d = np.sign(np.linalg.det(Vt.T @ U.T))
                    d = 1.0 if d == 0 else d
                    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
                    l1, l2 = S[0] + S[1] + d * S[2], S[0] - S[1] - d * S[2]
                    a = l1 / n0
                    gap[b] = (l1 - l2) / l1 if l1 != 0 else np.inf
            if a == 0.0:                                                       # the scale-0 rule: the target's centroid, whatever
                aligned[b] = np.where(np.isfinite(p).all(axis=1)[:, None], mu_t[None, :], np.nan)   # a finite joint held
            else:
                aligned[b] = a * (p - mu_p) @ R.T + mu_t
            err[2, b] = np.linalg.norm(aligned[b] - t, axis=1)
    return err, aligned, gap


def accumulate(err, w, groups, G, thresholds):
    """One pass over err (3, B, J) with the mask w > 0: sums (G, 3, J), counts (G, 3, T, J), n_poses (G + 1,) -- every pose
    of a group, fully invisible ones included; ids outside [0, G) only count in n_poses[G] -- and n_valid (G, J)."""
    _, B, J = err.shape
    v = visible(w)
    thr = np.asarray(thresholds, np.float32).astype(np.float64)
    sums = np.zeros((G, 3, J))
    counts = np.zeros((G, 3, len(thr), J), np.int64)
    n = np.zeros(G + 1, np.int64)
    n_valid = np.zeros((G, J), np.int64)
    groups = np.zeros(B, np.int64) if groups is None else np.asarray(groups, np.int64)
    with np.errstate(invalid="ignore"):
        for g in range(G):
            sel = groups == g
            n[g] = sel.sum()
            m = v[sel]                                                          # (n_g, J)
            e = err[:, sel]
            sums[g] = np.where(m[None], e, 0.0).sum(axis=1)
            counts[g] = (m[None, :, None, :] & (e[:, :, None, :] <= thr[None, None, :, None])).sum(axis=1)
            n_valid[g] = m.sum(axis=0)
    n[G] = ((groups < 0) | (groups >= G)).sum()
    return sums, counts, n, n_valid


def input_sets():
    """name -> (pred, tgt, w): the four sets every comparison with this oracle runs on, with the most poses each may lose to
    the gap condition in `MAX_EXCLUDED`."""
    out = {}
    for seed in (0, 1, 2):
        p, t = random_poses()
        out[f"random512 w{seed}"] = (p, t, weights(512, 17, seed))
        p, t = golden_poses()
        out[f"g13 w{seed}"] = (p, t, weights(128, 17, seed))
    p, t = well_conditioned_poses(64, 3, seed=203)
    out["J3x64"] = (p, t, np.random.default_rng(3).uniform(0.25, 2.0, (64, 3)).astype(np.float32))      # J = 3: no room for zeros
    p, t = well_conditioned_poses(64, 32, seed=232)
    out["J32x64"] = (p, t, weights(64, 32, 7))
    return out


MAX_EXCLUDED = {"random512": 0, "g13": 2, "J3x64": 0, "J32x64": 0}


def max_excluded(name):
    return MAX_EXCLUDED[name.split(" ")[0]]


def rotation_mask(gap, name):
    """(B,) bool: poses whose rotation-dependent outputs are compared.  Looks at the oracle's gap alone and asserts the cap of
    the set."""
    keep = gap >= MIN_GAP
    assert int((~keep).sum()) <= max_excluded(name), (name, int((~keep).sum()), np.sort(gap)[:4])
    return keep
