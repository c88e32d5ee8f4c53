"""Restatement of the criterion with per-pose joint weights (include/poselift.h PLRowWeightsCriterion) and of
the weights gather (pl_row_weights_gather) in numpy fp64, written from the definitions and checked against torch's own
modules in tests/test_row_weights_host.py.

    W = effective_weights(row_weights, joint_weights)          (B, J): rw, or fl32(w_j * rw) with both -- one fp32 product
    loss, grad = criterion(kind, pred, tgt, coords, W, beta=1.0, grad_scale=1.0)
    grad_fp32(...)       the gradient as the header documents it in fp32, rounding for rounding
    gather(table, src_idx, flipped)                            out[k][j] = table[s][flipped_k ? flip_src_joint(j) : j]

pred, tgt: (B, O) arrays, O = J * coords.  W stands where the joint weight w_j stands in every row of the criterion's table;
the normaliser stays 1 / (B O), for mpjpe 1 / (B J).  Weights multiply: a zero weight times a NaN is a NaN.
"""
import numpy as np

KINDS = ("mse", "l1", "smooth_l1", "mpjpe")
# flip_pose's joint swap (phase3_direct/my_HybrIK/utils.py:372-396): the source joint of output joint j
FLIP_SRC = np.array([0, 4, 5, 6, 1, 2, 3, 7, 8, 9, 10, 14, 15, 16, 11, 12, 13])


def effective_weights(row_weights, joint_weights=None):
    rw = np.asarray(row_weights, np.float32)
    assert rw.ndim == 2
    if joint_weights is None:
        return rw
    w = np.asarray(joint_weights, np.float32)
    assert w.shape == (rw.shape[1],)
    with np.errstate(invalid="ignore", over="ignore"):
        return (w[None, :] * rw).astype(np.float32)


def criterion(kind, pred, tgt, coords, W, beta=1.0, grad_scale=1.0):
    p, t = np.asarray(pred, np.float64), np.asarray(tgt, np.float64)
    B, O = p.shape
    assert O % coords == 0 and kind in KINDS
    J = O // coords
    W = np.asarray(W, np.float64)
    assert W.shape == (B, J)
    we = np.repeat(W, coords, axis=1)
    d = p - t
    s = float(grad_scale)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if kind == "mse":
            return (we * d * d).sum() / (B * O), s * 2.0 * we * d / (B * O)
        if kind == "l1":
            sign = np.where(d > 0, 1.0, np.where(d < 0, -1.0, 0.0))
            return (we * np.abs(d)).sum() / (B * O), s * we * sign / (B * O)
        if kind == "smooth_l1":
            assert beta > 0
            a = np.abs(d)
            lin = a >= beta
            rho = np.where(lin, a - 0.5 * beta, 0.5 * d * d / beta)
            g = np.where(lin, np.where(d > 0, 1.0, -1.0), d / beta)
            return (we * rho).sum() / (B * O), s * we * g / (B * O)
        dj = d.reshape(B, J, coords)
        r = np.sqrt((dj * dj).sum(-1))
        q = s * W / r / (B * J)
        g = np.where((r == 0)[..., None], 0.0, dj * q[..., None])
        return (W * r).sum() / (B * J), g.reshape(B, O)


def torch_criterion(kind, p, t, coords, W, beta, dtype=np.float64):
    """(loss, d loss / d p) from torch on the CPU: (W * elementwise(p, t)).mean() with nn.MSELoss / nn.L1Loss /
    nn.SmoothL1Loss(reduction="none"), and (W * torch.norm(d, dim=-1)).mean() -- what decides the non-finite sets"""
    import torch
    p = torch.from_numpy(np.asarray(p, dtype)).requires_grad_(True)
    t = torch.from_numpy(np.asarray(t, dtype))
    B, O = p.shape
    J = O // coords
    W = torch.from_numpy(np.asarray(W, dtype))
    if kind == "mpjpe":
        loss = (W * torch.norm((p - t).reshape(B, J, coords), dim=-1)).mean()
    else:
        mod = {"mse": torch.nn.MSELoss(reduction="none"), "l1": torch.nn.L1Loss(reduction="none"),
               "smooth_l1": torch.nn.SmoothL1Loss(reduction="none", beta=beta)}[kind]
        loss = (W.repeat_interleave(coords, dim=1) * mod(p, t)).mean()
    loss.backward()
    return loss.item(), p.grad.numpy()


def grad_fp32(kind, pred, tgt, coords, W, beta=1.0, grad_scale=1.0):
    """The documented fp32 expression of the gradient in numpy float32 (every operation rounded once); W (B, J) fp32."""
    f = np.float32
    p, t = np.asarray(pred, f), np.asarray(tgt, f)
    B, O = p.shape
    J = O // coords
    W = np.asarray(W, f)
    we = np.repeat(W, coords, axis=1)
    d = p - t
    n = f(B * O)
    s = f(grad_scale)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if kind == "mse":
            g = d * (s * f(2.0) / n)
        elif kind == "l1":
            coef = s / n
            g = np.where(d > 0, coef, np.where(d < 0, -coef, f(0.0))).astype(f)
        elif kind == "smooth_l1":
            coef = s / n
            cb = coef / f(beta)
            g = np.where(np.abs(d) >= f(beta), np.where(d > 0, coef, -coef), d * cb).astype(f)
        else:
            dj = d.reshape(B, J, coords)
            ss = dj[..., 0] * dj[..., 0]
            for c in range(1, coords):
                ss = (dj[..., c].astype(np.float64) ** 2 + ss.astype(np.float64)).astype(f)
            r = np.sqrt(ss)
            q = ((s / f(B * J)) * W / r).astype(f)
            return np.where((ss == 0)[..., None], f(0.0), dj * q[..., None]).astype(f).reshape(B, O)
        return (g * we).astype(f)


def gather(table, src_idx=None, flipped=None):
    """out[k][j] = table[s][flipped[k] ? FLIP_SRC[j] : j], s = src_idx[k] or k; flipped None = no pose is flipped"""
    table = np.asarray(table)
    src = np.arange(table.shape[0]) if src_idx is None else np.asarray(src_idx)
    out = table[src].copy()
    if flipped is not None:
        fl = np.asarray(flipped, bool)
        assert table.shape[1] == 17 and fl.shape == (len(src),)
        out[fl] = out[fl][:, FLIP_SRC]
    return out


def weights(B, J, seed=0):
    """The test weights: uniform in [0, 2) with about a quarter exact zeros, one all-zero row and one all-zero joint column
    (where the shape has more than one of each)."""
    rng = np.random.default_rng(seed)
    rw = rng.uniform(0.0, 2.0, (B, J)).astype(np.float32)
    rw[rng.random((B, J)) < 0.25] = 0.0
    if B > 1:
        rw[B // 2, :] = 0.0
    if J > 1:
        rw[:, J // 3] = 0.0
    return rw
