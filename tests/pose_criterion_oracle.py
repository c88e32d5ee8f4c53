"""Restatement of the train step's criteria (include/poselift.h PLCriterion) in numpy fp64, written from the
definitions and checked against torch's own modules in tests/test_pose_criterion_host.py.

    loss, grad = criterion(kind, pred, tgt, coords, weights=None, beta=1.0, grad_scale=1.0)

pred, tgt: (B, O) arrays, O = J * coords; weights: J floats or None.  Non-finite inputs give what the formulas give under
IEEE arithmetic with torch's masking rules (sign(NaN) = 0 for l1; the quadratic arm for a NaN in smooth_l1; the zero-norm
mask -- and nothing else -- for mpjpe), which is what torch computes on the CPU.

    grad_fp32(...)      the gradient as the header documents it in fp32, rounding for rounding (what the kernels must give)
"""
import numpy as np

KINDS = ("mse", "l1", "smooth_l1", "mpjpe")


def _w_elem(weights, J, coords):
    w = np.ones(J, np.float64) if weights is None else np.asarray(weights, np.float64)
    assert w.shape == (J,)
    return w, np.repeat(w, coords)


def criterion(kind, pred, tgt, coords, weights=None, beta=1.0, grad_scale=1.0):
    p, t = np.asarray(pred, np.float64), np.asarray(tgt, np.float64)
    B, O = p.shape
    assert O % coords == 0 and kind in KINDS
    J = O // coords
    w, we = _w_elem(weights, J, coords)
    d = p - t
    s = float(grad_scale)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if kind == "mse":
            return (we * d * d).sum() / (B * O), s * 2.0 * we * d / (B * O)
        if kind == "l1":
            sign = np.where(d > 0, 1.0, np.where(d < 0, -1.0, 0.0))            # 0 at d = 0 and at a NaN
            return (we * np.abs(d)).sum() / (B * O), s * we * sign / (B * O)
        if kind == "smooth_l1":
            assert beta > 0
            a = np.abs(d)
            lin = a >= beta                                                     # a NaN takes the quadratic arm: NaN
            rho = np.where(lin, a - 0.5 * beta, 0.5 * d * d / beta)
            g = np.where(lin, np.where(d > 0, 1.0, -1.0), d / beta)
            return (we * rho).sum() / (B * O), s * we * g / (B * O)
        dj = d.reshape(B, J, coords)
        r = np.sqrt((dj * dj).sum(-1))
        q = (s * w)[None, :] / r / (B * J)
        g = np.where((r == 0)[..., None], 0.0, dj * q[..., None])               # the whole joint 0 where its norm is 0
        return (w[None, :] * r).sum() / (B * J), g.reshape(B, O)


def torch_criterion(kind, p, t, coords, weights, beta, dtype=np.float64):
    """(loss, d loss / d p) from torch's own modules on the CPU: nn.MSELoss, nn.L1Loss, nn.SmoothL1Loss(beta) and
    (w * torch.norm(d, dim=-1)).mean() -- what the oracle above is checked against, and what decides the non-finite sets"""
    import torch
    p = torch.from_numpy(np.asarray(p, dtype)).requires_grad_(True)
    t = torch.from_numpy(np.asarray(t, dtype))
    B, O = p.shape
    J = O // coords
    w = torch.ones(J, dtype=p.dtype) if weights is None else torch.from_numpy(np.asarray(weights, dtype))
    we = w.repeat_interleave(coords)
    if kind == "mpjpe":
        loss = (w * torch.norm((p - t).reshape(B, J, coords), dim=-1)).mean()
    elif weights is None:
        mod = {"mse": torch.nn.MSELoss(), "l1": torch.nn.L1Loss(), "smooth_l1": torch.nn.SmoothL1Loss(beta=beta)}[kind]
        loss = mod(p, t)
    else:
        mod = {"mse": torch.nn.MSELoss(reduction="none"), "l1": torch.nn.L1Loss(reduction="none"),
               "smooth_l1": torch.nn.SmoothL1Loss(reduction="none", beta=beta)}[kind]
        loss = (we * mod(p, t)).mean()
    loss.backward()
    return loss.item(), p.grad.numpy()


def grad_fp32(kind, pred, tgt, coords, weights=None, beta=1.0, grad_scale=1.0):
    """The documented fp32 expression of the gradient, evaluated in numpy float32 (every operation rounded once)."""
    f = np.float32
    p, t = np.asarray(pred, f), np.asarray(tgt, f)
    B, O = p.shape
    J = O // coords
    d = p - t
    n = f(B * O)
    s = f(grad_scale)
    we = None if weights is None else np.repeat(np.asarray(weights, f), coords)[None, :]
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
            for c in range(1, coords):          # fmaf(d_c, d_c, ss): the product exact in fp64, one rounding to fp32
                ss = (dj[..., c].astype(np.float64) ** 2 + ss.astype(np.float64)).astype(f)
            r = np.sqrt(ss)
            coef = s / f(B * J)
            cw = coef if weights is None else coef * np.asarray(weights, f)[None, :]
            q = (cw / r).astype(f)
            return np.where((ss == 0)[..., None], f(0.0), dj * q[..., None]).astype(f).reshape(B, O)
        return g if we is None else (g * we).astype(f)
