"""TEST INFRASTRUCTURE ONLY.  A restatement of csrc/camera.h in torch on the CPU, parametrised by dtype: float64 is the
yardstick, float32 the same text in the library's precision, so that the error of one against the other bounds what an
equally valid fp32 rounding sequence may differ by.  The projection is written with torch ops, so torch.autograd gives the
gradients; the fit uses the same initialisation, the same fixed iteration count and torch.linalg.solve."""
import numpy as np
import torch

KINDS = ("l1", "mse", "l2")
DET_FLOOR = 1e-12


def _t(a, dtype):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype)


def cam_rows(cams, cam_ids, B, dtype):
    """(rows (B, 9), bad (B,) bool): an id outside the table reads no row -- its camera is nine NaN, and IEEE arithmetic
    does the rest (a gradient that a div == 0 column cuts off stays 0)"""
    cams = _t(cams, dtype)
    if cam_ids is None:
        return cams[0].expand(B, 9), torch.zeros(B, dtype=torch.bool)
    ids = torch.as_tensor(np.asarray(cam_ids), dtype=torch.int64)
    bad = (ids < 0) | (ids >= cams.shape[0])
    rows = cams[torch.where(bad, torch.zeros_like(ids), ids)]
    return torch.where(bad[:, None], torch.full_like(rows, float("nan")), rows), bad


def points(X, translation=None, sub=None, div=None):
    """p = (x div + sub) + t; a column with div == 0 is the constant sub"""
    p = X
    if sub is not None:
        p = torch.where(div == 0, sub.expand_as(X), X * div + sub)
    if translation is not None:
        p = p + translation[:, None, :]
    return p


def project_t(p, rows):
    """torch tensors: p (B, J, 3), rows (B, 9) -> uv (B, J, 2), in the header's operation order"""
    fx, fy, cx, cy, k1, k2, k3, p1, p2 = (rows[:, i, None] for i in range(9))
    x, y = p[..., 0] / p[..., 2], p[..., 1] / p[..., 2]
    r2 = x * x + y * y
    rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    tan = p1 * x + p2 * y
    u = fx * (x * (rad + tan) + p1 * r2) + cx
    v = fy * (y * (rad + tan) + p2 * r2) + cy
    return torch.stack([u, v], dim=-1)


def project(X, cams, cam_ids=None, translation=None, sub=None, div=None, dtype=torch.float64):
    X, translation, sub, div = (_t(a, dtype) for a in (X, translation, sub, div))
    rows, bad = cam_rows(cams, cam_ids, X.shape[0], dtype)
    return project_t(points(X, translation, sub, div), rows).numpy()


def project_bwd(X, duv, cams, cam_ids=None, translation=None, sub=None, div=None, dtype=torch.float64):
    """(dX, dT or None) by autograd"""
    X, translation, sub, div, duv = (_t(a, dtype) for a in (X, translation, sub, div, duv))
    rows, bad = cam_rows(cams, cam_ids, X.shape[0], dtype)
    X = X.clone().requires_grad_(True)
    if translation is not None:
        translation = translation.clone().requires_grad_(True)
    uv = project_t(points(X, translation, sub, div), rows)
    uv.backward(duv)
    return X.grad.numpy(), None if translation is None else translation.grad.numpy()


def residuals(uv, target, div):
    return (uv - target) / torch.as_tensor(div, dtype=uv.dtype)


def errors(X, target, cams, cam_ids=None, translation=None, sub=None, div=None, wh=(1.0, 1.0), dtype=torch.float64):
    uv = torch.as_tensor(project(X, cams, cam_ids, translation, sub, div, dtype))
    return torch.linalg.vector_norm(residuals(uv, _t(target, dtype), wh), dim=-1).numpy()


def loss(X, target, cams, cam_ids=None, translation=None, sub=None, div=None, weights=None, kind="l1", wh=(1.0, 1.0),
         dtype=torch.float64):
    """(loss, dX, dT or None)"""
    X, translation, sub, div, target, weights = (_t(a, dtype) for a in (X, translation, sub, div, target, weights))
    rows, bad = cam_rows(cams, cam_ids, X.shape[0], dtype)
    X = X.clone().requires_grad_(True)
    if translation is not None:
        translation = translation.clone().requires_grad_(True)
    r = residuals(project_t(points(X, translation, sub, div), rows), target, wh)
    if kind == "l1":
        e, n = r.abs().sum(-1), r.numel()
    elif kind == "mse":
        e, n = (r * r).sum(-1), r.numel()
    else:
        e, n = torch.linalg.vector_norm(r, dim=-1), r.numel() // 2
    if weights is not None:
        e = e * weights
    val = e.sum() / n
    val.backward()
    return float(val.detach()), X.grad.numpy(), None if translation is None else translation.grad.numpy()


def _jacobian(p, rows):
    """(uv (B, J, 2), Jm (B, J, 2, 3)) by autograd, joint by joint independent"""
    p = p.clone().requires_grad_(True)
    uv = project_t(p, rows)
    ju = torch.autograd.grad(uv[..., 0].sum(), p, retain_graph=True)[0]
    jv = torch.autograd.grad(uv[..., 1].sum(), p)[0]
    return uv.detach(), torch.stack([ju, jv], dim=-2)


def _solve(M, b):
    """x and ok: the determinant above DET_FLOOR times the diagonal's product (judged in float64 whatever the dtype)"""
    M64 = M.double()
    ok = torch.linalg.det(M64) > DET_FLOOR * M64[:, 0, 0] * M64[:, 1, 1] * M64[:, 2, 2]
    safe = torch.where(ok[:, None, None], M, torch.eye(3, dtype=M.dtype).expand_as(M))
    return torch.linalg.solve(safe, b), ok


def fit(X, target, cams, cam_ids=None, weights=None, sub=None, div=None, iters=3, dtype=torch.float64):
    """(t (B, 3), rms (B,)): camera.h's fit_pose, batched"""
    X, sub, div, target, weights = (_t(a, dtype) for a in (X, sub, div, target, weights))
    B, J = X.shape[:2]
    rows, bad = cam_rows(cams, cam_ids, B, dtype)
    q = points(X, None, sub, div)
    w = torch.ones(B, J, dtype=dtype) if weights is None else weights
    vis = w > 0
    w = torch.where(vis, w, torch.zeros_like(w))
    zero = torch.zeros((), dtype=dtype)
    qv, tv = torch.where(vis[..., None], q, zero), torch.where(vis[..., None], target, zero)      # weights select
    fx, fy, cx, cy = (rows[:, i, None] for i in range(4))
    nx, ny = (tv[..., 0] - cx) / fx, (tv[..., 1] - cy) / fy
    rx, ry = nx * qv[..., 2] - qv[..., 0], ny * qv[..., 2] - qv[..., 1]
    s = lambda v: (w * v).sum(-1)                                                                  # noqa: E731
    o = torch.zeros(B, dtype=dtype)
    M = torch.stack([torch.stack([s(torch.ones_like(nx)), o, -s(nx)], -1), torch.stack([o, s(torch.ones_like(nx)), -s(ny)], -1),
                     torch.stack([-s(nx), -s(ny), s(nx * nx + ny * ny)], -1)], -2)
    b = torch.stack([s(rx), s(ry), -s(nx * rx + ny * ry)], -1)
    t, ok = _solve(M, b)
    ok = ok & (vis.sum(-1) >= 2)
    # a visible joint's garbage must not reach an invisible joint's place: put the visible points at depth, the others at 1 m
    for it in range(iters + 1):
        p = torch.where(vis[..., None], qv + t[:, None, :], torch.ones((), dtype=dtype))
        uv, Jm = _jacobian(p, rows)
        r = torch.where(vis[..., None], tv - uv, zero)
        Jm = torch.where(vis[..., None, None], Jm, zero)
        if it == iters:
            break
        M = torch.einsum("bj,bjki,bjkl->bil", w, Jm, Jm)
        g = torch.einsum("bj,bjki,bjk->bi", w, Jm, r)
        d, ok_i = _solve(M, g)
        ok = ok & ok_i
        t = t + d
    rms = torch.sqrt((w * (r * r).sum(-1)).sum(-1) / w.sum(-1))
    ok = ok & ~bad & torch.isfinite(t).all(-1) & torch.isfinite(rms)
    nan = torch.full((), float("nan"), dtype=dtype)
    return torch.where(ok[:, None], t, nan).numpy(), torch.where(ok, rms, nan).numpy()


def bound(lo, hi, floor_of):
    """Twice the maximum error of the float32 restatement `lo` against the float64 one `hi`, with a floor of one fp32 ulp of
    the magnitude of `floor_of` (the output held to the bound)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ok = np.isfinite(hi) & np.isfinite(lo)
    err = float(np.abs(lo - hi)[ok].max()) if ok.any() else 0.0
    mag = np.abs(np.asarray(floor_of, np.float64))
    mag = float(mag[np.isfinite(mag)].max()) if np.isfinite(mag).any() else 0.0
    ulp = float(np.spacing(np.float32(mag))) if mag > 0 else float(np.finfo(np.float32).tiny)
    return max(2.0 * err, ulp)
