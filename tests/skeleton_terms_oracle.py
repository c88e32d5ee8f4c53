"""Restatement of the criterion's skeleton terms (include/poselift.h PLSkeleton) in numpy fp64, written from the
definitions: bone lengths, the bone-length and left/right symmetry terms, their gradient, and -- for the tests' bounds -- the
first-order propagation of the fp32 roundings of the documented expression.  TEST INFRASTRUCTURE ONLY.

    P = pred div + sub, T = tgt div + sub            (P = pred, T = tgt without a transform)
    lh_k = ||P_c - P_p||, l_k = ||T_c - T_p||         bone k = (c, p)
    L_bone = mean_{b,k} rho(lh_k - l_k),  L_sym = mean_{b,(a,b)} rho(lh_a - lh_b),  rho = |e| ("l1") or e^2 ("mse")
    value = lam_bone L_bone + lam_sym L_sym
"""
import numpy as np

U = 2.0 ** -24                     # half an ulp, relative: the most one fp32 rounding moves a result

H36M_PARENTS = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)
H36M_LEFT, H36M_RIGHT = (4, 5, 6, 11, 12, 13), (1, 2, 3, 14, 15, 16)
CHAIN_PARENTS = (-1, 0, 1, 0, 3)                    # five joints: two arms of two bones each; one pair
CHAIN_LEFT, CHAIN_RIGHT = (2,), (4,)


def tables(parents, left=(), right=()):
    """(child [K], parent [K], pairs [S][2] of bone indices): the bones are the non-root joints in joint order"""
    child = [j for j, p in enumerate(parents) if p != -1]
    bone_of = {j: k for k, j in enumerate(child)}
    pairs = [(bone_of[a], bone_of[b]) for a, b in zip(left, right)]
    return np.array(child), np.array([parents[j] for j in child]), np.array(pairs, dtype=np.int64).reshape(-1, 2)


def raw(x, G, sub=None, div=None):
    x = np.asarray(x, dtype=np.float64).reshape(x.shape[0], -1, G)
    if sub is None:
        return x
    return x * np.asarray(div, np.float64).reshape(-1, G) + np.asarray(sub, np.float64).reshape(-1, G)


def bone_lengths(x, G, child, parent, sub=None, div=None):
    P = raw(x, G, sub, div)
    return np.sqrt(((P[:, child] - P[:, parent]) ** 2).sum(-1))


def _rho(e, rho):
    return (np.abs(e), np.sign(e)) if rho == "l1" else (e * e, 2.0 * e)


def terms(pred, tgt, G, child, parent, pairs, lam_bone, lam_sym, rho="l1", sub=None, div=None, grad_scale=1.0):
    """dict: value, L_bone, L_sym, grad [B][J G], lh, l [B][K], e [B][K], es [B][S], and for the bounds absgrad [B][J G]
    (the sum of the absolute contributions to each gradient element: every bone at the joint, its bone term and each of its
    pair terms counted separately), err_units [B][J G] (the propagated roundings, in units of U) and touch [B][J][K + S] ."""
    B = pred.shape[0]
    J = pred.shape[1] * (pred.shape[2] if pred.ndim == 3 else 1) // G
    K, S = len(child), len(pairs)
    xf = sub is not None
    dv = np.asarray(div, np.float64).reshape(J, G) if xf else np.ones((J, G))
    P, T = raw(pred, G, sub, div), raw(tgt, G, sub, div)
    d, dt = P[:, child] - P[:, parent], T[:, child] - T[:, parent]                      # [B][K][G]
    lh, l = np.sqrt((d * d).sum(-1)), np.sqrt((dt * dt).sum(-1))
    e = lh - l
    rb, gb = _rho(e, rho)
    wb = lam_bone * grad_scale / (B * K)
    ub = wb * gb                                                                        # [B][K] d value / d lh_k, bone term
    L_bone = rb.sum() / (B * K)
    L_sym, es = 0.0, np.zeros((B, 0))
    us = np.zeros((B, K))                    # ... pair terms
    us_abs = np.zeros((B, K))                # sum of their absolute values
    npairs = np.zeros(K)
    ws = 0.0
    if S:
        a, b = pairs[:, 0], pairs[:, 1]
        es = lh[:, a] - lh[:, b]
        rs, gs = _rho(es, rho)
        L_sym = rs.sum() / (B * S)
        ws = lam_sym * grad_scale / (B * S)
        v = ws * gs
        np.add.at(us, (slice(None), a), v)
        np.add.at(us, (slice(None), b), -v)
        np.add.at(us_abs, (slice(None), a), np.abs(v))
        np.add.at(us_abs, (slice(None), b), np.abs(v))
        np.add.at(npairs, a, 1)
        np.add.at(npairs, b, 1)
    u = ub + us
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(lh == 0, 0.0, u / lh)
        r_abs = np.where(lh == 0, 0.0, (np.abs(ub) + us_abs) / lh)
        inv = np.where(lh == 0, 0.0, 1.0 / lh)
        invt = np.where(l == 0, 0.0, 1.0 / l)
    x = d * r[..., None]                                                                # [B][K][G]
    grad, absgrad = np.zeros((B, J, G)), np.zeros((B, J, G))
    cc, cp = x * dv[child], x * dv[parent]
    np.add.at(grad, (slice(None), child), cc)
    np.add.at(grad, (slice(None), parent), -cp)
    xa = np.abs(d) * r_abs[..., None]
    np.add.at(absgrad, (slice(None), child), xa * np.abs(dv[child]))
    np.add.at(absgrad, (slice(None), parent), xa * np.abs(dv[parent]))

    # ---- the roundings of the documented fp32 expression, propagated to first order, in units of U ------------------------
    def d_err(X, src, dd):
        """absolute error of d_g: its own rounding, and with a transform those of both raw coordinates (two each: the
        product and the sum)"""
        if not xf:
            return np.abs(dd)
        y = np.asarray(src, np.float64).reshape(B, J, G)
        ax = np.abs(y * dv) + np.abs(X)
        return np.abs(dd) + ax[:, child] + ax[:, parent]
    ad, adt = d_err(P, pred, d), d_err(T, tgt, dt)
    # a length: the d's through sum |d_g| ad_g / l; G rounded steps of ss, halved by the root; the root
    alh = (np.abs(d) * ad).sum(-1) * inv + (G / 2 + 1) * lh
    al = (np.abs(dt) * adt).sum(-1) * invt + (G / 2 + 1) * l
    if rho == "l1":
        au = np.full((B, K), 2 * abs(wb))                    # wb = lambda * cb, cb = s / (float)(B K): two roundings
        av = np.full((B, S), 2 * abs(ws))
    else:                                                    # u = e * (2 wb): e's rounding and both lengths' errors; wb; the product
        au = 2 * abs(wb) * (np.abs(e) + alh + al) + 3 * np.abs(ub)
        av = 2 * abs(ws) * (np.abs(es) + alh[:, pairs[:, 0]] + alh[:, pairs[:, 1]]) + 3 * np.abs(ws * _rho(es, rho)[1]) if S else 0
    aut = au.copy()
    if S:
        np.add.at(aut, (slice(None), pairs[:, 0]), av)
        np.add.at(aut, (slice(None), pairs[:, 1]), av)
        aut += npairs * (np.abs(ub) + us_abs)                # one rounded add per pair
    ar = aut * inv + np.abs(r) * alh * inv + np.abs(r)       # r = u / lh
    ax = ad * np.abs(r)[..., None] + np.abs(d) * ar[..., None] + np.abs(x)             # x = d_g * r
    err = np.zeros((B, J, G))
    for idx, c in ((child, cc), (parent, cp)):
        ac = ax * np.abs(dv[idx]) + (np.abs(c) if xf else 0)                            # * div
        np.add.at(err, (slice(None), idx), ac)
    m = np.zeros(J)
    np.add.at(m, child, 1)
    np.add.at(m, parent, 1)
    err += np.maximum(m - 1, 0)[None, :, None] * absgrad     # the adds into the gradient row: the first one is exact
    touch = np.zeros((J, K + S), dtype=bool)                 # which bones (and pairs, through their bones) reach a joint
    touch[child, np.arange(K)] = True
    touch[parent, np.arange(K)] = True
    for s_, (a_, b_) in enumerate(pairs):
        touch[:, K + s_] = touch[:, a_] | touch[:, b_]
    return {"value": lam_bone * L_bone + lam_sym * L_sym, "L_bone": L_bone, "L_sym": L_sym, "grad": grad.reshape(B, J * G),
            "lh": lh, "l": l, "e": e, "es": es, "absgrad": absgrad.reshape(B, J * G), "err_units": err.reshape(B, J * G),
            "touch": touch}


def undecided(o, rho, floor=16 * U):
    """(mask [B][J G] of gradient elements an undecidable l1 sign reaches, fraction of bones and pairs that are undecidable):
    |e| < floor * max of the two lengths.  Empty for mse."""
    B, K = o["e"].shape
    W = o["grad"].shape[1]
    if rho != "l1":
        return np.zeros((B, W), dtype=bool), 0.0
    bad = np.abs(o["e"]) < floor * np.maximum(o["lh"], o["l"])
    if o["es"].shape[1]:
        # (the pairs' lengths: recovered from es = lh_a - lh_b through the caller's tables is not needed -- the floor uses
        # the larger of the pose's lengths, which bounds both)
        big = o["lh"].max(axis=1, keepdims=True)
        bad = np.concatenate([bad, np.abs(o["es"]) < floor * big], axis=1)
    else:
        bad = np.concatenate([bad, np.zeros((B, 0), dtype=bool)], axis=1)
    frac = bad.mean() if bad.size else 0.0
    G = W // o["touch"].shape[0]
    joints = (bad[:, None, :] & o["touch"][None]).any(-1)                               # [B][J]
    return np.repeat(joints, G, axis=1), float(frac)


def torch_terms(pred, tgt, G, child, parent, pairs, lam_bone, lam_sym, rho="l1", sub=None, div=None, dtype=np.float64):
    """(value, gradient) by torch autograd on the CPU in `dtype`: norms by torch.linalg.vector_norm (subgradient 0 at 0)"""
    import torch
    td = torch.float64 if dtype == np.float64 else torch.float32
    p = torch.tensor(np.asarray(pred), dtype=td, requires_grad=True)
    t = torch.tensor(np.asarray(tgt), dtype=td)
    B = p.shape[0]

    def lengths(x):
        x = x.reshape(B, -1, G)
        if sub is not None:
            x = x * torch.tensor(np.asarray(div), dtype=td).reshape(-1, G) + torch.tensor(np.asarray(sub), dtype=td).reshape(-1, G)
        return torch.linalg.vector_norm(x[:, list(child)] - x[:, list(parent)], dim=-1)

    def rho_(e):
        return e.abs() if rho == "l1" else e * e
    lh, l = lengths(p), lengths(t)
    val = lam_bone * rho_(lh - l).mean()
    if len(pairs):
        val = val + lam_sym * rho_(lh[:, [a for a, _ in pairs]] - lh[:, [b for _, b in pairs]]).mean()
    val.backward()
    return val.item(), p.grad.numpy().reshape(B, -1)
