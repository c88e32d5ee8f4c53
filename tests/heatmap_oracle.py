"""fp64 oracle of the heat-map loss of the soft-argmax heads: the dense Gaussian target restated from its definition
(csrc/heatmap_target.h), torch softmax, autograd.  Shared by test_heatmap_target_host.py and test_gpu_heatmap_loss.py.

Only the centre index is formed in fp32, as the library and the dataset form it (alpha * (t + gamma), two roundings): where
the centre and its rounding tie fall is part of the definition.  Everything after it is fp64."""
import math

import numpy as np
import torch


def half_of_sigma(sigma):
    size = int(math.ceil(6 * sigma))
    if not size % 2:
        size += 1
    return size // 2


def centre_index(target, law, ncoord, depth):
    """(BJ, 3) fp32 centre indices (x, y, z); an unused axis (two coordinates, depth 1) is 0."""
    t = np.asarray(target, dtype=np.float32).reshape(-1, ncoord)
    mu = np.zeros((t.shape[0], 3), dtype=np.float32)
    for a in range(ncoord if depth > 1 else 2):
        mu[:, a] = np.float32(law[a]) * (t[:, a] + np.float32(law[3 + a]))
    return mu


def dense_target(target, D, H, W, sigma, law, ncoord=None):
    """(BJ, D, H, W) float64; NaN throughout for a pair whose centre is not finite."""
    ncoord = ncoord or (3 if D > 1 else 2)
    mu = centre_index(target, law, ncoord, D)
    half = half_of_sigma(sigma)
    out = np.zeros((mu.shape[0], D, H, W), dtype=np.float64)
    iw, ih, idd = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), np.arange(D, dtype=np.float64)
    for n in range(mu.shape[0]):
        if not np.all(np.isfinite(mu[n])):
            out[n] = np.nan
            continue
        m = mu[n].astype(np.float64)
        c = np.rint(mu[n]).astype(np.float64)                   # ties to even, on the fp32 centre
        fac = []
        for idx, a in ((idd, 2), (ih, 1), (iw, 0)):
            inside = np.abs(idx - c[a]) <= half
            fac.append((inside, (idx - m[a]) ** 2))
        (zd, qd), (zh, qh), (zw, qw) = fac
        q = qd[:, None, None] + qh[None, :, None] + qw[None, None, :]
        inside = zd[:, None, None] & zh[None, :, None] & zw[None, None, :]
        out[n] = np.where(inside, np.exp(-q / (2.0 * sigma * sigma)), 0.0)
    return out


def head_outputs(logits, g, centred):
    """logits (BJ, D, H, W) float64 torch tensor (may require grad), g the dense target as a torch tensor ->
    (coords (BJ, 3 | 2), sq (BJ,), p) in float64."""
    BJ, D, H, W = logits.shape
    p = torch.softmax(logits.reshape(BJ, -1), dim=1).reshape(BJ, D, H, W)
    ex = (p.sum(dim=(1, 2)) * torch.arange(W, dtype=torch.float64)).sum(dim=1)
    ey = (p.sum(dim=(1, 3)) * torch.arange(H, dtype=torch.float64)).sum(dim=1)
    ez = (p.sum(dim=(2, 3)) * torch.arange(D, dtype=torch.float64)).sum(dim=1)
    if centred:
        coords = torch.stack([(ex / W - 0.5) * 2, (ey / H - 0.5) * 2, (ez / D - 0.5) * 2], dim=1)
    else:
        coords = torch.stack([ex / W, ey / H], dim=1)
    sq = ((p - g) ** 2).sum(dim=(1, 2, 3))
    return coords, sq, p


def loss_and_grad(logits, target, sigma, law, centred, gcoords=None, gsq=None):
    """Everything the kernels compute, in fp64: dict(coords, sq, p2, g2, dlogits).  logits (BJ, D, H, W) array (fp32 values,
    -inf allowed); gcoords (BJ, ncoord) and gsq (BJ,) the upstream gradients (dlogits only with both)."""
    x = torch.tensor(np.asarray(logits, dtype=np.float64), requires_grad=gcoords is not None)
    BJ, D, H, W = x.shape
    g = torch.from_numpy(dense_target(target, D, H, W, sigma, law, 3 if centred else 2))
    coords, sq, p = head_outputs(x, g, centred)
    out = {"coords": coords.detach().numpy(), "sq": sq.detach().numpy(),
           "p2": (p.detach() ** 2).sum(dim=(1, 2, 3)).numpy(), "g2": (g ** 2).sum(dim=(1, 2, 3)).numpy()}
    if gcoords is not None:
        gc = torch.from_numpy(np.asarray(gcoords, dtype=np.float64))
        gs = torch.from_numpy(np.asarray(gsq, dtype=np.float64))
        ((coords * gc).sum() + (sq * gs).sum()).backward()
        out["dlogits"] = x.grad.numpy()
    return out
