"""numpy twin of the flat optimizers' gradient clipping and non-finite skip.  TEST INFRASTRUCTURE ONLY.

What the device does (csrc/gradnorm.hip, csrc/adamw.h), restated on the host:
  grad_norm    |grad_scale| * sqrt(sum of g^2 over the given [lo, hi) ranges), the sum in fp64, rounded to fp32 once
  clip_coef    torch's fp32 coefficient: min(1, max_norm / (norm + 1e-6)), a NaN staying a NaN
  ClipAdamW    torch.optim.AdamW / Adam (weight_decay 0) in fp32, single-tensor update order, over a flat arena; a
               non-finite norm with skip_nonfinite = "do not step, do not count"
"""
import numpy as np

F = np.float32


def grad_norm(g, ranges=None, grad_scale=1.0):
    g = np.asarray(g, np.float32).reshape(-1)
    ranges = [(0, g.size)] if ranges is None else ranges
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.float64(0.0)
        for lo, hi in ranges:
            x = g[lo:hi].astype(np.float64)
            s = s + np.sum(x * x)
        return F(abs(np.float64(F(grad_scale))) * np.sqrt(s))


def clip_coef(norm, max_norm):
    if max_norm is None:
        return F(1.0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        c = F(max_norm) / (F(norm) + F(1e-6))
    return F(1.0) if c > F(1.0) else F(c)


def adamw_update(p, g, m, v, t, lr, b1, b2, eps, wd, gscale):
    """One update of fp32 arrays in the order of adamw_one(); t is the 1-based count of TAKEN steps."""
    lr, b1, b2, wd = (float(F(x)) for x in (lr, b1, b2, wd))   # the C ABI takes them as fp32; the constants are formed in fp64
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        g = g * F(gscale)
        p = p * F(1.0 - lr * wd)
        m = m + (g - m) * F(1.0 - b1)
        v = v * F(b2) + (F(1.0 - b2) * g) * g
        denom = np.sqrt(v) / F(np.sqrt(1.0 - b2 ** t)) + F(eps)
        p = p - F(lr / (1.0 - b1 ** t)) * (m / denom)
    return p.astype(np.float32), m.astype(np.float32), v.astype(np.float32)


class ClipAdamW:
    """State over one flat fp32 arena; ranges = the [lo, hi) runs that hold a gradient in this step (None: all)."""

    def __init__(self, p, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, skip_nonfinite=False):
        self.p = np.array(p, np.float32).reshape(-1)
        self.m, self.v = np.zeros_like(self.p), np.zeros_like(self.p)
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.max_grad_norm, self.skip_nonfinite = max_grad_norm, skip_nonfinite
        self.t = self.skipped = 0
        self.norm = self.coef = None

    def step(self, g, ranges=None, grad_scale=1.0):
        g = np.asarray(g, np.float32).reshape(-1)
        ranges = [(0, g.size)] if ranges is None else ranges
        self.norm = grad_norm(g, ranges, grad_scale)
        self.coef = clip_coef(self.norm, self.max_grad_norm)
        if self.skip_nonfinite and not np.isfinite(self.norm):
            self.skipped += 1
            return False
        self.t += 1
        gscale = F(grad_scale) * self.coef                      # one fp32 product, as the kernel forms it
        for lo, hi in ranges:
            self.p[lo:hi], self.m[lo:hi], self.v[lo:hi] = adamw_update(
                self.p[lo:hi], g[lo:hi], self.m[lo:hi], self.v[lo:hi], self.t, self.lr, self.betas[0], self.betas[1],
                self.eps, self.wd, gscale)
        return True
