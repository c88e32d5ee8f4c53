"""Camera timings on the device: project_poses, its backward, reprojection_errors, reprojection_loss (forward + backward) and
fit_translation at B = 4096 and B = 1 000 000 poses (1 000 sequences of 1 000 frames) of J = 17 joints, four cameras with
cam_ids and a translation, each beside the same result composed from stock torch ops on the same device.  Device events
around windows of calls after a warm-up, the two forms alternated window by window, the median (min .. max) of the windows;
bytes are the least the operation moves (inputs once, outputs once), computed from the shapes.

    python tools/bench_camera.py [--out profiles/camera_time.txt] [--sizes 4096,1000000]

The torch compositions (checked against the library's result before anything is timed) restate csrc/camera.h with
elementwise ops: the projection as written there; its backward and the loss gradient by torch.autograd over that graph; the
fit with batched 3 x 3 normal equations (einsum), torch.linalg.solve and the Jacobian by two autograd passes per step.
"""
import argparse
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--sizes", default="4096,1000000")
ap.add_argument("--windows", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, HERE)
import __graft_entry__ as ge  # noqa: E402

pkg = ge.build()
assert torch.cuda.is_available(), "bench_camera.py measures on the device"
dev = torch.device("cuda", 0)
J = 17
ROWS = torch.tensor([[1145.0494, 1143.7811, 512.5415, 515.4515, -0.2071, 0.2478, -0.0031, -0.0010, -0.0014],
                     [1149.6757, 1147.5917, 508.8486, 508.0649, -0.1942, 0.2404, 0.0068, -0.0016, -0.0027],
                     [1149.1407, 1148.7990, 519.8159, 501.4026, -0.2083, 0.2555, -0.0025, 0.0015, -0.0008],
                     [1145.5114, 1144.7739, 514.9682, 501.8820, -0.1984, 0.2183, -0.0089, -0.0006, -0.0018]])
cams = pkg.CameraTable.from_table(ROWS.numpy()).to(dev)
table = cams.on(dev)
lines = [f"{torch.cuda.get_device_name(0)}, library version {pkg.lib().pl_version()}, J = {J} joints, {len(cams)} cameras with cam_ids, "
         "a translation per pose"]


# ---- the torch compositions ------------------------------------------------------------------------------------------------------
def t_project(X, t, ids):
    r = table[ids.long()]
    fx, fy, cx, cy, k1, k2, k3, p1, p2 = (r[:, i, None] for i in range(9))
    p = X + t[:, None, :]
    x, y = p[..., 0] / p[..., 2], p[..., 1] / p[..., 2]
    r2 = x * x + y * y
    s = 1 + r2 * (k1 + r2 * (k2 + r2 * k3)) + (p1 * x + p2 * y)
    return torch.stack([fx * (x * s + p1 * r2) + cx, fy * (y * s + p2 * r2) + cy], -1)


def t_project_bwd(X, t, ids, duv):
    Xg, tg = X.detach().requires_grad_(True), t.detach().requires_grad_(True)
    return torch.autograd.grad(t_project(Xg, tg, ids), (Xg, tg), duv)


def t_errors(X, t, ids, uv):
    return torch.linalg.vector_norm(t_project(X, t, ids) - uv, dim=-1)


def t_loss(X, t, ids, uv, w):
    Xg, tg = X.detach().requires_grad_(True), t.detach().requires_grad_(True)
    loss = (w * (t_project(Xg, tg, ids) - uv).abs().sum(-1)).sum() / (uv.numel())
    return (loss.detach(),) + torch.autograd.grad(loss, (Xg, tg))


def t_fit(X, ids, uv, w, iters=3):
    r = table[ids.long()]
    vis = (w > 0).to(X.dtype)
    ww = w * vis
    nx, ny = (uv[..., 0] - r[:, 2, None]) / r[:, 0, None], (uv[..., 1] - r[:, 3, None]) / r[:, 1, None]
    rx, ry = nx * X[..., 2] - X[..., 0], ny * X[..., 2] - X[..., 1]
    s = lambda v: (ww * v).sum(-1)                                       # noqa: E731
    o, one = torch.zeros_like(s(nx)), s(torch.ones_like(nx))
    M = torch.stack([torch.stack([one, o, -s(nx)], -1), torch.stack([o, one, -s(ny)], -1),
                     torch.stack([-s(nx), -s(ny), s(nx * nx + ny * ny)], -1)], -2)
    t = torch.linalg.solve(M.double(), torch.stack([s(rx), s(ry), -s(nx * rx + ny * ry)], -1).double()).float()
    for it in range(iters + 1):
        res = uv - t_project(X, t, ids)
        if it == iters:
            break
        Pg = (X + t[:, None, :]).detach().requires_grad_(True)           # the Jacobian d uv / d p, joint by joint
        uvj = t_project(Pg, torch.zeros_like(t), ids)
        ju = torch.autograd.grad(uvj[..., 0].sum(), Pg, retain_graph=True)[0]
        jv = torch.autograd.grad(uvj[..., 1].sum(), Pg)[0]
        Jm = torch.stack([ju, jv], -2).double()
        M = torch.einsum("bj,bjki,bjkl->bil", ww.double(), Jm, Jm)
        g = torch.einsum("bj,bjki,bjk->bi", ww.double(), Jm, res.double())
        t = (t.double() + torch.linalg.solve(M, g)).float()
    rms = torch.sqrt((ww * (res * res).sum(-1)).sum(-1) / ww.sum(-1))
    return t, rms


# ---- timing ----------------------------------------------------------------------------------------------------------------------
def window_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def compare(name, ours, theirs, nbytes, n_ours, n_theirs):
    for _ in range(5):
        ours()
    for _ in range(2):
        theirs()
    a, b = [], []
    for _ in range(args.windows):                                        # alternated: drift falls on both alike
        a.append(window_ms(ours, n_ours))
        b.append(window_ms(theirs, n_theirs))
    ma, mb = statistics.median(a), statistics.median(b)
    lines.append(f"{name:34s} {ma:8.4f} ({min(a):.4f} .. {max(a):.4f})  {nbytes / 2 ** 20:7.1f} MiB {nbytes / ma / 1e6:7.0f} GB/s "
                 f"({100 * nbytes / ma / 1e6 / 6300:4.1f} % of 6300) | torch {mb:9.4f} ({min(b):.4f} .. {max(b):.4f})  x{mb / ma:.1f}")


for B in [int(v) for v in args.sizes.split(",")]:
    g = torch.Generator().manual_seed(B)
    std = torch.from_numpy(pkg.synth.h36m_stats()["std_train_3d"])
    X = torch.randn(B, J, 3, generator=g) * std
    X[:, 0] = 0
    t = torch.stack([torch.rand(B, generator=g) * 1.2 - 0.6, torch.rand(B, generator=g) * 1.2 - 0.6, torch.rand(B, generator=g) * 4 + 3], -1)
    ids = torch.randint(0, 4, (B,), generator=g, dtype=torch.int32)
    w = torch.rand(B, J, generator=g) * 0.95 + 0.05
    w[torch.rand(B, J, generator=g) < 0.1] = 0.0
    duv = torch.randn(B, J, 2, generator=g)
    X, t, ids, w, duv = (v.to(dev) for v in (X, t, ids, w, duv))
    uv = t_project(X, t, ids) + 2.0 * torch.randn(B, J, 2, generator=g).to(dev)
    Xg, tg = X.clone().requires_grad_(True), t.clone().requires_grad_(True)

    # the same results first
    assert torch.allclose(pkg.project_poses(X, cams, ids, translation=t), t_project(X, t, ids), rtol=1e-6, atol=2e-4)
    ours = torch.autograd.grad(pkg.project_poses(Xg, cams, ids, translation=tg), (Xg, tg), duv)
    for a, b in zip(ours, t_project_bwd(X, t, ids, duv)):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-3 * float(b.abs().max())), "the torch composition of the backward disagrees"
    assert torch.allclose(pkg.reprojection_errors(X, uv, cams, ids, translation=t), t_errors(X, t, ids, uv), rtol=1e-4, atol=2e-4)
    lo = pkg.reprojection_loss(Xg, uv, cams, ids, translation=tg, weights=w)
    ours = (lo.detach(),) + torch.autograd.grad(lo, (Xg, tg))
    for a, b in zip(ours, t_loss(X, t, ids, uv, w)):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-3 * float(b.abs().max())), "the torch composition of the loss disagrees"
    ft, frms = pkg.fit_translation(X, uv, cams, ids, weights=w)
    tt, trms = t_fit(X, ids, uv, w)
    assert torch.allclose(ft, tt, rtol=1e-4, atol=1e-4) and torch.allclose(frms, trms, rtol=1e-3, atol=1e-3), "the fits disagree"
    lines.append(f"B = {B}: fitted translation against the one projected from, mean |t - t0| {float((ft - t).abs().mean()):.4f} m "
                 f"(2 px of noise on the target), mean rms {float(frms.mean()):.3f} px")
    del ours, tt, trms

    def loss_ours():
        lo = pkg.reprojection_loss(Xg, uv, cams, ids, translation=tg, weights=w)
        return torch.autograd.grad(lo, (Xg, tg))

    def bwd_ours(uvp=pkg.project_poses(Xg, cams, ids, translation=tg)):
        return torch.autograd.grad(uvp, (Xg, tg), duv, retain_graph=True)
    n = B * J
    big = B > 100000
    no, nt = (20, 3) if big else (200, 20)
    lines.append(f"B = {B}: ms per call (allocation of the outputs + the launches): median (min .. max) of {args.windows} windows of {no} "
                 f"calls; least bytes moved; GB/s (the README's 6300 sustainable) | the torch composition: windows of {nt} calls; its "
                 "time over ours")
    compare("project_poses", lambda: pkg.project_poses(X, cams, ids, translation=t), lambda: t_project(X, t, ids), n * 20 + B * 16, no, nt)
    compare("project_poses backward", bwd_ours, lambda: t_project_bwd(X, t, ids, duv), n * 32 + B * 28, no, nt)
    compare("reprojection_errors", lambda: pkg.reprojection_errors(X, uv, cams, ids, translation=t), lambda: t_errors(X, t, ids, uv),
            n * 24 + B * 16, no, nt)
    compare("reprojection_loss fwd + bwd, l1", loss_ours, lambda: t_loss(X, t, ids, uv, w), n * 36 + B * 28, no, nt)
    compare("fit_translation, iters = 3", lambda: pkg.fit_translation(X, uv, cams, ids, weights=w), lambda: t_fit(X, ids, uv, w),
            n * 24 + B * 20, no, max(1, nt // 3))
    del X, t, ids, w, duv, uv, Xg, tg
    torch.cuda.empty_cache()

text = "\n".join(lines)
print(text)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(f"python tools/bench_camera.py --out {args.out}\n\n{text}\n")
