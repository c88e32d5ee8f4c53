"""Video-track timings on the device: prepare_tracks, filter_tracks (K = 7 and K = 65, D = 3) and velocity_errors on
T = 1 000 000 frames of 17 joints in 1 000 sequences of 1 000 frames, each beside the same result composed from stock torch
ops on the same device.  Device events around windows of calls after a warm-up, the two forms alternated window by window,
the median (min .. max) of the windows; bytes are the least the operation moves, computed from the shapes.

    python tools/bench_track.py [--out profiles/track_time.txt] [--frames 1000000]

The torch compositions (checked against the library's result before anything is timed):
  prepare   index-select remap with midpoints, division, validity, the previous / next valid frame of every joint by
            cummax / cummin over frame indices, gathers, lerp and selects
  filter    the sequences as the batch dimension of F.conv1d (groups = columns, zero padding = the sequence boundary) of
            w x and of w, a division, and a select for empty windows
  velocity  differences of shifted views, a norm, the sequence mask
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as Fn

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--frames", type=int, default=1_000_000)
ap.add_argument("--windows", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, HERE)
import __graft_entry__ as ge  # noqa: E402

pkg = ge.build()
assert torch.cuda.is_available(), "bench_track.py measures on the device"
dev = torch.device("cuda", 0)
T, L = args.frames, 1000
assert T % L == 0
S, G = T // L, 8
lines = [f"{torch.cuda.get_device_name(0)}, library version {pkg.lib().pl_version()}, T = {T} frames of 17 joints in {S} sequences"]

g = torch.Generator().manual_seed(0)
det = torch.empty(T, 17, 3)
det[..., :2] = torch.rand(T, 17, 2, generator=g) * 1000
det[..., 2] = torch.rand(T, 17, generator=g) * 0.8 + 0.2
low = torch.rand(T, 17, generator=g) < 0.02
for k in range(1, 4):                                                    # runs: about one joint in ten below the threshold
    low[k:] |= low[:-k] & (torch.rand(T - k, 17, generator=g) < 0.6)
det[..., 2][low] = 0.05
det[torch.rand(T, generator=g) < 0.004] = 0.0
det = det.to(dev)
seq = torch.arange(T, dtype=torch.int32).div(L, rounding_mode="floor").to(dev)
DIV = (1000.0, 1002.0)

# ---- the torch compositions ------------------------------------------------------------------------------------------------------
SRC_A = torch.tensor([11, 12, 14, 16, 11, 13, 15, 0, 5, 0, 1, 5, 7, 9, 6, 8, 10], device=dev)
SRC_B = torch.tensor([12, 12, 14, 16, 11, 13, 15, 0, 6, 0, 2, 5, 7, 9, 6, 8, 10], device=dev)
t_idx = torch.arange(T, device=dev)
change = torch.ones(T, dtype=torch.bool, device=dev)
change[1:] = seq[1:] != seq[:-1]
start = torch.where(change, t_idx, torch.zeros_like(t_idx)).cummax(0).values
last = torch.ones(T, dtype=torch.bool, device=dev)
last[:-1] = change[1:]
end = torch.where(last, t_idx, torch.full_like(t_idx, T)).flip(0).cummin(0).values.flip(0)


def torch_prepare(det):
    a, b = det[:, SRC_A], det[:, SRC_B]
    h = torch.cat([(a[..., :2] + b[..., :2]) * 0.5, torch.minimum(a[..., 2:], b[..., 2:])], dim=-1)
    h[:, 7, :2] = (h[:, 0, :2] + h[:, 8, :2]) * 0.5
    h[:, 7, 2] = torch.minimum(h[:, 0, 2], h[:, 8, 2])
    s = h[..., :2] / torch.tensor(DIV, device=dev)
    conf = h[..., 2]
    valid = (conf >= 0.1) & torch.isfinite(s).all(-1)
    tt = t_idx[:, None]
    prev = torch.where(valid, tt, torch.full_like(tt, -1)).cummax(0).values
    nxt = torch.where(valid, tt, torch.full_like(tt, 2 * T)).flip(0).cummin(0).values.flip(0)
    da, db = tt - prev, nxt - tt
    has_a, has_b = (prev >= start[:, None]) & (da <= G), (nxt <= end[:, None]) & (db <= G)
    left_a, left_b = (tt - start[:, None]) < G, (end[:, None] - tt) < G
    pa, pb = prev.clamp(0, T - 1), nxt.clamp(0, T - 1)
    sa, sb = torch.gather(s, 0, pa[..., None].expand(-1, -1, 2)), torch.gather(s, 0, pb[..., None].expand(-1, -1, 2))
    ca, cb = torch.gather(conf, 0, pa), torch.gather(conf, 0, pb)
    interp = ~valid & has_a & has_b & (da + db - 1 <= G)
    held_a, held_b = ~valid & has_a & ~has_b & left_b, ~valid & has_b & ~has_a & left_a
    frac = (da.float() / (da + db).float())[..., None]
    own = torch.where(torch.isfinite(s), s, torch.zeros_like(s))
    xy = torch.where(valid[..., None], s, torch.where(interp[..., None], sa + (sb - sa) * frac,
                     torch.where(held_a[..., None], sa, torch.where(held_b[..., None], sb, own))))
    w = torch.where(valid, conf, torch.where(interp, 0.5 * torch.minimum(ca, cb),
                    torch.where(held_a, 0.5 * ca, torch.where(held_b, 0.5 * cb, torch.zeros_like(conf)))))
    state = torch.where(valid, 0, torch.where(interp, 1, torch.where(held_a | held_b, 2, 3))).to(torch.uint8)
    return xy, w, state


def torch_filter(x, w, taps):
    K, C = taps.numel(), x.shape[1] * x.shape[2]
    wx = (x * w[..., None]).reshape(S, L, C).transpose(1, 2)
    ww = w.reshape(S, L, 17).transpose(1, 2)
    num = Fn.conv1d(wx, taps.view(1, 1, K).expand(C, 1, K), padding=K // 2, groups=C)
    den = Fn.conv1d(ww, taps.view(1, 1, K).expand(17, 1, K), padding=K // 2, groups=17)
    num, den = num.transpose(1, 2).reshape(T, 17, -1), den.transpose(1, 2).reshape(T, 17, 1)
    return torch.where(den > 0, num / den, x)


def torch_velocity(p, q):
    d = (p[1:] - p[:-1]) - (q[1:] - q[:-1])
    ok = seq[1:] == seq[:-1]
    err = torch.zeros(T, 17, device=dev)
    err[1:] = torch.where(ok[:, None], d.norm(dim=-1), torch.zeros((), device=dev))
    cnt = torch.zeros(T, dtype=torch.uint8, device=dev)
    cnt[1:] = ok
    return err, cnt


# ---- the same results first ------------------------------------------------------------------------------------------------------
xy, w, state = pkg.prepare_tracks(det, "coco17", DIV, 0.1, G, 0.5, seq)
txy, tw, tstate = torch_prepare(det)
assert torch.equal(state, tstate), "the torch composition of prepare disagrees on the states"
assert torch.allclose(xy, txy, rtol=1e-6, atol=1e-6) and torch.allclose(w, tw, rtol=1e-6, atol=1e-7)
counts = torch.bincount(state.reshape(-1).long(), minlength=4).tolist()
lines.append(f"states of the {T * 17} joints: valid {counts[0]}, interpolated {counts[1]}, held {counts[2]}, lost {counts[3]}")
pose = torch.randn(T, 17, 3, generator=g).to(dev)
tgt = pose + 0.01 * torch.randn(T, 17, 3, generator=g).to(dev)
filters = {K: pkg.TemporalFilter.gaussian(K / 6.0, radius=K // 2) for K in (7, 65)}
for K, f in filters.items():
    a, b = pkg.filter_tracks(pose, f, w, seq), torch_filter(pose, w, torch.from_numpy(f.taps).to(dev))
    assert torch.allclose(a, b, rtol=1e-4, atol=1e-5), f"the torch composition of the filter disagrees at K = {K}"
e, c = pkg.velocity_errors(pose, tgt, seq, 1)
te, tc = torch_velocity(pose, tgt)
assert torch.equal(c, tc) and torch.allclose(e, te, rtol=1e-5, atol=1e-6)
del txy, tw, tstate, a, b, te, tc


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


def compare(name, ours, theirs, nbytes, n_ours=50, n_theirs=5):
    for _ in range(5):
        ours()
    for _ in range(2):
        theirs()
    a, b = [], []
    for _ in range(args.windows):                                        # alternated: drift falls on both alike
        a.append(window_ms(ours, n_ours))
        b.append(window_ms(theirs, n_theirs))
    ma, mb = statistics.median(a), statistics.median(b)
    lines.append(f"{name:28s} {ma:8.3f} ({min(a):.3f} .. {max(a):.3f})  {nbytes / 2 ** 20:6.0f} MiB {nbytes / ma / 1e6:7.0f} GB/s "
                 f"({100 * nbytes / ma / 1e6 / 6300:4.1f} % of 6300) | torch {mb:8.3f} ({min(b):.3f} .. {max(b):.3f})  x{mb / ma:.1f}")


lines.append(f"ms per call (allocation of the outputs + one launch): median (min .. max) of {args.windows} windows of 50 calls; least bytes "
             "moved; GB/s (the README's 6300 sustainable) | the torch composition: windows of 5 calls; its time over ours")
compare("prepare_tracks G = 8", lambda: pkg.prepare_tracks(det, "coco17", DIV, 0.1, G, 0.5, seq), lambda: torch_prepare(det),
        T * (204 + 4 + 136 + 68 + 17))
for K, f in filters.items():
    taps = torch.from_numpy(f.taps).to(dev)
    compare(f"filter_tracks K = {K}, D = 3", lambda f=f: pkg.filter_tracks(pose, f, w, seq), lambda taps=taps: torch_filter(pose, w, taps),
            T * (204 + 68 + 4 + 204))
compare("velocity_errors order 1", lambda: pkg.velocity_errors(pose, tgt, seq, 1), lambda: torch_velocity(pose, tgt),
        T * (2 * 204 + 4 + 68 + 1))
text = "\n".join(lines)
print(text)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(f"python tools/bench_track.py --out {args.out}\n\n{text}\n")
