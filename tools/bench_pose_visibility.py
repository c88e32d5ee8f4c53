"""What visibility weights cost in the evaluation: pl.pose_errors and one PoseMetrics.update at B = 4096, J = 17 (15 groups, 31
thresholds) without and with weights=, and the parent commit's calls beside them.

Protocol (that of tools/bench_weight_ema.py): every checkout is measured in a process of its own (one package name, one
library per process), started here one after the other in the order parent, this tree, parent, this tree (--parent-root;
without it: this tree twice).  Inside a process each case warms up, then times --windows windows of back-to-back calls between
a device event pair (the window ends in an event synchronise), the variants of a case (without / with weights) alternating
window by window; a variant's figure is the median window, per call.  The two passes of one checkout give its run-to-run spread
in this session: |difference of the two medians|.  "No weights costs nothing" is judged against the parent's median with the
parent's own spread as the margin; the weighted times are reported as measured.  The figures are those of the Python call
(allocation of the outputs and scratch included), as README's 25.6 us for pose_errors is.

    python tools/bench_pose_visibility.py [--parent-root OTHER_CHECKOUT (built)] [--out profiles/pose_visibility_time.txt]"""
import argparse
import importlib
import inspect
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the table to this file")
ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit, measured in the same session")
ap.add_argument("--root", default=None, help="(worker) checkout whose built package to measure; default: this one, built first")
ap.add_argument("--worker", action="store_true", help="(internal) measure one checkout and print one JSON line")
ap.add_argument("--windows", type=int, default=9)
ap.add_argument("--batch", type=int, default=4096)
args = ap.parse_args()

# (case, calls per window, warm-up calls)
CASES = [("pose_errors", 2000, 200), ("PoseMetrics.update", 1000, 100)]


def worker():
    import torch
    if args.root:
        sys.path.insert(0, os.path.abspath(args.root))
        pkg = importlib.import_module("3d_poseestimation_amd")
    else:
        sys.path.insert(0, HERE)
        import __graft_entry__ as ge
        pkg = ge.build()
    dev = torch.device("cuda", 0)
    B = args.batch
    g = torch.Generator().manual_seed(0)
    tgt = (torch.randn(B, 17, 3, generator=g) * 0.3).to(dev)
    pred = (tgt.cpu() + torch.randn(B, 17, 3, generator=g) * 0.04).to(dev)
    gid = (torch.arange(B) % 15).to(torch.int32).to(dev)
    w = torch.rand(B, 17, generator=g) * 2.0
    w[torch.rand(B, 17, generator=g) < 0.25] = 0.0                 # about a quarter of the joints invisible
    w = w.to(dev)
    weighted = "weights" in inspect.signature(pkg.pose_errors).parameters
    plain = pkg.PoseMetrics(groups=15, device=dev)
    makers = {"pose_errors": [("no weights", lambda: pkg.pose_errors(pred, tgt))],
              "PoseMetrics.update": [("no weights", lambda: plain.update(pred, tgt, gid))]}
    if weighted:
        vis = pkg.PoseMetrics(groups=15, device=dev, visibility=True)
        makers["pose_errors"].append(("weights", lambda: pkg.pose_errors(pred, tgt, weights=w)))
        makers["PoseMetrics.update"].append(("weights", lambda: vis.update(pred, tgt, gid, weights=w)))
    out = {"device": torch.cuda.get_device_name(0), "version": pkg.lib().pl_version(), "cases": {}}
    for name, per_window, warm in CASES:
        steps = makers[name]
        for _, fn in steps:
            for _ in range(warm):
                fn()
        torch.cuda.synchronize()
        times = {v: [] for v, _ in steps}
        for k in range(args.windows):
            for v, fn in (steps if k % 2 == 0 else reversed(steps)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(per_window):
                    fn()
                e1.record()
                e1.synchronize()
                times[v].append(e0.elapsed_time(e1) * 1e3 / per_window)          # us per call
        out["cases"][name] = {v: sorted(t) for v, t in times.items()}
    print("JSON " + json.dumps(out), flush=True)


def run_worker(root):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--windows", str(args.windows), "--batch", str(args.batch)]
    cmd += ["--root", root] if root else []
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("JSON ")]
    if r.returncode != 0 or not lines:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"bench_pose_visibility: the worker for {root or 'this tree'} failed (status {r.returncode})")
    return json.loads(lines[-1][5:])


def main():
    sys.path.insert(0, HERE)
    import __graft_entry__ as ge
    ge.build()
    order = [("parent", args.parent_root), ("this tree", None)] * 2 if args.parent_root else [("this tree", None)] * 2
    passes = {}
    for who, root in order:                       # one process at a time; a failed worker ends the run
        passes.setdefault(who, []).append(run_worker(root))
    first = next(iter(passes.values()))[0]
    lines = [f"{first['device']}; libraries: " + ", ".join(f"{who} version {p[0]['version']}" for who, p in passes.items()),
             f"B = {args.batch}, J = 17, 15 groups, 31 thresholds; weights: uniform in [0, 2) with a quarter of the joints at 0",
             f"us per call (the Python call: allocations and launches): median [min .. max] of {args.windows} windows of back-to-back "
             "calls between a device event pair (calls per window / warm-up calls: " + ", ".join(f"{n}: {k} / {w}" for n, k, w in CASES)
             + "); variants alternate window by window; every checkout in its own process, processes in the order "
             + ", ".join(w for w, _ in order) + "; spread = |difference of the medians of a checkout's two passes|",
             f"{'case':20s} {'checkout, variant':22s} {'pass 1':>28s} {'pass 2':>28s} {'spread':>7s}"]

    def med(t):
        return statistics.median(t)

    for name, _, _ in CASES:
        rows = {}
        for who, (p1, p2) in passes.items():
            for v in p1["cases"][name]:
                t1, t2 = p1["cases"][name][v], p2["cases"][name][v]
                rows[(who, v)] = (med(t1), med(t2))
                lines.append(f"{name:20s} {who + ', ' + v:22s} {med(t1):8.2f} [{t1[0]:7.2f} .. {t1[-1]:7.2f}] "
                             f"{med(t2):8.2f} [{t2[0]:7.2f} .. {t2[-1]:7.2f}] {abs(med(t1) - med(t2)):7.2f}")
        mean = {k: 0.5 * (a + b) for k, (a, b) in rows.items()}
        spread = {k: abs(a - b) for k, (a, b) in rows.items()}
        if ("parent", "no weights") in rows:
            d = mean[("this tree", "no weights")] - mean[("parent", "no weights")]
            lines.append(f"{'':20s} no weights - parent: {d:+.2f} us ({100 * d / mean[('parent', 'no weights')]:+.2f} %); the parent's "
                         f"own spread: {spread[('parent', 'no weights')]:.2f} us")
        if ("this tree", "weights") in rows:
            d = mean[("this tree", "weights")] - mean[("this tree", "no weights")]
            lines.append(f"{'':20s} weights - no weights: {d:+.2f} us ({100 * d / mean[('this tree', 'no weights')]:+.2f} %); spread of "
                         f"no weights / weights: {spread[('this tree', 'no weights')]:.2f} / {spread[('this tree', 'weights')]:.2f} us")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write("python tools/bench_pose_visibility.py" + (" --parent-root <a built checkout of the parent commit>"
                                                               if args.parent_root else "") + f" --out {args.out}\n\n" + text + "\n")


if __name__ == "__main__":
    worker() if args.worker else main()
