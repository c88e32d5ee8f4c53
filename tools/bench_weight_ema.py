"""What the averaged (EMA) weights cost: the training step with ema_decay off and on, and the parent commit's step beside them.

Cases: the f16x3 lifter LinearModel(34, 51, 1024) + FlatAdamW at B = 4096 (eager), B = 64 (eager) and B = 64 as GraphedTrainStep
replays; Model_3D + FlatAdam at B = 32 frames of 256 x 256.

Protocol: every checkout is measured in a process of its own (one package name, one library per process), started here one after
the other in the order parent, this tree, parent, this tree (--parent-root; without it: this tree twice).  Inside a process each
case warms up, then times --windows windows of back-to-back steps between a device event pair (the window ends in an event
synchronise), the variants of a case (off / on) alternating window by window; a variant's figure is the median window, per
step.  The two passes of one checkout give its run-to-run spread in this session: |difference of the two medians|.  "Off costs
nothing" is judged against the parent's median with the parent's own spread as the margin; the on-cost is reported as measured.

    python tools/bench_weight_ema.py [--parent-root OTHER_CHECKOUT (built)] [--out profiles/weight_ema_time.txt]"""
import argparse
import importlib
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
ap.add_argument("--skip-conv", action="store_true", help="without the Model_3D case")
args = ap.parse_args()

# (case, steps per window, warm-up steps)
CASES = [("lifter B=4096 eager", 300, 50), ("lifter B=64 eager", 2000, 200), ("lifter B=64 graph replay", 2000, 200),
         ("Model_3D B=32 FlatAdam", 20, 5)]


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
    import inspect
    has_ema = "ema_decay" in inspect.signature(pkg.FlatAdamW.__init__).parameters
    variants = [("off", {})] + ([("on", dict(ema_decay=0.999))] if has_ema else [])

    def lifter(B, graph, kw):
        torch.manual_seed(0)
        m = pkg.LinearModel(34, 51, linear_size=1024, num_stage=2, p_dropout=0.5, compute_dtype="f16x3").to(dev).train()
        opt = pkg.FlatAdamW(m, lr=1e-4, **kw)
        x, y = pkg.synth.synthetic_batch(B, 1234, dev)
        if graph:
            step = pkg.GraphedTrainStep(m, opt, x, y)
            xi, yi = step.inputs
            return lambda: step(xi, yi)
        return lambda: pkg.train_step(m, opt, x, y)

    def conv(kw):
        m = pkg.Model_3D().train()
        m.load_state_dict(pkg.synth.seeded_state(m.state_dict(), 31))
        with torch.no_grad():
            m.final_layer.weight.mul_(1e-3)
        m = m.to(dev)
        opt = pkg.FlatAdam(m, lr=1e-4, **kw)
        frames = pkg.synth.seeded_frames(32, 7, 256).to(dev)
        target = torch.randn(32, 51, generator=torch.Generator().manual_seed(8)).to(dev)

        def step():
            opt.zero_grad(set_to_none=True)
            torch.nn.functional.mse_loss(m.predict_nhwc(frames).reshape(32, 51), target).backward()
            opt.step()
        return step

    makers = {"lifter B=4096 eager": lambda kw: lifter(4096, False, kw), "lifter B=64 eager": lambda kw: lifter(64, False, kw),
              "lifter B=64 graph replay": lambda kw: lifter(64, True, kw), "Model_3D B=32 FlatAdam": conv}
    out = {"device": torch.cuda.get_device_name(0), "version": pkg.lib().pl_version(), "cases": {}}
    for name, per_window, warm in CASES:
        if args.skip_conv and name.startswith("Model_3D"):
            continue
        steps = [(v, makers[name](kw)) for v, kw in variants]
        for _, fn in steps:
            for _ in range(warm):
                fn()
        torch.cuda.synchronize()
        times = {v: [] for v, _ in steps}
        for w in range(args.windows):
            for v, fn in (steps if w % 2 == 0 else reversed(steps)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(per_window):
                    fn()
                e1.record()
                e1.synchronize()
                times[v].append(e0.elapsed_time(e1) * 1e3 / per_window)          # us per step
        out["cases"][name] = {v: sorted(t) for v, t in times.items()}
        del steps
        torch.cuda.empty_cache()
    print("JSON " + json.dumps(out), flush=True)


def run_worker(root):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--windows", str(args.windows)]
    cmd += ["--root", root] if root else []
    cmd += ["--skip-conv"] if args.skip_conv else []
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("JSON ")]
    if r.returncode != 0 or not lines:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"bench_weight_ema: the worker for {root or 'this tree'} failed (status {r.returncode})")
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
             f"us per training step: median [min .. max] of {args.windows} windows of back-to-back steps between a device event pair "
             "(steps per window / warm-up steps: " + ", ".join(f"{n}: {k} / {w}" for n, k, w in CASES) + "); variants alternate "
             "window by window; every checkout in its own process, processes in the order " + ", ".join(w for w, _ in order)
             + "; spread = |difference of the medians of a checkout's two passes|",
             f"{'case':26s} {'checkout, ema':18s} {'pass 1':>30s} {'pass 2':>30s} {'spread':>8s}"]

    def med(t):
        return statistics.median(t)

    for name, _, _ in CASES:
        if name not in first["cases"]:
            continue
        rows = {}
        for who, (p1, p2) in passes.items():
            for v in p1["cases"][name]:
                t1, t2 = p1["cases"][name][v], p2["cases"][name][v]
                rows[(who, v)] = (med(t1), med(t2))
                lines.append(f"{name:26s} {who + ', ' + v:18s} {med(t1):10.1f} [{t1[0]:8.1f} .. {t1[-1]:8.1f}] "
                             f"{med(t2):10.1f} [{t2[0]:8.1f} .. {t2[-1]:8.1f}] {abs(med(t1) - med(t2)):8.1f}")
        mean = {k: 0.5 * (a + b) for k, (a, b) in rows.items()}
        spread = {k: abs(a - b) for k, (a, b) in rows.items()}
        if ("parent", "off") in rows:
            d = mean[("this tree", "off")] - mean[("parent", "off")]
            lines.append(f"{'':26s} off - parent: {d:+.1f} us ({100 * d / mean[('parent', 'off')]:+.2f} %); the parent's own spread: "
                         f"{spread[('parent', 'off')]:.1f} us")
        if ("this tree", "on") in rows:
            d = mean[("this tree", "on")] - mean[("this tree", "off")]
            lines.append(f"{'':26s} on - off: {d:+.1f} us ({100 * d / mean[('this tree', 'off')]:+.2f} %); spread of off / on: "
                         f"{spread[('this tree', 'off')]:.1f} / {spread[('this tree', 'on')]:.1f} us")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write("python tools/bench_weight_ema.py" + (" --parent-root <a built checkout of the parent commit>" if args.parent_root
                                                          else "") + f" --out {args.out}\n\n" + text + "\n")


if __name__ == "__main__":
    worker() if args.worker else main()
