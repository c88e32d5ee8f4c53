"""Cost of gradient-norm clipping / non-finite skip in the flat optimizers (gradclip.py): the norm pass alone, and whole
training steps with clipping off and on, beside the parent commit's library in the same run.

    python tools/bench_grad_clip.py [--parent-lib PATH] [--rounds 5] [--out profiles/grad_clip_time.txt]

Every round starts one fresh worker process per library (this build; --parent-lib: another build of libposelift.so, the
parent commit's, loaded through POSELIFT_LIB), alternating, and each worker times every case with device events around
`iters` steps after a warm-up.  Reported: the median over the rounds and the spread (min .. max).
Cases: lifter (1024 wide, f16x3, dropout 0.5) train_step at B = 4096 and B = 64 eager, B = 64 as a GraphedTrainStep, and
Model_3D (f16x3, FlatAdam) at B = 32; "sep" is B = 64 without clipping but with AdamW as its own launch (what clipping
also pays there: the update no longer rides in the backward launches).
The norm pass is compared with bytes / 6.3 TB/s, the streaming rate an MI355X reaches on a float4 copy."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEW_SYMBOLS = ("pl_grad_norm_scratch_bytes", "pl_grad_norm_clip", "pl_adamw_flat_clip", "pl_adamw_flat_dev_clip",
               "pl_adamw_flat_planes_clip")
STREAM_BYTES_PER_S = 6.3e12
CLIP = dict(max_grad_norm=1.0, skip_nonfinite=True)


def _time(step, iters, warm=3):
    import torch
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def worker(is_parent):
    import torch
    pkg = importlib.import_module("3d_poseestimation_amd")
    if is_parent:                                       # the parent's library has no clipping entry points: only "off" cases
        for name in NEW_SYMBOLS:
            pkg._lib.SIGNATURES.pop(name)
    dev = torch.device("cuda", 0)
    out = {}

    def lifter(B, **kw):
        torch.manual_seed(0)
        m = pkg.LinearModel(34, 51, linear_size=1024, p_dropout=0.5, compute_dtype="f16x3").to(dev).train()
        return m, pkg.FlatAdamW(m, lr=1e-4, **kw), pkg.synth.synthetic_batch(B, 1, dev)

    variants = [("off", {})] + ([] if is_parent else [("on", CLIP)])
    for tag, kw in variants:
        m, opt, (x, y) = lifter(4096, **kw)
        out[f"lifter B=4096 eager {tag}"] = _time(lambda: pkg.train_step(m, opt, x, y), 50)
        m, opt, (x, y) = lifter(64, **kw)
        out[f"lifter B=64 eager {tag}"] = _time(lambda: pkg.train_step(m, opt, x, y), 200, warm=10)
        m, opt, (x, y) = lifter(64, **kw)
        step = pkg.GraphedTrainStep(m, opt, x, y)
        out[f"lifter B=64 graphed {tag}"] = _time(lambda: step(x, y), 500, warm=10)
    m, opt, (x, y) = lifter(64)
    x2, y2 = x.reshape(64, -1).contiguous(), y.reshape(64, -1).contiguous()

    def sep():
        m.fused_train_fwd_bwd(x2, y2)
        opt.step()
    out["lifter B=64 eager sep"] = _time(sep, 200, warm=10)

    m3 = pkg.Model_3D().train()
    m3.load_state_dict(pkg.synth.seeded_state(m3.state_dict(), 31))
    with torch.no_grad():
        m3.final_layer.weight.mul_(1e-3)
    m3 = m3.to(dev)
    m3.compute_dtype = m3.preact.compute_dtype = "f16x3"
    frames, target = pkg.synth.seeded_frames(32, 5).to(dev), torch.randn(32, 51, device=dev)
    for tag, kw in variants:
        o3 = pkg.FlatAdam(m3, lr=1e-5, **kw)

        def step3():
            o3.zero_grad()
            pkg.mse_loss(m3(frames), target).backward()
            o3.step()
        out[f"Model_3D B=32 eager {tag}"] = _time(step3, 8, warm=2)
    if not is_parent:
        for name, n in (("lifter arena", 4296755), ("Model_3D arena", o3.arena.numel)):
            g = torch.randn(n, device=dev) * 1e-3
            clip = pkg.gradclip.GradClip(dev)
            out[f"norm pass {name}"] = _time(lambda: clip.launch(g, [(0, n)], 1.0, 1.0, True), 500, warm=10)
            out[f"floats {name}"] = n
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", choices=["this", "parent"], default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker == "parent")
    libs = ["this"] + (["parent"] if args.parent_lib else [])
    res = {k: [] for k in libs}
    for r in range(args.rounds):
        for k in (libs if r % 2 == 0 else libs[::-1]):  # alternating, and the order too: one fresh process per library and round
            env = dict(os.environ)
            if k == "parent":
                env["POSELIFT_LIB"] = os.path.abspath(args.parent_lib)
            else:
                env.pop("POSELIFT_LIB", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", k], env=env, capture_output=True,
                               text=True, timeout=600)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"worker {k} failed in round {r} (exit {p.returncode})")
            res[k].append(json.loads(line[0][7:]))
            print(f"round {r} {k}: done", flush=True)
    cmd = "python tools/bench_grad_clip.py" + (" --parent-lib <the parent commit's libposelift.so>" if args.parent_lib else "") \
        + f" --rounds {args.rounds}"
    lines = [cmd, "", "times in ms per step: median over the rounds (min .. max); one fresh process per library and round, alternating", ""]

    def stat(k, name):
        v = [r[name] for r in res[k] if name in r]
        return (statistics.median(v), min(v), max(v)) if v else None

    names = [n for n in res["this"][0] if not n.startswith(("norm pass", "floats"))]
    lines.append(f"{'case':<30} {'this build':>28} {'parent build':>28}")
    for n in names:
        row = f"{n:<30}"
        for k in ("this", "parent"):
            s = stat(k, n) if k in res else None
            row += f" {'%9.4f (%8.4f .. %8.4f)' % s if s else '-':>28}"
        lines.append(row)
    lines.append("")
    for case in ("lifter B=4096 eager", "lifter B=64 eager", "lifter B=64 graphed", "Model_3D B=32 eager"):
        off, on = stat("this", case + " off")[0], stat("this", case + " on")[0]
        note = f"{case}: clipping on costs {1e3 * (on - off):+.1f} us ({100 * (on / off - 1):+.2f} %)"
        if "parent" in res:
            par = stat("parent", case + " off")
            note += (f"; off vs parent {100 * (off / par[0] - 1):+.2f} % (parent's own spread "
                     f"{100 * (par[1] / par[0] - 1):+.2f} .. {100 * (par[2] / par[0] - 1):+.2f} %)")
        lines.append(note)
    off, sep_, on = (stat("this", "lifter B=64 eager " + t)[0] for t in ("off", "sep", "on"))
    lines.append(f"lifter B=64 eager: AdamW as its own launch instead of riding in the backward launches {1e3 * (sep_ - off):+.1f} us "
                 f"of the {1e3 * (on - off):+.1f} us; the norm pass and the record {1e3 * (on - sep_):+.1f} us")
    lines.append("")
    for name in ("lifter arena", "Model_3D arena"):
        med, lo, hi = stat("this", "norm pass " + name)
        n = res["this"][0]["floats " + name]
        ideal = 4.0 * n / STREAM_BYTES_PER_S * 1e3
        lines.append(f"norm pass, {name} ({n} floats, {4 * n / 1e6:.1f} MB), two launches back to back: {1e3 * med:.2f} us "
                     f"({1e3 * lo:.2f} .. {1e3 * hi:.2f}); bytes / 6.3 TB/s = {1e3 * ideal:.2f} us; ratio {med / ideal:.2f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
