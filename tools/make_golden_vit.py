#!/usr/bin/env python3
"""Generate tests/golden/g12_vit.npz by running the REFERENCE MyViT on CPU.

Build-container only, like make_golden.py: imports phase1_lifting/baselineModel.py of the reference checkout as-is
(never copied) and records inputs and what the reference computed as data.  Initial weights are the seeded construction
(torch.manual_seed(seed) before MyViT(...)): the fixture stores samples of them to pin that recipe, plus the full
pos_embed.  Large tensors are stored as fixed samples of their elements (sorted flat indices + values).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_vit.py
"""
import os
import sys
import warnings

import numpy as np

warnings.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
REF = os.environ.get("POSELIFT_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "phase1_lifting"))
sys.dont_write_bytecode = True

import torch  # noqa: E402

import baselineModel as ref  # noqa: E402  (the reference, imported as-is)
from make_golden import h36m_stats, synth_batch  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)
SAMPLES = 256


def _idx(rng, n):
    return np.arange(n, dtype=np.int64) if n <= SAMPLES else np.sort(rng.choice(n, size=SAMPLES, replace=False)).astype(np.int64)


def _record(rec, prefix, tensors, rng, idx=None):
    """Sampled elements of every tensor: prefix:idx:<key>, prefix:val:<key>; idx reused when given."""
    idx = {} if idx is None else idx
    for k, v in tensors.items():
        flat = v.detach().cpu().numpy().reshape(-1)
        if k not in idx:
            idx[k] = _idx(rng, flat.size)
        rec[f"{prefix}:idx:{k}"] = idx[k]
        rec[f"{prefix}:val:{k}"] = flat[idx[k]]
    return idx


def fwd_bwd(model, x, t):
    model.zero_grad()
    y = model(x)
    loss = torch.nn.MSELoss(reduction="mean")(y, t)
    loss.backward()
    return y.detach(), loss.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def config(rec, tag, seed, chw, out_d, B, x, t, rng, adam_steps=0):
    torch.manual_seed(seed)
    m = ref.MyViT(chw=chw, out_d=out_d)
    init = {k: v.detach().clone() for k, v in m.state_dict().items()}
    rec[f"{tag}:seed"] = seed
    rec[f"{tag}:x"], rec[f"{tag}:t"] = x, t
    rec[f"{tag}:keys"] = np.array(list(init.keys()))
    rec[f"{tag}:shapes"] = np.array([",".join(str(s) for s in v.shape) for v in init.values()])
    rec[f"{tag}:trainable"] = np.array([k for k, p in m.named_parameters() if p.requires_grad])
    idx = _record(rec, f"{tag}:init", {k: v for k, v in init.items() if k != "pos_embed"}, rng)
    rec[f"{tag}:pos_embed"] = init["pos_embed"].numpy()
    m64 = ref.MyViT(chw=chw, out_d=out_d).double()
    m64.load_state_dict({k: v.double() for k, v in init.items()})
    xt, tt = torch.from_numpy(x), torch.from_numpy(t)
    y32, l32, g32 = fwd_bwd(m, xt, tt)
    y64, l64, g64 = fwd_bwd(m64, xt.double(), tt.double())
    rec[f"{tag}:y"], rec[f"{tag}:y_fp64"] = y32.numpy(), y64.numpy()
    rec[f"{tag}:loss"], rec[f"{tag}:loss_fp64"] = np.float32(l32), np.float64(l64)
    _record(rec, f"{tag}:grad64", g64, rng, idx)
    for k, v in g64.items():
        rec[f"{tag}:gmax64:{k}"] = np.float64(v.abs().max())
    if adam_steps:
        opt = torch.optim.AdamW(m.parameters(), lr=1e-4)
        losses = []
        for _ in range(adam_steps):
            opt.zero_grad()
            loss = torch.nn.MSELoss(reduction="mean")(m(xt), tt)
            loss.backward()
            opt.step()
            losses.append(float(loss))
        rec[f"{tag}:adam_losses"] = np.array(losses, dtype=np.float32)
        rec[f"{tag}:adam_lr"] = np.float32(1e-4)
        _record(rec, f"{tag}:adam", {k: v for k, v in m.state_dict().items()}, rng, idx)


def main():
    stats = h36m_stats()
    rng = np.random.default_rng(1201)
    rec = {}
    x, t = synth_batch(np.random.default_rng(1202), 64, stats)            # 2-D keypoints -> 3-D pose (train_1.py)
    config(rec, "lift", 0, (1, 17, 2), 3, 64, x, t, rng, adam_steps=3)
    x2, t2 = synth_batch(np.random.default_rng(1203), 16, stats)          # phase5 projector: 3-D pose -> 2-D keypoints
    config(rec, "proj", 1, (1, 17, 3), 2, 16, t2, x2, rng)
    path = os.path.join(OUT, "g12_vit.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
