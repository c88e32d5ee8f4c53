"""Per-pose joint weights under the scratch guard of tests/test_gpu_scratch_independence.py: the weights gather, the feeder's
weights, the stand-alone criterion and the fused steps with row_weights give the same bits whatever workspace, scratch and
fresh outputs held.  The case is registered in that module's REG, so its closure test (every __global__ function of csrc/
is launched by some case) sees row_weights_gather_kernel: collect both files together, as the whole suite does."""
import pytest
import torch

import row_weights_oracle as orc
import test_gpu_scratch_independence as sgi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASE = "row weights"
KINDS = ("mse", "l1", "smooth_l1", "mpjpe")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


def _row_weights_run(pkg):
    g = torch.Generator().manual_seed(21)
    n = 40
    x2d, y3d = torch.rand(n, 17, 2, generator=g) * 0.6 + 0.2, torch.randn(n, 17, 3, generator=g) * 0.3
    table = torch.from_numpy(orc.weights(n, 17, seed=4))
    aug = pkg.PoseAugment(p_flip=0.5, max_rot=0.3, scale_range=0.2, max_shift=0.05, jitter_sigma=0.01, seed=99)
    p, t = (torch.randn(65, 51, generator=g) * 0.3).to(DEV), (torch.randn(65, 51, generator=g) * 0.3).to(DEV)
    rw = torch.from_numpy(orc.weights(65, 17, seed=5)).to(DEV)
    w = torch.rand(17, generator=g) + 0.5
    # (B, H, dtype): SmallMse with AdamW riding, FromSlabs, PartialOnly (H = 40)
    lifters = ((8, 256, "fp32"), (100, 64, "fp32"), (100, 40, "fp32"))

    def run(E):
        rec = {}
        for resident in (True, False):
            f = pkg.PoseFeeder(x2d, y3d, 16, device=DEV, seed=7, resident=resident, augment=aug, weights=table,
                               crop=pkg.PersonCrop(), frame_hw=(480, 640))
            f.set_epoch(1)
            rec[f"feeder resident={resident}"] = [b.clone() for b in next(iter(f))]
        ids = torch.arange(n, device=DEV)
        rec["gather"] = pkg.gather_row_weights(table.to(DEV), augment=aug, row_ids=ids, epoch=1, src_idx=ids.flip(0))
        rec["gather plain"] = pkg.gather_row_weights(table.to(DEV)[:, :5].contiguous(), src_idx=ids[:9])
        for kind in KINDS:
            for jw in (None, w):
                crit = pkg.PoseCriterion(kind=kind, beta=0.1, joint_weights=jw).to(DEV)
                pd = p.clone().requires_grad_(True)
                loss = crit(pd, t, row_weights=rw)
                loss.backward()
                rec[f"criterion {kind} joint={jw is not None}"] = dict(loss=loss, dpred=pd.grad)
        for B, H, dtype in lifters:
            for kind in ("smooth_l1", "mpjpe"):
                torch.manual_seed(11)
                m = pkg.LinearModel(34, 51, linear_size=H, num_stage=1, p_dropout=0.5, compute_dtype=dtype).to(DEV).train()
                m.manual_seed(0xC0FFEE12345, step=0)
                opt = pkg.FlatAdamW(m, lr=1e-3)
                crit = pkg.PoseCriterion(kind=kind, beta=0.1, joint_weights=w).to(DEV)
                gb = torch.Generator().manual_seed(B + H)
                for k in range(2):                                             # (the second call reuses the first one's workspace)
                    x, y = torch.rand(B, 34, generator=gb).to(DEV), (torch.rand(B, 51, generator=gb) - 0.5).to(DEV)
                    r = torch.from_numpy(orc.weights(B, 17, seed=k)).to(DEV)
                    loss, out = pkg.train_step(m, opt, x, y, criterion=crit, row_weights=r)
                    rec[f"step {B}x{H} {kind} {k}"] = sgi._snap(dict(loss=loss, y=out, grads=m.flat_grads, params=m.flat_params))
        return rec
    return run


sgi.REG[CASE] = _row_weights_run


def test_row_weights_do_not_depend_on_scratch(pkg, monkeypatch):
    ran, _ = sgi._independent(pkg, monkeypatch, CASE, sgi.REG[CASE](pkg))
    assert {"row_weights_gather_kernel", "pose_augment_gather_kernel", "mse_partial_kernel", "mpjpe_loss_partial_kernel",
            "small_mse_kernel", "small_mpjpe_kernel", "mse_partial_from_slabs_kernel", "mpjpe_partial_from_slabs_kernel"} <= ran, sorted(ran)
