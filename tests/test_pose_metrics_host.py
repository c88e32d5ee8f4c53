"""CPU tests of the evaluation metrics: the per-pose arithmetic of csrc/pose_metrics.h through pl_pose_errors_host (the
same inline text the kernel runs, compiled for the CPU) against the fp64 SVD-route oracle, argument validation of the four
entry points without a device, metrics.summarise on hand-made accumulators, PoseMetrics state handling on the CPU and its
all-reduce in a world-2 gloo group."""
import ctypes
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import pose_metrics_oracle as orc
from conftest import ROOT


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()


@pytest.fixture(scope="module")
def cases():
    """name -> (pred, tgt, oracle err, oracle aligned, gap, S); computed once."""
    out = {}
    for name, (p, t) in orc.all_cases().items():
        err, aligned, gap = orc.pose_errors(p, t)
        out[name] = (p, t, err, aligned, gap, orc.coord_scale(p, t))
    return out


def _host(pkg, pred, tgt, want_aligned=True):
    B, J, _ = pred.shape
    err = np.empty((3, B, J), np.float32)
    aligned = np.empty((B, J, 3), np.float32) if want_aligned else None
    rc = pkg.lib().pl_pose_errors_host(pred.ctypes.data, tgt.ctypes.data, B, J, err.ctypes.data,
                                       aligned.ctypes.data if want_aligned else None)
    assert rc == 0, pkg.lib().pl_last_error()
    return err, aligned


def test_golden_fixture_is_the_oracle_on_its_own_inputs(cases):
    """g13 holds real skeletons and the oracle's answers at the time it was written: the oracle has not drifted."""
    with np.load(orc.GOLDEN, allow_pickle=False) as z:
        assert z["pred"].shape == z["tgt"].shape == (128, 17, 3) and z["pred"].dtype == np.float32
        _, _, err, aligned, gap, _ = cases["g13"]
        np.testing.assert_allclose(err, z["err"], rtol=0, atol=1e-13)
        np.testing.assert_allclose(aligned, z["aligned"], rtol=0, atol=1e-13)
        assert abs(z["err"][0].mean() - 0.0379) < 5e-5 and abs(z["err"][2].mean() - 0.0298) < 5e-5


def test_inputs_are_well_conditioned(cases):
    """On the oracle alone: every non-degenerate pose keeps the two largest eigenvalues of Horn's matrix at least 5 % apart
    (degenerate poses report inf), so the rotation -- and with it the per-joint split of the error -- is well determined."""
    for name, (_, _, _, _, gap, _) in cases.items():
        print(f"{name}: smallest relative eigenvalue gap {gap.min():.3f}")
        assert gap.min() >= 0.05, name
    assert np.isinf(cases["collapsed_pred"][4]).all() and np.isinf(cases["collapsed_tgt"][4]).all()
    assert np.isfinite(cases["mirrored_x"][4]).all()


@pytest.mark.parametrize("name", ["g13", "random512", "identical", "mirrored_x", "similarity", "planar", "near_180",
                                  "offset_1000m", "collapsed_pred", "collapsed_tgt", "J3", "J16", "J32"])
def test_pose_errors_host_vs_svd_oracle(pkg, cases, name):
    """|got - ref| <= 1e-5 ref + 64 eps32 S, S the largest absolute coordinate of the pose pair, for the three errors and
    for the aligned pose.  1e-5 is the project's bound for metric reductions (test_gpu_losses.py); 64 eps32 S leaves room
    for another sweep order and FMA contraction over the 12 eps32 S an fp32 emulation of the route reached; a logic error
    shows at 1e-3 or more.  Measured with this code on the CPU: at most 3.5 eps32 S (g13, the aligned pose)."""
    p, t, ref, ref_aligned, _, S = cases[name]
    err, aligned = _host(pkg, p, t)
    print(f"{name}: errors {orc.excess_in_eps(err, ref, S):.2f}, aligned {orc.excess_in_eps(aligned, ref_aligned, S):.2f} eps32 S")
    assert (np.abs(err - ref) <= orc.gate(ref, S)).all()
    assert (np.abs(aligned - ref_aligned) <= orc.gate(ref_aligned, S)).all()
    err_only, _ = _host(pkg, p, t, want_aligned=False)
    assert np.array_equal(err_only, err)


def test_degenerate_poses_follow_the_written_rules(pkg, cases):
    p, t, _, _, _, _ = cases["collapsed_pred"]
    err, aligned = _host(pkg, p, t)
    centroid = t[0].astype(np.float64).mean(axis=0)
    assert np.abs(aligned[0] - centroid).max() <= 2 * orc.EPS32            # scored against the target's centroid
    assert np.abs(err[2, 0] - np.linalg.norm(t[0] - centroid, axis=1)).max() <= 8 * orc.EPS32
    p, t, _, _, _, _ = cases["collapsed_tgt"]
    err, _ = _host(pkg, p, t)
    assert (err[2] == 0).all()
    zero = np.zeros((1, 17, 3), np.float32)
    err, aligned = _host(pkg, zero, cases["identical"][1])                 # sum P.P = 0: N-MPJPE scale 0, no 0/0
    assert np.isfinite(err).all() and np.isfinite(aligned).all() and np.array_equal(err[0], err[1])


def test_nan_stays_in_its_pose(pkg, cases):
    p, t = cases["random512"][0][:5].copy(), cases["random512"][1][:5].copy()
    clean, clean_aligned = _host(pkg, p, t)
    p[2, 7, 1] = np.nan
    t[4, 0, 0] = np.nan
    err, aligned = _host(pkg, p, t)
    # N-MPJPE, P-MPJPE and the aligned pose depend on the whole pose: all NaN.  MPJPE is per joint: NaN at that joint only
    assert np.isnan(err[1:, [2, 4]]).all() and np.isnan(aligned[[2, 4]]).all()
    assert np.isnan(err[0, 2, 7]) and np.isnan(err[0, 4, 0])
    keep = np.ones((5, 17), bool)
    keep[2, 7] = keep[4, 0] = False
    assert np.array_equal(err[0][keep], clean[0][keep])
    assert np.array_equal(err[:, [0, 1, 3]], clean[:, [0, 1, 3]]) and np.array_equal(aligned[[0, 1, 3]], clean_aligned[[0, 1, 3]])


def test_entry_points_reject_bad_arguments_without_a_device(pkg):
    L = pkg.lib()
    a16, a4 = ctypes.c_void_p(64), ctypes.c_void_p(68)       # never dereferenced on these paths
    for fn, tail in ((L.pl_pose_errors, (None,)), (L.pl_pose_errors_host, ())):
        assert fn(None, a16, 4, 17, a16, None, *tail) != 0 and b"null" in L.pl_last_error()
        assert fn(a16, a16, 4, 17, None, None, *tail) != 0 and b"null" in L.pl_last_error()
        assert fn(a16, a16, 0, 17, a16, None, *tail) != 0 and b"B=0" in L.pl_last_error()
        assert fn(a16, a16, 4, 2, a16, None, *tail) != 0 and b"J=2" in L.pl_last_error()
        assert fn(a16, a16, 4, 33, a16, None, *tail) != 0 and b"J=33" in L.pl_last_error()
        assert fn(a4, a16, 4, 17, a16, None, *tail) != 0 and b"aligned" in L.pl_last_error()
        assert fn(a16, a16, 4, 17, a16, a4, *tail) != 0 and b"aligned" in L.pl_last_error()
        assert fn(a16, a16, 4, 17, ctypes.c_void_p(66), None, *tail) != 0 and b"aligned" in L.pl_last_error()

    def accum(err=a16, B=4, J=17, grp=None, G=1, thr=a16, T=2, sums=a16, counts=a16, n=a16, scratch=a16):
        return L.pl_pose_metrics_accum(err, B, J, grp, G, thr, T, sums, counts, n, scratch, None)

    for kw, word in ((dict(err=None), b"null"), (dict(sums=None), b"null"), (dict(n=None), b"null"),
                     (dict(scratch=None), b"null"), (dict(thr=None), b"null"), (dict(counts=None), b"null"),
                     (dict(B=0), b"B=0"), (dict(J=2), b"J=2"), (dict(J=33), b"J=33"), (dict(G=0), b"groups=0"),
                     (dict(G=33), b"groups=33"), (dict(T=-1), b"n_thr=-1"), (dict(T=33), b"n_thr=33"),
                     (dict(err=ctypes.c_void_p(66)), b"aligned"), (dict(grp=ctypes.c_void_p(66)), b"aligned"),
                     (dict(counts=a4), b"aligned"), (dict(n=a4), b"aligned")):
        assert accum(**kw) != 0, kw
        assert word in L.pl_last_error(), (kw, L.pl_last_error())
    # the scratch size is a pure host function: 0 for a shape the accumulation would reject, and one 32-bit cell per
    # (chunk, metric, threshold-or-sum, group, joint) plus the chunk's pose counts otherwise
    assert L.pl_pose_metrics_scratch_bytes(0, 17, 1, 0) == 0 and L.pl_pose_metrics_scratch_bytes(4, 17, 33, 0) == 0
    assert L.pl_pose_metrics_scratch_bytes(4, 17, 1, 33) == 0 and L.pl_pose_metrics_scratch_bytes(4, 2, 1, 0) == 0
    assert L.pl_pose_metrics_scratch_bytes(128, 17, 15, 31) == 4 * (3 * 32 * 15 * 17 + 16)
    assert L.pl_pose_metrics_scratch_bytes(129, 17, 15, 31) == 2 * 4 * (3 * 32 * 15 * 17 + 16)
    assert L.pl_pose_metrics_scratch_bytes(64 * 128 + 1, 3, 1, 0) == 64 * 4 * (3 * 3 + 2)


def test_cpu_tensors_are_refused(pkg):
    """No CPU fallback: the computing entry points raise as every other one does."""
    p, t = torch.zeros(2, 17, 3), torch.zeros(2, 17, 3)
    for call in (lambda: pkg.pose_errors(p, t), lambda: pkg.procrustes_align(p, t),
                 lambda: pkg.PoseMetrics(device="cpu").update(p, t)):
        with pytest.raises(pkg.PoseliftError, match="no CPU path"):
            call()


def test_auc_thresholds():
    import importlib
    m = importlib.import_module("3d_poseestimation_amd.metrics")
    assert len(m.AUC_THRESHOLDS) == 31 and m.AUC_THRESHOLDS[0] == 0.0 and m.AUC_THRESHOLDS[-1] == 0.150
    assert np.allclose(np.diff(m.AUC_THRESHOLDS), 0.005, atol=1e-12)
    assert np.array_equal(np.asarray(m.AUC_THRESHOLDS, np.float32), orc.AUC_THRESHOLDS.astype(np.float32))


def test_summarise_on_hand_made_accumulators(pkg):
    """Three joints, two thresholds, three groups of which the middle one is empty."""
    G, J, thr = 3, 3, [0.05, 0.15]
    sums = torch.zeros(G, 3, J)
    counts = torch.zeros(G, 3, 2, J, dtype=torch.int64)
    n = torch.tensor([2, 0, 6, 0])
    sums[0] = torch.tensor([[0.2, 0.4, 0.6], [0.1, 0.2, 0.3], [0.02, 0.04, 0.06]])          # sums over 2 poses, metres
    sums[2] = torch.tensor([[0.6, 0.6, 0.6], [0.3, 0.3, 0.3], [0.06, 0.06, 0.06]])          # over 6 poses
    counts[0, 0] = torch.tensor([[0, 0, 0], [2, 1, 0]])
    counts[2, 0] = torch.tensor([[3, 3, 3], [6, 6, 3]])
    counts[0, 2] = torch.tensor([[2, 2, 1], [2, 2, 2]])
    out = pkg.metrics.summarise(sums, counts, n, thr, ["walk", "sit", "eat"])
    assert out["n_poses"] == 8 and out["n_out_of_range"] == 0 and out["pck_threshold_m"] == 0.15
    assert out["mpjpe_mm"] == pytest.approx((1.2 + 1.8) / (8 * 3) * 1000)
    assert out["n_mpjpe_mm"] == pytest.approx((0.6 + 0.9) / 24 * 1000)
    assert out["p_mpjpe_mm"] == pytest.approx((0.12 + 0.18) / 24 * 1000)
    assert out["mpjpe_per_joint_mm"] == pytest.approx([100.0, 125.0, 150.0])
    assert out["pck_mpjpe"] == pytest.approx((3 + 15) / 24)
    assert out["auc_mpjpe"] == pytest.approx(((0 + 9) / 24 + (3 + 15) / 24) / 2)
    walk, sit, eat = (out["groups"][k] for k in ("walk", "sit", "eat"))
    assert walk["n_poses"] == 2 and walk["mpjpe_mm"] == pytest.approx(200.0) and walk["pck_mpjpe"] == pytest.approx(0.5)
    assert walk["pck_p_mpjpe"] == pytest.approx(1.0) and walk["auc_p_mpjpe"] == pytest.approx((5 / 6 + 1.0) / 2)
    assert eat["mpjpe_per_joint_mm"] == pytest.approx([100.0] * 3) and eat["auc_mpjpe"] == pytest.approx((9 / 18 + 15 / 18) / 2)
    assert sit["n_poses"] == 0                                               # empty: NaN, no division error
    for k in ("mpjpe_mm", "n_mpjpe_mm", "p_mpjpe_mm", "pck_mpjpe", "auc_p_mpjpe"):
        assert math.isnan(sit[k])
    assert all(math.isnan(v) for v in sit["p_mpjpe_per_joint_mm"])
    # no thresholds: PCK and AUC are NaN, the means stay; one group: no per-group table; nothing at all: NaN
    out = pkg.metrics.summarise(sums[:1], torch.zeros(1, 3, 0, J, dtype=torch.int64), torch.tensor([2, 0]), [])
    assert out["mpjpe_mm"] == pytest.approx(200.0) and math.isnan(out["pck_mpjpe"]) and "groups" not in out
    out = pkg.metrics.summarise(torch.zeros(1, 3, J), torch.zeros(1, 3, 2, J, dtype=torch.int64), torch.tensor([0, 0]), thr)
    assert out["n_poses"] == 0 and math.isnan(out["mpjpe_mm"]) and math.isnan(out["auc_n_mpjpe"])
    with pytest.raises(ValueError):
        pkg.metrics.summarise(sums, counts, n, [0.05])


def test_cpu_meter_state_compute_and_out_of_range_groups(pkg):
    m = pkg.PoseMetrics(joints=3, groups=2, group_names=["a", "b"], pck_thresholds_m=[0.1], device="cpu")
    assert "epoch_mpjpe_mm" in pkg.PoseMetrics.__doc__ and "usual" in pkg.PoseMetrics.__doc__
    assert [tuple(t.shape) for t in m.state().values()] == [(2, 3, 3), (2, 3, 1, 3), (3,)]
    st = {"sums": torch.full((2, 3, 3), 0.3), "counts": torch.ones(2, 3, 1, 3, dtype=torch.int64),
          "n_poses": torch.tensor([2, 4, 0])}
    m.load_state(st)
    out = m.compute()
    assert out["n_poses"] == 6 and out["p_mpjpe_mm"] == pytest.approx(100.0, rel=1e-6)
    assert out["groups"]["a"]["mpjpe_mm"] == pytest.approx(150.0, rel=1e-6) and out["groups"]["b"]["pck_n_mpjpe"] == pytest.approx(0.25)
    st["n_poses"] = torch.tensor([2, 4, 1])
    m.load_state(st)
    with pytest.raises(pkg.PoseliftError, match="outside"):
        m.compute()
    m.reset()
    assert all(int(t.abs().sum()) == 0 for t in m.state().values()) and m.compute()["n_poses"] == 0
    with pytest.raises(ValueError):
        m.load_state({"sums": torch.zeros(1, 3, 3), "counts": st["counts"], "n_poses": st["n_poses"]})
    for bad in (dict(joints=2), dict(joints=33), dict(groups=0), dict(groups=33), dict(pck_thresholds_m=[0.1] * 33),
                dict(groups=2, group_names=["a"])):
        with pytest.raises(ValueError):
            pkg.PoseMetrics(device="cpu", **bad)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _reduce_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import importlib
    import torch.distributed as dist
    pkg = importlib.import_module("3d_poseestimation_amd")
    pkg.dp.init_from_env(backend="gloo")
    m = pkg.PoseMetrics(joints=3, groups=2, pck_thresholds_m=[0.05, 0.1], device="cpu")
    m.load_state({"sums": torch.full((2, 3, 3), 0.25 * (rank + 1)),
                  "counts": torch.full((2, 3, 2, 3), rank + 1, dtype=torch.int64),
                  "n_poses": torch.tensor([1 + rank, 10 * (1 + rank), 0])})
    m.all_reduce()
    ok = (torch.equal(m.sums, torch.full((2, 3, 3), 0.75)) and torch.equal(m.counts, torch.full((2, 3, 2, 3), 3))
          and m.n_poses.tolist() == [3, 30, 0] and m.compute()["n_poses"] == 33)
    dist.barrier()
    dist.destroy_process_group()
    out.put((rank, bool(ok)))


def test_all_reduce_sums_states_world2_gloo():
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_reduce_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res == [(0, True), (1, True)]
