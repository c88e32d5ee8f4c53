"""GPU tests of the evaluation metrics: pl.pose_errors / pl.procrustes_align against the fp64 SVD-route oracle and against
pl_pose_errors_host (the same inline arithmetic on the CPU), PoseMetrics accumulation per group with PCK counts, its
agreement with loss_MPJPE, eval_step's meter hook and NaN containment.  Inputs and oracle: tests/pose_metrics_oracle.py."""
import numpy as np
import pytest
import torch

import pose_metrics_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = orc.EPS32


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


@pytest.fixture(scope="module")
def cases():
    """name -> (pred, tgt, oracle err, oracle aligned, gap, S), computed once: the host test's cases plus multi-workgroup
    batches at J = 3, 16 and 32 (even row lengths are padded in LDS; 130 poses = two full workgroups and two poses)."""
    out = {}
    inputs = orc.all_cases()
    for J in (3, 16, 32):
        inputs[f"J{J}x130"] = orc.well_conditioned_poses(130, J, seed=200 + J)
    for name, (p, t) in inputs.items():
        err, aligned, gap = orc.pose_errors(p, t)
        out[name] = (p, t, err, aligned, gap, orc.coord_scale(p, t))
    return out


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(pkg, pred, tgt):
    B, J, _ = pred.shape
    err, aligned = np.empty((3, B, J), np.float32), np.empty((B, J, 3), np.float32)
    assert pkg.lib().pl_pose_errors_host(pred.ctypes.data, tgt.ctypes.data, B, J, err.ctypes.data, aligned.ctypes.data) == 0
    return err, aligned


def _check_device(pkg, p, t, ref, ref_aligned, S, what):
    dp, dt = _t(p), _t(t)
    err = pkg.pose_errors(dp, dt)
    aligned = pkg.procrustes_align(dp, dt)
    err2, aligned2 = pkg.pose_errors(dp, dt), pkg.procrustes_align(dp, dt)
    assert torch.equal(err, err2) and torch.equal(aligned, aligned2), "two device runs differ"
    err, aligned = err.cpu().numpy(), aligned.cpu().numpy()
    assert err.shape == ref.shape and aligned.shape == ref_aligned.shape
    herr, haligned = _host(pkg, p, t)
    print(f"{what}: vs oracle {orc.excess_in_eps(err, ref, S):.2f} / {orc.excess_in_eps(aligned, ref_aligned, S):.2f}, "
          f"vs host {orc.excess_in_eps(err, herr.astype(np.float64), S):.2f} / "
          f"{orc.excess_in_eps(aligned, haligned.astype(np.float64), S):.2f} eps32 S (errors / aligned)")
    assert (np.abs(err - ref) <= orc.gate(ref, S)).all()
    assert (np.abs(aligned - ref_aligned) <= orc.gate(ref_aligned, S)).all()
    assert (np.abs(err.astype(np.float64) - herr) <= 64 * EPS32 * S[None, :, None]).all()
    assert (np.abs(aligned.astype(np.float64) - haligned) <= 64 * EPS32 * S[:, None, None]).all()


@pytest.mark.parametrize("name", ["g13", "random512", "identical", "mirrored_x", "similarity", "planar", "near_180",
                                  "offset_1000m", "collapsed_pred", "collapsed_tgt", "J3", "J16", "J32", "J3x130", "J16x130",
                                  "J32x130"])
def test_pose_errors_vs_oracle_and_host(pkg, cases, name):
    """The host test's gate, |got - ref| <= 1e-5 ref + 64 eps32 S, for the errors and the aligned pose; the device and
    the host run of the same text within 64 eps32 S of each other (they differ by FMA contraction only); two device runs
    bit-identical."""
    p, t, ref, ref_aligned, gap, S = cases[name]
    assert gap.min() >= 0.05
    _check_device(pkg, p, t, ref, ref_aligned, S, name)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 193])
def test_pose_errors_batch_edges(pkg, cases, B):
    """One pose, one short of / exactly / one past a 64-pose workgroup, three workgroups and one pose.  (The launcher has
    no grid cap: one workgroup per 64 poses.)  193 * 51 floats is no multiple of 4: the last workgroup ends in a
    scalar tail."""
    p, t, ref, ref_aligned, _, S = cases["random512"]
    _check_device(pkg, p[:B], t[:B], ref[:, :B], ref_aligned[:B], S[:B], f"B={B}")


def test_meter_metric0_is_loss_mpjpe(pkg, cases):
    p, t = _t(cases["random512"][0]), _t(cases["random512"][1])
    m = pkg.PoseMetrics(device=DEV)
    m.update(p, t)
    want = pkg.loss_MPJPE(p, t).cpu().numpy().astype(np.float64)
    got = m.sums[0, 0].cpu().numpy().astype(np.float64)
    nz = want > 0
    print("metric 0 vs loss_MPJPE: max rel", np.abs(got[nz] - want[nz]).max() / want[nz].min())
    assert (np.abs(got - want) <= 1e-5 * want).all()
    assert int(m.n_poses[0]) == 512 and int(m.n_poses[1]) == 0


def _borderline(ref, S, thr):
    """(3, B, T, J) bool: the oracle's error lies within 64 eps32 S of the threshold."""
    return np.abs(ref[:, :, None, :] - thr[None, None, :, None]) <= 64 * EPS32 * S[None, :, None, None]


def _check_accumulators(m, ref, S, groups, G, thr, what):
    sums, counts, n = orc.accumulate(ref, groups, G, thr)
    got_sums = m.sums.cpu().numpy().astype(np.float64)
    got_n = m.n_poses.cpu().numpy()
    assert np.array_equal(got_n, n), (got_n, n)                            # pose counts and the out-of-range cell: exact
    assert (np.abs(got_sums - sums) <= 1e-5 * np.abs(sums)).all()
    assert (got_sums[n[:G] == 0] == 0).all()
    T = len(thr)
    got_counts = m.counts.cpu().numpy()
    assert got_counts.shape == (G, 3, T, ref.shape[2])
    if T == 0:
        return
    thr64 = np.asarray(thr, np.float32).astype(np.float64)
    border = _borderline(ref, S, thr64)
    frac = border.sum() / border.size
    g = np.zeros(ref.shape[1], np.int64) if groups is None else np.asarray(groups)
    slack = np.zeros_like(counts)
    for k in range(G):
        slack[k] = border[:, g == k].sum(axis=1)
    print(f"{what}: {border.sum()} borderline of {border.size} (entry, threshold) pairs; "
          f"{int((got_counts != counts).sum())} of {counts.size} count cells differ from the oracle's")
    assert frac <= 1e-3
    assert (np.abs(got_counts - counts) <= slack).all()


def test_accumulation_per_group_two_updates(pkg, cases):
    """15 groups (3, 8 and 11 empty), ids in shuffled order, five poses with ids outside [0, 15); two update() calls of 300
    and 212 poses (three row chunks and two) against ONE oracle pass over all 512.  Sums to 1e-5 relative (sequential
    fp32 sums of at most 64 positive terms per cell here, then a handful of adds: a few eps32); pose counts and the
    out-of-range cell exact; every PCK count cell exact unless an oracle error lies within 64 eps32 S of its threshold,
    then off by at most the number of such entries in the cell (on this set: 80 borderline pairs of 809,472 over the three metrics,
    far below the asserted 0.1 %)."""
    p, t, ref, _, _, S = cases["random512"]
    rng = np.random.default_rng(3)
    G = 15
    groups = rng.choice([g for g in range(G) if g not in (3, 8, 11)], size=512)
    groups[[5, 77, 301, 400, 511]] = [-1, 15, 99, -7, 2 ** 31 - 1]
    keep = (groups >= 0) & (groups < G)
    m = pkg.PoseMetrics(groups=G, device=DEV)
    assert len(m.thresholds) == 31
    gid = torch.from_numpy(groups).to(DEV)                                  # int64: update() narrows it on the device
    m.update(_t(p[:300]), _t(t[:300]), gid[:300])
    m.update(_t(p[300:]), _t(t[300:]), gid[300:].to(torch.int32))
    _check_accumulators(m, ref, S, groups, G, orc.AUC_THRESHOLDS, "G=15, T=31")
    with pytest.raises(pkg.PoseliftError, match="outside"):
        m.compute()
    # the same poses without the strays: compute() is the oracle's table
    m.reset()
    m.update(_t(p[keep]), _t(t[keep]), gid[torch.from_numpy(keep).to(DEV)])
    out = m.compute()
    assert out["n_poses"] == int(keep.sum()) and out["n_out_of_range"] == 0
    for k, name in enumerate(("mpjpe", "n_mpjpe", "p_mpjpe")):
        assert out[f"{name}_mm"] == pytest.approx(ref[k][keep].mean() * 1000, rel=1e-5)
        sel = keep & (groups == 4)
        assert out["groups"]["4"][f"{name}_mm"] == pytest.approx(ref[k][sel].mean() * 1000, rel=1e-5)
    assert np.isnan(out["groups"]["8"]["p_mpjpe_mm"]) and out["groups"]["8"]["n_poses"] == 0
    pck = (ref[2][keep] <= np.float32(0.150)).mean()
    edge = _borderline(ref[2:, keep], S[keep], np.array([np.float32(0.150)], np.float64)).sum()
    assert abs(out["pck_p_mpjpe"] - pck) <= edge / ref[2][keep].size + 1e-12


@pytest.mark.parametrize("n_thr", [0, 31])
def test_accumulation_past_the_chunk_cap_and_without_thresholds(pkg, cases, n_thr):
    """64 * 128 + 1 poses: one past the largest batch that 64 chunks of 128 rows hold, so the rows per chunk grow (129);
    one group, no ids.  n_thr = 0: no thresholds, no counts tensor is read or written."""
    p, t, ref, _, _, S = cases["random512"]
    reps = -(-(64 * 128 + 1) // 512)
    B = 64 * 128 + 1
    pp, tt = np.tile(p, (reps, 1, 1))[:B], np.tile(t, (reps, 1, 1))[:B]
    m = pkg.PoseMetrics(pck_thresholds_m=orc.AUC_THRESHOLDS[:n_thr], device=DEV)
    m.update(_t(pp), _t(tt))
    _check_accumulators(m, np.tile(ref, (1, reps, 1))[:, :B], np.tile(S, reps)[:B], None, 1, orc.AUC_THRESHOLDS[:n_thr],
                        f"B={B}, T={n_thr}")
    out = m.compute()
    assert out["n_poses"] == B and np.isnan(out["auc_mpjpe"]) == (n_thr == 0)


@pytest.mark.parametrize("flip", [False, True])
def test_eval_step_feeds_the_meter(pkg, flip):
    """eval_step(..., meter=m, group_ids=g) returns exactly what it returns without the meter, and the meter's table is
    the oracle's on the y2_hat it returned."""
    torch.manual_seed(0)
    model = pkg.LinearModel(34, 51, linear_size=64).to(DEV).eval()
    y1, y2 = pkg.synth.synthetic_batch(96, 4321, DEV)
    groups = torch.arange(96, device=DEV) % 4
    plain = pkg.eval_step(model, y1, y2, flip=flip)
    m = pkg.PoseMetrics(groups=4, group_names=["a", "b", "c", "d"], device=DEV)
    with_meter = pkg.eval_step(model, y1, y2, flip=flip, meter=m, group_ids=groups)
    assert len(plain) == len(with_meter) == 3
    for a, b in zip(plain, with_meter):
        assert torch.equal(a, b)
    y2_hat = with_meter[2].cpu().numpy()
    ref, _, gap = orc.pose_errors(y2_hat, y2.cpu().numpy())
    S = orc.coord_scale(y2_hat, y2.cpu().numpy())
    print(f"flip={flip}: smallest eigenvalue gap {gap.min():.3f}")
    assert gap.min() >= 0.05
    out = m.compute()
    assert out["n_poses"] == 96
    tol = lambda want: 1e-5 * want + 64 * EPS32 * S.max() * 1000            # noqa: E731  (the per-element gate, in mm)
    for k, name in enumerate(("mpjpe", "n_mpjpe", "p_mpjpe")):
        assert abs(out[f"{name}_mm"] - ref[k].mean() * 1000) <= tol(ref[k].mean() * 1000)
        want = ref[k][1::4].mean() * 1000
        assert abs(out["groups"]["b"][f"{name}_mm"] - want) <= tol(want)
        assert np.abs(np.array(out[f"{name}_per_joint_mm"]) - ref[k].mean(axis=0) * 1000).max() <= tol(ref[k].mean(axis=0).max() * 1000)


def test_nan_poisons_only_its_group(pkg, cases):
    p, t = cases["random512"][0][:200].copy(), cases["random512"][1][:200].copy()
    groups = torch.arange(200, device=DEV, dtype=torch.int32) % 3
    clean = pkg.PoseMetrics(groups=3, device=DEV)
    clean.update(_t(p), _t(t), groups)
    p[100, 5, 2] = np.nan                                                    # pose 100: group 1
    m = pkg.PoseMetrics(groups=3, device=DEV)
    m.update(_t(p), _t(t), groups)
    assert torch.equal(m.n_poses, clean.n_poses)
    for g in (0, 2):
        assert torch.equal(m.sums[g], clean.sums[g]) and torch.equal(m.counts[g], clean.counts[g])
    assert torch.isnan(m.sums[1, 1:]).all() and torch.isnan(m.sums[1, 0, 5]) and torch.isfinite(m.sums[1, 0, :5]).all()
    # the NaN pose is under no threshold: group 1 loses exactly the counts its clean errors earned (every joint of metrics
    # 1 and 2, joint 5 of metric 0)
    e = pkg.pose_errors(_t(cases["random512"][0][100:101]), _t(cases["random512"][1][100:101]))[:, 0]       # (3, J)
    earned = (e[:, None, :] <= clean._thr[None, :, None]).long()
    earned[0, :, :5] = 0
    earned[0, :, 6:] = 0
    assert torch.equal(clean.counts[1] - m.counts[1], earned)
