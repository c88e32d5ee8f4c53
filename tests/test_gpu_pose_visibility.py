"""GPU tests of the evaluation with missing joints: pl.pose_errors / pl.procrustes_align with weights= against the fp64
weighted-SVD oracle and pl_pose_errors_w_host, the visibility meter (masked sums, PCK counts, n_valid) per group, its
compute() table, NaN containment at invisible joints, eval_step's meter_weights, scratch independence and misaligned weights.
Inputs, oracle and the gap condition: tests/pose_visibility_oracle.py."""
import numpy as np
import pytest
import torch

import alignment_cases as ac
import pose_visibility_oracle as orc
import test_gpu_scratch_independence as sgi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = orc.EPS32
CASE = "pose visibility"


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


@pytest.fixture(scope="module")
def cases():
    """name -> (pred, tgt, w, oracle err, oracle aligned, gap, S), computed once and left unchanged."""
    out = {}
    for name, (p, t, w) in orc.input_sets().items():
        err, aligned, gap = orc.pose_errors(p, t, w)
        out[name] = (p, t, w, err, aligned, gap, orc.coord_scale(p, t))
    return out


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(pkg, pred, tgt, w, sub=None, div=None):
    B, J, _ = pred.shape
    err, aligned = np.empty((3, B, J), np.float32), np.empty((B, J, 3), np.float32)
    rc = pkg.lib().pl_pose_errors_w_host(pred.ctypes.data, tgt.ctypes.data, B, J, w.ctypes.data,
                                         sub.ctypes.data if sub is not None else None, div.ctypes.data if div is not None else None,
                                         err.ctypes.data, aligned.ctypes.data)
    assert rc == 0, pkg.lib().pl_last_error()
    return err, aligned


def _check_device(pkg, p, t, w, ref, ref_aligned, S, keep, what):
    """The gate |got - ref| <= 1e-5 |ref| + 64 eps32 S against the oracle (P-MPJPE and the aligned pose for the poses `keep`);
    device and host run of the same text within 64 eps32 S of each other, as the unweighted test holds them (they differ by
    FMA contraction, so not bitwise); two device runs bit-identical."""
    dp, dt, dw = _t(p), _t(t), _t(w)
    err, aligned = pkg.pose_errors(dp, dt, weights=dw), pkg.procrustes_align(dp, dt, weights=dw)
    err2, aligned2 = pkg.pose_errors(dp, dt, weights=dw), pkg.procrustes_align(dp, dt, weights=dw)
    assert torch.equal(err, err2) and torch.equal(aligned, aligned2), "two device runs differ"
    err, aligned = err.cpu().numpy(), aligned.cpu().numpy()
    assert err.shape == ref.shape and aligned.shape == ref_aligned.shape
    herr, haligned = _host(pkg, p, t, w)
    k = keep
    print(f"{what}: vs oracle {orc.excess(err[:2], ref[:2], S):.2f} / {orc.excess(err[2, k], ref[2, k], S[k]):.2f} / "
          f"{orc.excess(aligned[k], ref_aligned[k], S[k]):.2f}, vs host {orc.excess(err[:2], herr[:2].astype(np.float64), S):.2f} / "
          f"{orc.excess(err[2, k], herr[2, k].astype(np.float64), S[k]):.2f} / "
          f"{orc.excess(aligned[k], haligned[k].astype(np.float64), S[k]):.2f} eps32 S (MPJPE and N-MPJPE / P-MPJPE / aligned); "
          f"{int((~k).sum())} of {k.size} poses outside the gap condition")
    assert np.isfinite(err).all() and np.isfinite(aligned).all()
    assert (np.abs(err[:2] - ref[:2]) <= orc.gate_err(ref[:2], S)).all()
    assert (np.abs(err[2, k] - ref[2, k]) <= orc.gate_err(ref[2, k], S[k])).all()
    assert (np.abs(aligned[k] - ref_aligned[k]) <= orc.gate_aligned(ref_aligned[k], S[k])).all()
    assert (np.abs(err[:2].astype(np.float64) - herr[:2]) <= 64 * EPS32 * S[None, :, None]).all()
    assert (np.abs(err[2, k].astype(np.float64) - herr[2, k]) <= 64 * EPS32 * S[k, None]).all()
    assert (np.abs(aligned[k].astype(np.float64) - haligned[k]) <= 64 * EPS32 * S[k, None, None]).all()


SETS = ["random512 w0", "random512 w1", "random512 w2", "g13 w0", "g13 w1", "g13 w2", "J3x64", "J32x64"]


@pytest.mark.parametrize("name", SETS)
def test_weighted_pose_errors_vs_oracle_and_host(pkg, cases, name):
    p, t, w, ref, ref_aligned, gap, S = cases[name]
    _check_device(pkg, p, t, w, ref, ref_aligned, S, orc.rotation_mask(gap, name), name)


@pytest.mark.parametrize("B,name", [(1, "random512 w0"), (63, "random512 w0"), (64, "random512 w0"), (65, "random512 w0"),
                                    (193, "random512 w0"), (65, "J3x64"), (65, "J32x64")])
def test_weighted_pose_errors_batch_edges(pkg, cases, B, name):
    """One pose, one short of / exactly / one past a 64-pose workgroup, three workgroups and one pose (193 * 51 and 193 * 17
    floats are no multiples of 4: scalar tails of the poses' and of the weights' loads).  J = 3 and J = 32 (the LDS corner:
    58,112 bytes of dynamic LDS) have 64 well-conditioned poses each; their 65-pose batch, two workgroups, wraps around to
    pose 0 with pose 0's weights."""
    p, t, w, ref, ref_aligned, gap, S = cases[name]
    idx = np.arange(B) % p.shape[0]
    keep = orc.rotation_mask(gap, name)[idx]
    _check_device(pkg, np.ascontiguousarray(p[idx]), np.ascontiguousarray(t[idx]), np.ascontiguousarray(w[idx]), ref[:, idx],
                  ref_aligned[idx], S[idx], keep, f"{name}, B={len(idx)}")


def test_denorm_together_with_weights(pkg, cases):
    """Standardised inputs, taken back inside the launch, against the oracle on the inverted inputs."""
    p, t, w = (a[:130] for a in cases["random512 w1"][:3])
    rng = np.random.default_rng(9)
    sub = rng.uniform(-0.2, 0.2, (17, 3)).astype(np.float32)
    div = rng.uniform(0.5, 2.0, (17, 3)).astype(np.float32)
    T = pkg.PoseTransform(torch.from_numpy(sub), torch.from_numpy(div))
    sp, st = T.apply(_t(p)), T.apply(_t(t))                                 # the model's space
    raw_p, raw_t = T.invert(sp).cpu().numpy(), T.invert(st).cpu().numpy()     # what the launch computes on
    ref, ref_aligned, gap = orc.pose_errors(raw_p, raw_t, w)
    S = orc.coord_scale(raw_p, raw_t)
    keep = gap >= orc.MIN_GAP
    assert keep.all()
    dw = _t(w)
    err = pkg.pose_errors(sp, st, denorm=T, weights=dw).cpu().numpy()
    aligned = pkg.procrustes_align(sp, st, denorm=T, weights=dw).cpu().numpy()
    print(f"denorm + weights: {orc.excess(err, ref, S):.2f} / {orc.excess(aligned, ref_aligned, S):.2f} eps32 S")
    assert (np.abs(err - ref) <= orc.gate_err(ref, S)).all()
    assert (np.abs(aligned - ref_aligned) <= orc.gate_aligned(ref_aligned, S)).all()
    want = pkg.pose_errors(_t(raw_p), _t(raw_t), weights=dw)
    assert ac.same_bits(pkg.pose_errors(sp, st, denorm=T, weights=dw), want)
    herr, _ = _host(pkg, np.ascontiguousarray(sp.cpu().numpy()), np.ascontiguousarray(st.cpu().numpy()), np.ascontiguousarray(w),
                    sub.reshape(-1), div.reshape(-1))
    assert (np.abs(err.astype(np.float64) - herr) <= 64 * EPS32 * S[None, :, None]).all()


def test_weights_none_is_the_call_without_the_keyword(pkg, cases):
    p, t = _t(cases["random512 w0"][0][:200]), _t(cases["random512 w0"][1][:200])
    gid = torch.arange(200, device=DEV) % 3
    T = pkg.PoseTransform.normalize_3d()
    assert ac.same_bits(pkg.pose_errors(p, t, weights=None), pkg.pose_errors(p, t))
    assert ac.same_bits(pkg.procrustes_align(p, t, weights=None), pkg.procrustes_align(p, t))
    assert ac.same_bits(pkg.pose_errors(p, t, denorm=T, weights=None), pkg.pose_errors(p, t, T))
    a, b = pkg.PoseMetrics(groups=3, device=DEV), pkg.PoseMetrics(groups=3, device=DEV)
    a.update(p, t, gid)
    b.update(p, t, gid, weights=None)
    assert list(a.state()) == list(b.state()) == ["sums", "counts", "n_poses"]
    for k in a.state():
        assert ac.same_bits(a.state()[k], b.state()[k]), k
    assert repr(a.compute()) == repr(b.compute())


def test_weights_as_a_strided_view_and_as_fp64(pkg, cases):
    p, t, w = (_t(a[:130]) for a in cases["random512 w2"][:3])
    want = pkg.pose_errors(p, t, weights=w)
    wide = torch.zeros(130, 40, device=DEV)
    wide[:, 3:37:2] = w
    view = wide[:, 3:37:2]
    assert not view.is_contiguous()
    assert ac.same_bits(pkg.pose_errors(p, t, weights=view), want)
    assert ac.same_bits(pkg.pose_errors(p, t, weights=w.double()), want)
    m, n = pkg.PoseMetrics(device=DEV, visibility=True), pkg.PoseMetrics(device=DEV, visibility=True)
    m.update(p, t, weights=w)
    n.update(p, t, weights=view.double())
    for k in m.state():
        assert ac.same_bits(m.state()[k], n.state()[k]), k
    with pytest.raises(ValueError, match="weights"):
        pkg.pose_errors(p, t, weights=w[:, :16])
    with pytest.raises(ValueError, match="visibility=True"):
        pkg.PoseMetrics(device=DEV).update(p, t, weights=w)
    with pytest.raises(ValueError, match="needs weights"):
        m.update(p, t)


def _borderline(ref, S, thr):
    """(3, B, T, J) bool: the oracle's error lies within 64 eps32 S of the threshold (tests/test_gpu_pose_metrics.py)."""
    return np.abs(ref[:, :, None, :] - thr[None, None, :, None]) <= 64 * EPS32 * S[None, :, None, None]


def _check_accumulators(m, ref, w, S, groups, G, thr, what):
    sums, counts, n, n_valid = orc.accumulate(ref, w, groups, G, thr)
    got_sums = m.sums.cpu().numpy().astype(np.float64)
    assert np.array_equal(m.n_poses.cpu().numpy(), n), (m.n_poses, n)             # pose counts and the out-of-range cell: exact
    assert np.array_equal(m.n_valid.cpu().numpy(), n_valid)                      # visible entries: exact
    assert (np.abs(got_sums - sums) <= 1e-5 * np.abs(sums)).all()
    assert (got_sums[np.broadcast_to(n_valid[:, None, :] == 0, got_sums.shape)] == 0).all()
    T = len(thr)
    got_counts = m.counts.cpu().numpy()
    assert got_counts.shape == (G, 3, T, ref.shape[2])
    if T == 0:
        return
    thr64 = np.asarray(thr, np.float32).astype(np.float64)
    border = _borderline(ref, S, thr64) & orc.visible(w)[None, :, None, :]
    frac = border.sum() / border.size
    g = np.zeros(ref.shape[1], np.int64) if groups is None else np.asarray(groups)
    slack = np.zeros_like(counts)
    for k in range(G):
        slack[k] = border[:, g == k].sum(axis=1)
    print(f"{what}: {border.sum()} borderline of {border.size} (entry, threshold) pairs; "
          f"{int((got_counts != counts).sum())} of {counts.size} count cells differ from the oracle's")
    assert frac <= 1e-3                                                          # on the oracle: at most 0.1 % borderline pairs
    assert (np.abs(got_counts - counts) <= slack).all()


def _meter_inputs(cases):
    """The 512 random poses with their weights; the gap condition excludes none of them, so every cell is compared."""
    p, t, w, ref, _, gap, S = cases["random512 w0"]
    assert (gap >= orc.MIN_GAP).all()
    rng = np.random.default_rng(3)
    G = 15
    groups = rng.choice([g for g in range(G) if g not in (3, 8, 11)], size=512)
    groups[[5, 77, 301, 400, 511]] = [-1, 15, 99, -7, 2 ** 31 - 1]
    return p, t, w, ref, S, groups, G


def test_visibility_meter_per_group_two_updates(pkg, cases):
    """15 groups (3, 8 and 11 empty), five stray ids, two update() calls of 300 and 212 poses against ONE oracle pass.  Sums
    to 1e-5 relative; n_valid, n_poses and the out-of-range cell exact; PCK cells exact but for borderline pairs."""
    p, t, w, ref, S, groups, G = _meter_inputs(cases)
    m = pkg.PoseMetrics(groups=G, device=DEV, visibility=True)
    assert len(m.thresholds) == 31 and list(m.state()) == ["sums", "counts", "n_poses", "n_valid"]
    gid = torch.from_numpy(groups).to(DEV)
    m.update(_t(p[:300]), _t(t[:300]), gid[:300], weights=_t(w[:300]))
    m.update(_t(p[300:]), _t(t[300:]), gid[300:].to(torch.int32), weights=_t(w[300:]))
    _check_accumulators(m, ref, w, S, groups, G, orc.AUC_THRESHOLDS, "G=15, T=31, weighted")
    assert int(m.n_poses[:G].sum()) == 507 and int(m.n_valid[:, 5].sum()) == 0   # (the all-zero row is a pose; joint 5 is never seen)
    with pytest.raises(pkg.PoseliftError, match="outside"):
        m.compute()


def test_compute_is_the_oracles_masked_table(pkg, cases):
    p, t, w, ref, S, groups, G = _meter_inputs(cases)
    keep = (groups >= 0) & (groups < G)
    v = orc.visible(w)
    m = pkg.PoseMetrics(groups=G, device=DEV, visibility=True)
    m.update(_t(p[keep]), _t(t[keep]), _t(groups[keep]), weights=_t(w[keep]))
    out = m.compute()
    assert out["n_poses"] == int(keep.sum()) and out["n_out_of_range"] == 0 and out["n_joints"] == int(v[keep].sum())
    assert out["n_valid_per_joint"] == v[keep].sum(axis=0).tolist() and out["n_valid_per_joint"][5] == 0
    for k, name in enumerate(("mpjpe", "n_mpjpe", "p_mpjpe")):
        assert out[f"{name}_mm"] == pytest.approx(ref[k][keep][v[keep]].mean() * 1000, rel=1e-5)
        sel = keep & (groups == 4)
        assert out["groups"]["4"][f"{name}_mm"] == pytest.approx(ref[k][sel][v[sel]].mean() * 1000, rel=1e-5)
        assert out["groups"]["4"]["n_joints"] == int(v[sel].sum())
        per_joint = out[f"{name}_per_joint_mm"]
        assert np.isnan(per_joint[5])                                            # the all-zero joint column: NaN, absent from the mean
        for j in (0, 1, 4, 6, 16):
            assert per_joint[j] == pytest.approx(ref[k][keep, j][v[keep, j]].mean() * 1000, rel=1e-5)
    assert np.isnan(out["groups"]["8"]["p_mpjpe_mm"]) and out["groups"]["8"]["n_poses"] == 0 and out["groups"]["8"]["n_joints"] == 0
    e = ref[2][keep][v[keep]]
    pck = (e <= np.float32(0.150)).mean()
    edge = (_borderline(ref[2:, keep], S[keep], np.array([np.float32(0.150)], np.float64))[0, :, 0, :] & v[keep]).sum()
    assert abs(out["pck_p_mpjpe"] - pck) <= edge / e.size + 1e-12


@pytest.mark.parametrize("n_thr", [0, 31])
def test_visibility_meter_past_the_chunk_cap(pkg, cases, n_thr):
    """64 * 128 + 1 poses: the rows per chunk grow to 129; one group, no ids.  n_thr = 0: no counts tensor is read or
    written, the visible counts are still taken."""
    p, t, w, ref, _, _, S = cases["random512 w0"]
    B = 64 * 128 + 1
    reps = -(-B // 512)
    tile = lambda a, ax=0: np.concatenate([a] * reps, axis=ax)                   # noqa: E731
    pp, tt, ww = tile(p)[:B], tile(t)[:B], tile(w)[:B]
    m = pkg.PoseMetrics(pck_thresholds_m=orc.AUC_THRESHOLDS[:n_thr], device=DEV, visibility=True)
    m.update(_t(pp), _t(tt), weights=_t(ww))
    _check_accumulators(m, tile(ref, 1)[:, :B], ww, tile(S)[:B], None, 1, orc.AUC_THRESHOLDS[:n_thr], f"B={B}, T={n_thr}, weighted")
    out = m.compute()
    assert out["n_poses"] == B and out["n_joints"] == int(orc.visible(ww).sum()) and np.isnan(out["auc_mpjpe"]) == (n_thr == 0)


def test_nan_at_invisible_joints_leaves_the_table_bitwise(pkg, cases):
    """NaN-coded missing ground truth (and a NaN prediction) at joints with weight 0, joint 0 among them: every state tensor
    and every error outside those joints is bitwise that of the clean run."""
    p, t, w = (a[:200].copy() for a in cases["random512 w0"][:3])
    w[::7, 0] = 0.0
    gid = torch.arange(200, device=DEV, dtype=torch.int32) % 3
    clean = pkg.PoseMetrics(groups=3, device=DEV, visibility=True)
    clean.update(_t(p), _t(t), gid, weights=_t(w))
    clean_err = pkg.pose_errors(_t(p), _t(t), weights=_t(w))
    hidden = ~orc.visible(w)
    t[hidden] = np.nan
    p[hidden & (np.arange(200)[:, None] % 2 == 0)] = np.inf
    m = pkg.PoseMetrics(groups=3, device=DEV, visibility=True)
    m.update(_t(p), _t(t), gid, weights=_t(w))
    for k in clean.state():
        assert ac.same_bits(m.state()[k], clean.state()[k]), k
    assert torch.isfinite(m.sums).all()
    err = pkg.pose_errors(_t(p), _t(t), weights=_t(w))
    vis = _t(~hidden)
    assert ac.same_bits(err[:, vis], clean_err[:, vis]) and not torch.isfinite(err[:, ~vis]).any()
    assert repr(clean.compute()) == repr(m.compute())


@pytest.mark.parametrize("flip", [False, True])
def test_eval_step_hands_meter_weights_to_the_meter(pkg, flip):
    """eval_step(..., meter=m, meter_weights=w) returns what it returns without them and feeds the meter what a direct
    update(y2_hat, y2, group_ids, weights=w) would: the same bits in all four state tensors."""
    torch.manual_seed(0)
    model = pkg.LinearModel(34, 51, linear_size=64).to(DEV).eval()
    y1, y2 = pkg.synth.synthetic_batch(96, 4321, DEV)
    groups = torch.arange(96, device=DEV) % 4
    w = _t(orc.weights(96, 17, 11))
    plain = pkg.eval_step(model, y1, y2, flip=flip)
    m = pkg.PoseMetrics(groups=4, device=DEV, visibility=True)
    got = pkg.eval_step(model, y1, y2, flip=flip, meter=m, group_ids=groups, meter_weights=w)
    assert len(plain) == len(got) == 3
    for a, b in zip(plain, got):
        assert torch.equal(a, b)
    direct = pkg.PoseMetrics(groups=4, device=DEV, visibility=True)
    direct.update(got[2], y2, groups, weights=w)
    for k in m.state():
        assert ac.same_bits(m.state()[k], direct.state()[k]), k
    assert int(m.n_poses[:4].sum()) == 96 and int(m.n_valid.sum()) == int((w > 0).sum())
    with pytest.raises(ValueError, match="meter_weights"):
        pkg.eval_step(model, y1, y2, flip=flip, meter_weights=w)
    with pytest.raises(ValueError, match="meter_weights"):
        pkg.eval_step(model, y1, y2, flip=flip, meter=pkg.PoseMetrics(groups=4, device=DEV), meter_weights=w)


# ---- results do not depend on what scratch and outputs held (tests/test_gpu_scratch_independence.py's protocol) ---------------
def _visibility_run(pkg):
    g = torch.Generator().manual_seed(31)
    rec_in = {}
    for B in (65, 300):
        p = (torch.randn(B, 17, 3, generator=g) * 0.3).to(DEV)
        rec_in[B] = (p, (p.cpu() + torch.randn(B, 17, 3, generator=g) * 0.04).to(DEV), torch.from_numpy(orc.weights(B, 17, B)).to(DEV))
    gid = (torch.arange(300) % 3).to(DEV)
    tr = pkg.PoseTransform.normalize_3d()

    def run(E):
        rec = {}
        for B, (p, t, w) in rec_in.items():
            rec[f"errors {B}"] = pkg.pose_errors(p, t, weights=w)
            rec[f"aligned {B}"] = pkg.procrustes_align(p, t, weights=w)
            rec[f"errors denorm {B}"] = pkg.pose_errors(p, t, denorm=tr, weights=w)
        p, t, w = rec_in[300]
        m = pkg.PoseMetrics(groups=3, pck_thresholds_m=pkg.AUC_THRESHOLDS[:7], device=DEV, visibility=True)
        m.update(p, t, gid, weights=w)
        m.update(p, t, gid.to(torch.int32), denorm=tr, weights=w)
        rec.update(sums=m.sums, counts=m.counts, n_poses=m.n_poses, n_valid=m.n_valid)
        one = pkg.PoseMetrics(pck_thresholds_m=[], device=DEV, visibility=True)
        one.update(*rec_in[65][:2], weights=rec_in[65][2])
        rec.update(sums1=one.sums, n_valid1=one.n_valid)
        return rec
    return run


sgi.REG[CASE] = _visibility_run


def test_visibility_does_not_depend_on_scratch(pkg, monkeypatch):
    ran, _ = sgi._independent(pkg, monkeypatch, CASE, sgi.REG[CASE](pkg))
    assert {"pose_errors_kernel", "pose_metrics_partial_kernel", "pose_metrics_final_weighted_kernel"} <= ran, sorted(ran)


# ---- weights off 16-byte alignment ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,J", [(65, 17), (130, 3), (66, 32)])
def test_weights_off_16_byte_alignment_give_the_same_bits(pkg, B, J):
    """Weights need only be 4-byte aligned: contiguous views 4, 8 and 12 bytes past a 16-byte boundary (and the poses at the
    same offsets, which the wrapper realigns) give the bits of the aligned call; nothing around any view is written."""
    g = torch.Generator().manual_seed(B + J)
    p = (torch.randn(B, J, 3, generator=g) * 0.3).to(DEV)
    t = (p.cpu() + torch.randn(B, J, 3, generator=g) * 0.04).to(DEV)
    w = torch.from_numpy(orc.weights(B, J, 3)).to(DEV)
    gid = (torch.arange(B, dtype=torch.int32) % 2).to(DEV)

    def call(_state, p, t, w, gid):
        m = pkg.PoseMetrics(joints=J, groups=2, device=DEV, visibility=True)
        m.update(p, t, gid, weights=w)
        return [pkg.pose_errors(p, t, weights=w), pkg.procrustes_align(p, t, weights=w), m.sums, m.counts, m.n_poses, m.n_valid]

    ac.run_aligned_and_off(lambda: None, call, [p, t, w, gid])
