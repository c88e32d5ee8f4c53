"""GPU tests of the pose tables: the prepare, statistics and transform kernels against their _host forms (bit for bit: the
same inline text, no transcendental but fp64 sqrt), the transform inside the augmented gather (feeders in both modes), inside
pl_pose_errors_t / pl_mpjpe_accum_t (pose_errors, PoseMetrics, eval_step with denorm=), and one end-to-end run from raw arrays
to millimetres."""
import ctypes

import numpy as np
import pytest
import torch

import pose_augment_oracle as aorc
import pose_table_oracle as orc
from test_pose_augment_host import ALL_ON, TABLE_ROWS, aug_struct, make_table, same_bits
from test_pose_table_host import (H36M_17, STAT_WIDTHS, bits64, host_affine, host_augment_t, host_prepare, host_stats,
                                  make_cameras, make_columns, make_raw, make_transforms, prepare_cases, stat_sizes)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the configurations of test_gpu_pose_augment.py (copied)
EXACT = [dict(), dict(p_flip=1.0), dict(p_flip=0.5, seed=7), dict(p_flip=1.0, flip_offset=0.0),
         dict(scale_range=0.25, max_shift=0.1, seed=99), dict(scale_range=0.5, p_flip=0.5, cx=0.25, cy=0.75, seed=5),
         dict(max_shift=0.03, seed=2 ** 63 + 9)]
TRANSCENDENTAL = [ALL_ON, dict(max_rot=np.pi, seed=3), dict(jitter_sigma=0.05, seed=3),
                  dict(p_flip=0.5, max_rot=0.3, jitter_sigma=0.01, flip_offset=0.0, cx=0.0, cy=0.0, seed=8)]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


@pytest.fixture(scope="module")
def table(pkg):
    return make_table(pkg)


@pytest.fixture(scope="module")
def transforms(pkg):
    t2, t3 = make_transforms()
    return pkg.PoseTransform(*t2), pkg.PoseTransform(*t3), t2, t3


def same_bits_t(x, y):
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


# ---- prepare, affine: device == host --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 67, 4101])
def test_prepare_equals_host(pkg, n):
    for raw, joints, cams, cid, zc in prepare_cases(n):
        want = host_prepare(pkg, raw, joints, cams, cid, zc)
        got = pkg.prepare_poses(torch.from_numpy(raw).to(DEV), joints, cams, cid, zc)
        assert same_bits(got.cpu().numpy(), want), (raw.shape, joints, cams is not None, zc)
    cams = make_cameras()
    raw = make_raw(n, 32, 3)
    cid = (np.arange(n) % 7 - 1).astype(np.int32)                      # -1 and 5 are outside [0, 5)
    want = host_prepare(pkg, raw, H36M_17, cams, cid, True)
    got = pkg.prepare_poses(raw, H36M_17, cams, cid, True, device=DEV).cpu().numpy()
    bad = (cid < 0) | (cid >= 5)
    assert same_bits(got, want) and np.isnan(got[bad]).all() and not np.isnan(got[~bad]).any()
    with pytest.raises(pkg.PoseliftError):
        pkg.prepare_poses(torch.from_numpy(raw).to(DEV), (0, 32))
    with pytest.raises(pkg.PoseliftError):
        pkg.prepare_poses(make_raw(4, 17, 2), None, cams, np.zeros(4, np.int32), device=DEV)


def test_affine_equals_host(pkg):
    rs = np.random.RandomState(6)
    for n, (j, d) in ((1, (17, 3)), (67, (17, 2)), (4101, (17, 3)), (4101, (32, 3)), (67, (1, 2))):
        x = (rs.randn(n, j, d) * 3 + 1).astype(np.float32)
        sub, div = rs.randn(j, d).astype(np.float32), rs.uniform(-2, 2, (j, d)).astype(np.float32)
        div[0, 0] = 0.0
        x.reshape(-1)[::97] *= 1e-30                                    # tiny quotients, denormals on the way back
        if n > 1:
            x[1, 0, -1] = np.inf
        t = pkg.PoseTransform(sub, div)
        xd = torch.from_numpy(x).to(DEV)
        y = t.apply(xd)
        assert same_bits(y.cpu().numpy(), host_affine(pkg, x, sub, div, False))
        assert same_bits(y.cpu().numpy(), orc.apply(x, sub, div))
        back = t.invert(y)
        assert same_bits(back.cpu().numpy(), host_affine(pkg, y.cpu().numpy(), sub, div, True))
        z = xd.clone()
        assert t.apply_(z) is z and same_bits_t(z, y)                   # in place == out of place
        assert t.invert_(z) is z and same_bits_t(z, back)
        xn = xd.clone()
        xn[0, -1, -1] = float("nan")
        yn = t.apply(xn)
        assert torch.isnan(yn[0, -1, -1]) and int(torch.isnan(yn).sum()) == 1
        with pytest.raises(ValueError):
            t.apply(torch.zeros(3, j + 1, d, device=DEV))
    assert len(t._dev) == 1                                             # one cached device copy


# ---- statistics -----------------------------------------------------------------------------------------------------------
def test_stats_equal_host_at_every_size(pkg):
    side = torch.cuda.Stream(DEV)
    for n in stat_sizes(pkg):
        for w in STAT_WIDTHS:
            x = make_columns(n, w)
            want = host_stats(pkg, x)
            j, d = (w // 3, 3) if w % 3 == 0 else (w // 2, 2)
            xd = torch.from_numpy(x).to(DEV).reshape(n, j, d)
            got = pkg.pose_table.pose_stats_record(xd)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):                               # a second launch sequence on another stream
                again = pkg.pose_table.pose_stats_record(xd)
            side.synchronize()
            assert np.array_equal(bits64(got.cpu().numpy()), bits64(want)), (n, w)
            assert np.array_equal(bits64(again.cpu().numpy()), bits64(want)), (n, w)
    st = pkg.pose_stats(xd)
    assert tuple(st.mean.shape) == (j, d) and np.array_equal(bits64(st.std.numpy().reshape(-1)), bits64(want[1]))


def test_stats_nan_inf_and_constant_columns_equal_host(pkg):
    R = pkg.lib().pl_pose_stats_chunk_rows()
    n = 2 * R + 1
    x = make_columns(n, 51)
    x[n - 1, 3], x[0, 7], x[n // 2, 11] = np.nan, np.nan, np.inf
    x[:, 20], x[:, 0] = np.float32(0.1), 0.0
    want = host_stats(pkg, x)
    got = pkg.pose_table.pose_stats_record(torch.from_numpy(x).to(DEV).reshape(n, 17, 3)).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(bits64(got[ok]), bits64(want[ok]))
    assert np.isnan(got[:, [3, 7]]).all() and got[1, 20] == 0 and got[0, 20] == float(np.float32(0.1))


# ---- the transform inside the augmented gather -----------------------------------------------------------------------------
def dev_augment_t(pkg, a_t, b_t, src, rows, cfg, T2, T3, epoch=0):
    rid = torch.tensor(np.asarray(rows, dtype=np.uint64).view(np.int64), device=DEV)
    s = None if src is None else torch.tensor(np.asarray(src, dtype=np.int64), device=DEV)
    n = rid.numel()
    oa, ob = torch.full((n, 17, 2), -7.0, device=DEV), torch.full((n, 17, 3), -7.0, device=DEV)
    p2 = (None, None) if T2 is None else tuple(t.data_ptr() for t in T2.device_pair(DEV))
    p3 = (None, None) if T3 is None else tuple(t.data_ptr() for t in T3.device_pair(DEV))
    rc = pkg.lib().pl_pose_augment_gather_t(a_t.data_ptr(), b_t.data_ptr(), None if s is None else s.data_ptr(), rid.data_ptr(),
                                            n, a_t.shape[0], oa.data_ptr(), ob.data_ptr(), ctypes.byref(aug_struct(pkg, cfg)),
                                            int(epoch), p2[0], p2[1], p3[0], p3[1], pkg._lib.current_stream_ptr())
    assert rc == 0, pkg.lib().pl_last_error()
    torch.cuda.synchronize()
    return oa, ob


def test_augment_gather_t(pkg, table, transforms):
    T2, T3, t2, t3 = transforms
    a, b, idx = table
    a_t, b_t = torch.tensor(a).to(DEV), torch.tensor(b).to(DEV)
    rs = np.random.RandomState(11)
    big_src = rs.randint(0, TABLE_ROWS, 4096 + 5).astype(np.int64)
    big_rows = (np.arange(4096 + 5, dtype=np.uint64) * np.uint64(7919) + np.uint64(2 ** 32 - 1000))
    cases = [(idx, idx.astype(np.uint64)), (idx[3:4], idx[3:4].astype(np.uint64)), (big_src, big_rows)]
    for src, rows in cases:
        for kw in EXACT:                                               # no sincosf / logf: the host's bits
            cfg = aorc.config(**kw)
            for epoch in (0, 2 ** 32 + 3):
                ha, hb = host_augment_t(pkg, a, b, src, rows, cfg, t2, t3, epoch=epoch)
                da, db = dev_augment_t(pkg, a_t, b_t, src, rows, cfg, T2, T3, epoch=epoch)
                assert same_bits(da.cpu().numpy(), ha) and same_bits(db.cpu().numpy(), hb), (len(src), kw, epoch)
        for kw in TRANSCENDENTAL:                                      # the device's own augmentation, then the transform
            cfg = aorc.config(**kw)
            pa, pb = dev_augment_t(pkg, a_t, b_t, src, rows, cfg, None, None, epoch=1)
            da, db = dev_augment_t(pkg, a_t, b_t, src, rows, cfg, T2, T3, epoch=1)
            assert same_bits_t(da, T2.apply(pa)) and same_bits_t(db, T3.apply(pb)), (len(src), kw)
            oa, ob = dev_augment_t(pkg, a_t, b_t, src, rows, cfg, None, T3, epoch=1)
            assert same_bits_t(oa, pa) and same_bits_t(ob, db)
    # both NULL is pl_pose_augment_gather
    ya, yb = pkg.augment_poses(a_t[:67], b_t[:67], pkg.PoseAugment(p_flip=1.0), row_ids=torch.arange(67))
    na, nb = dev_augment_t(pkg, a_t[:67].contiguous(), b_t[:67].contiguous(), None, np.arange(67), aorc.config(p_flip=1.0), None, None)
    assert same_bits_t(ya, na) and same_bits_t(yb, nb)
    wa, wb = pkg.augment_poses(a_t[:67], b_t[:67], pkg.PoseAugment(p_flip=1.0), row_ids=torch.arange(67), transform_2d=T2,
                               transform_3d=T3)
    assert same_bits_t(wa, T2.apply(ya)) and same_bits_t(wb, T3.apply(yb))


def to_aug(pkg, cfg):
    return pkg.PoseAugment(p_flip=cfg["p_flip"], flip_offset=cfg["flip_offset"], max_rot=cfg["max_rot"],
                           scale_range=cfg["scale_range"], max_shift=cfg["max_shift"], jitter_sigma=cfg["jitter_sigma"],
                           centre=(cfg["cx"], cfg["cy"]), seed=cfg["seed"])


@pytest.mark.parametrize("resident", [True, False])
@pytest.mark.parametrize("augmented", [True, False])
def test_pose_feeder_with_transforms(pkg, table, transforms, resident, augmented):
    T2, T3, _, _ = transforms
    a, b, _ = table
    x, y = torch.tensor(a), torch.tensor(b)
    aug = to_aug(pkg, aorc.config(**ALL_ON)) if augmented else None
    plain = pkg.PoseFeeder(x, y, 96, device=DEV, seed=7, resident=resident, augment=aug)
    feed = pkg.PoseFeeder(x, y, 96, device=DEV, seed=7, resident=resident, augment=aug, transform_2d=T2, transform_3d=T3)
    only3 = pkg.PoseFeeder(x, y, 96, device=DEV, seed=7, resident=resident, augment=aug, transform_3d=T3)
    for f in (plain, feed, only3):
        f.set_epoch(1)
    sizes = []
    for (pa, pb), (fa, fb), (oa, ob) in zip(plain, feed, only3):
        sizes.append(pa.shape[0])
        assert same_bits_t(fa, T2.apply(pa)) and same_bits_t(fb, T3.apply(pb))
        assert same_bits_t(oa, pa) and same_bits_t(ob, fb)
        assert int((fb[:, 0] != 0).sum()) == 0                         # the root column has div = 0
    assert sizes == [96] * 10 + [40]
    with pytest.raises(ValueError):
        pkg.PoseFeeder(x, y, 96, device=DEV, transform_2d=T3)
    with pytest.raises(ValueError):
        pkg.PoseFeeder(x[:, :16], y[:, :16], 96, device=DEV, transform_3d=T3)


def test_resident_feeder_with_transforms_is_one_launch_per_batch(pkg, table, transforms):
    from torch.profiler import ProfilerActivity, profile
    T2, T3, _, _ = transforms
    a, b, _ = table
    for aug in (to_aug(pkg, aorc.config(**ALL_ON)), None):
        feeder = pkg.PoseFeeder(torch.tensor(a), torch.tensor(b), 96, device=DEV, seed=7, augment=aug, transform_2d=T2,
                                transform_3d=T3)
        for _ in feeder:                                               # code objects loaded, allocator warm
            pass
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            n_batches = sum(1 for _ in feeder)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        kernels = [n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()]
        assert n_batches == 11 and len(kernels) == 11, names
        assert all("pose_augment_gather_kernel" in n for n in kernels), kernels


@pytest.mark.parametrize("resident", [True, False])
def test_frame_feeder_with_transforms(pkg, table, transforms, resident):
    T2, T3, _, _ = transforms
    a, b, _ = table
    frames = torch.from_numpy(np.random.RandomState(9).randint(0, 256, (TABLE_ROWS, 8, 8, 3)).astype(np.uint8))
    x, y = torch.tensor(a), torch.tensor(b)
    aug = to_aug(pkg, aorc.config(**ALL_ON))
    kw = dict(out_hw=(8, 8), augment=aug, device=DEV, seed=7, resident=resident)
    plain = pkg.FrameFeeder(frames, x, y, 96, **kw)
    feed = pkg.FrameFeeder(frames, x, y, 96, transform_2d=T2, transform_3d=T3, **kw)
    n = 0
    for (pf, pa, pb), (ff, fa, fb) in zip(plain, feed):
        assert same_bits_t(ff, pf)                                     # frames are unchanged
        assert same_bits_t(fa, T2.apply(pa)) and same_bits_t(fb, T3.apply(pb))
        n += pf.shape[0]
    assert n == TABLE_ROWS


# ---- denorm: errors, meter, eval_step ------------------------------------------------------------------------------------
def joint_transform(pkg, J, seed=0):
    rs = np.random.RandomState(100 + J + seed)
    sub, div = rs.uniform(-0.3, 0.3, (J, 3)).astype(np.float32), rs.uniform(0.05, 0.6, (J, 3)).astype(np.float32)
    sub[0], div[0] = 0.0, 0.0
    return pkg.PoseTransform(sub, div)


@pytest.mark.parametrize("J", [3, 17, 32])
def test_pose_errors_denorm(pkg, J):
    T = joint_transform(pkg, J)
    for B in (1, 67, 4101):
        g = torch.Generator().manual_seed(B + J)
        t = torch.randn(B, J, 3, generator=g).to(DEV)
        p = (t.cpu() + 0.3 * torch.randn(B, J, 3, generator=g)).to(DEV)
        want = pkg.pose_errors(T.invert(p), T.invert(t))
        got = pkg.pose_errors(p, t, denorm=T)
        assert same_bits_t(got, want), (B, J)
        assert same_bits_t(pkg.procrustes_align(p, t, denorm=T), pkg.procrustes_align(T.invert(p), T.invert(t)))
        assert same_bits_t(pkg.loss_MPJPE(p, t, denorm=T), pkg.loss_MPJPE(T.invert(p), T.invert(t)))
        assert not same_bits_t(got, pkg.pose_errors(p, t))
    with pytest.raises(ValueError):
        pkg.pose_errors(p, t, denorm=joint_transform(pkg, J + 1))


def test_pose_metrics_denorm(pkg):
    T = joint_transform(pkg, 17)
    m1, m2 = pkg.PoseMetrics(groups=4, device=DEV), pkg.PoseMetrics(groups=4, device=DEV)
    for k, B in enumerate((67, 1, 300)):
        g = torch.Generator().manual_seed(k)
        t = torch.randn(B, 17, 3, generator=g).to(DEV)
        p = (t.cpu() + 0.3 * torch.randn(B, 17, 3, generator=g)).to(DEV)
        grp = torch.randint(0, 4, (B,), generator=g).to(DEV)
        m1.update(p, t, grp, denorm=T)
        m2.update(T.invert(p), T.invert(t), grp)
    assert m1.compute() == m2.compute()


def test_eval_step_denorm(pkg):
    torch.manual_seed(3)
    T = joint_transform(pkg, 17)
    model = pkg.LinearModel(34, 51, linear_size=64).to(DEV).eval()
    y1, y2 = pkg.synth.synthetic_batch(300, 77, DEV)
    y2 = T.apply(y2)
    grp = (torch.arange(300, device=DEV) % 3).int()
    loss0, metric0, hat0 = pkg.eval_step(model, y1, y2)
    m = pkg.PoseMetrics(groups=3, device=DEV)
    loss, metric, hat = pkg.eval_step(model, y1, y2, denorm=T, meter=m, group_ids=grp)
    assert same_bits_t(loss, loss0) and same_bits_t(hat, hat0)         # the MSE stays in the model's space
    assert same_bits_t(metric, pkg.loss_MPJPE(T.invert(hat), T.invert(y2))) and not same_bits_t(metric, metric0)
    m2 = pkg.PoseMetrics(groups=3, device=DEV)
    m2.update(T.invert(hat), T.invert(y2), grp)
    assert m.compute() == m2.compute()
    acc = metric.clone()
    pkg.eval_step(model, y1, y2, denorm=T, metric_out=acc)
    assert torch.allclose(acc, 2 * metric, rtol=1e-6)
    with pytest.raises(ValueError, match="flip_average"):
        pkg.eval_step(model, y1, y2, flip=True, denorm=T)


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_raw_arrays_to_millimetres(pkg):
    N = 2000
    rs = np.random.RandomState(21)
    cams = make_cameras()[:4]
    cams[:, 0:3] = rs.uniform(-0.5, 0.5, (4, 3))
    cid = rs.randint(0, 4, N).astype(np.int32)
    bones = rs.randn(1, 32, 3) * 0.25
    raw3d = (rs.randn(N, 1, 3) * 0.5 + bones * (1 + 0.3 * rs.randn(N, 1, 1)) + 0.05 * rs.randn(N, 32, 3)).astype(np.float32)
    cam3d = orc.prepare(raw3d, None, cams, cid).astype(np.float64)
    raw2d = (0.5 + cam3d[..., :2] / 8.0 + 0.02 * cam3d[..., 2:3]).astype(np.float32)      # a smooth stand-in for a projection
    t2d = pkg.prepare_poses(raw2d, pkg.H36M_17_OF_32, device=DEV)
    t3d = pkg.prepare_poses(raw3d, pkg.H36M_17_OF_32, cams, cid, zero_centre=True, device=DEV)
    assert same_bits(t3d.cpu().numpy(), orc.prepare(raw3d, H36M_17, cams, cid, True))
    s2, s3 = pkg.pose_stats(t2d), pkg.pose_stats(t3d)
    assert float(s3.std[0].abs().max()) == 0.0 and float(s3.std[1:].min()) > 0.0
    T2, T3 = pkg.PoseTransform.standardize(s2), pkg.PoseTransform.standardize(s3)
    torch.manual_seed(5)
    model = pkg.LinearModel(34, 51, linear_size=64, p_dropout=0.0).to(DEV).train()
    opt = pkg.FlatAdamW(model, lr=1e-3)
    feeder = pkg.PoseFeeder(t2d, t3d, 100, device=DEV, seed=1, augment=pkg.PoseAugment(p_flip=0.5, jitter_sigma=0.002, seed=4),
                            transform_2d=T2, transform_3d=T3)
    losses = [pkg.train_step(model, opt, y1, y2)[0] for y1, y2 in feeder]
    assert len(losses) == 20
    losses = torch.stack(losses).cpu().numpy()
    print(f"loss: first {losses[0]:.4f}, last {losses[-1]:.4f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    model.eval()
    B = 256
    y1, y2 = T2.apply(t2d[:B].contiguous()), T3.apply(t3d[:B].contiguous())
    loss, metric, hat = pkg.eval_step(model, y1, y2, denorm=T3)
    mm = float(metric.mean()) / B * 1000.0
    sub, div = T3.sub.numpy().astype(np.float64), T3.div.numpy().astype(np.float64)
    hat64 = np.where(div == 0, sub, hat.cpu().numpy().astype(np.float64) * div + sub)
    tgt64 = np.where(div == 0, sub, y2.cpu().numpy().astype(np.float64) * div + sub)
    want = np.linalg.norm(hat64 - tgt64, axis=-1).mean() * 1000.0
    raw_tgt = t3d[:B].cpu().numpy().astype(np.float64)
    against_raw = np.linalg.norm(hat64 - raw_tgt, axis=-1).mean() * 1000.0
    print(f"MPJPE {mm:.6f} mm; host recomputation {want:.6f} mm; against the raw table {against_raw:.6f} mm")
    assert abs(mm - want) < 1e-3 and abs(mm - against_raw) < 1e-3
    assert 1.0 < mm < 2000.0                                           # millimetres, not standard deviations
