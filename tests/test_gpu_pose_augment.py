"""GPU tests of the pose augmentation: pl_pose_augment_gather against pl_pose_augment_host (bit for bit where no sincosf /
logf is involved, otherwise both against the fp64 restatement under the 8x-fp32-twin gate of test_pose_augment_host.py),
PoseFeeder(augment=...) in both modes, augment_poses, and one augmented training epoch."""
import ctypes

import numpy as np
import pytest
import torch

import pose_augment_oracle as orc
from test_pose_augment_host import (ALL_ON, N_CASE, TABLE_ROWS, aug_struct, check_against_fp64, host_augment, make_table,
                                    same_bits)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


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
def cases(table):
    """(source rows, row ids) of the three sizes: 67 of 1000 (ragged group tail, non-monotone), 1, and 4096 + 5 (more than
    one wave per workgroup, many workgroups, a partial last one; row ids past 2^32)."""
    _, _, idx = table
    rs = np.random.RandomState(11)
    big_src = rs.randint(0, TABLE_ROWS, 4096 + 5).astype(np.int64)
    big_rows = (np.arange(4096 + 5, dtype=np.uint64) * np.uint64(7919) + np.uint64(2 ** 32 - 1000))
    return [(idx, idx.astype(np.uint64)), (idx[3:4], idx[3:4].astype(np.uint64)), (big_src, big_rows)]


def dev_augment(pkg, a_t, b_t, src, rows, cfg, epoch=0):
    """pl_pose_augment_gather on device tables a_t (R,17,2), b_t (R,17,3); src None = rows in order."""
    rid = torch.tensor(np.asarray(rows, dtype=np.uint64).view(np.int64), device=DEV)
    s = None if src is None else torch.tensor(np.asarray(src, dtype=np.int64), device=DEV)
    n = rid.numel()
    oa = torch.full((n, 17, 2), -7.0, device=DEV)
    ob = torch.full((n, 17, 3), -7.0, device=DEV)
    st = aug_struct(pkg, cfg)
    rc = pkg.lib().pl_pose_augment_gather(a_t.data_ptr(), b_t.data_ptr(), None if s is None else s.data_ptr(), rid.data_ptr(),
                                          n, a_t.shape[0], oa.data_ptr(), ob.data_ptr(), ctypes.byref(st), int(epoch),
                                          pkg._lib.current_stream_ptr())
    assert rc == 0, pkg.lib().pl_last_error()
    torch.cuda.synchronize()
    return oa.cpu().numpy(), ob.cpu().numpy()


EXACT = [dict(), dict(p_flip=1.0), dict(p_flip=0.5, seed=7), dict(p_flip=1.0, flip_offset=0.0),
         dict(scale_range=0.25, max_shift=0.1, seed=99), dict(scale_range=0.5, p_flip=0.5, cx=0.25, cy=0.75, seed=5),
         dict(max_shift=0.03, seed=2 ** 63 + 9)]
TRANSCENDENTAL = [ALL_ON, dict(max_rot=np.pi, seed=3), dict(jitter_sigma=0.05, seed=3),
                  dict(p_flip=0.5, max_rot=0.3, jitter_sigma=0.01, flip_offset=0.0, cx=0.0, cy=0.0, seed=8)]


def test_kernel_equals_host_entry_bit_for_bit(pkg, table, cases):
    a, b, _ = table
    a_t, b_t = torch.tensor(a).to(DEV), torch.tensor(b).to(DEV)
    for src, rows in cases:
        for kw in EXACT:
            cfg = orc.config(**kw)
            for epoch in (0, 2 ** 32 + 3):
                ha, hb = host_augment(pkg, a, b, src, rows, cfg, epoch=epoch)
                da, db = dev_augment(pkg, a_t, b_t, src, rows, cfg, epoch=epoch)
                assert same_bits(da, ha) and same_bits(db, hb), (len(src), kw, epoch)
        # the ungathered mode
        ga, gb = np.ascontiguousarray(a[src]), np.ascontiguousarray(b[src])
        cfg = orc.config(**EXACT[5])
        ha, hb = host_augment(pkg, ga, gb, None, rows, cfg, epoch=1)
        da, db = dev_augment(pkg, torch.from_numpy(ga).to(DEV), torch.from_numpy(gb).to(DEV), None, rows, cfg, epoch=1)
        assert same_bits(da, ha) and same_bits(db, hb)
        assert same_bits(da, host_augment(pkg, a, b, src, rows, cfg, epoch=1)[0])


def test_identity_writes_the_plain_gather(pkg, table, cases):
    a, b, _ = table
    a_t, b_t = torch.tensor(a).to(DEV), torch.tensor(b).to(DEV)
    for src, rows in cases:
        n = len(src)
        idx = torch.tensor(src, device=DEV)
        oa, ob = torch.empty(n, 17, 2, device=DEV), torch.empty(n, 17, 3, device=DEV)
        assert pkg.lib().pl_gather_rows2(a_t.data_ptr(), 34, b_t.data_ptr(), 51, idx.data_ptr(), n, TABLE_ROWS, oa.data_ptr(),
                                         ob.data_ptr(), pkg._lib.current_stream_ptr()) == 0
        da, db = dev_augment(pkg, a_t, b_t, src, rows, orc.config())
        assert same_bits(da, oa.cpu().numpy()) and same_bits(db, ob.cpu().numpy())


def test_kernel_rotation_and_jitter_against_fp64(pkg, table, cases):
    a, b, _ = table
    a_t, b_t = torch.tensor(a).to(DEV), torch.tensor(b).to(DEV)
    for src, rows in cases:
        for kw in TRANSCENDENTAL:
            cfg = orc.config(**kw)
            da, db = dev_augment(pkg, a_t, b_t, src, rows, cfg, epoch=1)
            if len(src) == 1:                    # the pose alone is the pose inside the n = 67 call
                full = dev_augment(pkg, a_t, b_t, cases[0][0], cases[0][1], cfg, epoch=1)
                assert same_bits(da, full[0][3:4]) and same_bits(db, full[1][3:4])
            what = f"device, n = {len(src)}, {'all stages on' if kw is ALL_ON else kw}"
            check_against_fp64(da, db, cfg, 1, rows, a[src], b[src], what)
            assert np.all(db[:, 0] == 0)
    # a source index outside the table reads nothing and yields a NaN pose; its neighbours are untouched
    src = cases[0][0].copy()
    src[[0, 40]] = [TABLE_ROWS, -1]
    da, db = dev_augment(pkg, a_t, b_t, src, cases[0][1], orc.config(**ALL_ON), epoch=1)
    good = dev_augment(pkg, a_t, b_t, cases[0][0], cases[0][1], orc.config(**ALL_ON), epoch=1)
    bad = np.zeros(N_CASE, bool)
    bad[[0, 40]] = True
    assert np.isnan(da[bad]).all() and np.isnan(db[bad]).all()
    assert same_bits(da[~bad], good[0][~bad]) and same_bits(db[~bad], good[1][~bad])


def to_aug(pkg, cfg):
    return pkg.PoseAugment(p_flip=cfg["p_flip"], flip_offset=cfg["flip_offset"], max_rot=cfg["max_rot"],
                           scale_range=cfg["scale_range"], max_shift=cfg["max_shift"], jitter_sigma=cfg["jitter_sigma"],
                           centre=(cfg["cx"], cfg["cy"]), seed=cfg["seed"])


def _epoch(feeder, epoch):
    feeder.set_epoch(epoch)
    out = [(ya.cpu().numpy(), yb.cpu().numpy()) for ya, yb in feeder]
    torch.cuda.synchronize()
    return out


def test_feeder_with_augment(pkg, table):
    a, b, _ = table
    x, y = torch.tensor(a), torch.tensor(b)
    a_t, b_t = x.to(DEV), y.to(DEV)
    cfg = orc.config(**ALL_ON)
    aug = to_aug(pkg, cfg)
    feed = lambda bs, **kw: pkg.PoseFeeder(x, y, bs, device=DEV, seed=7, augment=aug, **kw)
    for epoch in (0, 1):
        res = _epoch(feed(96), epoch)
        stre = _epoch(feed(96, resident=False), epoch)
        idx = pkg.epoch_indices(TABLE_ROWS, 96, epoch=epoch, seed=7)
        assert len(res) == len(stre) == len(idx) == 11 and idx[-1].numel() == 40
        for (ra, rb), (sa, sb), ix in zip(res, stre, idx):
            assert same_bits(ra, sa) and same_bits(rb, sb)
            ka, kb = dev_augment(pkg, a_t, b_t, ix.numpy(), ix.numpy(), cfg, epoch=epoch)
            assert same_bits(ra, ka) and same_bits(rb, kb)
        # two ranks of 48 concatenated are the world-1 batch
        for resident in (True, False):
            r0 = _epoch(feed(48, rank=0, world=2, resident=resident), epoch)
            r1 = _epoch(feed(48, rank=1, world=2, resident=resident), epoch)
            assert len(r0) == len(r1) == 11
            for (wa, wb), (pa, pb), (qa, qb) in zip(res, r0, r1):
                assert same_bits(wa, np.concatenate([pa, qa])) and same_bits(wb, np.concatenate([pb, qb]))
        # another batch size: every dataset row gets the same augmented pose
        by_row = {}
        for bs, batches in ((96, res), (40, _epoch(feed(40), epoch))):
            ix = torch.cat(pkg.epoch_indices(TABLE_ROWS, bs, epoch=epoch, seed=7)).numpy()
            fa, fb = np.empty_like(a), np.empty_like(b)
            fa[ix], fb[ix] = np.concatenate([p for p, _ in batches]), np.concatenate([q for _, q in batches])
            by_row[bs] = (fa, fb)
        assert same_bits(by_row[96][0], by_row[40][0]) and same_bits(by_row[96][1], by_row[40][1])
    assert not same_bits(_epoch(feed(96, shuffle=False), 0)[0][0], _epoch(feed(96, shuffle=False), 1)[0][0])   # fresh draws
    # no augment, and the default one: today's batches
    for resident in (True, False):
        for augment in (None, pkg.PoseAugment()):
            fd = pkg.PoseFeeder(x, y, 96, device=DEV, seed=7, resident=resident, augment=augment)
            for (pa, pb), ix in zip(_epoch(fd, 1), pkg.epoch_indices(TABLE_ROWS, 96, epoch=1, seed=7)):
                assert same_bits(pa, a[ix.numpy()]) and same_bits(pb, b[ix.numpy()])


def test_resident_feeder_is_one_launch_per_batch(pkg, table):
    """With an augment the resident feeder launches one kernel per batch -- the augmenting gather -- and nothing else."""
    from torch.profiler import ProfilerActivity, profile
    a, b, _ = table
    feeder = pkg.PoseFeeder(torch.tensor(a), torch.tensor(b), 96, device=DEV, seed=7, augment=to_aug(pkg, orc.config(**ALL_ON)))
    for _ in feeder:                                                   # code objects loaded, allocator warm
        pass
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        n_batches = sum(1 for _ in feeder)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    kernels = [n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()]
    assert n_batches == 11 and len(kernels) == 11, names
    assert all("pose_augment_gather_kernel" in n for n in kernels), kernels


def test_augment_poses(pkg, table):
    a, b, _ = table
    x, y = torch.tensor(a), torch.tensor(b)
    aug = to_aug(pkg, orc.config(**ALL_ON))
    plain = pkg.PoseFeeder(x, y, 96, device=DEV, seed=7)
    augd = pkg.PoseFeeder(x, y, 96, device=DEV, seed=7, augment=aug)
    plain.set_epoch(1), augd.set_epoch(1)
    ix = pkg.epoch_indices(TABLE_ROWS, 96, epoch=1, seed=7)[0]
    (y1, y2), (w1, w2) = next(iter(plain)), next(iter(augd))
    k1, k2 = y1.clone(), y2.clone()
    o1, o2 = pkg.augment_poses(y1, y2, aug, row_ids=ix, epoch=1)
    assert torch.equal(o1, w1) and torch.equal(o2, w2)
    assert torch.equal(y1, k1) and torch.equal(y2, k2)
    assert len({t.data_ptr() for t in (y1, y2, o1, o2)}) == 4 and o1.shape == y1.shape and o2.shape == y2.shape
    d1, d2 = pkg.augment_poses(y1, y2, aug)                           # row_ids = arange(B), epoch 0
    e1, e2 = pkg.augment_poses(y1, y2, aug, row_ids=torch.arange(96, device=DEV), epoch=0)
    assert torch.equal(d1, e1) and torch.equal(d2, e2) and not torch.equal(d1, o1)
    with pytest.raises(ValueError):
        pkg.augment_poses(y1[:, :16].contiguous(), y2[:, :16].contiguous(), aug)
    with pytest.raises(ValueError):
        pkg.augment_poses(y1, y2, aug, row_ids=ix[:5])
    with pytest.raises(pkg.PoseliftError):
        pkg.augment_poses(y1.cpu(), y2, aug)


def test_one_augmented_training_epoch(pkg, table):
    a, b, _ = table
    torch.manual_seed(0)
    model = pkg.LinearModel(34, 51, linear_size=64).to(DEV)
    opt = pkg.FlatAdamW(model, lr=1e-3)
    aug = pkg.PoseAugment(p_flip=0.5, jitter_sigma=0.05, seed=3)
    feeder = pkg.PoseFeeder(torch.tensor(a), torch.tensor(b), 96, device=DEV, seed=7, augment=aug)
    model.train()
    losses, last = [], None
    for y1, y2 in feeder:
        loss, _ = pkg.train_step(model, opt, y1, y2)
        losses.append(loss)
        last = y1
    assert len(losses) == 11 and bool(torch.isfinite(torch.stack([l.reshape(()) for l in losses])).all())
    model.eval()
    got = pkg.predict_flip_tta(model, last)
    with torch.no_grad():
        two_pass = (pkg.flip_pose(model(pkg.flip_pose(last)).reshape(-1, 17, 3)) + model(last).reshape(-1, 17, 3)) / 2
    assert torch.equal(got.reshape(-1, 17, 3), two_pass)


def test_feeder_rejects_other_tables_with_an_augment(pkg):
    x, y = torch.zeros(8, 16, 2), torch.zeros(8, 16, 3)
    pkg.PoseFeeder(x, y, 4, device=DEV)                               # fine without
    with pytest.raises(ValueError):
        pkg.PoseFeeder(x, y, 4, device=DEV, augment=pkg.PoseAugment(p_flip=0.5))
    with pytest.raises(ValueError):
        pkg.PoseFeeder(torch.zeros(8, 34), torch.zeros(8, 51), 4, device=DEV, augment=pkg.PoseAugment())
    with pytest.raises(TypeError):
        pkg.PoseFeeder(torch.zeros(8, 17, 2), torch.zeros(8, 17, 3), 4, device=DEV, augment=dict(p_flip=0.5))
