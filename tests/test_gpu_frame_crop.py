"""GPU tests of the person-centred crop: the crop forms of pl_pose_augment_gather and pl_frame_warp_gather, pl_pose_crop_boxes
and pl_crop_poses against their _host forms (bit for bit where no sincosf is involved, otherwise against the fp64 restatement
under the 8x-fp32-twin gate of test_frame_crop_host.py; boxes bit for bit always), every kernel form, FrameFeeder(crop=) in
both modes, and crop_poses / uncrop_poses with their gradients."""
import ctypes

import numpy as np
import pytest
import torch

import frame_crop_oracle as fco
import pose_augment_oracle as pao
from test_frame_warp_host import ALL_ON, DTYPES, EXACT, U8, F32, aug_struct, default_scale, make_frames, same_bits, warp_args
from test_frame_crop_host import (ROWS, SHAPES, SPECIAL_HW, SPECS, SRC_IDX, TABLE_FRAMES, check_crop_against_fp64, crop_struct,
                                  host_augment, host_boxes, host_crop_map, host_crop_warp, make_poses, make_targets, rotation_case,
                                  same_or_nan, slice_with_fill, special_poses)
from test_gpu_frame_warp import dev_warp, to_aug

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


def to_crop(pkg, sp):
    return pkg.PersonCrop(margin=sp["margin"], centre=sp["centre"], min_side=sp["min_side"])


def dev_crop_warp(pkg, table_t, a_t, src, rows, cfg, sp, out_hw, epoch=0, scale=None, fill=0.0):
    """pl_frame_warp_gather_crop on a device table (N, Hs, Ws, 3) and device poses indexed like it; sp None = no PLPoseCrop."""
    rid = torch.tensor(np.asarray(rows, dtype=np.uint64).view(np.int64), device=DEV)
    s = None if src is None else torch.tensor(np.asarray(src, dtype=np.int64), device=DEV)
    n = rid.numel()
    out = torch.full((n,) + tuple(out_hw) + (3,), -7.0, device=DEV)
    u8 = table_t.dtype == torch.uint8
    scale = (1.0 / 256.0 if u8 else 1.0) if scale is None else scale
    w = warp_args(pkg, table_t.data_ptr(), U8 if u8 else F32, table_t.shape, None if s is None else s.data_ptr(), rid.data_ptr(),
                  n, out.data_ptr(), out_hw, scale, fill, None if cfg is None else aug_struct(pkg, cfg), epoch)
    cs = None if sp is None else crop_struct(pkg, sp, table_t.shape[1:3])
    rc = pkg.lib().pl_frame_warp_gather_crop(ctypes.byref(w), ctypes.byref(cs) if cs is not None else None,
                                             a_t.data_ptr() if cs is not None else None, pkg._lib.current_stream_ptr())
    assert rc == 0, pkg.lib().pl_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def dev_augment(pkg, a_t, b_t, src, rows, cfg, sp, src_hw, epoch=0, xf=None):
    """pl_pose_augment_gather_crop(_t) on device tables; sp None = no PLPoseCrop.  -> numpy (oa, ob, boxes)."""
    rid = torch.tensor(np.asarray(rows, dtype=np.uint64).view(np.int64), device=DEV)
    s = None if src is None else torch.tensor(np.asarray(src, dtype=np.int64), device=DEV)
    n = rid.numel()
    oa, ob, bx = torch.full((n, 17, 2), -7.0, device=DEV), torch.full((n, 17, 3), -7.0, device=DEV), torch.full((n, 4), -7.0, device=DEV)
    st, cs = aug_struct(pkg, cfg), None if sp is None else crop_struct(pkg, sp, src_hw)
    crop_args = (ctypes.byref(cs) if cs is not None else None, bx.data_ptr() if cs is not None else None)
    head = (a_t.data_ptr(), b_t.data_ptr(), None if s is None else s.data_ptr(), rid.data_ptr(), n, a_t.shape[0], oa.data_ptr(),
            ob.data_ptr(), ctypes.byref(st), int(epoch))
    if xf is None:
        rc = pkg.lib().pl_pose_augment_gather_crop(*head, *crop_args, pkg._lib.current_stream_ptr())
    else:
        keep = [None if t is None else torch.tensor(t, device=DEV) for t in xf]
        rc = pkg.lib().pl_pose_augment_gather_crop_t(*head, *(None if t is None else t.data_ptr() for t in keep), *crop_args,
                                                     pkg._lib.current_stream_ptr())
    assert rc == 0, pkg.lib().pl_last_error()
    torch.cuda.synchronize()
    return oa.cpu().numpy(), ob.cpu().numpy(), bx.cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernels_equal_host_entries_bit_for_bit(pkg, dtype):
    """Rotation-free configurations, VEC (Wo % 4 == 0) and the tail path, gathered and in order; uint8 tables take the packed
    tap loads (the allocation is 4-byte aligned)."""
    a, b = make_poses(TABLE_FRAMES, 17), make_targets(TABLE_FRAMES, 18)
    a_t, b_t = torch.tensor(a).to(DEV), torch.tensor(b).to(DEV)
    for src_hw, out_hw in SHAPES:
        table = make_frames(src_hw, dtype)
        table_t = torch.tensor(table).to(DEV)
        assert table_t.data_ptr() % 4 == 0
        for sp in SPECS[:3]:
            for kw in EXACT:
                cfg = pao.config(**kw)
                for epoch, fill in ((3, 0.0), (2 ** 32 + 3, 0.5)):
                    h = host_crop_warp(pkg, table, a, SRC_IDX, ROWS, cfg, sp, out_hw, epoch=epoch, fill=fill)
                    d = dev_crop_warp(pkg, table_t, a_t, SRC_IDX, ROWS, cfg, sp, out_hw, epoch=epoch, fill=fill)
                    assert same_bits(d, h), (src_hw, out_hw, sp, kw, epoch)
                    if out_hw == SHAPES[0][1]:                                  # the pose launch does not depend on the output size
                        hp, dp = host_augment(pkg, a, b, SRC_IDX, ROWS, cfg, sp, src_hw, epoch=epoch), \
                            dev_augment(pkg, a_t, b_t, SRC_IDX, ROWS, cfg, sp, src_hw, epoch=epoch)
                        assert all(same_bits(x, y) for x, y in zip(dp, hp)), (src_hw, sp, kw, epoch)
        # no PLPoseAug, and the ungathered mode
        sp, cfg = SPECS[0], pao.config(**EXACT[4])
        assert same_bits(dev_crop_warp(pkg, table_t, a_t, SRC_IDX, ROWS, None, sp, out_hw), host_crop_warp(pkg, table, a, SRC_IDX, ROWS, None, sp, out_hw))
        g, ga, gb = np.ascontiguousarray(table[SRC_IDX]), np.ascontiguousarray(a[SRC_IDX]), np.ascontiguousarray(b[SRC_IDX])
        d = dev_crop_warp(pkg, torch.tensor(g).to(DEV), torch.tensor(ga).to(DEV), None, ROWS, cfg, sp, out_hw, epoch=1)
        assert same_bits(d, host_crop_warp(pkg, g, ga, None, ROWS, cfg, sp, out_hw, epoch=1))
        assert same_bits(d, dev_crop_warp(pkg, table_t, a_t, SRC_IDX, ROWS, cfg, sp, out_hw, epoch=1))
        dp = dev_augment(pkg, torch.tensor(ga).to(DEV), torch.tensor(gb).to(DEV), None, ROWS, cfg, sp, src_hw, epoch=1)
        assert all(same_bits(x, y) for x, y in zip(dp, host_augment(pkg, a, b, SRC_IDX, ROWS, cfg, sp, src_hw, epoch=1)))
        # a table at an odd address: the kernel's aligned-dword tap loads do not apply
        if dtype == np.uint8:
            flat = torch.zeros(table.size + 1, dtype=torch.uint8, device=DEV)
            odd = flat[1:].view(table.shape)
            odd.copy_(table_t)
            assert odd.data_ptr() % 4 == 1
            assert same_bits(dev_crop_warp(pkg, odd, a_t, SRC_IDX, ROWS, cfg, sp, out_hw, epoch=1), host_crop_warp(pkg, table, a, SRC_IDX, ROWS, cfg, sp, out_hw, epoch=1))
    # the _t form: the transform behind the crop and the augmentation
    sub = (np.random.RandomState(1).rand(34).astype(np.float32), np.random.RandomState(2).rand(34).astype(np.float32) + 0.5,
           np.random.RandomState(3).rand(51).astype(np.float32), np.random.RandomState(4).rand(51).astype(np.float32) + 0.5)
    for xf in (sub, sub[:2] + (None, None)):
        dp = dev_augment(pkg, a_t, b_t, SRC_IDX, ROWS, pao.config(**EXACT[4]), SPECS[0], (37, 53), epoch=1, xf=xf)
        assert all(same_bits(x, y) for x, y in zip(dp, host_augment(pkg, a, b, SRC_IDX, ROWS, pao.config(**EXACT[4]), SPECS[0], (37, 53), epoch=1, xf=xf)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_three_exact_cases_on_the_device(pkg, dtype):
    """side == Wo == Ho against slicing and torch.flip, 12 (VEC) and 13 (tail path); side == 2 Wo against the block mean."""
    table = make_frames((37, 53), dtype)
    n = 24
    frames = np.ascontiguousarray(table[(np.arange(n) * 5) % TABLE_FRAMES])
    rows = np.arange(n, dtype=np.uint64)
    tight = make_poses(n, 3, lo=0.0, hi=1.0, rmin=0.001, rmax=0.01)
    f_t, tight_t = torch.tensor(frames).to(DEV), torch.tensor(tight).to(DEV)
    scale = default_scale(dtype)
    for side in (12, 13):
        sp = fco.spec(1.25, "bbox", side)
        bx = host_boxes(pkg, tight, sp, (37, 53))
        want, ok = slice_with_fill(frames, bx, side, 0.25, scale)
        assert (~ok).any() and ok.all(axis=(1, 2)).any()
        assert same_bits(dev_crop_warp(pkg, f_t, tight_t, None, rows, pao.config(), sp, (side, side), fill=0.25), want)
        d = dev_crop_warp(pkg, f_t, tight_t, None, rows, pao.config(p_flip=1.0), sp, (side, side), fill=0.25)
        assert same_bits(d, torch.flip(torch.from_numpy(want), (2,)).numpy())
    inner = make_poses(n, 4, lo=0.45, hi=0.55, rmin=0.001, rmax=0.01)
    sp = fco.spec(1.25, "bbox", 24)
    f, ok = slice_with_fill(frames, host_boxes(pkg, inner, sp, (37, 53)), 24, 0.0, 1.0)
    assert ok.all()
    h = np.float32(0.5)
    want = np.float32(scale) * (h * (h * f[:, 0::2, 0::2] + h * f[:, 0::2, 1::2]) + h * (h * f[:, 1::2, 0::2] + h * f[:, 1::2, 1::2]))
    assert same_bits(dev_crop_warp(pkg, f_t, torch.tensor(inner).to(DEV), None, rows, pao.config(), sp, (12, 12)), want)


def test_box_on_the_last_bytes_of_the_table(pkg):
    """A box over the bottom-right corner of the LAST frame of a 4-byte-aligned uint8 table: its taps are the table's last
    bytes, where the packed tap loads' dword triples would reach past the end and the quads fall back to single loads.  The
    table is exactly its allocation's size request; the result is the host's, bit for bit."""
    src_hw = (37, 53)
    table = make_frames(src_hw, np.uint8)
    a = np.array(make_poses(TABLE_FRAMES, 17))
    a[TABLE_FRAMES - 1] = np.float32([51.0 / 53, 35.0 / 37])                      # all joints in the corner: a min_side box around it
    table_t, a_t = torch.tensor(table).to(DEV), torch.tensor(a).to(DEV)
    assert table_t.data_ptr() % 4 == 0
    src, rows = np.array([TABLE_FRAMES - 1, 0, TABLE_FRAMES - 1]), np.array([5, 6, 7], dtype=np.uint64)
    for side, out_hw in ((8, (8, 8)), (8, (18, 27)), (12, (20, 28))):
        sp = fco.spec(1.25, "bbox", side)
        bx = host_boxes(pkg, a[src], sp, src_hw)
        assert bx[0, 0] + side > 53 > bx[0, 0] and bx[0, 1] + side > 37 > bx[0, 1]      # the corner pixel is inside the box
        for cfg in (pao.config(), pao.config(p_flip=1.0), pao.config(**EXACT[3])):
            h = host_crop_warp(pkg, table, a, src, rows, cfg, sp, out_hw, epoch=2)
            assert same_bits(dev_crop_warp(pkg, table_t, a_t, src, rows, cfg, sp, out_hw, epoch=2), h)
        if out_hw == (8, 8):                                                        # the corner pixel itself is copied
            last = table[-1, -1, -1].astype(np.float32) * np.float32(1.0 / 256.0)
            j, i = int(52 - bx[0, 0]), int(36 - bx[0, 1])
            assert same_bits(host_crop_warp(pkg, table, a, src, rows, pao.config(), sp, out_hw)[0, i, j], last)


def test_bad_source_index_and_nan_poses(pkg):
    """A source index outside the table: NaN frame, NaN 2-D and 3-D pose, NaN box, every other row bitwise that of a clean
    call.  A pose with a non-finite coordinate: NaN frame, NaN 2-D pose and NaN box, as on the host."""
    table = make_frames((37, 53), np.uint8)
    a, b = make_poses(TABLE_FRAMES, 17), make_targets(TABLE_FRAMES, 18)
    table_t, a_t, b_t = torch.tensor(table).to(DEV), torch.tensor(a).to(DEV), torch.tensor(b).to(DEV)
    cfg, sp = pao.config(**ALL_ON), SPECS[0]
    src = SRC_IDX.copy()
    src[[1, 3]] = [TABLE_FRAMES, -1]
    bad = np.zeros(5, bool)
    bad[[1, 3]] = True
    for out_hw in ((20, 28), (18, 27)):
        good = dev_crop_warp(pkg, table_t, a_t, SRC_IDX, ROWS, cfg, sp, out_hw, epoch=1)
        d = dev_crop_warp(pkg, table_t, a_t, src, ROWS, cfg, sp, out_hw, epoch=1)
        assert np.isnan(d[bad]).all() and np.isfinite(good).all() and same_bits(d[~bad], good[~bad])
    good = dev_augment(pkg, a_t, b_t, SRC_IDX, ROWS, cfg, sp, (37, 53), epoch=1)
    d = dev_augment(pkg, a_t, b_t, src, ROWS, cfg, sp, (37, 53), epoch=1)
    for x, y in zip(d, good):
        assert np.isnan(x[bad]).all() and np.isfinite(y).all() and same_bits(x[~bad], y[~bad])
    for dtype in DTYPES:
        sa, sb = special_poses(), make_targets(8, 2)
        st = make_frames(SPECIAL_HW, dtype, n=8)
        rows = np.arange(8, dtype=np.uint64)
        exact = pao.config(**dict(ALL_ON, max_rot=0.0, jitter_sigma=0.0))          # no sincosf, no logf: host and device agree bit for bit
        for out_hw in ((20, 28), (18, 27)):
            d = dev_crop_warp(pkg, torch.tensor(st).to(DEV), torch.tensor(sa).to(DEV), None, rows, exact, sp, out_hw, epoch=1)
            assert same_or_nan(d, host_crop_warp(pkg, st, sa, None, rows, exact, sp, out_hw, epoch=1)) and np.isnan(d[2:6]).all()
        dp = dev_augment(pkg, torch.tensor(sa).to(DEV), torch.tensor(sb).to(DEV), None, rows, exact, sp, SPECIAL_HW, epoch=1)
        hp = host_augment(pkg, sa, sb, None, rows, exact, sp, SPECIAL_HW, epoch=1)
        assert all(same_or_nan(x, y) for x, y in zip(dp, hp)) and np.isnan(dp[0][2:6]).all() and np.isnan(dp[2][2:6]).all()
        assert np.isfinite(dp[1]).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernels_with_rotation_against_fp64(pkg, dtype):
    for src_hw, out_hw in SHAPES:
        case = rotation_case(src_hw, out_hw)
        cfg, epoch, rows, src, a, b, sp = case
        table = make_frames(src_hw, dtype)
        a_t, b_t = torch.tensor(a).to(DEV), torch.tensor(b).to(DEV)
        d = dev_crop_warp(pkg, torch.tensor(table).to(DEV), a_t, src, rows, cfg, sp, out_hw, epoch=epoch)
        oa, ob, bx = dev_augment(pkg, a_t, b_t, src, rows, cfg, sp, src_hw, epoch=epoch)
        assert same_bits(bx, host_boxes(pkg, a[src], sp, src_hw))                      # boxes: bit for bit always
        check_crop_against_fp64(d, oa, bx, case, table, out_hw, default_scale(dtype), 0.0,
                                f"device, crop + all stages on, {np.dtype(dtype).name} {src_hw} -> {out_hw}, rows 0..39")


def test_boxes_and_pose_maps_on_the_device(pkg):
    """crop_boxes against the host boxes; crop_poses / uncrop_poses forward and backward against the host results."""
    src_hw = (37, 53)
    for sp in SPECS:
        for a in (make_poses(40, 48), special_poses()):
            hw = src_hw if len(a) == 40 else SPECIAL_HW
            d = pkg.crop_boxes(torch.tensor(a).to(DEV), to_crop(pkg, sp), hw)
            assert d.shape == (len(a), 4) and same_or_nan(d.cpu().numpy(), host_boxes(pkg, a, sp, hw))
    p, g = make_poses(40, 31), np.random.RandomState(33).randn(40, 17, 2).astype(np.float32)
    bx = host_boxes(pkg, make_poses(40, 32), SPECS[0], src_hw)
    bx[3] = np.nan
    bx_t = torch.tensor(bx).to(DEV)
    pt = torch.tensor(p, device=DEV, requires_grad=True)
    c = pkg.crop_poses(pt, bx_t, src_hw)
    back = pkg.uncrop_poses(c, bx_t, src_hw)
    back.backward(torch.tensor(g).to(DEV))
    hc = host_crop_map(pkg, p, bx, src_hw, 0)
    assert same_or_nan(c.detach().cpu().numpy(), hc) and same_or_nan(back.detach().cpu().numpy(), host_crop_map(pkg, hc, bx, src_hw, 1))
    hg = host_crop_map(pkg, host_crop_map(pkg, g, bx, src_hw, 1, offset=0), bx, src_hw, 0, offset=0)
    assert same_or_nan(pt.grad.cpu().numpy(), hg) and np.isnan(hg[3]).all() and np.isfinite(np.delete(hg, 3, 0)).all()
    for fn, inv in ((pkg.crop_poses, 0), (pkg.uncrop_poses, 1)):                      # each map's own gradient
        q = torch.tensor(p, device=DEV, requires_grad=True)
        fn(q, bx_t, src_hw).backward(torch.tensor(g).to(DEV))
        assert same_or_nan(q.grad.cpu().numpy(), host_crop_map(pkg, g, bx, src_hw, inv, offset=0))
    with torch.no_grad():
        assert not pkg.uncrop_poses(pt, bx_t, src_hw).requires_grad


def test_no_crop_is_the_call_without(pkg):
    """crop=None: augment_poses, augment_frames and the device entry points give the bits of the calls without a crop."""
    table = make_frames((37, 53), np.uint8)
    a, b = make_poses(TABLE_FRAMES, 17), make_targets(TABLE_FRAMES, 18)
    table_t, a_t, b_t = torch.tensor(table).to(DEV), torch.tensor(a).to(DEV), torch.tensor(b).to(DEV)
    rid = torch.tensor(ROWS.view(np.int64), device=DEV)
    idx = torch.tensor(SRC_IDX, device=DEV)
    for kw in EXACT + [ALL_ON]:
        cfg = pao.config(**kw)
        aug = to_aug(pkg, cfg)
        for out_hw in ((20, 28), (18, 27)):
            assert same_bits(dev_crop_warp(pkg, table_t, a_t, SRC_IDX, ROWS, cfg, None, out_hw, epoch=3),
                             dev_warp(pkg, table_t, SRC_IDX, ROWS, cfg, out_hw, epoch=3))
        fr, ya, yb = table_t[idx].contiguous(), a_t[idx].contiguous(), b_t[idx].contiguous()
        plain = pkg.augment_frames(fr, aug, row_ids=rid, epoch=3, out_hw=(20, 28))
        assert torch.equal(pkg.augment_frames(fr, aug, row_ids=rid, epoch=3, out_hw=(20, 28), crop=None, x2d=ya), plain)
        assert same_bits(plain.cpu().numpy(), dev_warp(pkg, table_t, SRC_IDX, ROWS, cfg, (20, 28), epoch=3))
        out = pkg.augment_poses(ya, yb, aug, row_ids=rid, epoch=3, crop=None, frame_hw=(37, 53))
        assert len(out) == 2
        da, db, _ = dev_augment(pkg, a_t, b_t, SRC_IDX, ROWS, cfg, None, None, epoch=3)
        assert same_bits(out[0].cpu().numpy(), da) and same_bits(out[1].cpu().numpy(), db)
        ref = pkg.augment_poses(ya, yb, aug, row_ids=rid, epoch=3)
        assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])


@pytest.fixture(scope="module")
def feeder_tables(pkg):
    n = 23
    frames = torch.tensor(make_frames((19, 25), np.uint8, n=n))
    return frames, torch.tensor(make_poses(n, 77)), torch.tensor(make_targets(n, 78))


def _epoch(feeder, epoch):
    feeder.set_epoch(epoch)
    out = [tuple(t.cpu().numpy() for t in batch) for batch in feeder]
    torch.cuda.synchronize()
    return out


def test_frame_feeder_with_a_crop(pkg, feeder_tables):
    frames, x, y = feeder_tables
    f_t, x_t, y_t = frames.to(DEV), x.to(DEV), y.to(DEV)
    aug, sp = to_aug(pkg, pao.config(**ALL_ON)), SPECS[0]
    crop, hw, src_hw = to_crop(pkg, sp), (12, 16), (19, 25)
    feed = lambda bs, **kw: pkg.FrameFeeder(frames, x, y, bs, out_hw=hw, device=DEV, seed=7, augment=aug, crop=crop, **kw)
    for epoch in (0, 1):
        res, stre = _epoch(feed(8), epoch), _epoch(feed(8, resident=False), epoch)
        idx = pkg.epoch_indices(23, 8, epoch=epoch, seed=7)
        assert len(res) == len(stre) == len(idx) == 3
        by_row = {}
        for r4, s4, ix in zip(res, stre, idx):
            assert len(r4) == len(s4) == 4 and r4[0].shape == (ix.numel(),) + hw + (3,) and r4[3].shape == (ix.numel(), 4)
            assert all(same_bits(p, q) for p, q in zip(r4, s4))                        # resident and streamed: the same bits
            ixd = ix.to(DEV)
            xs = x_t[ixd].contiguous()
            # the frame launch's box is the pose launch's: the same frames from augment_frames(x2d=...), the same boxes from
            # augment_poses, crop_boxes and the host
            kf = pkg.augment_frames(f_t[ixd].contiguous(), aug, row_ids=ixd, epoch=epoch, out_hw=hw, crop=crop, x2d=xs)
            ka, kb, kbx = pkg.augment_poses(xs, y_t[ixd].contiguous(), aug, row_ids=ixd, epoch=epoch, crop=crop, frame_hw=src_hw)
            assert same_bits(r4[0], kf.cpu().numpy()) and same_bits(r4[1], ka.cpu().numpy()) and same_bits(r4[2], kb.cpu().numpy())
            assert same_bits(r4[3], kbx.cpu().numpy()) and same_bits(r4[3], pkg.crop_boxes(xs, crop, src_hw).cpu().numpy())
            assert same_bits(r4[3], host_boxes(pkg, x.numpy()[ix.numpy()], sp, src_hw))
            # and that box is the one the frame shows: the frame is the host's warp with the crop
            if epoch == 0 and ix is idx[0]:
                exact_frame = host_crop_warp(pkg, frames.numpy(), x.numpy(), ix.numpy(), ix.numpy(), None, sp, hw)
                pf = _epoch(pkg.FrameFeeder(frames, x, y, 8, out_hw=hw, device=DEV, seed=7, crop=crop), 0)[0]
                assert same_bits(pf[0], exact_frame) and same_bits(pf[3], r4[3])
                assert same_bits(pf[1], host_crop_map(pkg, x.numpy()[ix.numpy()], pf[3], src_hw, 0)) and same_bits(pf[2], y.numpy()[ix.numpy()])
            for k, r in enumerate(ix.tolist()):
                by_row[r] = tuple(t[k] for t in r4)
        assert sorted(by_row) == list(range(23))
        # another batch size, and two ranks of 4: every row the same bits
        for got, ixs in [(_epoch(feed(5), epoch), pkg.epoch_indices(23, 5, epoch=epoch, seed=7))] + \
                [(_epoch(feed(4, rank=rank, world=2, resident=resident), epoch), pkg.epoch_indices(23, 4, epoch=epoch, seed=7, rank=rank, world=2))
                 for rank in (0, 1) for resident in (True, False)]:
            assert len(got) == len(ixs)
            for g4, ix in zip(got, ixs):
                for k, r in enumerate(ix.tolist()):
                    assert all(same_bits(g4[t][k], by_row[r][t]) for t in range(4)), (r, epoch)
    # without a crop the batches are the 3-tuples they were
    three = _epoch(pkg.FrameFeeder(frames, x, y, 8, out_hw=hw, device=DEV, seed=7, augment=aug), 0)
    assert all(len(t) == 3 for t in three)


def test_crop_feeder_is_two_launches_per_batch(pkg, feeder_tables):
    from torch.profiler import ProfilerActivity, profile
    frames, x, y = feeder_tables
    feeder = pkg.FrameFeeder(frames, x, y, 8, out_hw=(12, 16), device=DEV, seed=7, augment=to_aug(pkg, pao.config(**ALL_ON)),
                             crop=pkg.PersonCrop())
    for _ in feeder:                                                   # code objects loaded, allocator warm
        pass
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in feeder:
            pass
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    ks = [n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()]
    assert len(ks) == 6, ks
    assert sum("frame_warp_gather_kernel" in n for n in ks) == 3 and sum("pose_augment_gather_kernel" in n for n in ks) == 3, ks
