"""GPU tests of the frame warp: pl_frame_warp_gather against pl_frame_warp_host (bit for bit where no sincosf is involved,
otherwise against the fp64 restatement under the 8x-fp32-twin gate of test_frame_warp_host.py), the reference's frame size,
a table past 2^31 bytes, FrameFeeder in both modes, augment_frames and its capture in a graph."""
import ctypes

import numpy as np
import pytest
import torch

import frame_warp_oracle as fwo
import pose_augment_oracle as pao
from test_frame_warp_host import (ALL_ON, DTYPES, EXACT, ROWS, SHAPES, SRC_IDX, TABLE_FRAMES, U8, F32, aug_struct,
                                  check_against_fp64, default_scale, host_warp, make_frames, same_bits, warp_args)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


def dev_warp(pkg, table_t, src, rows, cfg, out_hw, epoch=0, scale=None, fill=0.0):
    """pl_frame_warp_gather on a device table (N, Hs, Ws, 3); src None = frames in order; cfg None = no PLPoseAug."""
    rid = torch.tensor(np.asarray(rows, dtype=np.uint64).view(np.int64), device=DEV)
    s = None if src is None else torch.tensor(np.asarray(src, dtype=np.int64), device=DEV)
    n = rid.numel()
    out = torch.full((n,) + tuple(out_hw) + (3,), -7.0, device=DEV)
    u8 = table_t.dtype == torch.uint8
    scale = (1.0 / 256.0 if u8 else 1.0) if scale is None else scale
    a = warp_args(pkg, table_t.data_ptr(), U8 if u8 else F32, table_t.shape, None if s is None else s.data_ptr(), rid.data_ptr(),
                  n, out.data_ptr(), out_hw, scale, fill, None if cfg is None else aug_struct(pkg, cfg), epoch)
    rc = pkg.lib().pl_frame_warp_gather(ctypes.byref(a), pkg._lib.current_stream_ptr())
    assert rc == 0, pkg.lib().pl_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def to_aug(pkg, cfg):
    return pkg.PoseAugment(p_flip=cfg["p_flip"], flip_offset=cfg["flip_offset"], max_rot=cfg["max_rot"],
                           scale_range=cfg["scale_range"], max_shift=cfg["max_shift"], jitter_sigma=cfg["jitter_sigma"],
                           centre=(cfg["cx"], cfg["cy"]), seed=cfg["seed"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_equals_host_entry_bit_for_bit(pkg, dtype):
    """Rotation-free configurations: no contracted product and no division that is not correctly rounded."""
    for src_hw, out_hw in SHAPES + [((8, 12), (4, 6))]:
        table = make_frames(src_hw, dtype)
        table_t = torch.tensor(table).to(DEV)
        for kw in EXACT:
            cfg = pao.config(**kw)
            for epoch, fill in ((3, 0.0), (2 ** 32 + 3, 0.5)):
                h = host_warp(pkg, table, SRC_IDX, ROWS, cfg, out_hw, epoch=epoch, fill=fill)
                d = dev_warp(pkg, table_t, SRC_IDX, ROWS, cfg, out_hw, epoch=epoch, fill=fill)
                assert same_bits(d, h), (src_hw, out_hw, kw, epoch)
        # no PLPoseAug, and the ungathered mode
        assert same_bits(dev_warp(pkg, table_t, SRC_IDX, ROWS, None, out_hw), host_warp(pkg, table, SRC_IDX, ROWS, None, out_hw))
        cfg = pao.config(**EXACT[4])
        g = np.ascontiguousarray(table[SRC_IDX])
        d = dev_warp(pkg, torch.tensor(g).to(DEV), None, ROWS, cfg, out_hw, epoch=1)
        assert same_bits(d, host_warp(pkg, g, None, ROWS, cfg, out_hw, epoch=1))
        assert same_bits(d, dev_warp(pkg, table_t, SRC_IDX, ROWS, cfg, out_hw, epoch=1))
    # same-size: the scaled source and its mirror image
    table = make_frames((20, 28), dtype)
    table_t = torch.tensor(table).to(DEV)
    plain = table[SRC_IDX].astype(np.float32) * np.float32(default_scale(dtype))
    assert same_bits(dev_warp(pkg, table_t, SRC_IDX, ROWS, pao.config(), (20, 28)), plain)
    assert same_bits(dev_warp(pkg, table_t, SRC_IDX, ROWS, pao.config(p_flip=1.0), (20, 28)), plain[:, :, ::-1])
    # a table at an odd address: the kernel's aligned-dword tap loads do not apply
    if dtype == np.uint8:
        flat = torch.zeros(table.size + 1, dtype=torch.uint8, device=DEV)
        odd = flat[1:].view(table.shape)
        odd.copy_(table_t)
        assert odd.data_ptr() % 4 == 1
        cfg = pao.config(**EXACT[4])
        assert same_bits(dev_warp(pkg, odd, SRC_IDX, ROWS, cfg, (18, 27), epoch=1), host_warp(pkg, table, SRC_IDX, ROWS, cfg, (18, 27), epoch=1))
        assert same_bits(dev_warp(pkg, odd, SRC_IDX, ROWS, cfg, (20, 28), epoch=1), host_warp(pkg, table, SRC_IDX, ROWS, cfg, (20, 28), epoch=1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_with_rotation_against_fp64(pkg, dtype):
    cfg = pao.config(**ALL_ON)
    rows = np.arange(40, dtype=np.uint64)
    src = (np.arange(40) * 5) % TABLE_FRAMES
    for src_hw, out_hw in SHAPES:
        table = make_frames(src_hw, dtype)
        d = dev_warp(pkg, torch.tensor(table).to(DEV), src, rows, cfg, out_hw, epoch=3)
        check_against_fp64(d, cfg, 3, rows, table[src], out_hw, default_scale(dtype), 0.0,
                           f"device, all stages on, {np.dtype(dtype).name} {src_hw} -> {out_hw}, rows 0..39")
    rot = pao.config(max_rot=np.pi, seed=3)
    table = make_frames((37, 53), dtype)
    d = dev_warp(pkg, torch.tensor(table).to(DEV), src, rows, rot, (18, 27), fill=-1.0)
    check_against_fp64(d, rot, 0, rows, table[src], (18, 27), default_scale(dtype), -1.0, f"device, rotation alone, {np.dtype(dtype).name}")


def test_reference_frame_size(pkg):
    """B = 2 at 1000 x 1002 (a Human3.6M frame) into 256 x 256, every stage on, against the oracle."""
    table = make_frames((1000, 1002), np.uint8, n=2)
    cfg = pao.config(**ALL_ON)
    rows = np.array([5, 12], dtype=np.uint64)
    d = dev_warp(pkg, torch.tensor(table).to(DEV), None, rows, cfg, (256, 256), epoch=3)
    check_against_fp64(d, cfg, 3, rows, table, (256, 256), 1.0 / 256.0, 0.0, "device, all stages on, uint8 (1000, 1002) -> (256, 256)")
    exact = pao.config(scale_range=0.25, max_shift=0.1, p_flip=0.5, seed=5)
    d = dev_warp(pkg, torch.tensor(table).to(DEV), None, rows, exact, (256, 256), epoch=3)
    assert same_bits(d, fwo.warp(exact, 3, rows, table, (256, 256), 1.0 / 256.0, 0.0, np.float32)["out"])


def test_out_of_range_source_is_a_nan_frame(pkg):
    table = make_frames((37, 53), np.uint8)
    table_t = torch.tensor(table).to(DEV)
    cfg = pao.config(**ALL_ON)
    for out_hw in ((20, 28), (18, 27)):
        good = dev_warp(pkg, table_t, SRC_IDX, ROWS, cfg, out_hw, epoch=1)
        src = SRC_IDX.copy()
        src[[1, 3]] = [TABLE_FRAMES, -1]
        d = dev_warp(pkg, table_t, src, ROWS, cfg, out_hw, epoch=1)
        bad = np.zeros(5, bool)
        bad[[1, 3]] = True
        assert np.isnan(d[bad]).all() and np.isfinite(good).all()
        assert same_bits(d[~bad], good[~bad])


def test_table_past_two_gib(pkg):
    """64-bit offsets: frame 799 of an (800, 1000, 1000, 3) uint8 table starts 2.4e9 bytes in.  The table is allocated, not
    filled: frames 0 and 799 alone are written and read."""
    two = make_frames((1000, 1000), np.uint8, n=2)
    two_t = torch.tensor(two).to(DEV)
    big = torch.empty((800, 1000, 1000, 3), dtype=torch.uint8, device=DEV)
    assert big.numel() > 2 ** 31
    big[0].copy_(two_t[1])
    big[799].copy_(two_t[0])
    cfg = pao.config(**ALL_ON)
    rows = np.array([123, 77], dtype=np.uint64)
    d = dev_warp(pkg, big, [799, 0], rows, cfg, (64, 64), epoch=2)
    del big
    assert same_bits(d, dev_warp(pkg, two_t, [0, 1], rows, cfg, (64, 64), epoch=2))
    assert not same_bits(d[0], d[1])


@pytest.fixture(scope="module")
def feeder_tables(pkg):
    n = 23
    x, y = pkg.synth.synthetic_batch(n, 77)
    frames = torch.tensor(make_frames((19, 25), np.uint8, n=n))
    return frames, x.reshape(n, 17, 2).contiguous(), y.reshape(n, 17, 3).contiguous()


def _epoch(feeder, epoch):
    feeder.set_epoch(epoch)
    out = [tuple(t.cpu().numpy() for t in batch) for batch in feeder]
    torch.cuda.synchronize()
    return out


def test_frame_feeder(pkg, feeder_tables):
    frames, x, y = feeder_tables
    f_t, x_t, y_t = frames.to(DEV), x.to(DEV), y.to(DEV)
    aug = to_aug(pkg, pao.config(**ALL_ON))
    hw = (12, 16)
    feed = lambda bs, **kw: pkg.FrameFeeder(frames, x, y, bs, out_hw=hw, device=DEV, seed=7, augment=aug, **kw)
    first = {}
    for epoch in (0, 1):
        res, stre = _epoch(feed(8), epoch), _epoch(feed(8, resident=False), epoch)
        idx = pkg.epoch_indices(23, 8, epoch=epoch, seed=7)
        assert len(res) == len(stre) == len(idx) == len(feed(8)) == 3 and idx[-1].numel() == 7
        by_row = {}
        for (rf, ra, rb), (sf, sa, sb), ix in zip(res, stre, idx):
            assert rf.shape == (ix.numel(),) + hw + (3,) and rf.dtype == np.float32
            assert same_bits(rf, sf) and same_bits(ra, sa) and same_bits(rb, sb)
            ixd = ix.to(DEV)
            kf = pkg.augment_frames(f_t[ixd].contiguous(), aug, row_ids=ixd, epoch=epoch, out_hw=hw)
            ka, kb = pkg.augment_poses(x_t[ixd].contiguous(), y_t[ixd].contiguous(), aug, row_ids=ixd, epoch=epoch)
            assert same_bits(rf, kf.cpu().numpy()) and same_bits(ra, ka.cpu().numpy()) and same_bits(rb, kb.cpu().numpy())
            for k, r in enumerate(ix.tolist()):
                by_row[r] = (rf[k], ra[k], rb[k])
        assert sorted(by_row) == list(range(23))
        first[epoch] = res[0][0]
        # two ranks of 4: together the rows of the world-1 epoch (its tail of 7 trimmed to 2 x 3), every row the same bits
        for resident in (True, False):
            seen = []
            for rank in (0, 1):
                got = _epoch(feed(4, rank=rank, world=2, resident=resident), epoch)
                ixs = pkg.epoch_indices(23, 4, epoch=epoch, seed=7, rank=rank, world=2)
                assert len(got) == len(ixs) == 3
                for (gf, ga, gb), ix in zip(got, ixs):
                    for k, r in enumerate(ix.tolist()):
                        assert same_bits(gf[k], by_row[r][0]) and same_bits(ga[k], by_row[r][1]) and same_bits(gb[k], by_row[r][2])
                        seen.append(r)
            assert len(seen) == len(set(seen)) == 22 and set(seen) == set(torch.cat(idx).tolist()[:22])
    assert not same_bits(_epoch(feed(8, shuffle=False), 0)[0][0], _epoch(feed(8, shuffle=False), 1)[0][0])     # fresh draws
    # no augment: the plain resize and the plain gather's poses
    for resident in (True, False):
        fd = pkg.FrameFeeder(frames, x, y, 8, out_hw=hw, device=DEV, seed=7, resident=resident)
        for (pf, pa_, pb), ix in zip(_epoch(fd, 1), pkg.epoch_indices(23, 8, epoch=1, seed=7)):
            want = pkg.augment_frames(f_t[ix.to(DEV)].contiguous(), None, out_hw=hw)
            assert same_bits(pf, want.cpu().numpy())
            assert same_bits(pf, host_warp(pkg, frames.numpy(), ix.numpy(), ix.numpy(), None, hw))
            assert same_bits(pa_, x.numpy()[ix.numpy()]) and same_bits(pb, y.numpy()[ix.numpy()])
    with pytest.raises(ValueError):
        pkg.FrameFeeder(frames[:5], x, y, 8, device=DEV)


def test_augment_frames_and_its_graph(pkg):
    """augment_frames against the host entry point, and captured in a graph (one node, no branches): a replay writes the
    eager call's bits, also on new frames in the captured buffer."""
    table = make_frames((37, 53), np.uint8)
    cfg = pao.config(scale_range=0.25, max_shift=0.1, p_flip=0.5, seed=5)
    aug = to_aug(pkg, cfg)
    rid = torch.tensor(ROWS.view(np.int64), device=DEV)
    fr = torch.tensor(np.ascontiguousarray(table[SRC_IDX])).to(DEV)
    eager = pkg.augment_frames(fr, aug, row_ids=rid, epoch=2, out_hw=(20, 28), fill=0.25)
    assert eager.shape == (5, 20, 28, 3) and eager.dtype == torch.float32
    assert same_bits(eager.cpu().numpy(), host_warp(pkg, table, SRC_IDX, ROWS, cfg, (20, 28), epoch=2, fill=0.25))
    ff = fr.float()
    e32 = pkg.augment_frames(ff, aug, row_ids=rid, epoch=2, out_hw=(20, 28), fill=0.25, scale=1.0 / 256.0)
    assert torch.equal(e32, eager)                                               # uint8 taps are converted to fp32 first
    assert torch.equal(pkg.augment_frames(ff, aug, row_ids=rid, epoch=2, out_hw=(20, 28)) / 256.0,
                       pkg.augment_frames(fr, aug, row_ids=rid, epoch=2, out_hw=(20, 28)))
    d0 = pkg.augment_frames(fr, aug, out_hw=(20, 28))                            # row_ids = arange(B), epoch 0
    assert torch.equal(d0, pkg.augment_frames(fr, aug, row_ids=torch.arange(5), epoch=0, out_hw=(20, 28)))
    assert pkg.augment_frames(fr, None).shape == (5, 256, 256, 3)
    with pytest.raises(ValueError):
        pkg.augment_frames(fr, aug, row_ids=rid[:3])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pkg.augment_frames(fr, aug, row_ids=rid, epoch=2, out_hw=(20, 28), fill=0.25)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    buf = fr.clone()
    with torch.cuda.graph(g):
        out = pkg.augment_frames(buf, aug, row_ids=rid, epoch=2, out_hw=(20, 28), fill=0.25)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    other = torch.tensor(np.ascontiguousarray(table[[1, 3, 4, 6, 2]])).to(DEV)
    buf.copy_(other)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, pkg.augment_frames(other, aug, row_ids=rid, epoch=2, out_hw=(20, 28), fill=0.25))
    assert not torch.equal(out, eager)


def test_resident_feeder_is_two_launches_per_batch(pkg, feeder_tables):
    """With an augment the resident feeder launches two kernels per batch -- the augmenting pose gather and the frame warp --
    and augment_frames one."""
    from torch.profiler import ProfilerActivity, profile
    frames, x, y = feeder_tables
    aug = to_aug(pkg, pao.config(**ALL_ON))
    feeder = pkg.FrameFeeder(frames, x, y, 8, out_hw=(12, 16), device=DEV, seed=7, augment=aug)
    rid = torch.arange(23, device=DEV)
    f_t = frames.to(DEV)
    for _ in feeder:                                                   # code objects loaded, allocator warm
        pass
    pkg.augment_frames(f_t, aug, row_ids=rid, out_hw=(12, 16))
    torch.cuda.synchronize()

    def kernels(fn):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        return [n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()]

    ks = kernels(lambda: [None for _ in feeder])
    assert len(ks) == 6, ks
    assert sum("frame_warp_gather_kernel" in n for n in ks) == 3 and sum("pose_augment_gather_kernel" in n for n in ks) == 3, ks
    ks = kernels(lambda: pkg.augment_frames(f_t, aug, row_ids=rid, out_hw=(12, 16)))
    assert len(ks) == 1 and "frame_warp_gather_kernel" in ks[0], ks
