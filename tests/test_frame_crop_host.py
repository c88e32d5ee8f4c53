"""CPU tests of the person-centred crop: csrc/frame_crop.h through the _host entry points (the same inline text the kernels
run, compiled for the CPU) against the fp64 restatement and the fp32 twin of frame_crop_oracle.py, against slicing,
torch.flip and the block mean, against the pose it has to agree with, and on the argument checks.

Gate of the configurations with a rotation (sincosf): 8x the worst absolute error of the fp32 numpy twin against fp64 on the
same cases (computed and printed by the test, never typed in), the rule of test_frame_warp_host.py; pixels whose fp64 source
position lies within BOUNDARY_PX of the frame's extent are left out and have to be at most 1 % of the pixels.  The box is an
integer decision like the flip bit: the rotation cases assert that the fp64 oracle and the fp32 twin agree on it."""
import ctypes
import re
import os

import numpy as np
import pytest
import torch

import frame_crop_oracle as fco
import pose_augment_oracle as pao
from test_frame_warp_host import (ALL_ON, BOUNDARY_PX, DTYPES, EINVAL, ESHAPE, EXACT, GATE_FACTOR, RAMP, RAMP_HW, RAMP_UP, U8, F32,
                                  aug_struct, default_scale, host_warp, make_frames, near_boundary, ramp_at, same_bits, warp_args)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_FRAMES = 9
SRC_IDX = np.array([7, 2, 8, 0, 5], dtype=np.int64)
ROWS = np.array([31, 4, 1000003, 17, 2 ** 33 + 5], dtype=np.uint64)
# (source (Hs, Ws), output (Ho, Wo)): Hs != Ws, a Wo % 4 == 0 and a Wo % 4 != 0 output
SHAPES = [((37, 53), (20, 28)), ((37, 53), (18, 27)), ((9, 7), (20, 28)), ((9, 7), (18, 27))]
SPECS = [fco.spec(1.25, "bbox", 8), fco.spec(1.0, "root", 8), fco.spec(1.25, "root", 3), fco.spec(1.0, "bbox", 14)]
NEW_SYMBOLS = ["pl_pose_augment_gather_crop", "pl_pose_augment_gather_crop_t", "pl_pose_augment_host_crop",
               "pl_pose_augment_host_crop_t", "pl_frame_warp_gather_crop", "pl_frame_warp_host_crop", "pl_pose_crop_boxes",
               "pl_pose_crop_boxes_host", "pl_crop_poses", "pl_crop_poses_host"]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()


def make_poses(n, seed, lo=0.3, hi=0.7, rmin=0.1, rmax=0.3):
    """n poses (n,17,2) fp32: 17 joints in a disc of radius in [rmin, rmax) about a centre in [lo, hi)^2 -- with the defaults
    some boxes start before 0 and some end past the frame."""
    rs = np.random.RandomState(seed)
    c = lo + (hi - lo) * rs.rand(n, 1, 2)
    r = (rmin + (rmax - rmin) * rs.rand(n, 1)) * np.sqrt(rs.rand(n, 17))
    phi = 2 * np.pi * rs.rand(n, 17)
    a = (c + np.stack([r * np.cos(phi), r * np.sin(phi)], axis=2)).astype(np.float32)
    a.setflags(write=False)
    return a


def make_targets(n, seed):
    b = np.random.RandomState(seed).randn(n, 17, 3).astype(np.float32)
    b[:, 0] = 0
    return b


def crop_struct(pkg, sp, src_hw):
    return pkg._lib.PLPoseCrop(sp["margin"], 1 if sp["centre"] == "root" else 0, float(sp["min_side"]), 0, src_hw[0], src_hw[1])


def host_boxes(pkg, a, sp, src_hw, expect=0):
    a = np.ascontiguousarray(a, np.float32)
    out = np.full((len(a), 4), -7.0, np.float32)
    st = crop_struct(pkg, sp, src_hw)
    rc = pkg.lib().pl_pose_crop_boxes_host(a.ctypes.data, len(a), ctypes.byref(st), out.ctypes.data)
    assert rc == expect, pkg.lib().pl_last_error()
    return out


def host_augment(pkg, a, b, src_idx, row_id, cfg, sp, src_hw, epoch=0, xf=None):
    """pl_pose_augment_host_crop(_t) on numpy tables; sp None = no PLPoseCrop.  -> (oa, ob, boxes)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    rid = np.ascontiguousarray(row_id, dtype=np.uint64).view(np.int64)
    n = len(rid)
    src = None if src_idx is None else np.ascontiguousarray(src_idx, dtype=np.int64)
    oa, ob, bx = np.full((n, 17, 2), -7.0, np.float32), np.full((n, 17, 3), -7.0, np.float32), np.full((n, 4), -7.0, np.float32)
    st, cs = aug_struct(pkg, cfg), None if sp is None else crop_struct(pkg, sp, src_hw)
    crop_args = (ctypes.byref(cs) if cs is not None else None, bx.ctypes.data if cs is not None else None)
    head = (a.ctypes.data, b.ctypes.data, None if src is None else src.ctypes.data, rid.ctypes.data, n, len(a), oa.ctypes.data,
            ob.ctypes.data, ctypes.byref(st), int(epoch))
    if xf is None:
        rc = pkg.lib().pl_pose_augment_host_crop(*head, *crop_args)
    else:
        rc = pkg.lib().pl_pose_augment_host_crop_t(*head, *(None if t is None else t.ctypes.data for t in xf), *crop_args)
    assert rc == 0, pkg.lib().pl_last_error()
    return oa, ob, bx


def host_crop_warp(pkg, table, a, src_idx, row_id, cfg, sp, out_hw, epoch=0, scale=None, fill=0.0, expect=0):
    """pl_frame_warp_host_crop on a numpy table (N, Hs, Ws, 3) with the poses a indexed like the frames; sp None = no crop."""
    a = np.ascontiguousarray(a, np.float32)
    rid = np.ascontiguousarray(row_id, dtype=np.uint64).view(np.int64)
    n = len(rid)
    src = None if src_idx is None else np.ascontiguousarray(src_idx, dtype=np.int64)
    out = np.full((n,) + tuple(out_hw) + (3,), -7.0, np.float32)
    aug = None if cfg is None else aug_struct(pkg, cfg)
    scale = default_scale(table.dtype) if scale is None else scale
    w = warp_args(pkg, table.ctypes.data, U8 if table.dtype == np.uint8 else F32, table.shape,
                  None if src is None else src.ctypes.data, rid.ctypes.data, n, out.ctypes.data, out_hw, scale, fill, aug, epoch)
    cs = None if sp is None else crop_struct(pkg, sp, table.shape[1:3])
    rc = pkg.lib().pl_frame_warp_host_crop(ctypes.byref(w), ctypes.byref(cs) if cs is not None else None,
                                           a.ctypes.data if cs is not None else None)
    assert rc == expect, pkg.lib().pl_last_error()
    return out


def host_crop_map(pkg, p, bx, src_hw, invert, offset=1):
    p, bx = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(bx, np.float32)
    out = np.full(p.shape, -7.0, np.float32)
    rc = pkg.lib().pl_crop_poses_host(p.ctypes.data, bx.ctypes.data, len(p), src_hw[0], src_hw[1], invert, offset, out.ctypes.data)
    assert rc == 0, pkg.lib().pl_last_error()
    return out


def same_or_nan(x, y):
    """Bit for bit where finite, NaN where NaN (a NaN's payload is nobody's contract)."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    nx, ny = np.isnan(x), np.isnan(y)
    return np.array_equal(nx, ny) and same_bits(np.where(nx, np.float32(0), x), np.where(ny, np.float32(0), y))


SPECIAL_HW = (32, 64)


def special_poses():
    """Rows whose box the definition decides on an edge, for a (32, 64) frame and min_side 8: 0, 1: all joints equal (side =
    min_side) with ccx - 4 = 12.5 and 13.5 -- the two ties of rint; 2: one NaN coordinate; 3: one inf coordinate; 4: an extent
    whose side passes 2^20; 5: -inf; 6: all joints equal in a corner (the box starts before 0); 7: the opposite corner."""
    a = np.tile(make_poses(1, 5), (8, 1, 1)).copy()
    a[0] = [16.5 / 64, 0.5]
    a[1] = [17.5 / 64, 10.5 / 32]
    a[2, 9, 1] = np.nan
    a[3, 16, 0] = np.inf
    a[4, 3, 0], a[4, 4, 0] = -1.0e5, 1.0e5
    a[5, 0, 1] = -np.inf
    a[6] = [0.01, 0.02]
    a[7] = [0.99, 0.98]
    return a


def test_boxes_bit_for_bit(pkg):
    for src_hw in ((37, 53), (9, 7), (1000, 1002)):
        a = make_poses(40, 11 + src_hw[0])
        for sp in SPECS + [fco.spec(1.25, "bbox", 1), fco.spec(1.0, "root", 40)]:
            got = host_boxes(pkg, a, sp, src_hw)
            twin = fco.boxes(sp, a, src_hw, np.float32)
            assert same_bits(got, twin), (src_hw, sp)
            assert np.array_equal(got, np.rint(got)) and np.array_equal(got[:, 2], got[:, 3]) and (got[:, 2] >= sp["min_side"]).all()
            if sp is SPECS[0]:
                before, past = (got[:, 0] < 0) | (got[:, 1] < 0), (got[:, 0] + got[:, 2] > src_hw[1]) | (got[:, 1] + got[:, 2] > src_hw[0])
                # an 8-px box always leaves the 9 x 7 frame; in the others some boxes do and some do not
                assert before.any() and past.any() and (before | past).all() == (src_hw == (9, 7)), src_hw
    for centre in ("bbox", "root"):
        for margin in (1.0, 1.25):
            sp = fco.spec(margin, centre, 8)
            a = special_poses()
            got = host_boxes(pkg, a, sp, SPECIAL_HW)
            assert same_or_nan(got, fco.boxes(sp, a, SPECIAL_HW, np.float32)) and same_or_nan(got, fco.boxes(sp, a, SPECIAL_HW, np.float64))
            assert got[0].tolist() == [12.0, 12.0, 8.0, 8.0] and got[1].tolist() == [14.0, 6.0, 8.0, 8.0]      # 12.5 -> 12, 13.5 -> 14, 6.5 -> 6
            assert np.isnan(got[2:6]).all() and np.isfinite(got[[0, 1, 6, 7]]).all()
            assert got[6, 0] < 0 and got[6, 1] < 0 and got[7, 0] + 8 > 64 and got[7, 1] + 8 > 32
    # a row's box is its own: another row's NaN, order and n change nothing
    sp, a = SPECS[0], special_poses()
    assert same_or_nan(host_boxes(pkg, a[::-1], sp, SPECIAL_HW), host_boxes(pkg, a, sp, SPECIAL_HW)[::-1])
    assert same_bits(host_boxes(pkg, a[6:7], sp, SPECIAL_HW), host_boxes(pkg, a, sp, SPECIAL_HW)[6:7])


def slice_with_fill(frames, bx, side, fill, scale):
    """scale * frames[k, y0:y0+side, x0:x0+side] with `fill` where the slice leaves the frame, fp32."""
    n, Hs, Ws, _ = frames.shape
    x0, y0 = bx[:, 0].astype(np.int64), bx[:, 1].astype(np.int64)
    ys, xs = y0[:, None, None] + np.arange(side)[None, :, None], x0[:, None, None] + np.arange(side)[None, None, :]
    ok = (ys >= 0) & (ys < Hs) & (xs >= 0) & (xs < Ws)
    v = frames[np.arange(n)[:, None, None], np.clip(ys, 0, Hs - 1), np.clip(xs, 0, Ws - 1)].astype(np.float32) * np.float32(scale)
    return np.where(ok[..., None], v, np.float32(fill)), ok


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_three_exact_cases(pkg, dtype):
    """side == Wo == Ho: the scaled slice; with a flip its mirror image; side == 2 Wo == 2 Ho: the 2 x 2 block mean."""
    table = make_frames((37, 53), dtype)
    n = 24
    src = (np.arange(n) * 5) % TABLE_FRAMES
    frames = np.ascontiguousarray(table[src])                                  # gathered: frame k goes with pose k
    rows = np.arange(n, dtype=np.uint64)
    tight = make_poses(n, 3, lo=0.0, hi=1.0, rmin=0.001, rmax=0.01)          # extent < 1 px: side = min_side, boxes anywhere
    scale = default_scale(dtype)
    for centre in ("bbox", "root"):
        sp = fco.spec(1.25, centre, 12)
        bx = host_boxes(pkg, tight, sp, (37, 53))
        assert (bx[:, 2] == 12).all()
        want, ok = slice_with_fill(frames, bx, 12, 0.25, scale)
        assert (~ok).any() and ok.all(axis=(1, 2)).any()                           # some slices leave the frame, some do not
        out = host_crop_warp(pkg, frames, tight, None, rows, pao.config(), sp, (12, 12), fill=0.25)
        assert same_bits(out, want)
        assert same_bits(host_crop_warp(pkg, frames, tight, None, rows, None, sp, (12, 12), fill=0.25), want)
        out = host_crop_warp(pkg, frames, tight, None, rows, pao.config(p_flip=1.0), sp, (12, 12), fill=0.25)
        assert same_bits(out, torch.flip(torch.from_numpy(want), (2,)).numpy())
    inner = make_poses(n, 4, lo=0.45, hi=0.55, rmin=0.001, rmax=0.01)         # 24-px boxes inside the 37 x 53 frame
    sp = fco.spec(1.25, "bbox", 24)
    bx = host_boxes(pkg, inner, sp, (37, 53))
    f, ok = slice_with_fill(frames, bx, 24, 0.0, 1.0)
    assert (bx[:, 2] == 24).all() and ok.all() and len(np.unique(bx[:, :2], axis=0)) > 4
    h = np.float32(0.5)
    top = h * f[:, 0::2, 0::2] + h * f[:, 0::2, 1::2]
    bot = h * f[:, 1::2, 0::2] + h * f[:, 1::2, 1::2]
    want = np.float32(scale) * (h * top + h * bot)
    assert want.dtype == np.float32
    assert same_bits(host_crop_warp(pkg, frames, inner, None, rows, pao.config(), sp, (12, 12)), want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("src_hw,out_hw", SHAPES)
def test_rotation_free_configurations_equal_the_fp32_twin_bit_for_bit(pkg, dtype, src_hw, out_hw):
    table = make_frames(src_hw, dtype)
    a, b = make_poses(TABLE_FRAMES, 17), make_targets(TABLE_FRAMES, 18)
    scale = default_scale(dtype)
    for sp in SPECS[:3]:
        for kw in EXACT:
            cfg = pao.config(**kw)
            for epoch, fill in ((3, 0.0), (2 ** 32 + 3, 0.5)):
                out = host_crop_warp(pkg, table, a, SRC_IDX, ROWS, cfg, sp, out_hw, epoch=epoch, fill=fill)
                twin = fco.warp(cfg, epoch, ROWS, table[SRC_IDX], a[SRC_IDX], sp, out_hw, scale, fill, np.float32)
                assert same_bits(out, twin["out"]), (sp, kw, epoch)
                oa, ob, bx = host_augment(pkg, a, b, SRC_IDX, ROWS, cfg, sp, src_hw, epoch=epoch)
                ta, tb, tbx, _ = fco.augment(cfg, epoch, ROWS, a[SRC_IDX], b[SRC_IDX], sp, src_hw, np.float32)
                assert same_bits(oa, ta) and same_bits(ob, tb) and same_bits(bx, tbx), (sp, kw, epoch)
    # the crop moves pixels and poses, and leaves the 3-D pose alone
    plain = host_warp(pkg, table, SRC_IDX, ROWS, pao.config(), out_hw)
    assert not same_bits(host_crop_warp(pkg, table, a, SRC_IDX, ROWS, pao.config(), SPECS[0], out_hw), plain)
    oa, ob, _ = host_augment(pkg, a, b, SRC_IDX, ROWS, pao.config(), SPECS[0], src_hw)
    assert not same_bits(oa, a[SRC_IDX]) and same_bits(ob, b[SRC_IDX])


def rotation_case(src_hw, out_hw):
    """The seed, epoch and rows of test_frame_warp_host's rotation case; poses and spec with side >= Wo / 2."""
    cfg = pao.config(**ALL_ON)
    rows = np.arange(40, dtype=np.uint64)
    src = (np.arange(40) * 5) % TABLE_FRAMES
    a, b = make_poses(TABLE_FRAMES, 23, rmin=0.2, rmax=0.3), make_targets(TABLE_FRAMES, 24)
    sp = fco.spec(1.25, "bbox", (max(out_hw) + 1) // 2)
    return cfg, 3, rows, src, a, b, sp


def check_crop_against_fp64(out, oa, bx, case, frames, out_hw, scale, fill, what):
    """The 8x-twin gates of the frame (away from the extent's boundary) and of the 2-D pose; prints every figure.
    frames: the table; returns (frame error, frame gate, pose error, pose gate)."""
    cfg, epoch, rows, src, a, b, sp = case
    src_hw = frames.shape[1:3]
    o64 = fco.warp(cfg, epoch, rows, frames[src], a[src], sp, out_hw, scale, fill, np.float64)
    o32 = fco.warp(cfg, epoch, rows, frames[src], a[src], sp, out_hw, scale, fill, np.float32)
    assert np.array_equal(o64["boxes"], o32["boxes"].astype(np.float64)) and same_bits(bx, o32["boxes"])   # the integer decision
    assert (o64["boxes"][:, 2] >= out_hw[1] / 2).all()
    edge = near_boundary(o64, src_hw)
    keep = ~edge
    twin = float(np.abs(o32["out"].astype(np.float64) - o64["out"])[keep].max())
    err = float(np.abs(out.astype(np.float64) - o64["out"])[keep].max())
    a64 = fco.augment(cfg, epoch, rows, a[src], b[src], sp, src_hw, np.float64)[0]
    a32 = fco.augment(cfg, epoch, rows, a[src], b[src], sp, src_hw, np.float32)[0]
    ptwin, perr = float(np.abs(a32.astype(np.float64) - a64).max()), float(np.abs(oa.astype(np.float64) - a64).max())
    print(f"{what}: frame worst |error| vs fp64 {err:.3e}; fp32 twin {twin:.3e}; gate {GATE_FACTOR * twin:.3e}; "
          f"{100 * edge.mean():.2f} % of the pixels within {BOUNDARY_PX} px of the extent left out, "
          f"{100 * (~o64['inside']).mean():.1f} % outside; pose worst |error| {perr:.3e}; twin {ptwin:.3e}; gate {GATE_FACTOR * ptwin:.3e}")
    assert edge.mean() <= 0.01
    assert twin > 0.0 and ptwin > 0.0
    assert err <= GATE_FACTOR * twin and perr <= GATE_FACTOR * ptwin
    return err, GATE_FACTOR * twin, perr, GATE_FACTOR * ptwin


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_stage_on_against_fp64(pkg, dtype):
    for src_hw, out_hw in SHAPES:
        case = rotation_case(src_hw, out_hw)
        cfg, epoch, rows, src, a, b, sp = case
        flips = pao.decisions(cfg, epoch, rows, np.float64)["flip"]
        assert flips.any() and not flips.all()
        table = make_frames(src_hw, dtype)
        out = host_crop_warp(pkg, table, a, src, rows, cfg, sp, out_hw, epoch=epoch)
        oa, ob, bx = host_augment(pkg, a, b, src, rows, cfg, sp, src_hw, epoch=epoch)
        check_crop_against_fp64(out, oa, bx, case, table, out_hw, default_scale(dtype), 0.0,
                                f"host, crop + all stages on, {np.dtype(dtype).name} {src_hw} -> {out_hw}, rows 0..39")


def bilinear_at_valid(img, u, v, bad_value):
    """img (n, H, W, 3) sampled at image-normalised (u, v) (n, J), pixel centres at (j + 0.5) / W, in fp64 -> (values, ok):
    ok where all four taps are pixels of the image and none of them is `bad_value` (the fill)."""
    n, H, W, _ = img.shape
    x, y = u * W - 0.5, v * H - 0.5
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    ok = (x0 >= 0) & (x0 + 1 < W) & (y0 >= 0) & (y0 + 1 < H)
    x0, y0 = np.clip(x0, 0, W - 2), np.clip(y0, 0, H - 2)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    k = np.arange(n)[:, None]
    img = img.astype(np.float64)
    taps = [img[k, y0, x0], img[k, y0, x0 + 1], img[k, y0 + 1, x0], img[k, y0 + 1, x0 + 1]]
    for t in taps:
        ok &= (t != bad_value).all(axis=-1)
    return (1 - fy) * ((1 - fx) * taps[0] + fx * taps[1]) + fy * ((1 - fx) * taps[2] + fx * taps[3]), ok


def test_frame_follows_its_cropped_pose(pkg):
    """A linear-ramp frame, cropped and warped into 8x its size, read at the cropped and augmented 2-D joints shows the ramp's
    value at the SOURCE joints: the two outputs agree, without the frame oracle.  Tolerance and method of
    test_frame_warp_host.test_frame_follows_its_pose: 8x the error of the fp32 round trip (the ramp evaluated, in fp32, at the
    source position of every output pixel centre, read at the fp32 twin's joints).  Joints with a tap in `fill` are left out."""
    (Hs, Ws), n, FILL = RAMP_HW, 40, -1000.0
    out_hw = (Hs * RAMP_UP, Ws * RAMP_UP)
    yy, xx = np.meshgrid(np.arange(Hs), np.arange(Ws), indexing="ij")
    table = np.ascontiguousarray(ramp_at(xx, yy).astype(np.uint8)[None])
    a, b = make_poses(n, 21, lo=0.35, hi=0.65, rmin=0.15, rmax=0.25), np.zeros((n, 17, 3), np.float32)
    sp = fco.spec(2.5, "bbox", 8)                                   # joints within 0.2 of the crop's centre: every stage keeps them in
    cfg = pao.config(**dict(ALL_ON, jitter_sigma=0.0))
    rows, epoch = np.arange(n, dtype=np.uint64), 3
    flips = pao.decisions(cfg, epoch, rows, np.float64)["flip"]
    assert flips.any() and not flips.all()
    oa, _, bx = host_augment(pkg, a, b, None, rows, cfg, sp, RAMP_HW, epoch=epoch)
    assert (bx[:, 2] > max(RAMP_HW)).any()                           # boxes larger than the frame: fill on their rim
    img = host_crop_warp(pkg, np.ascontiguousarray(np.repeat(table, n, axis=0)), a, None, rows, cfg, sp, out_hw, epoch=epoch,
                         scale=1.0, fill=FILL)
    got, ok = bilinear_at_valid(img, oa[:, :, 0].astype(np.float64), oa[:, :, 1].astype(np.float64), FILL)
    srcj = np.where(flips[:, None], np.array(pao.SWAP)[None, :], np.arange(17)[None, :])
    sa = np.take_along_axis(a.astype(np.float64), srcj[:, :, None], axis=1)
    want = ramp_at(sa[:, :, 0] * Ws - 0.5, sa[:, :, 1] * Hs - 0.5)

    def round_trip(T):
        ta = fco.augment(cfg, epoch, rows, a, b, sp, RAMP_HW, T, bx=bx)[0]
        xs, ys, _ = fco.source_positions(cfg, epoch, rows, bx, out_hw, T)
        ideal = RAMP[:, 0].astype(T) * xs[..., None] + RAMP[:, 1].astype(T) * ys[..., None] + RAMP[:, 2].astype(T)
        assert ideal.dtype == T
        return bilinear_at_valid(ideal, ta[:, :, 0].astype(np.float64), ta[:, :, 1].astype(np.float64), FILL)

    (t32, ok32), (t64, ok64) = round_trip(np.float32), round_trip(np.float64)
    assert ok32.all() and ok64.all()                                 # every joint stays inside the crop
    err, twin = float(np.abs(got - want)[ok].max()), float(np.abs(t32 - want)[ok].max())
    floor64 = float(np.abs(t64 - want)[ok].max())
    print(f"cropped frame at the cropped and augmented joints vs the ramp at the source joints: {int(ok.sum())} of {ok.size} joints "
          f"({100 * ok.mean():.1f} %), {int(flips.sum())} of {n} rows flipped: worst |error| {err:.3e}; fp32 round trip {twin:.3e} "
          f"(fp64 round trip {floor64:.3e}); gate {GATE_FACTOR * twin:.3e}")
    assert ok.mean() >= 0.9
    assert floor64 < 1e-9 and twin > 0.0
    assert err <= GATE_FACTOR * twin
    # and the uncropped frame under the cropped joints does not pass: the check can fail
    plain = host_warp(pkg, table, np.zeros(n, np.int64), rows, cfg, out_hw, epoch=epoch, scale=1.0, fill=FILL)
    wrong, wok = bilinear_at_valid(plain, oa[:, :, 0].astype(np.float64), oa[:, :, 1].astype(np.float64), FILL)
    assert np.abs(wrong - want)[wok].max() > 1.0


def test_crop_then_uncrop_and_its_gradient(pkg):
    """uncrop_poses(crop_poses(p)) against the fp64 oracle under the 8x-twin gate, each map against its twin bit for bit, and
    the gradient of the composition (the same calls without the offset, in reverse) against stock torch's autograd in fp64,
    with torch's fp32 autograd of the same composition as the twin."""
    src_hw = (37, 53)
    p = make_poses(40, 31)
    bx = host_boxes(pkg, make_poses(40, 32), SPECS[0], src_hw)
    c = host_crop_map(pkg, p, bx, src_hw, 0)
    back = host_crop_map(pkg, c, bx, src_hw, 1)
    assert same_bits(c, fco.crop_poses(p, bx, src_hw, np.float32))
    assert same_bits(back, fco.uncrop_poses(c, bx, src_hw, np.float32))
    o64 = fco.uncrop_poses(fco.crop_poses(p, bx, src_hw, np.float64), bx, src_hw, np.float64)
    twin = float(np.abs(fco.uncrop_poses(fco.crop_poses(p, bx, src_hw, np.float32), bx, src_hw, np.float32).astype(np.float64) - o64).max())
    err = float(np.abs(back.astype(np.float64) - o64).max())
    print(f"uncrop(crop(p)) vs fp64: {err:.3e}; twin {twin:.3e}; fp64 round trip vs p {np.abs(o64 - p).max():.3e}")
    assert np.abs(o64 - p).max() < 1e-12 and twin > 0.0 and err <= GATE_FACTOR * twin
    g = np.random.RandomState(33).randn(40, 17, 2).astype(np.float32)
    got = host_crop_map(pkg, host_crop_map(pkg, g, bx, src_hw, 1, offset=0), bx, src_hw, 0, offset=0)

    def torch_grad(T):
        tp = torch.tensor(p, dtype=T, requires_grad=True)
        tb, W = torch.tensor(bx, dtype=T), torch.tensor([src_hw[1], src_hw[0]], dtype=T)
        cc = (tp * W - tb[:, None, 0:2]) / tb[:, None, 2:3]
        ((cc * tb[:, None, 2:3] + tb[:, None, 0:2]) / W).backward(torch.tensor(g, dtype=T))
        return tp.grad.numpy().astype(np.float64)

    g64, g32 = torch_grad(torch.float64), torch_grad(torch.float32)
    twin, err = float(np.abs(g32 - g64).max()), float(np.abs(got - g64).max())
    print(f"gradient of uncrop(crop(p)) vs torch fp64 autograd: {err:.3e}; torch fp32 autograd {twin:.3e}")
    assert twin > 0.0 and err <= GATE_FACTOR * twin
    # each map's gradient alone is its factor: W / side and side / W
    W = np.array([src_hw[1], src_hw[0]], np.float32)
    assert same_bits(host_crop_map(pkg, g, bx, src_hw, 0, offset=0), (g * W) / bx[:, None, 2:3])
    assert same_bits(host_crop_map(pkg, g, bx, src_hw, 1, offset=0), (g * bx[:, None, 2:3]) / W)
    # a NaN box is a NaN pose
    nb = bx.copy()
    nb[3] = np.nan
    out = host_crop_map(pkg, p, nb, src_hw, 0)
    assert np.isnan(out[3]).all() and same_bits(np.delete(out, 3, 0), np.delete(c, 3, 0))


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_box_is_a_nan_frame_and_pose(pkg, dtype):
    table = make_frames(SPECIAL_HW, dtype, n=8)
    a, b = special_poses(), make_targets(8, 2)
    rows = np.arange(8, dtype=np.uint64)
    cfg = pao.config(**dict(ALL_ON, max_rot=0.0))
    for out_hw in ((20, 28), (18, 27)):
        out = host_crop_warp(pkg, table, a, None, rows, cfg, SPECS[0], out_hw, epoch=1)
        oa, ob, bx = host_augment(pkg, a, b, None, rows, cfg, SPECS[0], SPECIAL_HW, epoch=1)
        bad = np.isnan(bx[:, 2])
        assert bad.tolist() == [False, False, True, True, True, True, False, False]
        assert np.isnan(out[bad]).all() and np.isfinite(out[~bad]).all() and np.isnan(oa[bad]).all() and np.isfinite(oa[~bad]).all()
        assert np.isfinite(ob).all()
        twin = fco.warp(cfg, 1, rows, table, a, SPECS[0], out_hw, default_scale(dtype), 0.0, np.float32)
        assert same_or_nan(out, twin["out"])
        # the other rows are those of a call without the bad ones
        good = np.where(~bad)[0]
        assert same_bits(out[good], host_crop_warp(pkg, table, a, good, rows[good], cfg, SPECS[0], out_hw, epoch=1))


def test_no_crop_is_the_entry_point_without(pkg):
    """crop NULL: the _crop host entry points give the bits of the entry points without, on the same inputs."""
    L = pkg.lib()
    a, b = make_poses(TABLE_FRAMES, 17), make_targets(TABLE_FRAMES, 18)
    rid = ROWS.view(np.int64)
    sub = (np.random.RandomState(1).rand(34).astype(np.float32), np.random.RandomState(2).rand(34).astype(np.float32) + 0.5, None, None)
    for kw in EXACT + [ALL_ON]:
        cfg = pao.config(**kw)
        st = aug_struct(pkg, cfg)
        oa, ob = np.empty((5, 17, 2), np.float32), np.empty((5, 17, 3), np.float32)
        assert L.pl_pose_augment_host(a.ctypes.data, b.ctypes.data, SRC_IDX.ctypes.data, rid.ctypes.data, 5, TABLE_FRAMES,
                                      oa.ctypes.data, ob.ctypes.data, ctypes.byref(st), 3) == 0
        ca, cb, _ = host_augment(pkg, a, b, SRC_IDX, ROWS, cfg, None, None, epoch=3)
        assert same_bits(ca, oa) and same_bits(cb, ob)
        assert L.pl_pose_augment_host_t(a.ctypes.data, b.ctypes.data, SRC_IDX.ctypes.data, rid.ctypes.data, 5, TABLE_FRAMES,
                                        oa.ctypes.data, ob.ctypes.data, ctypes.byref(st), 3, sub[0].ctypes.data, sub[1].ctypes.data,
                                        None, None) == 0
        ca, cb, _ = host_augment(pkg, a, b, SRC_IDX, ROWS, cfg, None, None, epoch=3, xf=sub)
        assert same_bits(ca, oa) and same_bits(cb, ob)
        for dtype in DTYPES:
            table = make_frames((37, 53), dtype)
            for out_hw in ((20, 28), (18, 27)):
                assert same_bits(host_crop_warp(pkg, table, a, SRC_IDX, ROWS, cfg, None, out_hw, epoch=3),
                                 host_warp(pkg, table, SRC_IDX, ROWS, cfg, out_hw, epoch=3))
    # and with a crop the _t form is the plain form followed by the transform
    cfg = pao.config(**EXACT[4])
    pa_, pb_, bx = host_augment(pkg, a, b, SRC_IDX, ROWS, cfg, SPECS[0], (37, 53), epoch=3)
    ta, tb, tbx = host_augment(pkg, a, b, SRC_IDX, ROWS, cfg, SPECS[0], (37, 53), epoch=3, xf=sub)
    assert same_bits(ta, ((pa_.reshape(5, 34) - sub[0]) / sub[1]).reshape(5, 17, 2)) and same_bits(tb, pb_) and same_bits(tbx, bx)


def test_errors(pkg):
    L = pkg.lib()
    table = make_frames((9, 7), np.uint8)
    a, b = make_poses(TABLE_FRAMES, 17), make_targets(TABLE_FRAMES, 18)
    out = np.zeros((5, 4, 6, 3), np.float32)
    oa, ob, bx = np.zeros((5, 17, 2), np.float32), np.zeros((5, 17, 3), np.float32), np.zeros((5, 4), np.float32)
    rid = ROWS.view(np.int64)
    raw = lambda **kw: dict(pao.config(), **kw)

    def crop(margin=1.25, centre=0, min_side=8.0, hw=(9, 7)):
        return pkg._lib.PLPoseCrop(margin, centre, min_side, 0, hw[0], hw[1])

    def warp(fn=L.pl_frame_warp_host_crop, cs=crop(), x2d=a.ctypes.data, cfg=pao.config(), extra=()):
        w = warp_args(pkg, table.ctypes.data, U8, table.shape, SRC_IDX.ctypes.data, rid.ctypes.data, 5, out.ctypes.data, (4, 6),
                      1.0, 0.0, aug_struct(pkg, cfg), 0)
        return fn(ctypes.byref(w), ctypes.byref(cs) if cs is not None else None, x2d, *extra)

    def pose(fn=L.pl_pose_augment_host_crop, cs=crop(), boxes=bx.ctypes.data, cfg=pao.config(), extra=()):
        st = aug_struct(pkg, cfg)
        return fn(a.ctypes.data, b.ctypes.data, SRC_IDX.ctypes.data, rid.ctypes.data, 5, TABLE_FRAMES, oa.ctypes.data, ob.ctypes.data,
                  ctypes.byref(st), 0, ctypes.byref(cs) if cs is not None else None, boxes, *extra)

    def only_boxes(fn=L.pl_pose_crop_boxes_host, cs=crop(), x2d=a.ctypes.data, n=5, boxes=bx.ctypes.data, extra=()):
        return fn(x2d, n, ctypes.byref(cs) if cs is not None else None, boxes, *extra)

    assert warp() == 0 and pose() == 0 and only_boxes() == 0
    assert warp(cs=None, x2d=None) == 0 and pose(cs=None, boxes=None) == 0            # no crop: neither pointer is read
    bad_specs = [(dict(margin=0.0), b"margin"), (dict(margin=-1.0), b"margin"), (dict(margin=float("nan")), b"margin"),
                 (dict(margin=float("inf")), b"margin"), (dict(min_side=0.0), b"min_side"), (dict(min_side=0.5), b"min_side"),
                 (dict(min_side=8.5), b"min_side"), (dict(min_side=float(2 ** 20 + 1)), b"min_side"),
                 (dict(min_side=float("nan")), b"min_side"), (dict(centre=2), b"centre"), (dict(centre=-1), b"centre")]
    device = [(dict(fn=L.pl_frame_warp_gather_crop, extra=(None,)), warp), (dict(fn=L.pl_pose_augment_gather_crop, extra=(None,)), pose),
              (dict(fn=L.pl_pose_crop_boxes, extra=(None,)), only_boxes)]
    for kw, text in bad_specs:
        for call, name in ((warp, b"pl_frame_warp_host_crop"), (pose, b"pl_pose_augment_host_crop"), (only_boxes, b"pl_pose_crop_boxes_host")):
            assert call(cs=crop(**kw)) == EINVAL and text in L.pl_last_error() and name in L.pl_last_error(), kw
        for g, call in device:                                                        # the same checks before a device is touched
            assert call(cs=crop(**kw), **g) == EINVAL and text in L.pl_last_error(), kw
    assert crop(min_side=float(2 ** 20)).min_side == 2 ** 20 and only_boxes(cs=crop(min_side=float(2 ** 20))) == 0
    for call in (warp, pose):
        assert call(cfg=raw(p_flip=0.5, flip_offset=0.0)) == EINVAL and b"flip_offset" in L.pl_last_error()
        assert call(cfg=raw(p_flip=1.0, flip_offset=0.5)) == EINVAL
        assert call(cfg=raw(flip_offset=0.0)) == 0                                    # no flip: the offset is not read
    assert pose(cs=None, boxes=None, cfg=raw(p_flip=0.5, flip_offset=0.0)) == 0       # without a crop the pose gather takes any offset
    assert warp(x2d=None) == EINVAL and b"x2d" in L.pl_last_error()
    assert pose(boxes=None) == EINVAL and b"boxes" in L.pl_last_error()
    assert only_boxes(boxes=None) == EINVAL and only_boxes(x2d=None) == EINVAL and only_boxes(cs=None) == EINVAL
    assert b"null" in L.pl_last_error()
    for g, call in device:
        assert call(**{"x2d" if call is not pose else "boxes": None}, **g) == EINVAL and b"null" in L.pl_last_error()
    # the crop's frame is the table's; sizes
    assert warp(cs=crop(hw=(9, 8))) == ESHAPE and b"crop" in L.pl_last_error()
    for hw in ((0, 7), (9, -1), (2 ** 22 + 1, 7)):
        assert pose(cs=crop(hw=hw)) == ESHAPE and b"crop" in L.pl_last_error(), hw
        assert only_boxes(cs=crop(hw=hw)) == ESHAPE
    assert only_boxes(n=0) == ESHAPE and only_boxes(n=-3) == ESHAPE
    # aliasing
    assert pose(boxes=oa.ctypes.data) == EINVAL and b"aliased" in L.pl_last_error()
    assert only_boxes(boxes=a.ctypes.data) == EINVAL and b"aliased" in L.pl_last_error()
    assert warp(x2d=out.ctypes.data) == EINVAL and b"aliased" in L.pl_last_error()
    # the checks of the entry points without a crop still come first
    w = warp_args(pkg, None, U8, table.shape, SRC_IDX.ctypes.data, rid.ctypes.data, 5, out.ctypes.data, (4, 6), 1.0, 0.0, None, 0)
    cs = crop()
    assert L.pl_frame_warp_host_crop(ctypes.byref(w), ctypes.byref(cs), a.ctypes.data) == EINVAL and b"null" in L.pl_last_error()
    assert L.pl_frame_warp_host_crop(None, ctypes.byref(cs), a.ctypes.data) == EINVAL
    # pl_crop_poses
    p = np.zeros((5, 17, 2), np.float32)
    cp = lambda fn=L.pl_crop_poses_host, pp=p.ctypes.data, bb=bx.ctypes.data, n=5, hw=(9, 7), oo=oa.ctypes.data, extra=(): \
        fn(pp, bb, n, hw[0], hw[1], 0, 1, oo, *extra)
    assert cp() == 0
    for g in (dict(), dict(fn=L.pl_crop_poses, extra=(None,))):
        assert cp(pp=None, **g) == EINVAL and cp(bb=None, **g) == EINVAL and cp(oo=None, **g) == EINVAL and b"null" in L.pl_last_error()
        assert cp(n=0, **g) == ESHAPE and cp(hw=(0, 7), **g) == ESHAPE and cp(hw=(9, 2 ** 22 + 1), **g) == ESHAPE
        assert cp(oo=p.ctypes.data, **g) == EINVAL and b"aliased" in L.pl_last_error()
    assert ctypes.sizeof(pkg._lib.PLPoseCrop) == 32 and ctypes.sizeof(pkg._lib.PLFrameWarp) == 112
    assert ctypes.sizeof(pkg._lib.PLPoseAug) == 40


def test_header_declares_what_the_library_exports(pkg):
    header = open(os.path.join(ROOT, "include", "poselift.h")).read()
    declared = set(re.findall(r"\b(pl_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg._lib.SIGNATURES and hasattr(raw, name), name
    assert declared == set(pkg._lib.SIGNATURES)
    assert "typedef struct PLPoseCrop" in header and pkg.lib().pl_version() >= 118


def test_python_surface(pkg):
    assert pkg.PersonCrop is pkg.data.PersonCrop and pkg.crop_boxes is pkg.data.crop_boxes
    assert pkg.crop_poses is pkg.train.crop_poses and pkg.uncrop_poses is pkg.train.uncrop_poses
    c = pkg.PersonCrop()
    assert (c.margin, c.centre, c.min_side) == (1.25, "bbox", 8)
    s = pkg.PersonCrop(margin=1.5, centre="root", min_side=12).struct((37, 53))
    assert (s.margin, s.centre, s.min_side, s.Hs, s.Ws) == (1.5, 1, 12.0, 37, 53)
    for kw in (dict(margin=0.0), dict(margin=float("nan")), dict(margin=-1), dict(centre="hip"), dict(min_side=0), dict(min_side=2.5),
               dict(min_side=2 ** 20 + 1)):
        with pytest.raises(ValueError):
            pkg.PersonCrop(**kw)
    with pytest.raises(dataclasses_frozen_error()):
        c.margin = 2.0
    frames = torch.zeros(4, 9, 7, 3, dtype=torch.uint8)
    x, y = torch.zeros(4, 17, 2), torch.zeros(4, 17, 3)
    with pytest.raises(ValueError):
        pkg.FrameFeeder(frames, x, y, 2, crop=c, augment=pkg.PoseAugment(p_flip=1.0, flip_offset=0.0))
    with pytest.raises(TypeError):
        pkg.FrameFeeder(frames, x, y, 2, crop=dict(margin=1.25))
    with pytest.raises(ValueError):
        pkg.augment_frames(frames, None, crop=c)                                       # a crop needs x2d
    with pytest.raises(ValueError):
        pkg.augment_poses(x, y, pkg.PoseAugment(), crop=c)                             # and frame_hw
    with pytest.raises(pkg.PoseliftError):
        pkg.crop_boxes(x, c, (9, 7))                                                   # no CPU path
    with pytest.raises(pkg.PoseliftError):
        pkg.uncrop_poses(x, torch.zeros(4, 4), (9, 7))


def dataclasses_frozen_error():
    import dataclasses
    return dataclasses.FrozenInstanceError
