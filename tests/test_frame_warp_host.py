"""CPU tests of the frame warp: csrc/frame_warp.h through pl_frame_warp_host (the same inline text the kernel runs, compiled
for the CPU) against the fp64 restatement and the fp32 twin of frame_warp_oracle.py, against stock torch, against the pose
augmentation it has to agree with, and on structural properties.

Gate of the configurations with a rotation (sincosf): 8x the worst absolute error of the fp32 numpy twin against fp64 on the
same cases (computed and printed by the test, never typed in), the rule of test_pose_augment_host.py.  Pixels whose fp64
source position lies within BOUNDARY_PX of the frame's extent are left out of that comparison -- `fill` switches there, and
a position that differs in the last bits lands on the other side -- and have to be at most 1 % of the pixels."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import frame_warp_oracle as fwo
import pose_augment_oracle as pao

EINVAL, ESHAPE = -1, -2
GATE_FACTOR = 8.0
BOUNDARY_PX = 1e-2
U8, F32 = 0, 1
TABLE_FRAMES = 9
SRC_IDX = np.array([7, 2, 8, 0, 5], dtype=np.int64)              # n = 5, non-monotone, into the 9-frame table
ROWS = np.array([31, 4, 1000003, 17, 2 ** 33 + 5], dtype=np.uint64)
# (source (Hs, Ws), output (Ho, Wo)): down- and up-scaling into a Wo % 4 == 0 and a Wo % 4 != 0 output, and same-size
SHAPES = [((37, 53), (20, 28)), ((37, 53), (18, 27)), ((9, 7), (20, 28)), ((9, 7), (18, 27)), ((20, 28), (20, 28))]
DTYPES = [np.uint8, np.float32]
ALL_ON = dict(p_flip=0.5, max_rot=np.pi, scale_range=0.25, max_shift=0.1, jitter_sigma=0.05, seed=11)
# flip, scale, shift: no sincosf, so the host, the device and the numpy twin give the same bits
EXACT = [dict(), dict(p_flip=1.0), dict(p_flip=0.5, seed=7), dict(scale_range=0.25, max_shift=0.1, seed=99),
         dict(scale_range=0.5, p_flip=0.5, cx=0.25, cy=0.75, seed=5), dict(max_shift=0.03, seed=2 ** 63 + 9)]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()


def make_frames(hw, dtype, n=TABLE_FRAMES, seed=3):
    """A table of n random frames (Hs, Ws, 3): uint8 over the whole range, or fp32 in [0, 1)."""
    rs = np.random.RandomState(seed + 1000 * hw[0] + hw[1])
    if dtype == np.uint8:
        t = rs.randint(0, 256, (n,) + tuple(hw) + (3,)).astype(np.uint8)
    else:
        t = rs.rand(n, hw[0], hw[1], 3).astype(np.float32)
    t.setflags(write=False)
    return t


def default_scale(dtype):
    return 1.0 / 256.0 if dtype == np.uint8 else 1.0


def aug_struct(pkg, cfg):
    return pkg._lib.PLPoseAug(cfg["p_flip"], cfg["flip_offset"], cfg["max_rot"], cfg["scale_range"], cfg["max_shift"],
                              cfg["jitter_sigma"], cfg["cx"], cfg["cy"], cfg["seed"])


def warp_args(pkg, table_ptr, code, table_shape, src_ptr, rid_ptr, n, out_ptr, out_hw, scale, fill, aug, epoch, C=3):
    return pkg._lib.PLFrameWarp(table_ptr, code, C, table_shape[0], table_shape[1], table_shape[2], src_ptr, rid_ptr, n,
                                out_ptr, out_hw[0], out_hw[1], scale, fill,
                                ctypes.pointer(aug) if aug is not None else None, int(epoch))


def host_warp(pkg, table, src_idx, row_id, cfg, out_hw, epoch=0, scale=None, fill=0.0, expect=0):
    """pl_frame_warp_host on a numpy table (N, Hs, Ws, 3); src_idx None = frames in order; cfg None = no PLPoseAug."""
    row_id = np.ascontiguousarray(row_id, dtype=np.uint64).view(np.int64)
    n = len(row_id)
    src = None if src_idx is None else np.ascontiguousarray(src_idx, dtype=np.int64)
    out = np.full((n,) + tuple(out_hw) + (3,), -7.0, np.float32)
    aug = None if cfg is None else aug_struct(pkg, cfg)
    scale = default_scale(table.dtype) if scale is None else scale
    a = warp_args(pkg, table.ctypes.data, U8 if table.dtype == np.uint8 else F32, table.shape,
                  None if src is None else src.ctypes.data, row_id.ctypes.data, n, out.ctypes.data, out_hw, scale, fill, aug, epoch)
    rc = pkg.lib().pl_frame_warp_host(ctypes.byref(a))
    assert rc == expect, pkg.lib().pl_last_error()
    return out


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same_bits(x, y):
    return np.array_equal(bits(x), bits(y))


def near_boundary(o64, src_hw):
    """Pixels whose fp64 source position is within BOUNDARY_PX of the extent [-0.5, Ws - 0.5] x [-0.5, Hs - 0.5]."""
    hs, ws = src_hw
    xs, ys = o64["xs"], o64["ys"]
    dist = np.minimum(np.minimum(np.abs(xs + 0.5), np.abs(xs - (ws - 0.5))), np.minimum(np.abs(ys + 0.5), np.abs(ys - (hs - 0.5))))
    return dist < BOUNDARY_PX


def check_against_fp64(out, cfg, epoch, rows, frames, out_hw, scale, fill, what):
    """The 8x-twin gate away from the extent's boundary; prints every figure.  Returns (error, gate)."""
    o64 = fwo.warp(cfg, epoch, rows, frames, out_hw, scale, fill, np.float64)
    o32 = fwo.warp(cfg, epoch, rows, frames, out_hw, scale, fill, np.float32)
    edge = near_boundary(o64, frames.shape[1:3])
    keep = ~edge
    twin = float(np.abs(o32["out"].astype(np.float64) - o64["out"])[keep].max())
    err = float(np.abs(out.astype(np.float64) - o64["out"])[keep].max())
    gate = GATE_FACTOR * twin
    print(f"{what}: worst |error| vs fp64 {err:.3e}; fp32 twin {twin:.3e}; gate {gate:.3e}; {100 * edge.mean():.2f} % of the "
          f"pixels within {BOUNDARY_PX} px of the extent left out, {100 * (~o64['inside']).mean():.1f} % outside")
    assert edge.mean() <= 0.01
    assert twin > 0.0
    assert err <= gate
    return err, gate


@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_same_size_is_the_scaled_source(pkg, dtype):
    table = make_frames((20, 28), dtype)
    for scale in (default_scale(dtype), 0.75):
        want = table[SRC_IDX].astype(np.float32) * np.float32(scale)
        assert same_bits(host_warp(pkg, table, SRC_IDX, ROWS, pao.config(), (20, 28), scale=scale), want)
        assert same_bits(host_warp(pkg, table, SRC_IDX, ROWS, None, (20, 28), scale=scale), want)
        assert same_bits(host_warp(pkg, table, None, ROWS, None, (20, 28), scale=scale), table[:5].astype(np.float32) * np.float32(scale))


@pytest.mark.parametrize("dtype", DTYPES)
def test_flip_same_size_is_the_mirrored_frame(pkg, dtype):
    table = make_frames((20, 28), dtype)
    out = host_warp(pkg, table, SRC_IDX, ROWS, pao.config(p_flip=1.0), (20, 28))
    want = torch.flip(torch.from_numpy(table[SRC_IDX].astype(np.float32) * np.float32(default_scale(dtype))), (2,)).numpy()
    assert same_bits(out, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_halving_is_the_2x2_block_mean(pkg, dtype):
    """8 x 12 into 4 x 6: every weight is exactly 0.5."""
    table = make_frames((8, 12), dtype)
    out = host_warp(pkg, table, SRC_IDX, ROWS, pao.config(), (4, 6))
    f = table[SRC_IDX].astype(np.float32)
    h = np.float32(0.5)
    top = h * f[:, 0::2, 0::2] + h * f[:, 0::2, 1::2]
    bot = h * f[:, 1::2, 0::2] + h * f[:, 1::2, 1::2]
    want = np.float32(default_scale(dtype)) * (h * top + h * bot)
    assert want.dtype == np.float32 and same_bits(out, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("src_hw,out_hw", SHAPES)
def test_rotation_free_configurations_equal_the_fp32_twin_bit_for_bit(pkg, dtype, src_hw, out_hw):
    table = make_frames(src_hw, dtype)
    scale = default_scale(dtype)
    for kw in EXACT:
        cfg = pao.config(**kw)
        for epoch, fill in ((3, 0.0), (2 ** 32 + 3, 0.5)):
            out = host_warp(pkg, table, SRC_IDX, ROWS, cfg, out_hw, epoch=epoch, fill=fill)
            twin = fwo.warp(cfg, epoch, ROWS, table[SRC_IDX], out_hw, scale, fill, np.float32)
            assert same_bits(out, twin["out"]), (kw, epoch)
    # and the stages move pixels
    moved = host_warp(pkg, table, SRC_IDX, ROWS, pao.config(**EXACT[3]), out_hw)
    assert not same_bits(moved, host_warp(pkg, table, SRC_IDX, ROWS, pao.config(), out_hw))


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_stage_on_against_fp64(pkg, dtype):
    cfg = pao.config(**ALL_ON)
    rows = np.arange(40, dtype=np.uint64)
    src = (np.arange(40) * 5) % TABLE_FRAMES
    flips = pao.decisions(cfg, 3, rows, np.float64)["flip"]
    assert flips.any() and not flips.all()
    for src_hw, out_hw in SHAPES:
        table = make_frames(src_hw, dtype)
        out = host_warp(pkg, table, src, rows, cfg, out_hw, epoch=3)
        check_against_fp64(out, cfg, 3, rows, table[src], out_hw, default_scale(dtype), 0.0,
                           f"host, all stages on, {np.dtype(dtype).name} {src_hw} -> {out_hw}, rows 0..39")
    out = host_warp(pkg, make_frames((37, 53), dtype), src, rows, pao.config(max_rot=np.pi, seed=3), (20, 28), fill=-1.0)
    check_against_fp64(out, pao.config(max_rot=np.pi, seed=3), 0, rows, make_frames((37, 53), dtype)[src], (20, 28),
                       default_scale(dtype), -1.0, f"host, rotation alone, {np.dtype(dtype).name}")


def test_stock_torch_fp64(pkg):
    """The definition against torch's own resampling, in fp64: with every stage off F.interpolate(bilinear, align_corners=False),
    with every stage on F.grid_sample(padding_mode="border") at the oracle's source positions on the pixels inside the extent.
    TORCH_TOL: both sides are fp64 (eps 2.2e-16) on values below 1 and positions below 64: 1e-10 is five orders above their
    round-off and five below the fp32 errors the gates above measure.  The library is then held to the torch result under the
    8x-twin gate."""
    TORCH_TOL = 1e-10
    rows = np.arange(40, dtype=np.uint64)
    src = (np.arange(40) * 5) % TABLE_FRAMES
    for src_hw, out_hw in SHAPES:
        table = make_frames(src_hw, np.uint8)
        fr = table[src]
        t = torch.from_numpy(fr.astype(np.float64)).permute(0, 3, 1, 2) / 256.0
        # identity
        want = F.interpolate(t, size=out_hw, mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
        o64 = fwo.warp(pao.config(), 0, rows, fr, out_hw, 1.0 / 256.0, 0.0, np.float64)
        o32 = fwo.warp(pao.config(), 0, rows, fr, out_hw, 1.0 / 256.0, 0.0, np.float32)
        d_oracle = float(np.abs(o64["out"] - want).max())
        twin = float(np.abs(o32["out"].astype(np.float64) - want).max())
        out = host_warp(pkg, table, src, rows, pao.config(), out_hw)
        err = float(np.abs(out.astype(np.float64) - want).max())
        print(f"{src_hw} -> {out_hw} identity vs F.interpolate: oracle {d_oracle:.2e}, library {err:.2e}, twin {twin:.2e}")
        assert d_oracle <= TORCH_TOL and err <= GATE_FACTOR * twin
        # every stage on
        cfg = pao.config(**ALL_ON)
        o64 = fwo.warp(cfg, 3, rows, fr, out_hw, 1.0 / 256.0, 0.0, np.float64)
        o32 = fwo.warp(cfg, 3, rows, fr, out_hw, 1.0 / 256.0, 0.0, np.float32)
        grid = np.stack([(o64["xs"] + 0.5) * 2.0 / src_hw[1] - 1.0, (o64["ys"] + 0.5) * 2.0 / src_hw[0] - 1.0], axis=-1)
        want = F.grid_sample(t, torch.from_numpy(grid), mode="bilinear", padding_mode="border",
                             align_corners=False).permute(0, 2, 3, 1).numpy()
        keep = o64["inside"] & ~near_boundary(o64, src_hw)
        assert 0.5 < keep.mean() < 1.0
        d_oracle = float(np.abs(o64["out"] - want)[keep].max())
        twin = float(np.abs(o32["out"].astype(np.float64) - want)[keep].max())
        out = host_warp(pkg, table, src, rows, cfg, out_hw, epoch=3)
        err = float(np.abs(out.astype(np.float64) - want)[keep].max())
        print(f"{src_hw} -> {out_hw} all stages on vs F.grid_sample(border): oracle {d_oracle:.2e}, library {err:.2e}, "
              f"twin {twin:.2e}, {100 * keep.mean():.1f} % of the pixels compared")
        assert d_oracle <= TORCH_TOL and twin > 0.0 and err <= GATE_FACTOR * twin


# ---- agreement with the poses: the reason the feature exists ------------------------------------------------------------
RAMP_HW, RAMP_UP = (16, 24), 8
# three integer planes a x + b y + d over pixel indices, all within 0..255 on a 16 x 24 frame
RAMP = np.array([[4, 3, 0], [2, 9, 5], [-5, -7, 250]], dtype=np.int64)


def ramp_at(x, y):
    """The planes' values (..., 3) at pixel-index coordinates (x, y), fp64."""
    return RAMP[:, 0] * np.asarray(x, np.float64)[..., None] + RAMP[:, 1] * np.asarray(y, np.float64)[..., None] + RAMP[:, 2]


def bilinear_at(img, u, v):
    """img (n, H, W, 3) sampled at image-normalised (u, v) (n, J) -- pixel centres at (j + 0.5) / W -- in fp64; every tap has
    to be a pixel of the image."""
    n, H, W, _ = img.shape
    x, y = u * W - 0.5, v * H - 0.5
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    assert x0.min() >= 0 and x0.max() + 1 < W and y0.min() >= 0 and y0.max() + 1 < H
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    k = np.arange(n)[:, None]
    img = img.astype(np.float64)
    return (1 - fy) * ((1 - fx) * img[k, y0, x0] + fx * img[k, y0, x0 + 1]) + fy * ((1 - fx) * img[k, y0 + 1, x0] + fx * img[k, y0 + 1, x0 + 1])


def round_trip_twin(cfg, epoch, rows, a, T):
    """The yardstick of the agreement test, without the frame oracle: the ideal warped ramp -- the planes evaluated, in T,
    at the source position of every output pixel centre, the forward transform of pose_augment_oracle solved for its
    input -- sampled at the T twin's output joints exactly as the library's image is sampled at the library's."""
    (Hs, Ws), (Ho, Wo) = RAMP_HW, (RAMP_HW[0] * RAMP_UP, RAMP_HW[1] * RAMP_UP)
    oa, _, d = pao.augment(cfg, epoch, rows, a, np.zeros((len(rows), 17, 3)), T)
    per = lambda x: np.asarray(x, T)[:, None, None]
    cx, cy = T(cfg["cx"]), T(cfg["cy"])
    u = ((np.arange(Wo).astype(T) + T(0.5)) / T(Wo))[None, None, :] - per(d["tx"])
    v = ((np.arange(Ho).astype(T) + T(0.5)) / T(Ho))[None, :, None] - per(d["ty"])
    du, dv = (u - cx) / per(d["s"]), (v - cy) / per(d["s"])
    c, s = per(np.cos(d["theta"])), per(np.sin(d["theta"]))
    u, v = (c * du + s * dv) + cx, (c * dv - s * du) + cy
    u = np.where(d["flip"][:, None, None], T(1) - u, u)
    x, y = u * T(Ws) - T(0.5), v * T(Hs) - T(0.5)
    img = RAMP[:, 0].astype(T) * x[..., None] + RAMP[:, 1].astype(T) * y[..., None] + RAMP[:, 2].astype(T)
    assert img.dtype == T
    return bilinear_at(img, oa[:, :, 0].astype(np.float64), oa[:, :, 1].astype(np.float64))


def test_frame_follows_its_pose(pkg):
    """A linear-ramp frame, warped, read at the augmented 2-D joints shows the ramp's value at the SOURCE joints: frame and
    pose of a row moved together.  Goes through pl_pose_augment_host and pl_frame_warp_host only."""
    (Hs, Ws), n = RAMP_HW, 40
    yy, xx = np.meshgrid(np.arange(Hs), np.arange(Ws), indexing="ij")
    frame = ramp_at(xx, yy)
    assert frame.min() >= 0 and frame.max() <= 255 and len({tuple(r) for r in RAMP}) == 3
    table = np.ascontiguousarray(frame.astype(np.uint8)[None])
    rs = np.random.RandomState(21)
    r, phi = 0.25 * np.sqrt(rs.rand(n, 17)), 2 * np.pi * rs.rand(n, 17)           # joints within 0.25 of the centre: every stage
    a = np.stack([0.5 + r * np.cos(phi), 0.5 + r * np.sin(phi)], axis=2).astype(np.float32)   # keeps them inside the image
    b = np.zeros((n, 17, 3), np.float32)
    cfg = pao.config(**dict(ALL_ON, jitter_sigma=0.0))
    rows, epoch = np.arange(n, dtype=np.uint64), 3
    flips = pao.decisions(cfg, epoch, rows, np.float64)["flip"]
    assert flips.any() and not flips.all()
    oa, ob = np.empty_like(a), np.empty_like(b)
    rid = rows.view(np.int64)
    st = aug_struct(pkg, cfg)
    assert pkg.lib().pl_pose_augment_host(a.ctypes.data, b.ctypes.data, None, rid.ctypes.data, n, n, oa.ctypes.data,
                                          ob.ctypes.data, ctypes.byref(st), epoch) == 0
    img = host_warp(pkg, table, np.zeros(n, np.int64), rows, cfg, (Hs * RAMP_UP, Ws * RAMP_UP), epoch=epoch, scale=1.0, fill=-1000.0)
    got = bilinear_at(img, oa[:, :, 0].astype(np.float64), oa[:, :, 1].astype(np.float64))
    srcj = np.where(flips[:, None], np.array(pao.SWAP)[None, :], np.arange(17)[None, :])       # flip_src_joint under a flip
    sa = np.take_along_axis(a.astype(np.float64), srcj[:, :, None], axis=1)
    want = ramp_at(sa[:, :, 0] * Ws - 0.5, sa[:, :, 1] * Hs - 0.5)
    err = float(np.abs(got - want).max())
    twin = float(np.abs(round_trip_twin(cfg, epoch, rows, a, np.float32) - want).max())
    floor64 = float(np.abs(round_trip_twin(cfg, epoch, rows, a, np.float64) - want).max())
    print(f"frame at the augmented joints vs the ramp at the source joints, {n * 17} joints, {int(flips.sum())} of {n} rows "
          f"flipped: worst |error| {err:.3e}; fp32 round trip {twin:.3e} (fp64 round trip {floor64:.3e}); gate {GATE_FACTOR * twin:.3e}")
    assert floor64 < 1e-9 and twin > 0.0
    assert err <= GATE_FACTOR * twin
    # and an unflipped frame under flipped joints does not pass: the check can fail
    wrong = bilinear_at(host_warp(pkg, table, np.zeros(n, np.int64), rows, pao.config(**dict(ALL_ON, jitter_sigma=0.0, p_flip=0.0)),
                                  (Hs * RAMP_UP, Ws * RAMP_UP), epoch=epoch, scale=1.0, fill=-1000.0),
                        oa[:, :, 0].astype(np.float64), oa[:, :, 1].astype(np.float64))
    assert np.abs(wrong - want)[flips].max() > 1.0 and np.abs(wrong - want)[~flips].max() <= GATE_FACTOR * twin


@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_of_the_draws(pkg, dtype):
    table = make_frames((37, 53), dtype)
    cfg = pao.config(**ALL_ON)
    out_hw = (18, 27)
    ref = host_warp(pkg, table, SRC_IDX, ROWS, cfg, out_hw, epoch=5)
    # other places in the batch, another n, and a pre-gathered table: the same (seed, epoch, row, frame) -> the same bits
    order = np.array([3, 0, 4])
    assert same_bits(host_warp(pkg, table, SRC_IDX[order], ROWS[order], cfg, out_hw, epoch=5), ref[order])
    assert same_bits(host_warp(pkg, table, SRC_IDX[4:], ROWS[4:], cfg, out_hw, epoch=5), ref[4:])
    assert same_bits(host_warp(pkg, np.ascontiguousarray(table[SRC_IDX]), None, ROWS, cfg, out_hw, epoch=5), ref)
    # seed, epoch, row: each changes the draws
    assert not same_bits(host_warp(pkg, table, SRC_IDX, ROWS, cfg, out_hw, epoch=6), ref)
    assert not same_bits(host_warp(pkg, table, SRC_IDX, ROWS, pao.config(**dict(ALL_ON, seed=12)), out_hw, epoch=5), ref)
    assert not same_bits(host_warp(pkg, table, SRC_IDX, ROWS + np.uint64(1), cfg, out_hw, epoch=5), ref)
    # jitter_sigma is pose noise
    for sigma in (0.0, 0.5):
        assert same_bits(host_warp(pkg, table, SRC_IDX, ROWS, pao.config(**dict(ALL_ON, jitter_sigma=sigma)), out_hw, epoch=5), ref)
    # the frame's flip bit is the pose's
    exact = pao.config(p_flip=0.5, seed=7)
    rows = np.arange(64, dtype=np.uint64)
    one = np.ascontiguousarray(table[:1])
    out = host_warp(pkg, one, np.zeros(64, np.int64), rows, exact, (37, 53), epoch=2)
    plain = one[0].astype(np.float32) * np.float32(default_scale(dtype))
    flips = pao.decisions(exact, 2, rows, np.float64)["flip"]
    assert flips.any() and not flips.all()
    for k in range(64):
        assert same_bits(out[k], plain[:, ::-1] if flips[k] else plain), k


def test_errors(pkg):
    L = pkg.lib()
    table = make_frames((9, 7), np.uint8)
    out = np.zeros((5, 4, 6, 3), np.float32)
    rid = ROWS.view(np.int64)

    def call(fn=L.pl_frame_warp_host, tp=table.ctypes.data, code=U8, shape=table.shape, src=SRC_IDX.ctypes.data,
             rows=rid.ctypes.data, n=5, op=out.ctypes.data, out_hw=(4, 6), scale=1.0, fill=0.0, cfg=pao.config(), C=3, extra=()):
        a = warp_args(pkg, tp, code, shape, src, rows, n, op, out_hw, scale, fill, None if cfg is None else aug_struct(pkg, cfg), 0, C=C)
        return fn(ctypes.byref(a), *extra)

    assert call() == 0 and call(cfg=None, rows=None) == 0 and call(rows=None) == 0      # no draw is read: row_id may be absent
    for kw in (dict(tp=None), dict(op=None), dict(rows=None, cfg=pao.config(p_flip=0.5))):
        assert call(**kw) == EINVAL and b"null" in L.pl_last_error(), kw
    assert L.pl_frame_warp_host(None) == EINVAL
    assert call(C=4) == ESHAPE and b"C=4" in L.pl_last_error()
    assert call(C=1) == ESHAPE
    for kw in (dict(n=0), dict(n=-2), dict(out_hw=(0, 6)), dict(out_hw=(4, -1)), dict(shape=(9, 0, 7)), dict(shape=(0, 9, 7)),
               dict(shape=(9, 9, -7)), dict(src=None, n=10), dict(n=70000)):
        assert call(**kw) == ESHAPE and b"pl_frame_warp_host" in L.pl_last_error(), kw
    assert call(code=2) == EINVAL
    bad = SRC_IDX.copy()
    for v in (TABLE_FRAMES, -1):
        bad[2] = v
        assert call(src=bad.ctypes.data) == EINVAL and b"outside the table" in L.pl_last_error()
    assert call(op=table.ctypes.data) == EINVAL and b"aliased" in L.pl_last_error()
    # a frame flip mirrors about the image centre
    raw = lambda **kw: dict(pao.config(), **kw)
    assert call(cfg=raw(p_flip=0.5, flip_offset=0.0)) == EINVAL and b"flip_offset" in L.pl_last_error()
    assert call(cfg=raw(p_flip=1.0, flip_offset=0.5)) == EINVAL
    assert call(cfg=raw(flip_offset=0.0)) == 0                                        # no flip: the offset is not read
    # the PLPoseAug checks of the pose gather
    for kw, text in ((dict(scale_range=1.0), b"scale_range"), (dict(max_rot=float("nan")), b"max_rot"),
                     (dict(p_flip=-0.1), b"p_flip"), (dict(max_shift=float("inf")), b"max_shift"), (dict(cx=float("nan")), b"cx")):
        assert call(cfg=raw(**kw)) == EINVAL and text in L.pl_last_error(), kw
    assert call(scale=float("nan")) == EINVAL and call(fill=float("inf")) == EINVAL
    # the device entry point runs the same checks before it touches a device
    g = dict(fn=L.pl_frame_warp_gather, extra=(None,))
    assert call(C=4, **g) == ESHAPE and call(tp=None, **g) == EINVAL and call(n=0, **g) == ESHAPE
    assert call(cfg=raw(p_flip=0.5, flip_offset=0.0), **g) == EINVAL and b"pl_frame_warp_gather" in L.pl_last_error()
    assert ctypes.sizeof(pkg._lib.PLFrameWarp) == 112


def test_python_surface(pkg):
    assert pkg.augment_frames is pkg.data.augment_frames and pkg.FrameFeeder is pkg.data.FrameFeeder
    frames = torch.zeros(4, 9, 7, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        pkg.augment_frames(frames, pkg.PoseAugment(p_flip=0.5, flip_offset=0.0))
    with pytest.raises(ValueError):
        pkg.FrameFeeder(frames, torch.zeros(4, 17, 2), torch.zeros(4, 17, 3), 2, augment=pkg.PoseAugment(p_flip=1.0, flip_offset=0.0))
    with pytest.raises(TypeError):
        pkg.augment_frames(frames, dict(p_flip=0.5))
    with pytest.raises(ValueError):
        pkg.augment_frames(torch.zeros(4, 9, 7, 4, dtype=torch.uint8), None)
    with pytest.raises(ValueError):
        pkg.augment_frames(frames.to(torch.int32), None)
    with pytest.raises(ValueError):
        pkg.augment_frames(frames, None, out_hw=(0, 4))
    with pytest.raises(pkg.PoseliftError):
        pkg.augment_frames(frames, None)                                              # no CPU path
