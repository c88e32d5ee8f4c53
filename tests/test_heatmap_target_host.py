"""CPU tests of the Gaussian heat-map target: csrc/heatmap_target.h through pl_heatmap_gaussian_host (the same inline text the
kernels run, compiled for the CPU) against the reference's own function (fixture g14: H36_dataset._keypoint_to_heatmap_3D at
both of its sigmas), against the fp64 restatement in heatmap_oracle.py, and on hand-built edge cases."""
import ctypes

import numpy as np
import pytest

import heatmap_oracle as orc
from conftest import load_golden

# The reference evaluates exp in fp64 and rounds to fp32.  The header forms the exponent in fp64 and hands expf a fp32 head
# and a first-order tail: measured worst case over all of g14 on the host 2 ulps of the value (1 ulp at sigma 0.5); the
# gate is 4x that.  (The fp64 restatement of heatmap_oracle.py is within 0.5 ulp -- the rounding -- of every g14 value.)
G14_GATE_ULPS = 8.0


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()


@pytest.fixture(scope="module")
def g14():
    return load_golden("g14_heatmap_targets.npz")


def host_target(pkg, target, D, H, W, sigma, law, ncoord=None, expect=0):
    ncoord = ncoord or (3 if D > 1 else 2)
    t = np.ascontiguousarray(target, dtype=np.float32).reshape(-1, ncoord)
    out = np.full((t.shape[0], D, H, W), -7.0, np.float32)
    rc = pkg.lib().pl_heatmap_gaussian_host(t.ctypes.data, t.shape[0], D, H, W, ncoord, float(sigma), (ctypes.c_float * 6)(*law),
                                            out.ctypes.data)
    assert rc == expect, pkg.lib().pl_last_error()
    return out


def g14_maps(g14, si):
    """(keypoint in the head's (x, y, z) order, flat indices, values, sum g^2) per map: the reference indexes its volume
    [u][v][w] by the keypoint's (first, second, third) entry, the library's maps are [D][H][W] <-> (z, y, x)."""
    off = 0
    for n, c in enumerate(g14[f"s{si}:count"]):
        yield (g14["keypoints"][n][::-1], g14[f"s{si}:index"][off:off + c], g14[f"s{si}:value"][off:off + c],
               g14[f"s{si}:sumsq"][n])
        off += c


def check_against_g14(dense, g14, si, gate=G14_GATE_ULPS):
    """dense (24, 64, 64, 64) fp32 of the g14 keypoints -> the worst error in ulps of the reference's value."""
    worst = 0.0
    for n, (_, idx, val, sumsq) in enumerate(g14_maps(g14, si)):
        flat = dense[n].reshape(-1)
        assert np.array_equal(np.flatnonzero(flat), idx), f"map {n}: the non-zero set differs from the reference's"
        ulps = np.abs(flat[idx].astype(np.float64) - val.astype(np.float64)) / np.spacing(val).astype(np.float64)
        worst = max(worst, float(ulps.max()))
        assert abs((flat.astype(np.float64) ** 2).sum() - sumsq) <= 1e-5 * sumsq
    print(f"sigma {g14['sigmas'][si]}: worst error {worst:.2f} ulps of the reference's value (gate {gate})")
    assert worst <= gate
    return worst


def test_fixture_holds_what_the_issue_asks_for(g14):
    kp = g14["keypoints"]
    assert kp.dtype == np.float32 and kp.shape == (24, 3) and list(g14["sigmas"]) == [0.5, 1.75]
    assert kp.min() >= -1 and kp.max() <= 1
    for corner in ((-1, -1, -1), (1, 1, 1), (0, 0, 0)):
        assert (kp == np.float32(corner)).all(axis=1).any()
    c0 = g14["s0:count"]
    assert c0[0] == 8 and c0[1] == 8 and c0[2] == 27 and g14["s1:count"].max() == 11 ** 3
    # the rounding tie: 31.5 goes to 32, so the window of (0, 0, 0) at sigma 0.5 is 31..33 on every axis
    idx = g14["s0:index"][16:16 + 27]
    assert idx.min() == (31 * 64 + 31) * 64 + 31 and idx.max() == (33 * 64 + 33) * 64 + 33


@pytest.mark.parametrize("si", [0, 1])
def test_host_target_matches_the_reference_function(pkg, g14, si):
    heads = pkg.heads
    law = heads.heatmap_law(64, 64, 64, True, "reference")
    assert law == [31.5, 31.5, 31.5, 1.0, 1.0, 1.0]
    kp = np.stack([k for k, _, _, _ in g14_maps(g14, si)])
    dense = host_target(pkg, kp, 64, 64, 64, g14["sigmas"][si], law)
    check_against_g14(dense, g14, si)


@pytest.mark.parametrize("si", [0, 1])
def test_oracle_restatement_matches_the_reference_function(g14, si):
    """The fp64 oracle the GPU tests lean on is the same function: within its own rounding to fp32 of every g14 value."""
    kp = np.stack([k for k, _, _, _ in g14_maps(g14, si)])
    dense = orc.dense_target(kp, 64, 64, 64, float(g14["sigmas"][si]), [31.5] * 3 + [1.0] * 3).astype(np.float32)
    assert check_against_g14(dense, g14, si, gate=1.0) <= 0.5


def test_widest_supported_window_and_the_first_refused_one(pkg):
    heads = pkg.heads
    law = heads.heatmap_law(24, 20, 20, True, "head")
    assert orc.half_of_sigma(2.75) == 8 and orc.half_of_sigma(2.9) == 9
    t = np.array([[0.1, -0.2, 0.05], [-1.0, 1.0, 0.9]], np.float32)
    got = host_target(pkg, t, 20, 20, 24, 2.75, law)
    want = orc.dense_target(t, 20, 20, 24, 2.75, law)
    assert np.array_equal(got != 0, want != 0) and (got[0] != 0).sum() == 17 ** 3
    assert np.abs(got - want).max() <= 8 * np.finfo(np.float32).eps
    host_target(pkg, t, 20, 20, 24, 2.9, law, expect=-2)               # PL_ESHAPE
    assert b"half-width 9" in pkg.lib().pl_last_error()


def test_window_off_the_map_is_zero_and_a_nan_coordinate_is_nan_for_its_pair_only(pkg):
    heads = pkg.heads
    law = heads.heatmap_law(16, 16, 16, True, "head")
    t = np.array([[0.0, 0.0, 0.0], [5.0, 0.0, 0.0], [0.0, np.nan, 0.0], [0.0, 0.0, -np.inf], [1.0e30, -1.0e30, 1.0e20],
                  [1.2, 0.0, 0.0]], np.float32)
    got = host_target(pkg, t, 16, 16, 16, 0.5, law)
    assert (got[0] != 0).sum() == 27 and got[0, 8, 8, 8] == 1.0
    assert not got[1].any() and not got[4].any()                    # wholly outside: all zero, no error
    assert np.isnan(got[2]).all() and np.isnan(got[3]).all()
    # mu = 17.6 -> c = 18, window 17..19: off a 16-wide map, while t = 1.0 (mu = 16, window 15..17) still touches it
    assert not got[5].any()
    edge = host_target(pkg, np.array([[1.0, 0.0, 0.0]], np.float32), 16, 16, 16, 0.5, law)
    assert (edge != 0).sum() == 9 and np.flatnonzero(edge.sum(axis=(0, 1, 2))).tolist() == [15]


def test_2d_head_law_and_depth_one_has_no_depth_factor(pkg):
    heads = pkg.heads
    law = heads.heatmap_law(12, 8, 1, False, "head")
    assert law == [12.0, 8.0, 1.0, 0.0, 0.0, 0.0]
    t = np.array([[0.5, 0.25], [0.29166667, 0.9375]], np.float32)       # mu = (6, 2) exactly; (3.5, 7.5): ties -> (4, 8)
    got = host_target(pkg, t, 1, 8, 12, 0.5, law)
    want = orc.dense_target(t, 1, 8, 12, 0.5, law)
    assert got.shape == (2, 1, 8, 12) and got[0, 0, 2, 6] == 1.0 and (got[0] != 0).sum() == 9
    assert np.array_equal(got != 0, want != 0) and np.abs(got - want).max() <= 8 * np.finfo(np.float32).eps
    assert np.flatnonzero(got[1].sum(axis=(0, 2))).tolist() == [7]      # rows 7..9 clipped to 7; columns 3..5
    assert np.flatnonzero(got[1].sum(axis=(0, 1))).tolist() == [3, 4, 5]
    with pytest.raises(ValueError, match="centred heads only"):
        heads.heatmap_law(12, 8, 1, False, "reference")
    with pytest.raises(ValueError, match="centre is"):
        heads.heatmap_law(12, 8, 1, True, "dataset")


def test_entry_points_reject_bad_arguments_without_a_device(pkg):
    L = pkg.lib()
    law = (ctypes.c_float * 6)(8, 8, 8, 1, 1, 1)
    buf = np.zeros(4096, np.float32)
    p = buf.ctypes.data
    assert L.pl_heatmap_gaussian_host(None, 1, 4, 4, 4, 3, 0.5, law, p) == -1
    assert L.pl_heatmap_gaussian_host(p, 1, 4, 4, 4, 3, 0.5, None, p) == -1
    assert L.pl_heatmap_gaussian_host(p, 1, 4, 4, 4, 3, 0.0, law, p) == -1
    assert L.pl_heatmap_gaussian_host(p, 1, 4, 4, 4, 3, float("nan"), law, p) == -1
    assert L.pl_heatmap_gaussian_host(p, 1, 4, 4, 4, 2, 0.5, law, p) == -2          # two coordinates need depth 1
    assert L.pl_heatmap_gaussian_host(p, 0, 4, 4, 4, 3, 0.5, law, p) == -2
    assert L.pl_softargmax_hm_fwd(p, p, 1, 4, 4, 4, 3, 1, 3.0, law, p, p, p, None) == -2    # half 9
    assert L.pl_softargmax_hm_fwd(p, p, 1, 4, 4, 6, 3, 1, 0.5, law, p, p, p, None) == -2    # W % 4
    assert L.pl_softargmax_hm_fwd(p, None, 1, 4, 4, 4, 3, 1, 0.5, law, p, p, p, None) == -1
    assert L.pl_softargmax_hm_bwd(p, p, p, p, None, 1, 4, 4, 4, 3, 1, 0.5, law, p, None) == -1
    assert L.pl_softargmax3d_nhwc_hm_fwd(p, p, 1, 0, 4, 4, 0.5, law, p, p, p, None) == -2
    assert L.pl_softargmax3d_nhwc_hm_bwd_ex(p, p, p, p, p, 1, 1, 4, 4, 0.5, law, None, None, 0, None, None) == -1
    assert L.pl_softargmax3d_nhwc_hm_bwd_ex(p, p, p, p, p, 1, 1, 4, 4, 9.0, law, p, None, 0, None, None) == -2
    assert L.pl_softargmax_hm_dl_scale(p, None, 4, 3, p, None) == -1
    assert L.pl_softargmax_hm_dl_scale(p, p, 4, 4, p, None) == -2
