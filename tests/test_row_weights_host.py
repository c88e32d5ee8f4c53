"""CPU tests of the criterion's per-pose joint weights (PoseCriterion(...)(pred, target, row_weights=); include/poselift.h
PLRowWeightsCriterion): the numpy oracle against torch's own modules, the ctypes mirror against the header, the
entry points' refusals before a device is touched, the Python argument checks, and pl_row_weights_gather_host -- the text the
gather kernel runs -- against the oracle and against the flip the pose augmentation makes for the same (seed, epoch, row)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import row_weights_oracle as orc
from conftest import ROOT

EINVAL, ESHAPE = -1, -2


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()          # compiles libposelift.so for gfx950 if missing (no GPU needed)


def _joint_weights(J, seed=3):
    w = np.random.default_rng(seed).uniform(0.25, 2.0, J).astype(np.float32)
    w[0] = 0.0
    return w


# ------------------------------------------------------------------------------------------------- oracle against torch
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("G", [1, 2, 3])
@pytest.mark.parametrize("kind", orc.KINDS)
def test_oracle_is_torch_on_the_cpu(kind, G, both):
    """(W * (p - t)**2).mean(), |.|, SmoothL1Loss(reduction="none") and (W * norm(d, dim=-1)).mean() in fp64: values and
    autograd gradients, with W = rw or fl32(w_j * rw)."""
    B, J = 9, 7
    rng = np.random.default_rng(10 * G + both)
    p, t = rng.standard_normal((B, J * G)), rng.standard_normal((B, J * G))
    t[0, :G] = p[0, :G]                                                  # a zero joint
    W = orc.effective_weights(orc.weights(B, J, seed=G), _joint_weights(J) if both else None)
    if both:
        assert np.array_equal(W, _joint_weights(J)[None, :] * orc.weights(B, J, seed=G))
    loss, grad = orc.criterion(kind, p, t, G, W, beta=0.5)
    want_l, want_g = orc.torch_criterion(kind, p, t, G, W, 0.5)
    assert abs(loss - want_l) <= 1e-14 * abs(want_l)
    np.testing.assert_allclose(grad, want_g, rtol=1e-13, atol=1e-300)
    assert (grad[W.repeat(G, axis=1) == 0] == 0).all() and (grad[0, :G] == 0).all()
    g32 = orc.grad_fp32(kind, p.astype(np.float32), t.astype(np.float32), G, W, beta=0.5)
    _, g64 = orc.criterion(kind, p.astype(np.float32), t.astype(np.float32), G, W, beta=0.5)
    np.testing.assert_allclose(g32, g64, rtol=1e-6, atol=0)


@pytest.mark.parametrize("zero_weight", [False, True])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("kind", orc.KINDS)
def test_oracle_nonfinite_set_is_torchs(kind, bad, zero_weight):
    """One poisoned element, under a non-zero and under a zero weight: 0 * NaN = NaN, the set is torch's (fp32, CPU)."""
    B, J, G = 6, 17, 3
    rng = np.random.default_rng(5)
    p, t = rng.standard_normal((B, J * G)).astype(np.float32), rng.standard_normal((B, J * G)).astype(np.float32)
    W = rng.uniform(0.5, 1.5, (B, J)).astype(np.float32)
    p[2, 7] = bad
    if zero_weight:
        W[2, 7 // G] = 0.0
    loss, grad = orc.criterion(kind, p, t, G, W, beta=0.5)
    want_l, want_g = orc.torch_criterion(kind, p, t, G, W, 0.5, dtype=np.float32)
    assert np.isnan(loss) == np.isnan(want_l) and np.isinf(loss) == np.isinf(want_l)
    assert np.array_equal(np.isnan(grad), np.isnan(want_g)) and np.array_equal(np.isinf(grad), np.isinf(want_g))
    if zero_weight:
        assert np.isnan(loss)                                            # the zero weight hid nothing


# ------------------------------------------------------------------------------------------------- ABI
def test_ctypes_mirror_follows_the_header(pkg):
    header = open(os.path.join(ROOT, "include", "poselift.h")).read()
    L, lib = pkg._lib, pkg.lib()
    assert int(re.search(r"#define PL_CRIT_HAS_ROW_WEIGHTS (0x[0-9a-fA-F]+)", header).group(1), 16) == L.CRIT_HAS_ROW_WEIGHTS == 0x200
    body = re.search(r"typedef struct PLRowWeightsCriterion \{(.*?)\} PLRowWeightsCriterion;", header, re.S).group(1)
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    assert decls == ["PLSkeletonCriterion sc", "const float* row_weights"]
    assert lib.pl_criterion_abi_bytes(3) == ctypes.sizeof(L.PLRowWeightsCriterion) == 40
    assert L.PLRowWeightsCriterion.row_weights.offset == 32 and L.PLRowWeightsCriterion.skeleton.offset == 24
    assert L.PLRowWeightsCriterion.kind.offset == 0 and L.PLRowWeightsCriterion.weights.offset == 16
    assert issubclass(L.PLRowWeightsCriterion, L.PLSkeletonCriterion) and issubclass(L.PLRowWeightsCriterion, L.PLCriterion)
    # the structs that were there keep their sizes, and the older query its answers
    assert [lib.pl_skeleton_abi_bytes(i) for i in range(3)] == [24, 72, 32] == [lib.pl_criterion_abi_bytes(i) for i in range(3)]
    assert lib.pl_criterion_abi_bytes(4) == 0 and lib.pl_criterion_abi_bytes(-1) == 0
    for name in ("pl_criterion_abi_bytes", "pl_row_weights_gather", "pl_row_weights_gather_host"):
        assert name in L.SIGNATURES and re.search(r"\b%s\s*\(" % name, header)


def test_entry_points_refuse_before_touching_a_device(pkg):
    L, lib = pkg._lib, pkg.lib()
    one = ctypes.c_void_p(16)

    def call(B=4, O=51, group=3, kind=0, rw=16, flags=L.CRIT_HAS_ROW_WEIGHTS, skeleton=False):
        st = L.PLRowWeightsCriterion(kind | flags, group, 1.0, None)
        st.row_weights = rw
        if skeleton:
            sk = L.PLSkeleton(17, 16, 6, 0, 16, 16, 16, 16, 16, None, None)
            st.skeleton = ctypes.pointer(sk)
        return lib.pl_pose_loss_fwd_bwd(one, one, B, O, ctypes.byref(st), 1.0, None, one, one, None)

    for kind in range(4):
        assert call(kind=kind, rw=None) == EINVAL and b"row_weights" in lib.pl_last_error()
        both = L.CRIT_HAS_ROW_WEIGHTS | L.CRIT_HAS_SKELETON
        assert call(kind=kind, flags=both, skeleton=True) == EINVAL and b"not built" in lib.pl_last_error()
        assert call(kind=kind, flags=both) == EINVAL and b"not built" in lib.pl_last_error()          # (a NULL skeleton too)
        assert call(kind=kind, B=(2 ** 31 - 1) // 51 + 1) == ESHAPE and b"32 bits" in lib.pl_last_error()
        assert call(kind=kind, B=2 ** 40) == ESHAPE
    assert call(kind=7) == EINVAL and b"kind" in lib.pl_last_error()
    assert call(O=50) == ESHAPE and call(B=0) == ESHAPE
    # the scratch query reads nothing past the flag
    st = L.PLRowWeightsCriterion(L.CRIT_MPJPE | L.CRIT_HAS_ROW_WEIGHTS, 3, 1.0, None)
    for B in (1, 64, 4096):
        assert lib.pl_pose_loss_scratch_bytes(B, 51, ctypes.byref(st)) == lib.pl_mse_scratch_bytes(B * 51)
    # the lifter's entry points refuse the same criteria (a descriptor that passes its own checks is needed to get there;
    # tests/test_gpu_row_weights.py covers them on the device)


def test_python_argument_checks(pkg):
    crit = pkg.PoseCriterion("l1", coords=3)
    p, t = torch.zeros(4, 51), torch.zeros(4, 51)
    for bad in (torch.ones(4, 51), torch.ones(17), torch.ones(5, 17), torch.ones(4, 17, 1)):
        with pytest.raises(ValueError, match="row_weights has shape"):
            crit(p, t, row_weights=bad)
    with pytest.raises(ValueError, match="requires grad"):
        crit(p, t, row_weights=torch.ones(4, 17, requires_grad=True))
    with pytest.raises(TypeError):
        crit(p, t, row_weights=np.ones((4, 17), np.float32))
    sk = pkg.PoseCriterion("l1", coords=3, skeleton=pkg.H36M_SKELETON, bone_weight=0.1)
    with pytest.raises(ValueError, match="skeleton"):
        sk(p, t, row_weights=torch.ones(4, 17))
    with pytest.raises(ValueError, match="skeleton"):
        sk.struct(51, torch.device("cpu"), torch.ones(4, 17))
    for fn in (pkg.train.train_step, pkg.train.eval_step):
        with pytest.raises(ValueError, match="criterion"):
            fn(None, None, p, t, row_weights=torch.ones(4, 17)) if fn is pkg.train.train_step else \
                fn(None, p, t, row_weights=torch.ones(4, 17))
    with pytest.raises(ValueError, match="criterion"):
        pkg.GraphedTrainStep(None, None, p, t, row_weights=torch.ones(4, 17))
    # the struct carries the flag and the pointer; a bool mask is converted (a copy)
    rw = torch.ones(4, 17)
    st = crit.struct(51, torch.device("cpu"), rw)
    assert st.kind == pkg._lib.CRIT_L1 | pkg._lib.CRIT_HAS_ROW_WEIGHTS and st.row_weights == rw.data_ptr()
    from importlib import import_module
    chk = import_module(pkg.__name__ + ".criterion").check_row_weights
    mask = torch.ones(4, 17, dtype=torch.bool)
    out = chk(mask, 4, 17, mask.device)
    assert out.dtype == torch.float32 and out.data_ptr() != mask.data_ptr() and chk(rw, 4, 17, rw.device).data_ptr() == rw.data_ptr()


def test_normalize_row_weights(pkg):
    rw = torch.from_numpy(orc.weights(8, 17))
    out = pkg.normalize_row_weights(rw)
    assert abs(out.sum().item() - 8 * 17) < 1e-3 and torch.equal(out == 0, rw == 0)
    np.testing.assert_allclose(out.numpy(), rw.numpy() * (8 * 17 / rw.double().sum().item()), rtol=1e-6)
    assert torch.equal(pkg.normalize_row_weights(torch.zeros(3, 5)), torch.zeros(3, 5))
    mask = torch.tensor([[True, False], [True, True]])
    assert torch.equal(pkg.normalize_row_weights(mask), mask.float() * (4.0 / 3.0))
    assert "normalize_row_weights" in dir(pkg) and "gather_row_weights" in dir(pkg)


# ------------------------------------------------------------------------------------------------- the gather
def _aug(pkg, p_flip, seed=1234, **kw):
    cfg = dict(flip_offset=1.0, max_rot=0.0, scale_range=0.0, max_shift=0.0, jitter_sigma=0.0, cx=0.5, cy=0.5)
    cfg.update(kw)
    return pkg._lib.PLPoseAug(p_flip, cfg["flip_offset"], cfg["max_rot"], cfg["scale_range"], cfg["max_shift"],
                              cfg["jitter_sigma"], cfg["cx"], cfg["cy"], seed)


def _gather(pkg, w, src, rid, aug, epoch=0, expect=0):
    w = np.ascontiguousarray(w, np.float32)
    n = len(src) if src is not None else (len(rid) if rid is not None else w.shape[0])
    out = np.full((n, w.shape[1]), -7.0, np.float32)
    src = None if src is None else np.ascontiguousarray(src, np.int64)
    rid = None if rid is None else np.ascontiguousarray(rid, np.int64)
    rc = pkg.lib().pl_row_weights_gather_host(w.ctypes.data, None if src is None else src.ctypes.data,
                                              None if rid is None else rid.ctypes.data, n, w.shape[0], w.shape[1],
                                              out.ctypes.data, None if aug is None else ctypes.byref(aug), epoch)
    assert rc == expect, pkg.lib().pl_last_error()
    return out


def test_gather_with_flip_never_and_always(pkg):
    rng = np.random.default_rng(0)
    w = rng.uniform(0, 2, (40, 17)).astype(np.float32)
    src = rng.integers(0, 40, 23)
    rid = rng.integers(0, 10 ** 6, 23)
    for p_flip, flipped in ((0.0, None), (1.0, np.ones(23, bool))):
        got = _gather(pkg, w, src, rid, _aug(pkg, p_flip))
        assert np.array_equal(got, orc.gather(w, src, flipped))
        got = _gather(pkg, w[:23], None, rid, _aug(pkg, p_flip))
        assert np.array_equal(got, orc.gather(w[:23], None, flipped))
    assert np.array_equal(_gather(pkg, w, src, None, None), w[src])                  # no augmentation: table[idx]
    # the other stages of the augmentation move no joint: their parameters change nothing
    busy = _aug(pkg, 1.0, max_rot=0.3, scale_range=0.2, max_shift=0.1, jitter_sigma=0.05)
    assert np.array_equal(_gather(pkg, w, src, rid, busy), orc.gather(w, src, np.ones(23, bool)))
    # any J without a flip; J = 17 with one
    w5 = rng.uniform(0, 2, (40, 5)).astype(np.float32)
    assert np.array_equal(_gather(pkg, w5, src, rid, _aug(pkg, 0.0)), w5[src])
    assert np.array_equal(_gather(pkg, w5, src, None, None), w5[src])
    _gather(pkg, w5, src, rid, _aug(pkg, 0.5), expect=ESHAPE)
    _gather(pkg, w5, src, rid, _aug(pkg, 1.0), expect=ESHAPE)
    # a bad index, a missing row_id under a drawn flip, a bad parameter
    for bad in (-1, 40):
        s2 = src.copy()
        s2[5] = bad
        _gather(pkg, w, s2, rid, _aug(pkg, 0.0), expect=EINVAL)
        assert b"outside the table" in pkg.lib().pl_last_error()
    out = np.empty((23, 17), np.float32)
    s64 = np.ascontiguousarray(src, np.int64)
    assert pkg.lib().pl_row_weights_gather_host(w.ctypes.data, s64.ctypes.data, None, 23, 40, 17, out.ctypes.data,
                                                ctypes.byref(_aug(pkg, 0.5)), 0) == EINVAL
    assert pkg.lib().pl_row_weights_gather_host(w.ctypes.data, s64.ctypes.data, None, 0, 40, 17, out.ctypes.data, None, 0) == ESHAPE
    assert pkg.lib().pl_row_weights_gather_host(None, s64.ctypes.data, None, 23, 40, 17, out.ctypes.data, None, 0) == EINVAL
    assert pkg.lib().pl_row_weights_gather_host(w.ctypes.data, None, None, 41, 40, 17, out.ctypes.data, None, 0) == ESHAPE


@pytest.mark.parametrize("epoch", [0, 3])
def test_gather_follows_the_poses_flip(pkg, epoch):
    """p_flip = 0.5 with every other stage on: the joint order read from z of the augmented 3-D pose (z of joint j is j in the
    table, and no stage moves z) equals the gathered weights of w[n][j] = j, row by row, and both flip states occur."""
    n = 64
    rng = np.random.default_rng(2)
    a = rng.uniform(0.2, 0.8, (n, 17, 2)).astype(np.float32)
    b = rng.standard_normal((n, 17, 3)).astype(np.float32)
    b[:, :, 2] = np.arange(17, dtype=np.float32)[None, :]
    rows = np.ascontiguousarray(rng.permutation(100000)[:n], np.int64)
    aug = _aug(pkg, 0.5, seed=0xDEADBEEF12345, max_rot=0.4, scale_range=0.2, max_shift=0.05, jitter_sigma=0.01)
    oa, ob = np.empty_like(a), np.empty_like(b)
    assert pkg.lib().pl_pose_augment_host(a.ctypes.data, b.ctypes.data, None, rows.ctypes.data, n, n, oa.ctypes.data,
                                          ob.ctypes.data, ctypes.byref(aug), epoch) == 0
    w = np.tile(np.arange(17, dtype=np.float32), (n, 1))
    got = _gather(pkg, w, None, rows, aug, epoch=epoch)
    assert np.array_equal(got, ob[:, :, 2])
    flipped = ob[:, 1, 2] == 4.0
    assert 0 < flipped.sum() < n
    assert np.array_equal(got, orc.gather(w, None, flipped))
