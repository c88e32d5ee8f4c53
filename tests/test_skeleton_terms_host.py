"""CPU tests of the criterion's skeleton terms (pl.Skeleton, PoseCriterion(skeleton=); include/poselift.h PLSkeleton; DESIGN
3d.2): the numpy oracle against torch autograd in fp64, the per-pose arithmetic of csrc/skeleton_terms.h through
pl_skeleton_terms_host (the same text the kernel runs) against the oracle, Skeleton's validation, H36M_SKELETON against the
joint selection and the flip tables, and the ctypes mirror of the C structs."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import skeleton_terms_oracle as orc
from conftest import ROOT
from pose_augment_oracle import LEFT, RIGHT

U = orc.U
EINVAL, ESHAPE = -1, -2
GOLDEN = os.path.join(ROOT, "tests", "golden", "g13_pose_metrics.npz")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()          # compiles libposelift.so for gfx950 if missing (no GPU needed)


def _skel(name):
    if name == "h36m":
        return orc.tables(orc.H36M_PARENTS, orc.H36M_LEFT, orc.H36M_RIGHT)
    return orc.tables(orc.CHAIN_PARENTS, orc.CHAIN_LEFT, orc.CHAIN_RIGHT)


def _transform(J, G, seed=2):
    rng = np.random.default_rng(seed)
    sub = rng.uniform(-300.0, 300.0, (J, G)).astype(np.float32)
    div = rng.uniform(50.0, 250.0, (J, G)).astype(np.float32)
    sub[0], div[0] = 0.0, 0.0                       # the zeroed root: a dead column
    div[J - 1, G - 1] = 0.0                         # ... and one inside a live joint
    return sub.reshape(-1), div.reshape(-1)


def _standardise(ref, p, t, G):
    """(pred, target in the model's space, sub, div) for raw poses p, t: the transform a user has -- the mean and std of each
    column of a reference set `ref` of the same data, the root zeroed (div == 0 on its columns, and on any constant column).
    The accuracy tests use this transform, not _transform's arbitrary one: the 1e-5 bound on the loss needs e = lh - l not to
    be a small difference of long lengths, and offsets of hundreds of units on every joint make every bone long (lh / e of
    1e3: no fp32 evaluation of the documented expression reaches 1e-5 then), which no statistics of real poses do."""
    sub, div = ref.astype(np.float64).mean(0), ref.astype(np.float64).std(0)
    sub[:G], div[:G] = 0.0, 0.0
    sub, div = sub.astype(np.float32), div.astype(np.float32)

    def apply(x):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(div > 0, (x - sub) / div, 0.0).astype(np.float32)
    return apply(p), apply(t), sub, div


def _poses(name, B, G, scale=1.0, seed=0):
    rng = np.random.default_rng(seed + 17 * B)
    if name == "g13":
        with np.load(GOLDEN, allow_pickle=False) as z:
            p, t = z["pred"][:B, :, :G].copy(), z["tgt"][:B, :, :G].copy()
        return (p * scale).astype(np.float32).reshape(B, -1), (t * scale).astype(np.float32).reshape(B, -1)
    J = 17 if name == "h36m" else 5
    t = (rng.standard_normal((B, J, G)) * scale).astype(np.float32)
    p = (t + 0.1 * scale * rng.standard_normal((B, J, G))).astype(np.float32)
    return p.reshape(B, -1), t.reshape(B, -1)


def _host(pkg, p, t, G, tabs, lam, rho, sub=None, div=None, grad_scale=1.0, want_grad=True):
    """pl_skeleton_terms_host on numpy arrays: (value, gradient or None, lengths)"""
    child, parent, pairs = tabs
    B, W = p.shape
    K, S = len(child), len(pairs)
    c32, p32 = child.astype(np.int32), parent.astype(np.int32)
    pa, pb = np.ascontiguousarray(pairs[:, 0].astype(np.int32)), np.ascontiguousarray(pairs[:, 1].astype(np.int32))
    tw = np.array(lam, dtype=np.float32)
    keep = [c32, p32, pa, pb, tw, sub, div]
    sk = pkg._lib.PLSkeleton(W // G, K, S, 0 if rho == "l1" else 1, c32.ctypes.data, p32.ctypes.data, pa.ctypes.data if S else None,
                             pb.ctypes.data if S else None, tw.ctypes.data, sub.ctypes.data if sub is not None else None,
                             div.ctypes.data if div is not None else None)
    g = np.zeros((B, W), np.float32)
    loss, lh = np.zeros(1, np.float32), np.zeros((B, K), np.float32)
    p, t = np.ascontiguousarray(p), np.ascontiguousarray(t)
    rc = pkg.lib().pl_skeleton_terms_host(p.ctypes.data, t.ctypes.data, B, G, ctypes.byref(sk), grad_scale,
                                          g.ctypes.data if want_grad else None, loss.ctypes.data, lh.ctypes.data)
    assert rc == 0, pkg.lib().pl_last_error()
    del keep
    return float(loss[0]), (g if want_grad else None), lh


LAMBDAS = [(0.7, 0.0), (0.0, 0.3), (0.7, 0.3)]


@pytest.mark.parametrize("xf", [False, True])
@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("rho", ["l1", "mse"])
def test_oracle_is_torch_autograd_in_fp64(rho, G, xf):
    for name in ("h36m", "chain"):
        tabs = _skel(name)
        p, t = _poses(name, 9, G)
        p[0], p[1, :G] = t[0], p[1, G:2 * G]                       # a pose that equals its target; a zero-length bone (joints 0, 1)
        sub, div = _transform(p.shape[1] // G, G) if xf else (None, None)
        for lam in LAMBDAS:
            o = orc.terms(p, t, G, *tabs, *lam, rho, sub, div)
            val, grad = orc.torch_terms(p, t, G, *tabs, *lam, rho, sub, div)
            assert abs(o["value"] - val) <= 1e-12 * max(1.0, abs(val))
            np.testing.assert_allclose(o["grad"], grad, rtol=1e-10, atol=1e-14)
            assert (o["absgrad"] + 1e-300 >= np.abs(o["grad"]) * (1 - 1e-12)).all()
    lh = orc.bone_lengths(p, G, tabs[0], tabs[1], sub, div)
    assert lh.shape == (9, 4) and np.allclose(lh, o["lh"])


def test_skeleton_validation(pkg):
    S = pkg.Skeleton
    ok = S((-1, 0, 1, 0, 3), left=(2,), right=(4,))
    assert ok.bones == (1, 2, 3, 4) and ok.bone_parents == (0, 1, 0, 3) and ok.pairs == ((1, 3),) and ok.root == 0 and ok.joints == 5
    assert S((1, -1, 1)).bones == (0, 2)                                            # the root need not be joint 0
    for bad, what in (((0, 0, 1), "root"), ((-1, -1, 0), "root"), ((-1, 5, 0), "outside"), ((-1, 2, 1), "cycle"),
                      ((-1, 1, 0), "cycle"), ((-1,), "joints"), ((-1,) + (0,) * 32, "joints")):
        with pytest.raises(ValueError, match=what):
            S(bad)
    for left, right, what in (((1,), (2, 3), "left joints"), ((1, 1), (2, 3), "twice"), ((1,), (1,), "twice"), ((0,), (2,), "root"),
                              ((9,), (2,), "outside")):
        with pytest.raises(ValueError, match=what):
            S((-1, 0, 1, 0, 3), left=left, right=right)
    P = pkg.PoseCriterion
    with pytest.raises(ValueError, match="need a skeleton"):
        P("mse", bone_weight=0.1)
    with pytest.raises(ValueError, match="need a skeleton"):
        P("mse", symmetry_weight=0.1)
    with pytest.raises(ValueError, match="without left / right pairs"):
        P("mse", skeleton=S((-1, 0, 1)), symmetry_weight=0.1)
    with pytest.raises(ValueError, match="2 or 3 coordinates"):
        P("mse", coords=1, skeleton=pkg.H36M_SKELETON)
    with pytest.raises(ValueError, match="bone_rho"):
        P("mse", skeleton=pkg.H36M_SKELETON, bone_rho="huber")
    with pytest.raises(ValueError, match="denorm has shape"):
        P("mse", skeleton=pkg.H36M_SKELETON, denorm=pkg.PoseTransform(np.zeros((16, 3)), np.ones((16, 3))))
    c = P("mpjpe", skeleton=pkg.H36M_SKELETON, bone_weight=0.5, symmetry_weight=0.25, bone_rho="mse",
          denorm=pkg.PoseTransform(np.zeros((17, 3)), np.ones((17, 3))))
    assert c.term_weights.tolist() == [0.5, 0.25] and c.bone_child.dtype == torch.int32 and c.denorm_div.shape == (51,)
    assert {"term_weights", "bone_child", "bone_parent", "pair_a", "pair_b", "denorm_sub", "denorm_div"} <= set(dict(c.named_buffers()))
    assert "skeleton" in repr(c)
    with pytest.raises(ValueError, match="skeleton of 17 joints"):
        c(torch.zeros(2, 48), torch.zeros(2, 48))
    with pytest.raises(pkg.PoseliftError, match="no CPU path"):
        c(torch.zeros(2, 51), torch.zeros(2, 51))
    with pytest.raises(pkg.PoseliftError, match="no CPU path"):
        pkg.bone_lengths(torch.zeros(2, 17, 3), pkg.H36M_SKELETON)


def test_h36m_skeleton_is_the_selection_and_the_flip_tables(pkg):
    sk = pkg.H36M_SKELETON
    assert sk.joints == len(pkg.H36M_17_OF_32) == 17 and sk.root == 0
    assert list(sk.left) == LEFT and list(sk.right) == RIGHT
    assert sk.parents == orc.H36M_PARENTS
    assert len(sk.bones) == 16 and sk.bones == tuple(range(1, 17))       # one bone per selected joint but the root (hip)
    # a mirrored pair's bones hang on mirrored (or shared) parents
    mirror = {**dict(zip(sk.left, sk.right)), **dict(zip(sk.right, sk.left))}
    for a, b in zip(sk.left, sk.right):
        assert mirror.get(sk.parents[a], sk.parents[a]) == sk.parents[b]
    child, parent, pairs = _skel("h36m")
    assert tuple(child) == sk.bones and tuple(parent) == sk.bone_parents and [tuple(p) for p in pairs] == list(sk.pairs)
    # on the real skeletons of g13: plausible limbs, and the paired ones alike
    with np.load(GOLDEN, allow_pickle=False) as z:
        lh = orc.bone_lengths(z["tgt"].reshape(128, -1), 3, child, parent).mean(0)
    assert 0.07 < lh.min() and lh.max() < 0.29
    assert max(abs(lh[a] - lh[b]) for a, b in sk.pairs) < 0.01


def test_ctypes_mirror_follows_the_header(pkg):
    header = open(os.path.join(ROOT, "include", "poselift.h")).read()
    L, lib = pkg._lib, pkg.lib()
    body = re.search(r"typedef struct PLSkeleton \{(.*?)\} PLSkeleton;", header, re.S).group(1)
    names = [n for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in L.PLSkeleton._fields_]
    assert lib.pl_skeleton_abi_bytes(0) == ctypes.sizeof(L.PLCriterion) == 24
    assert lib.pl_skeleton_abi_bytes(1) == ctypes.sizeof(L.PLSkeleton) == 72
    assert lib.pl_skeleton_abi_bytes(2) == ctypes.sizeof(L.PLSkeletonCriterion) == 32 and lib.pl_skeleton_abi_bytes(3) == 0
    assert L.PLSkeletonCriterion.skeleton.offset == 24 and L.PLSkeletonCriterion.kind.offset == 0
    assert (L.PLSkeleton.rho.offset, L.PLSkeleton.bone_child.offset, L.PLSkeleton.term_weights.offset, L.PLSkeleton.div.offset) == (12, 16, 48, 64)
    assert int(re.search(r"#define PL_CRIT_HAS_SKELETON (0x[0-9a-fA-F]+)", header).group(1), 16) == L.CRIT_HAS_SKELETON
    assert issubclass(L.PLSkeletonCriterion, L.PLCriterion)              # byref() of one passes as a PLCriterion*
    assert lib.pl_version() >= 121
    for name in ("pl_bone_lengths", "pl_skeleton_terms_host", "pl_skeleton_abi_bytes"):
        assert name in L.SIGNATURES and re.search(r"\b%s\s*\(" % name, header)


def test_entry_points_reject_a_bad_skeleton_before_touching_a_device(pkg):
    L, lib = pkg._lib, pkg.lib()
    one = ctypes.c_void_p(16)

    def call(O=51, group=3, kind=0, **kw):
        f = dict(joints=17, bones=16, pairs=6, rho=0, bone_child=16, bone_parent=16, pair_a=16, pair_b=16, term_weights=16,
                 sub=None, div=None)
        f.update(kw)
        sk = L.PLSkeleton(**f)
        st = L.PLSkeletonCriterion(kind | L.CRIT_HAS_SKELETON, group, 1.0, None)
        st.skeleton = ctypes.pointer(sk)
        return lib.pl_pose_loss_fwd_bwd(one, one, 4, O, ctypes.byref(st), 1.0, None, one, one, None)

    assert call(joints=16) == ESHAPE and b"skeleton" in lib.pl_last_error()
    assert call(O=34, group=2, joints=16) == ESHAPE
    assert call(O=52, group=4, joints=13) == ESHAPE and b"2 or 3" in lib.pl_last_error()
    assert call(O=17, group=1) == ESHAPE
    for bones in (0, -1, 32):
        assert call(bones=bones) == ESHAPE and b"bones" in lib.pl_last_error()
    for pairs in (-1, 17):
        assert call(pairs=pairs) == ESHAPE and b"pairs" in lib.pl_last_error()
    assert call(joints=33, O=99) == ESHAPE
    for null in ("bone_child", "bone_parent", "pair_a", "pair_b", "term_weights"):
        assert call(**{null: None}) == EINVAL, null
    assert call(pairs=0, pair_a=None, pair_b=None, joints=16) == ESHAPE          # (no pairs: no pair table needed; the shape is next)
    assert call(rho=2) == EINVAL and b"rho" in lib.pl_last_error()
    assert call(sub=16) == EINVAL and call(div=16) == EINVAL and b"sub and div" in lib.pl_last_error()
    assert call(kind=7) == EINVAL and b"kind" in lib.pl_last_error()
    # the flag without a skeleton, and no flag at all: as before
    st = L.PLSkeletonCriterion(L.CRIT_MPJPE | L.CRIT_HAS_SKELETON, 3, 1.0, None)
    assert lib.pl_pose_loss_fwd_bwd(one, one, 0, 51, ctypes.byref(st), 1.0, None, one, one, None) == ESHAPE and b"B=0" in lib.pl_last_error()
    # scratch: the base pass's partials and 64 more
    sk = L.PLSkeleton(17, 16, 6, 0, 16, 16, 16, 16, 16, None, None)
    st.skeleton = ctypes.pointer(sk)
    for B in (1, 64, 4096, 100000):
        assert lib.pl_pose_loss_scratch_bytes(B, 51, ctypes.byref(st)) == lib.pl_mse_scratch_bytes(B * 51) + 256
    assert lib.pl_bone_lengths(one, 4, 3, None, one, None) == EINVAL
    assert lib.pl_bone_lengths(one, 4, 4, ctypes.byref(sk), one, None) == ESHAPE
    assert lib.pl_bone_lengths(one, 0, 3, ctypes.byref(sk), one, None) == ESHAPE
    assert lib.pl_bone_lengths(None, 4, 3, ctypes.byref(sk), one, None) == EINVAL


CASES = [("g13", "h36m", 128, 3), ("g13", "h36m", 128, 2), ("h36m", "h36m", 130, 3), ("h36m", "h36m", 65, 2), ("chain", "chain", 63, 3),
         ("chain", "chain", 1, 2)]


@pytest.mark.parametrize("scale", [1.0, 1e3])
@pytest.mark.parametrize("xf", [False, True])
@pytest.mark.parametrize("rho", ["l1", "mse"])
def test_host_arithmetic_vs_fp64_oracle(pkg, rho, xf, scale):
    """The text the kernel runs, on the CPU: value within 1e-5 relative, every gradient element within the propagated roundings
    of the documented expression (orc.terms: err_units x 2^-24), bone lengths within (G / 2 + 2) x 2^-24 relative (no
    transform).  Gradient elements an undecidable l1 sign reaches (|e| < 16 x 2^-24 x length) are left out: under 1 % of bones."""
    worst = 0.0
    for data, skel, B, G in CASES:
        tabs = _skel(skel)
        p, t = _poses(data, B, G, scale)
        sub, div = None, None
        if xf:
            p, t, sub, div = _standardise(_poses(data, 128, G, scale, seed=5)[1], p, t, G)
            assert (div == 0).sum() >= G and (div > 0).any()
        for lam in LAMBDAS:
            o = orc.terms(p, t, G, *tabs, *lam, rho, sub, div)
            val, g, lh = _host(pkg, p, t, G, tabs, lam, rho, sub, div)
            assert abs(val - o["value"]) <= 1e-5 * abs(o["value"]), (data, B, G, lam, val, o["value"])
            assert _host(pkg, p, t, G, tabs, lam, rho, sub, div, want_grad=False)[0] == val
            skip, frac = orc.undecided(o, rho)
            assert frac <= 0.01, (data, B, G, frac)
            err = np.abs(g.astype(np.float64) - o["grad"])
            bound = 1.001 * U * o["err_units"] + 1e-45
            ok = ~skip
            assert (err[ok] <= bound[ok]).all(), (data, B, G, lam, (err[ok] / bound[ok]).max())
            worst = max(worst, (err[ok] / bound[ok]).max())
            assert (g[o["absgrad"] == 0] == 0).all()
            if not xf:
                assert (np.abs(lh - o["lh"]) <= 1.001 * (G / 2 + 2) * U * o["lh"]).all()
    print(f"{rho} transform={xf} scale={scale}: gradient error at most {worst:.3f} of its bound")


@pytest.mark.parametrize("rho", ["l1", "mse"])
def test_host_special_poses(pkg, rho):
    tabs = _skel("h36m")
    child, parent, pairs = tabs
    p, t = _poses("g13", 16, 3)
    lam = (0.7, 0.3)
    # prediction = target: the bone term and its gradient vanish exactly (l1: rho'(0) = 0)
    val, g, _ = _host(pkg, t, t, 3, tabs, (0.7, 0.0), rho)
    assert val == 0.0 and (g == 0).all()
    # a collapsed prediction: every lh is 0, so is the whole gradient; the value is lambda mean rho(l)
    c = np.tile(p[:, :3], (1, 17))
    val, g, lh = _host(pkg, c, t, 3, tabs, lam, rho)
    o = orc.terms(c, t, 3, *tabs, *lam, rho)
    l = orc.bone_lengths(t, 3, child, parent)
    assert (g == 0).all() and (lh == 0).all() and o["L_sym"] == 0
    assert abs(val - 0.7 * (np.abs(l) if rho == "l1" else l * l).mean()) <= 1e-5 * val
    # a mirrored prediction (flip_pose: x -> -x, left and right swapped): the symmetry term is unchanged
    f = p.reshape(16, 17, 3).copy()
    f[:, :, 0] *= -1
    f[:, LEFT + RIGHT] = f[:, RIGHT + LEFT]
    a = _host(pkg, p, t, 3, tabs, (0.0, 0.3), rho)[0]
    b = _host(pkg, f.reshape(16, 51), t, 3, tabs, (0.0, 0.3), rho)[0]
    assert a > 0 and abs(a - b) <= 4 * U * a
    # lambda = 0: exactly nothing, and grad_scale multiplies everything
    val, g, _ = _host(pkg, p, t, 3, tabs, (0.0, 0.0), rho)
    assert val == 0.0 and (g == 0).all()
    g1, g2 = _host(pkg, p, t, 3, tabs, lam, rho)[1], _host(pkg, p, t, 3, tabs, lam, rho, grad_scale=4.0)[1]
    assert np.array_equal(g2, 4.0 * g1)                                  # (a power of two: exact)
    # a dead column gets gradient 0
    sub, div = _transform(17, 3)
    g = _host(pkg, p, t, 3, tabs, lam, rho, sub, div)[1]
    assert (g[:, div == 0] == 0).all() and (g[:, div != 0] != 0).any()


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("rho", ["l1", "mse"])
def test_host_nonfinite_set_is_torch_cpus(pkg, rho, bad):
    """One poisoned element of the prediction: the non-finite values sit where torch's (fp32, CPU) do; other poses are clean."""
    tabs = _skel("h36m")
    p, t = _poses("g13", 6, 3)
    p[2, 3 * 5 + 1] = bad                                                # joint 5: bones (5, 4) and (6, 5); bone (5, 4) is paired
    for lam in LAMBDAS:
        want_v, want_g = orc.torch_terms(p, t, 3, *tabs, *lam, rho, dtype=np.float32)
        val, g, _ = _host(pkg, p, t, 3, tabs, lam, rho)
        assert np.isnan(val) == np.isnan(want_v) and np.isinf(val) == np.isinf(want_v), (lam, val, want_v)
        assert np.array_equal(np.isnan(g), np.isnan(want_g)) and np.array_equal(np.isinf(g), np.isinf(want_g)), lam
        fin = np.isfinite(want_g)
        np.testing.assert_allclose(g[fin], want_g[fin], rtol=1e-4, atol=1e-9)
        assert np.isfinite(g[[0, 1, 3, 4, 5]]).all()
