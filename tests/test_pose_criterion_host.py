"""Host-side tests of the train step's criterion (no GPU): the fp64 oracle of tests/pose_criterion_oracle.py against
torch's own modules (values and autograd gradients, weights, a zero weight, an exactly-zero joint, |d| == beta, one NaN),
argument validation of pl.PoseCriterion and of the C entry points, and the ctypes mirror of PLCriterion."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pose_criterion_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESHAPE = -1, -2


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()


torch_criterion = orc.torch_criterion


def inputs(B, J, coords, seed):
    """random poses with an exactly-zero joint, a single zero coordinate and -- coordinates 0 and 1 of sample 0, joint 1 --
    |d| == beta = 0.5 exactly, once from each side"""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((B, J * coords)).astype(np.float32)
    t = rng.standard_normal((B, J * coords)).astype(np.float32)
    t[0, :coords] = p[0, :coords]                                  # joint 0 of sample 0: d = 0 on every coordinate
    if J > 1:
        p[0, coords], t[0, coords] = 1.5, 1.0                      # d = +beta
        if coords > 1:
            p[0, coords + 1], t[0, coords + 1] = 1.0, 1.5          # d = -beta
    t[B - 1, -1] = p[B - 1, -1]                                    # one zero coordinate inside a non-zero joint
    return p, t


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B,J,coords", [(1, 1, 3), (4, 17, 3), (3, 17, 2), (5, 7, 1)])
@pytest.mark.parametrize("kind", orc.KINDS)
def test_oracle_is_torchs_module(kind, B, J, coords, weighted):
    p, t = inputs(B, J, coords, 100 * B + J)
    w = None
    if weighted:
        w = np.random.default_rng(J).uniform(0.25, 2.0, J)
        w[0] = 0.0                                                 # the dead root joint taken out
    want_l, want_g = torch_criterion(kind, p, t, coords, w, 0.5)
    got_l, got_g = orc.criterion(kind, p, t, coords, w, beta=0.5)
    assert abs(got_l - want_l) <= 1e-13 * max(1.0, abs(want_l))
    np.testing.assert_allclose(got_g, want_g, rtol=1e-13, atol=0)
    if kind in ("l1", "mpjpe"):
        assert (got_g[0, :coords] == 0).all()                      # exact zeros where the table says 0
    # grad_scale scales the gradient and nothing else
    l2, g2 = orc.criterion(kind, p, t, coords, w, beta=0.5, grad_scale=0.25)
    assert l2 == got_l and np.allclose(g2, 0.25 * got_g, rtol=1e-15, atol=0)
    # the documented fp32 expression is that gradient to fp32 round-off
    g32 = orc.grad_fp32(kind, p, t, coords, w, beta=0.5)
    np.testing.assert_allclose(g32, got_g, rtol=2e-6, atol=0)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("kind", orc.KINDS)
def test_oracle_nonfinite_set_is_torchs(kind, bad):
    """One poisoned element: the set of non-finite loss and gradient values is torch's (L1's gradient at a NaN is 0,
    smooth-L1's is NaN, MPJPE's whole joint is NaN), with and without (positive) weights."""
    for w in (None, np.linspace(0.5, 1.5, 17)):
        p, t = inputs(4, 17, 3, 9)
        p[2, 7] = bad
        want_l, want_g = torch_criterion(kind, p, t, 3, w, 0.5)
        got_l, got_g = orc.criterion(kind, p, t, 3, w, beta=0.5)
        assert np.isnan(got_l) == np.isnan(want_l) and np.isinf(got_l) == np.isinf(want_l)
        assert np.array_equal(np.isnan(got_g), np.isnan(want_g)) and np.array_equal(np.isinf(got_g), np.isinf(want_g))
        fin = np.isfinite(want_g)
        np.testing.assert_allclose(got_g[fin], want_g[fin], rtol=1e-13, atol=0)
        g32 = orc.grad_fp32(kind, p, t, 3, w, beta=0.5)
        assert np.array_equal(np.isnan(g32), np.isnan(want_g))
    if np.isnan(bad):
        nan_g = np.isnan(want_g)
        assert nan_g.sum() == {"mse": 1, "l1": 0, "smooth_l1": 1, "mpjpe": 3}[kind]


def test_pose_criterion_validates_its_arguments(pkg):
    PC = pkg.PoseCriterion
    with pytest.raises(ValueError, match="kind"):
        PC("huber")
    for beta in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="beta"):
            PC("smooth_l1", beta=beta)
    PC("l1", beta=0.0)                                             # beta is smooth_l1's alone
    for coords in (0, -3, 2.5):
        with pytest.raises(ValueError, match="coords"):
            PC("l1", coords=coords)
    with pytest.raises(ValueError, match="mpjpe"):
        PC("mpjpe", coords=5)
    with pytest.raises(ValueError, match="joint_weights"):
        PC("l1", joint_weights=np.ones((17, 3)))
    c = PC("mpjpe", joint_weights=np.ones(17))
    assert "joint_weights" in dict(c.named_buffers()) and c.joint_weights.dtype == torch.float32
    assert PC("mse").joint_weights is None and "joint_weights" not in PC("mse").state_dict()
    with pytest.raises(ValueError, match="whole joints"):
        c.check_outputs(50)
    with pytest.raises(ValueError, match="joint weights"):
        c.check_outputs(48)
    c.check_outputs(51)
    with pytest.raises(ValueError, match="shapes differ"):
        c(torch.zeros(2, 51), torch.zeros(2, 48))
    with pytest.raises(ValueError, match="coords"):
        c(torch.zeros(2, 17, 2), torch.zeros(2, 17, 2))
    with pytest.raises(pkg.PoseliftError, match="no CPU path"):    # the library is the product: nothing runs on the host
        c(torch.zeros(2, 51), torch.zeros(2, 51))
    assert "PoseCriterion" in repr(c) and "mpjpe" in repr(c)


def test_entry_points_reject_a_bad_criterion_before_touching_a_device(pkg):
    L, PLC = pkg.lib(), pkg._lib.PLCriterion
    one = ctypes.c_void_p(16)

    def call(crit, B=4, O=51):
        return L.pl_pose_loss_fwd_bwd(one, one, B, O, ctypes.byref(crit) if crit is not None else None, 1.0, None, one, one, None)

    assert call(PLC(7, 3, 1.0, None)) == EINVAL and b"kind" in L.pl_last_error()
    assert call(PLC(-1, 3, 1.0, None)) == EINVAL
    for beta in (0.0, -2.0, float("inf"), float("nan")):
        assert call(PLC(pkg._lib.CRIT_SMOOTH_L1, 3, beta, None)) == EINVAL and b"beta" in L.pl_last_error()
    assert call(PLC(pkg._lib.CRIT_L1, 2, 1.0, None)) == ESHAPE and b"whole joints" in L.pl_last_error()      # 51 % 2
    assert call(PLC(pkg._lib.CRIT_L1, 0, 1.0, None)) == ESHAPE
    assert call(PLC(pkg._lib.CRIT_MPJPE, 17, 1.0, None)) == ESHAPE and b"mpjpe" in L.pl_last_error()
    assert call(PLC(pkg._lib.CRIT_MSE, 3, 1.0, None), B=0) == ESHAPE
    assert call(None, O=0) == ESHAPE
    assert L.pl_pose_loss_fwd_bwd(None, one, 4, 51, None, 1.0, None, one, one, None) == EINVAL      # null pred
    # scratch: what the MSE pass of as many elements needs, whatever the kind (the grouped kind has fewer work items)
    for B, O in ((1, 3), (64, 51), (4096, 51), (100000, 51)):
        want = L.pl_mse_scratch_bytes(B * O)
        assert L.pl_pose_loss_scratch_bytes(B, O, None) == want
        assert L.pl_pose_loss_scratch_bytes(B, O, ctypes.byref(PLC(pkg._lib.CRIT_MPJPE, 3, 1.0, None))) == want


def test_ctypes_mirror_of_plcriterion_follows_the_header(pkg):
    header = open(os.path.join(ROOT, "include", "poselift.h")).read()
    body = re.search(r"typedef struct PLCriterion \{(.*?)\} PLCriterion;", header, re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    PLC = pkg._lib.PLCriterion
    assert fields == [f[0] for f in PLC._fields_] == ["kind", "group", "beta", "weights"]
    assert ctypes.sizeof(PLC) == 24 and (PLC.kind.offset, PLC.group.offset, PLC.beta.offset, PLC.weights.offset) == (0, 4, 8, 16)
    kinds = dict(re.findall(r"(PL_CRIT_\w+) = (\d+)", header))
    assert {k: int(v) for k, v in kinds.items()} == {"PL_CRIT_MSE": pkg._lib.CRIT_MSE, "PL_CRIT_L1": pkg._lib.CRIT_L1,
                                                     "PL_CRIT_SMOOTH_L1": pkg._lib.CRIT_SMOOTH_L1,
                                                     "PL_CRIT_MPJPE": pkg._lib.CRIT_MPJPE}
    assert pkg.criterion.KINDS == {"mse": 0, "l1": 1, "smooth_l1": 2, "mpjpe": 3}
    for name in ("pl_pose_loss_scratch_bytes", "pl_pose_loss_fwd_bwd", "pl_lifter_train_fwd_bwd_crit", "pl_lifter_train_step_crit"):
        assert name in pkg._lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, header)
