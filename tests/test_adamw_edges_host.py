"""What the gate of tests/adamw_oracle.py means, without a GPU.

A numpy-fp32 emulation of the kernel's order (adamw_oracle.emulate32: constants in double rounded once, every element
operation rounded, no fused multiply-add -- FMA contraction only removes roundings) stays inside the bounds on every case of
the grid, with and without a clip coefficient, and the worst ratio per quantity is printed in units of the bounds at K = 1 and at
K = 16.  Each fault the hyper-parameter edges are there for leaves a bound on a case named here."""
import importlib

import numpy as np
import pytest

import adamw_oracle as ao

COEFS = (1.0, 0.37)

# fault -> a case of the grid (with the clip coefficient 0.37) on which it has to leave a bound
NAMED = {
    "pow32": "mixed/hp3/gs3.7/t7",                 # 1 - b2^t = 7e-5: the fp32 pow's rounding is 1e-3 of it
    "eps_fixed": "tiny/hp2/gs3.7/t2",              # eps = 1e-3 is the whole denominator
    "beta_swap": "mixed/hp1/gs0.125/t2",
    "t_off_by_one": "huge/hp1/gs1/t1",             # bc2 at t = 1 against t = 2: sqrt(2) in the update
    "gscale_m_only": "huge/hp2/gs0.125/t1",
    "wd_after": "mixed/hp3/gs3.7/t1000",           # lr * wd = 0.03 of an update as large as p
    "eps_scaled": "tiny/hp1/gs3.7/t1",             # sqrt(v) below eps, 1 / sqrt(bc2) = 32
    "coef_dropped": "normal/hp0/gs3.7/t1",
}


def test_oracle_rounds_hyper_parameters_to_fp32_and_keeps_t_exact():
    p, g, m, v = ao.values("normal", 64, 7)
    hp = (1e-3, 0.9, 0.99999, 1e-8, 0.01, 3.7)
    a = ao.step64(p, g, m, v, hp, 7)
    b = ao.step64(p, g, m, v, ao.round_hp(hp), 7)
    assert all(np.array_equal(x, y) for x, y in zip(a, b) if isinstance(x, np.ndarray))
    b2 = ao.f32(0.99999)
    assert b2 != 0.99999
    # den at t = 1 from zero moments: sqrt((1 - b2) g^2) / sqrt(1 - b2) + eps = |g| + eps with the ROUNDED beta on both sides
    z = np.zeros_like(p)
    r = ao.step64(p, g, z, z, hp, 1)
    np.testing.assert_allclose(r.den, np.abs(g.astype(np.float64) * ao.f32(3.7)) + ao.f32(1e-8), rtol=1e-12)
    # the corrections equal 1 at t = 1e9
    r9 = ao.step64(p, g, m, v, hp, 10 ** 9)
    assert r9.step == ao.f32(1e-3)
    # lr = 0: p comes back exactly in the reference too; m and v move
    r0 = ao.step64(p, g, m, v, ao.HP_TUPLES[5] + (1.0,), 2)
    assert np.array_equal(r0.p, p.astype(np.float64)) and not np.array_equal(r0.m, m) and not np.array_equal(r0.v, v)


def test_case_grid_is_what_the_edges_need():
    cs = ao.cases()
    assert len(cs) == len(ao.CLASSES) * len(ao.HP_TUPLES) * len(ao.GSCALES) * len(ao.TS) and len({c.id for c in cs}) == len(cs)
    for cls in ao.CLASSES:
        p, g, m, v = ao.values(cls, ao.N_GRID, 7)
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in (p, g, m, v)) and (v >= 0).all()
        g2 = (g.astype(np.float64) * 3.7) ** 2
        assert g2.max() < float(np.finfo(np.float32).max)
        if cls == "tiny":
            assert (g2[g != 0] < 2.0 ** -126).all() and (v < 2.0 ** -126).all() and (v > 0).all()
        if cls == "huge":
            assert np.abs(g).min() >= 5e14 and v.min() >= 5e29
        if cls == "zero":
            assert not g.any() and not m.any() and not v.any()
        _, _, m1, v1 = ao.values(cls, ao.N_GRID, 1)
        assert not m1.any() and not v1.any()


def test_emulation_stays_inside_the_bounds_on_every_case():
    worst = {"p": (0.0, ""), "m": (0.0, ""), "v": (0.0, "")}
    for c in ao.cases():
        p, g, m, v = ao.values(c.cls, ao.N_GRID, c.t)
        for coef in COEFS:
            ref = ao.step64(p, g, m, v, c.hp, c.t, coef)
            pn, mn, vn = ao.emulate32(p, g, m, v, c.hp, c.t, coef)
            r = ao.ratios(pn, mn, vn, p, m, ref, k=1)
            for q, x in r.items():
                if x > worst[q][0]:
                    worst[q] = (x, f"{c.id}/coef{coef:g}")
            if c.hp[0] == 0.0:
                assert np.array_equal(pn, p), c.id          # lr = 0: bitwise
    for q, (x, where) in worst.items():
        print(f"    emulate32 {q}: worst {x:.3g} of the bound at K = 1, {x / ao.K:.3g} at K = {ao.K}   ({where})")
    assert all(x / ao.K <= 1.0 for x, _ in worst.values()), worst


@pytest.mark.parametrize("fault", ao.FAULTS)
def test_each_fault_leaves_a_bound_on_its_named_case(fault):
    by_id = {c.id: c for c in ao.cases()}
    c = by_id[NAMED[fault]]
    p, g, m, v = ao.values(c.cls, ao.N_GRID, c.t)
    ref = ao.step64(p, g, m, v, c.hp, c.t, 0.37)
    good = ao.ratios(*ao.emulate32(p, g, m, v, c.hp, c.t, 0.37), p, m, ref)
    bad = ao.ratios(*ao.emulate32(p, g, m, v, c.hp, c.t, 0.37, fault=fault), p, m, ref)
    print(f"    {fault} on {c.id}: p {bad['p']:.3g} m {bad['m']:.3g} v {bad['v']:.3g} of the bounds (fault-free: "
          f"p {good['p']:.3g} m {good['m']:.3g} v {good['v']:.3g})")
    assert max(good.values()) <= 1.0
    assert max(bad.values()) > 1.0
    # and over the whole grid it is not a one-case accident
    n_bad = 0
    for c2 in ao.cases():
        p, g, m, v = ao.values(c2.cls, 64, c2.t)
        ref = ao.step64(p, g, m, v, c2.hp, c2.t, 0.37)
        n_bad += max(ao.ratios(*ao.emulate32(p, g, m, v, c2.hp, c2.t, 0.37, fault=fault), p, m, ref).values()) > 1.0
    print(f"    {fault}: leaves a bound on {n_bad} of {len(ao.cases())} cases")
    assert n_bad >= 10


def test_captured_hyper_parameter_signature_sees_every_baked_value_and_not_lr():
    """What GraphedTrainStep / GraphedModuleStep record at capture and compare before a replay (the replay itself needs the
    GPU: tests/test_gpu_adamw_edges.py): betas, eps and weight_decay change the signature and are refused with the graph
    errors' "capture a new one"; lr, which the captured launches read from device memory, does not."""
    import __graft_entry__ as ge
    pkg = ge.build()
    train = importlib.import_module("3d_poseestimation_amd.train")
    opt = pkg.FlatAdamW(pkg.LinearModel(34, 51, linear_size=64), lr=1e-3, betas=(0.5, 0.9), eps=1e-3, weight_decay=0.3)
    g = opt.param_groups[0]
    sig = opt._hyper_signature()
    assert sig == (0.5, 0.9, 1e-3, 0.3, True)
    g["lr"] = 5e-2
    train._check_hyper("a step", opt, sig)
    for name, new, word in (("weight_decay", 0.05, "weight_decay"), ("betas", (0.5, 0.95), "beta2"), ("betas", [0.4, 0.9], "beta1"),
                            ("eps", 1e-6, "eps")):
        old, g[name] = g[name], new
        with pytest.raises(pkg.PoseliftError, match=f"{word} .*capture a new one"):
            train._check_hyper("a step", opt, sig)
        g[name] = old
        train._check_hyper("a step", opt, sig)
    g["betas"] = [0.5, 0.9]                                 # (a loaded state_dict may hold a list: the same values)
    train._check_hyper("a step", opt, sig)


def test_ema_reference_follows_the_kernel_definition():
    e, p = np.float32([1.0, -2.0, 0.0]), np.float32([1.5, -2.0, 1e-3])
    assert ao.ema_omd(0.999, False, 1) == ao.f32(1.0 - ao.f32(0.999))
    assert ao.ema_omd(0.999, True, 1) == ao.f32(1.0 - 2.0 / 11.0) and ao.ema_omd(0.5, True, 100) == 0.5
    ref, bound = ao.ema64(e, p, 0.9, False, 3)
    F = np.float32
    got = (p - e) * F(ao.ema_omd(0.9, False, 3)) + e
    assert (np.abs(got.astype(np.float64) - ref) <= bound).all()
