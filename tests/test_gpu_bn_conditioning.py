"""Training-mode BatchNorm statistics on ill-conditioned columns, every route that computes them.

The columns are oracle/bn_cases.py's: a control, |mean| / sigma ~ 1e3, constants (var = 0, rstd = 1 / sqrt(eps)), a one-row
outlier alone in the last statistics group, a mean that moves from one 64-row group to the next.  The reference is always
fp64 numpy on the GPU's OWN z, so nothing is amplified through the layers, and every bound is K u_c with K = 64 and
u_c = 2^-24 (|mu_c| + s_c) / s_c (bn_cases.bound: the fp32 resolution of zhat at that column).  tests/
test_bn_conditioning_host.py shows what that gate means: the kernels' scheme -- sums per 64 rows, M2 about the group mean, a
Chan merge with the true row count of the last group -- stays inside 16 u_c, while each of the faults the columns are
there for -- sum z^2 - (sum z)^2, a dropped or halved between-group term n d^2, a last group counted as full, a mean that
loses its low bits in a pre-folded shift -- leaves 64 u_c on the kind of column meant for it.

Where an assertion adds 2^-22 |ref| it is the fp32 rounding of the result itself (its own storage and one more operation)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import bn_cases
from oracle import lifter_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, U24 = bn_cases.K, bn_cases.EPS24
EPS, MOMENTUM = 1e-5, 0.1


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float64)


def _worst(name, err, allowed, check=True):
    """Print the worst err / allowed (the measured figure, in units of the bound) and assert it is <= 1 and finite (check
    False: return whether it is, for a caller that wants every figure printed before it asserts)."""
    err, allowed = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(allowed, np.float64))
    assert np.isfinite(err).all(), f"{name}: non-finite"
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(allowed > 0, err / allowed, np.where(err > 0, np.inf, 0.0))
    print(f"    {name}: worst {float(ratio.max()):.3g} of the bound")
    if not check:
        return bool((err <= allowed).all())
    assert (err <= allowed).all(), (name, float(ratio.max()), np.unravel_index(int(ratio.argmax()), ratio.shape))


def _check_stats(tag, z, mean, rstd):
    """|mean - mu| <= K u s and |rstd s - 1| <= K u against fp64 statistics of z; returns (mu, var, s, u)."""
    mu, var, s = bn_cases.stats64(z, EPS)
    u = bn_cases.bound(z, EPS)
    _worst(f"{tag} mean", np.abs(_n(mean) - mu), K * u * s)
    _worst(f"{tag} rstd", np.abs(_n(rstd) * s - 1), K * u)
    return mu, var, s, u


def _check_running(tag, rm, rv, rm0, rv0, mu, var, s, u, n):
    """running_mean / running_var after one momentum-0.1 update with the unbiased variance.  The same relative bounds: the
    batch mean within K u s; s^2 = var + eps within the factor (1 -+ K u)^-2 that |rstd s - 1| <= K u allows."""
    ref_m = (1 - MOMENTUM) * rm0 + MOMENTUM * mu
    ref_v = (1 - MOMENTUM) * rv0 + MOMENTUM * var * n / (n - 1)
    _worst(f"{tag} running_mean", np.abs(_n(rm) - ref_m), MOMENTUM * K * u * s + 2.0 ** -22 * np.abs(ref_m))
    dv = ((1 - K * u) ** -2 - 1) * s * s * n / (n - 1)
    _worst(f"{tag} running_var", np.abs(_n(rv) - ref_v), MOMENTUM * dv + 2.0 ** -22 * np.abs(ref_v))


def _check_act(tag, got, z, mu, s, u, gamma, beta, relu=True, resid=None):
    """|y - ref| <= K u |gamma| + 2^-22 |ref|, ref = [relu](gamma zhat + beta) [+ resid] in fp64.  (ReLU is 1-Lipschitz: no
    allowance for flips.)"""
    ref = gamma * ((np.asarray(z, np.float64) - mu) / s) + beta
    if relu:
        ref = np.maximum(ref, 0)
    if resid is not None:
        ref = ref + resid
    _worst(f"{tag} y", np.abs(_n(got) - ref), K * u * np.abs(gamma) + 2.0 ** -22 * np.abs(ref))
    return ref


# ---------------------------------------------------------------------------- a, b: the conv path's BatchNorm entry
def _bn_params(C, seed):
    rng = np.random.default_rng(seed)
    return {"gamma": (0.5 + rng.random(C)).astype(np.float32), "beta": (0.2 * rng.standard_normal(C)).astype(np.float32),
            "rm0": (0.1 * rng.standard_normal(C)).astype(np.float32), "rv0": (0.5 + rng.random(C)).astype(np.float32)}


def _bn_fwd_raw(pkg, z, p, relu, gemm_stat=None):
    """pl_bn_train_fwd_ex on z [rows][C] (numpy fp32) -> (y, mean, rstd, running_mean, running_var) device tensors."""
    L = pkg.lib()
    rows, C = z.shape
    zd, ga, be, rm, rv = _t(z), _t(p["gamma"]), _t(p["beta"]), _t(p["rm0"]), _t(p["rv0"])
    nb = torch.zeros((), dtype=torch.int64, device=DEV)
    y = torch.full((rows, C), float("nan"), device=DEV)
    bits = torch.empty(rows, 4 * ((C + 255) // 256), dtype=torch.int64, device=DEV)
    mean, rstd = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    scratch = torch.empty(L.pl_bn_train_scratch_bytes(rows, C), dtype=torch.uint8, device=DEV)
    gs = _t(gemm_stat) if gemm_stat is not None else None
    rc = L.pl_bn_train_fwd_ex(zd.data_ptr(), rows, C, ga.data_ptr(), be.data_ptr(), EPS, MOMENTUM, rm.data_ptr(), rv.data_ptr(),
                              nb.data_ptr(), int(relu), y.data_ptr(), bits.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                              scratch.data_ptr(), None, 0, gs.data_ptr() if gs is not None else None, None,
                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.pl_last_error()
    torch.cuda.synchronize()
    assert int(nb) == 1
    return y, mean, rstd, rm, rv


def _check_bn_entry(tag, z, p, relu, out):
    y, mean, rstd, rm, rv = out
    rows = z.shape[0]
    g64, b64 = p["gamma"].astype(np.float64), p["beta"].astype(np.float64)
    mu, var, s, u = _check_stats(tag, z, mean, rstd)
    ref = _check_act(tag, y, z, mu, s, u, g64, b64, relu)
    _check_running(tag, rm, rv, p["rm0"].astype(np.float64), p["rv0"].astype(np.float64), mu, var, s, u, rows)
    const = var == 0                # the dead units: y = [relu](beta) within the bound
    assert const.sum() >= z.shape[1] // 5
    want = np.maximum(b64, 0) if relu else b64
    assert (ref[:, const] == want[const]).all()
    _worst(f"{tag} constant columns", np.abs(_n(y)[:, const] - want[const]), (K * u * np.abs(g64) + 2.0 ** -22 * np.abs(want))[const])


BN_SHAPES = [
    (105, 64),       # no replication (105 rows do not split in four), ragged last group of 41 rows
    (1000, 64),      # 4 replicas: the [250][256] view, ragged last group of 58 rows
    (4160, 256),     # 65 partials per column: the finalize's streaming branch (> 64 partials)
    (16449, 64),     # > 16384 rows: 256-row groups merged pairwise inside bn_colstats (the last: 64 rows + ONE), 65 partials
]


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("rows,C", BN_SHAPES)
def test_conv_batchnorm_from_z(pkg, rows, C, relu):
    """a. pl_bn_train_fwd_ex straight from z: bn_colstats (replica layout, in-kernel pairwise merge), bn_finalize (register
    and streaming branch), the shift fold of bn_apply."""
    z = bn_cases.columns(rows, C, seed=rows + C)
    p = _bn_params(C, rows)
    _check_bn_entry(f"[{rows}x{C}]", z, p, relu, _bn_fwd_raw(pkg, z, p, relu))


def _host_gemm_stat(pkg, z):
    """What a GEMM epilogue leaves for z: [2][pl_gemm_stat_groups(rows)][C] -- per 64-row group the column sums, then the
    sums of squares about the group mean (rows past the end: empty groups of zeros) -- in fp64, cast to fp32."""
    rows, C = z.shape
    G = pkg.lib().pl_gemm_stat_groups(rows)
    assert G * 64 >= rows
    st = np.zeros((2, G, C), np.float64)
    z64 = z.astype(np.float64)
    for g in range((rows + 63) // 64):
        blk = z64[64 * g:64 * (g + 1)]
        st[0, g] = blk.sum(0)
        st[1, g] = ((blk - blk.mean(0)) ** 2).sum(0)
    return st.astype(np.float32)


@pytest.mark.parametrize("rows,C,groups", [
    (1000, 64, 16),       # 16 partials, ragged last group
    (33025, 64, 518),     # 517 groups with rows (+ 1 empty) > 512: merged two at a time first; ONE row in the last group
])
def test_conv_batchnorm_from_gemm_stat(pkg, rows, C, groups):
    """b. The same entry fed the partial statistics of a GEMM epilogue instead of a pass over z (the merge of more than 512
    groups F at a time, bn_finalize on 64 F-row groups)."""
    assert pkg.lib().pl_gemm_stat_groups(rows) == groups
    z = bn_cases.columns(rows, C, seed=rows + C + 1)
    p = _bn_params(C, rows + 1)
    _check_bn_entry(f"[{rows}x{C} gemm_stat]", z, p, True, _bn_fwd_raw(pkg, z, p, True, _host_gemm_stat(pkg, z)))


# ---------------------------------------------------------------------------- c: the GEMM epilogue's own partials
def test_gemm_epilogue_partials(pkg):
    """c. pl_gemm_planes_raw (NT, fp16 planes) with `stat`: C = A B^T reproduces the column kinds -- column 0 of A is 1 and row c
    of B holds the kind's mean there, the other slots carry the noise, the last-row outlier and the group shift -- and per
    64-row group (the last has 8 rows) and column, against fp64 on the returned C:
        |sum - S| <= K 2^-24 sum |C|,    |M2 - ref| <= K u ref + K 2^-24 n s^2 u     (the group's own mu, s, u),
    the second term being all a constant column (ref = 0) is allowed.  That floor asks for an M2 that does not carry the
    rounding of the group mean: 64 equal values v sum with a rounding unless v is dyadic, the fp32 mean then misses v by
    d ~ ulp(v) and the plain sum of squares about it is 64 d^2.  Measured on an MI355X with the plain form: up to 192 x the
    floor on the constant columns and 173 x on the 7.3 columns of the full groups (an fp32 emulation of the epilogue's order
    gives the same 173), every other figure below 0.06 of its bound.  The planes GEMM's epilogue therefore uses the
    corrected two-pass form M2 = sum d^2 - (sum d)^2 / n (gemm_planes.hip staged_epilogue): measured after it, M2 = 0 on
    every constant column of the full groups, as the emulation of that form gives.  The floor is this entry's alone: it is
    the one that hands partials to a caller.  The fp32 routes' epilogues (gemm_epilogue.h, gemm_thin.hip, skinny.hip,
    small_layer.hip) keep the plain sum, whose 64 d^2 is of second order (d^2 / s^2 ~ u^2) in the mean, rstd and zhat
    that test d. holds them to."""
    from importlib import import_module
    cv = import_module("3d_poseestimation_amd.conv")
    L = pkg.lib()
    M, N, Kd = 200, 40, 32
    rng = np.random.default_rng(7)
    A = np.zeros((M, Kd), np.float32)
    A[:, 0] = 1.0
    A[M - 1, 1] = 1.0                                  # the one-row outlier
    A[:, 2] = np.arange(M) // 64                       # the group shift
    A[:, 3:] = rng.standard_normal((M, Kd - 3))
    Bw = np.zeros((N, Kd), np.float32)                 # weights: planes scaled by 16, 200 * 16 < 65504
    for c in range(N):
        kind, n = c % 5, c // 5
        noise = rng.standard_normal(Kd - 3) / np.sqrt(Kd - 3)
        if kind == 0:
            Bw[c, 0], Bw[c, 3:] = 0.5, 2.0 * noise
        elif kind == 1:
            Bw[c, 0], Bw[c, 3:] = (1 - 2 * (n % 2)) * 100.0 * (1.0 + rng.random()), 0.1 * noise
        elif kind == 2:
            Bw[c, 0] = bn_cases.CONSTANTS[n % 4]
        elif kind == 3:
            Bw[c, 0], Bw[c, 1] = 7.3, 1e-2
        else:
            Bw[c, 2], Bw[c, 3:] = 10.0, 0.05 * noise
    ap, bp = cv._planes_of(_t(A), 1.0, 3), cv._planes_of(_t(Bw), 16.0, 3)
    G = L.pl_gemm_stat_groups(M)
    assert G == 4
    stat = torch.full((2, G, N), float("nan"), device=DEV)
    Cd = cv._gemm_planes_raw(0, ap, (M, Kd), bp, (N, Kd), M, N, Kd, 1.0 / 16.0, None, 3, stat)
    torch.cuda.synchronize()
    C64, st = _n(Cd), _n(stat)
    # the product is what it was built to be: the kinds' means, constants that ARE constant
    mu_all = C64.mean(0)
    assert (np.abs(mu_all[1::5]) > 99).all() and (C64[:, 2::5] == C64[0, 2::5]).all() and (C64[:-1, 3::5] == C64[0, 3::5]).all()
    ok = []
    for g in range(G):
        blk = C64[64 * g:64 * (g + 1)]
        n = len(blk)
        mu, var, s = bn_cases.stats64(blk, EPS)
        u = bn_cases.bound(blk, EPS)
        ref = var * n
        ok.append(_worst(f"group {g} sum", np.abs(st[0, g] - blk.sum(0)), K * U24 * np.abs(blk).sum(0), check=False))
        for kind in range(5):
            sel = np.arange(N) % 5 == kind
            ok.append(_worst(f"group {g} M2, {bn_cases.KINDS[kind]} columns", np.abs(st[1, g] - ref)[sel],
                             (K * u * ref + K * U24 * n * s * s * u)[sel], check=False))
    assert all(ok), ok


# ---------------------------------------------------------------------------- d: the lifter, one case per statistics route
def _lifter(pkg, B, H, S, i_dim, o_dim, dtype, seed=0):
    """A lifter whose hidden Linears feed their BatchNorm the column kinds 0 - 2 (c % 3): as initialised; a bias of
    +-100 (1 + U); a zeroed weight row under a constant bias (a dead unit).  p_dropout = 0, gamma in [0.5, 1.5), beta = 0.2 N,
    fresh running statistics."""
    torch.manual_seed(B + H + seed)
    m = pkg.LinearModel(i_dim, o_dim, linear_size=H, num_stage=S, p_dropout=0.0, BN=True, compute_dtype=dtype)
    rng = np.random.default_rng(B * 3 + H + seed)
    st = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
    cols = np.arange(H)
    for lin, bn in orc.hidden_layer_names(S):
        b, W = st[lin + ".bias"], st[lin + ".weight"]
        k1, k2 = cols % 3 == 1, cols % 3 == 2
        b[k1] = ((1 - 2 * ((cols // 3) % 2)) * 100.0 * (1.0 + rng.random(H)))[k1]
        W[k2] = 0.0
        b[k2] = np.asarray(bn_cases.CONSTANTS, np.float32)[(cols // 3) % 4][k2]
        st[bn + ".weight"] = (0.5 + rng.random(H)).astype(np.float32)
        st[bn + ".bias"] = (0.2 * rng.standard_normal(H)).astype(np.float32)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in st.items()})
    m = m.to(DEV).train()
    x = _t(rng.random((B, i_dim)).astype(np.float32))
    return m, st, x


LIFTER_CASES = [
    # (B, H, stages, in, out, dtype, bitmap format per hidden layer, the fused step carries AdamW)
    # Stats::InLayer: Linear, statistics, finalize and apply in one small_layer.hip launch (the tile-format bitmap says so)
    (64, 256, 1, 34, 51, "fp32", [1, 1, 1], True),
    (37, 256, 1, 34, 51, "fp32", [1, 1, 1], True),         # ... ragged rows
    (2, 256, 1, 34, 51, "fp32", [1, 1, 1], True),          # ... two rows
    (2, 128, 1, 34, 51, "fp32", [0, 0, 0], False),         # two rows, K = 128 is no contraction of the layer kernels: Stats::Small
    (64, 1024, 2, 34, 51, "f16x3", [1] * 5, True),         # InLayer contracting on fp16 planes
    (32, 256, 1, 300, 70, "fp32", [0, 1, 1], False),       # 300 inputs: layer 0 a GEMM + Stats::Small (bn_small_fwd), InLayer above
    (48, 36, 0, 20, 7, "fp32", [0], False),                # H = 36: Stats::Small throughout
    # 65 ... 512 rows, H a contraction of the layer kernels (K % 256 == 0): skinny first layer (2 groups), Lin::F32Mid above
    # (launch_small_linear_stats, exact fp32 contraction); Stats::InApply
    (100, 256, 1, 34, 51, "fp32", [0, 0, 0], False),
    # H = 128 is no such contraction: Lin::Gemm above the skinny first layer, M = 100 off the tile grid -> gemm_thin.hip's
    # epilogue (2 groups); Stats::InApply
    (100, 128, 1, 34, 51, "fp32", [0, 0, 0], False),
    (200, 36, 0, 20, 7, "fp32", [0], False),               # tile-GEMM epilogue (4 groups, the last of 8 rows) + Stats::InApply
    (640, 128, 1, 34, 51, "fp32", [0, 0, 0], False),       # skinny / Lin::Gemm, 10 groups: Stats::Finalize (register branch)
    (4161, 128, 1, 34, 51, "fp32", [0, 0, 0], False),      # 66 partials: the finalize's streaming branch; ONE row in the last group
    # planes path, <= 512 rows, H = 256: Lin::PlanesMid (launch_small_linear_stats contracting on fp16 planes) + InApply
    (256, 256, 1, 34, 51, "f16x3", [0, 0, 0], False),
    (256, 128, 1, 34, 51, "f16x3", [0, 0, 0], False),      # H = 128: Lin::Planes, the planes tile GEMM's epilogue (4 groups) + InApply
    (1024, 128, 1, 34, 51, "f16x3", [0, 0, 0], False),     # planes tile GEMM's epilogue (16 groups) + Stats::Finalize
    (1024, 128, 1, 34, 51, "bf16", [0, 0, 0], False),      # ... on one bf16 plane per operand
]


@pytest.mark.parametrize("B,H,S,i_dim,o_dim,dtype,formats,adamw", LIFTER_CASES)
def test_lifter_statistics_routes(pkg, B, H, S, i_dim, o_dim, dtype, formats, adamw):
    """d. One training forward; per hidden layer the saved z, mean, rstd (and the activation where it exists as fp32: even
    layers >= 2 add the GPU's own act[l - 2]) against fp64 statistics of that z, and the running-statistics update.  The
    route in each case's comment is read from plan() in api.hip; only the bitmap format and step_carries_adamw tell routes
    apart at run time."""
    m, st, x = _lifter(pkg, B, H, S, i_dim, o_dim, dtype)
    L = pkg.lib()
    nl = 1 + 2 * S
    # the planes path (api.hip planes_kind): 16-bit operands, whole 128-row tiles, H % 128 == 0, at least one stage
    planes = dtype in ("f16x3", "bf16") and B % 128 == 0 and H % 128 == 0 and S >= 1
    assert [L.pl_workspace_bitmap_format(ctypes.byref(m._desc), B, l) for l in range(nl)] == formats
    assert m.step_carries_adamw(B) == adamw
    with torch.no_grad():
        pred = m(x)
    torch.cuda.synchronize()
    assert torch.isfinite(pred).all()
    ws = m.last_workspace
    sd = {k: _n(v) for k, v in m.state_dict().items()}
    acts = {}
    for l, (lin, bn) in enumerate(orc.hidden_layer_names(S)):
        z = _n(m.workspace_view(ws, 0, l))
        kinds = np.arange(H) % 3
        assert (np.abs(z.mean(0))[kinds == 1] > 90).all() and (z[:, kinds == 2] == z[0, kinds == 2]).all()
        tag = f"[B={B} H={H} {dtype}] layer {l}"
        mu, var, s, u = _check_stats(tag, z, m.workspace_view(ws, 3, l)[:H], m.workspace_view(ws, 4, l)[:H])
        _check_running(tag, sd[bn + ".running_mean"], sd[bn + ".running_var"], 0.0, 1.0, mu, var, s, u, B)
        assert int(sd[bn + ".num_batches_tracked"]) == 1
        if planes and l % 2 == 1 and l < nl - 1:        # feeds GEMMs only: the planes path keeps it as 16-bit planes, no fp32 copy
            with pytest.raises(pkg.PoseliftError):
                m.workspace_view(ws, 1, l)
            continue
        act = m.workspace_view(ws, 1, l)
        acts[l] = _n(act)
        resid = acts[l - 2] if (l >= 2 and l % 2 == 0) else None
        _check_act(tag, act, z, mu, s, u, st[bn + ".weight"].astype(np.float64), st[bn + ".bias"].astype(np.float64), True, resid)
    assert len(acts) == nl - (S if planes else 0)


# ---------------------------------------------------------------------------- e: backward on the same data
@pytest.mark.parametrize("rows,C", BN_SHAPES[:3])
def test_conv_batchnorm_backward(pkg, rows, C):
    """e. batchnorm_relu_train(...).backward(dy) (pl_bn_train_bwd_ex) against fp64 autograd of the same function:
        |dz - ref| <= K u gamma rstd max|dy| (1 + max|zhat|) + 2^-22 |ref|,
        |dgamma - ref|, |dbeta - ref| <= K u sum|dy| max(1, max|zhat|).
    A ReLU decision within K u gamma of zero may fall either way in fp32: the reference takes the GPU's own decisions (y > 0),
    after checking that every one that differs from its own sits on such a pre-activation."""
    relu = rows != 1000
    z = bn_cases.columns(rows, C, seed=rows + C)
    p = _bn_params(C, rows)
    rng = np.random.default_rng(rows)
    dy = rng.standard_normal((rows, C)).astype(np.float32)
    bn = torch.nn.BatchNorm2d(C, eps=EPS, momentum=MOMENTUM)
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(p["gamma"])); bn.bias.copy_(torch.from_numpy(p["beta"]))
        bn.running_mean.copy_(torch.from_numpy(p["rm0"])); bn.running_var.copy_(torch.from_numpy(p["rv0"]))
    bn = bn.to(DEV).train()
    zd = _t(z).requires_grad_(True)
    y = pkg.conv.batchnorm_relu_train(zd.reshape(1, rows, 1, C), bn, relu)
    y.backward(_t(dy).reshape(1, rows, 1, C))
    torch.cuda.synchronize()
    # the autograd node is the entry point test a. calls: the same bits
    assert torch.equal(y.detach().reshape(rows, C), _bn_fwd_raw(pkg, z, p, relu)[0])
    g, b = torch.from_numpy(p["gamma"]).double().requires_grad_(True), torch.from_numpy(p["beta"]).double().requires_grad_(True)
    z64 = torch.from_numpy(z).double().requires_grad_(True)
    mu = z64.mean(0)
    var = ((z64 - mu) ** 2).mean(0)
    zhat = (z64 - mu) / torch.sqrt(var + EPS)
    pre = g * zhat + b
    u = bn_cases.bound(z, EPS)
    on = y.detach().reshape(rows, C).cpu() > 0 if relu else torch.ones(rows, C, dtype=torch.bool)
    if relu:
        differ = on != (pre.detach() > 0)
        assert bool((pre.detach().abs()[differ].numpy() <= (K * u * p["gamma"])[None, :].repeat(rows, 0)[differ.numpy()]).all())
    (pre * on).backward(torch.from_numpy(dy).double())
    s = np.sqrt(var.detach().numpy() + EPS)
    zmax = np.abs(zhat.detach().numpy()).max(0)
    ga = p["gamma"].astype(np.float64)
    ref = z64.grad.numpy()
    _worst(f"[{rows}x{C}] dz", np.abs(_n(zd.grad) - ref), K * u * ga / s * np.abs(dy).max() * (1 + zmax) + 2.0 ** -22 * np.abs(ref))
    lim = K * u * np.abs(dy).sum(0) * np.maximum(1, zmax)
    _worst(f"[{rows}x{C}] dgamma", np.abs(_n(bn.weight.grad) - g.grad.numpy()), lim)
    _worst(f"[{rows}x{C}] dbeta", np.abs(_n(bn.bias.grad) - b.grad.numpy()), lim)


@pytest.mark.parametrize("B,H,S,dtype", [(64, 256, 1, "fp32"), (256, 128, 1, "f16x3"), (256, 256, 1, "f16x3"),
                                         (1024, 128, 1, "f16x3")])
def test_lifter_step_gradients(pkg, B, H, S, dtype):
    """e. Every gradient of a whole training step on the lifters of d. (and dx) against the fp64 oracle run on the GPU's own
    ReLU decisions.  The yardstick is measured, not fixed: the fp32 numpy oracle on the same decisions against the fp64 one,
    per tensor, relative in the 2-norm; the HIP path must stay within 8 x that (another summation order) or 2e-4 (the suite's
    fp32-grade tolerance), whichever is larger.  Hidden Linear biases are skipped as elsewhere: their true gradient is zero.

    Measured on an MI355X, relative error against fp64 as HIP / fp32 oracle (the test prints every tensor's pair):
        B = 64, H = 256, fp32:     worst HIP 6.6e-4 (w2.weight; oracle 3.9e-4), worst ratio 2.4 (batch_norm2.bias 5.6e-4 / 2.3e-4)
        B = 256, H = 128, f16x3:   worst HIP 5.7e-4 (w2.weight; oracle 1.6e-3), every tensor below the fp32 oracle's error
        B = 256, H = 256, f16x3:   worst HIP 8.7e-4 (w2.weight; oracle 1.9e-3), every tensor below 0.61 of the oracle's
                                   (Lin::PlanesMid, the route H = 128 does not reach)
        B = 1024, H = 128, f16x3:  worst HIP 8.8e-4 (w2.weight; oracle 8.4e-3), every tensor below a fifth of the oracle's
    (the oracle's plain fp32 sums over the batch lose digits on the +-100 columns; the kernels' grouped sums do not).
    """
    m, st, x = _lifter(pkg, B, H, S, 34, 51, dtype, seed=1)
    rng = np.random.default_rng(B)
    t = _t((rng.random((B, 51)) - 0.5).astype(np.float32))
    x.requires_grad_(True)
    pred = m(x)
    pkg.mse_loss(pred, t).backward()
    torch.cuda.synchronize()
    nl = 1 + 2 * S
    ws = m.last_workspace                 # the HIP path's own positive decisions of that forward (the ReLU bitmaps)
    on = [pkg.layout.unpack_bitmap(m.workspace_view(ws, 2, l).cpu().numpy().view(np.uint64), H) for l in range(nl)]
    xn, tn = x.detach().cpu().numpy(), t.cpu().numpy()
    res = {}
    for dt in (np.float64, np.float32):
        p, cache = orc.forward({k: v.copy() for k, v in st.items()}, xn, num_stage=S, train=True, p_dropout=0.0, dtype=dt, on_masks=on)
        _, dpred = orc.mse_loss(p, tn, dtype=dt)
        res[dt] = orc.backward(st, cache, dpred)
    (g64, dx64), (g32, dx32) = res[np.float64], res[np.float32]
    got = {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters()}
    got["dx"], g64["dx"], g32["dx"] = x.grad.cpu().numpy(), dx64, dx32

    def rel(a, ref):
        return float(np.linalg.norm(a.astype(np.float64) - ref) / (np.linalg.norm(ref) + 1e-300))
    bad = []
    for k, ref in g64.items():
        if k.endswith(".bias") and "batch_norm" not in k and k != "w2.bias":
            continue
        e_hip, e_32 = rel(got[k], ref), rel(g32[k], ref)
        print(f"    [B={B} H={H} {dtype}] {k}: HIP {e_hip:.3g}, fp32 oracle {e_32:.3g}")
        assert np.isfinite(got[k]).all()
        if not e_hip <= max(8 * e_32, 2e-4):
            bad.append((k, e_hip, e_32))
    assert not bad, bad
