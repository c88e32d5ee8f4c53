"""GPU tests of the cameras: the five kernels against their _host forms, bit for bit (the same inline text, contraction off,
correctly rounded division and square root, the host replaying the device's summation order; a NaN for a NaN), on every
case list of test_camera_host.py; inputs and outputs off 16-byte alignment and outputs / scratch that held NaN or 0xFF bytes; the autograd
functions against the float64 oracle; the loss beside a PoseCriterion under a model; SequenceLifter.locate on the recorded
track against the hand composition of the public pieces; the loss captured in a graph."""
import numpy as np
import pytest
import torch

import camera_oracle as orc
import test_gpu_scratch_independence as tsi
from conftest import load_golden
from test_camera_host import (DIVS, F, KIND, Scene, cases, host_errors, host_fit, host_loss, host_project, host_project_bwd,
                              recorded_track)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return None if t is None else t.detach().cpu().numpy()


def same_bits(a, b):
    """Bit for bit, a NaN standing where the other has a NaN: the sign and payload of a NaN that arithmetic produced (the
    negated entries of the Jacobian of a pose without a camera, say) are the processor's choice, not the library's."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a.view(np.uint32)[ok], b.view(np.uint32)[ok])


def same_bits_t(x, y):
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def off16(a, fill=None):
    """A device copy of `a` that starts 4 bytes past a 16-byte boundary (fill: what the buffer holds instead of a's values)."""
    a = np.ascontiguousarray(a)
    itemsize = a.dtype.itemsize
    pad = 4 // itemsize
    buf = torch.empty(a.size + 16 // itemsize, dtype=torch.from_numpy(a).dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[pad:pad + a.size].view(a.shape)
    if fill is None:
        v.copy_(torch.from_numpy(a))
    else:
        v.view(-1).view(torch.uint8).fill_(fill) if isinstance(fill, int) else v.fill_(fill)
    assert v.data_ptr() % 16 == 4
    return v


def device_scene(pkg, c):
    """(cams, keyword arguments) of a test_camera_host.Scene for the Python functions"""
    dn = None if c.sub is None else pkg.PoseTransform(c.sub, c.div)
    return pkg.CameraTable.from_table(c.cams), dict(cam_ids=_t(c.ids), translation=_t(c.t), denorm=dn)


# ---- device == host on every case list ------------------------------------------------------------------------------------------
def test_project_errors_and_backward_equal_host(pkg):
    for c in cases("scene"):
        cams, kw = device_scene(pkg, c)
        s = c.scene()
        X = _t(c.X).requires_grad_(True)
        if kw["translation"] is not None:
            kw["translation"].requires_grad_(True)
        uv = pkg.project_poses(X, cams, **kw)
        assert same_bits(_n(uv), host_project(pkg, c.X, c.cams, **s)), c.tag
        uv.backward(_t(c.duv))
        dX, dT = host_project_bwd(pkg, c.X, c.duv, c.cams, **s)
        assert same_bits(_n(X.grad), dX), c.tag
        if c.t is not None:
            assert same_bits(_n(kw["translation"].grad), dT), c.tag
        kw = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in kw.items()}
        for wh in DIVS:
            err = pkg.reprojection_errors(X.detach(), _t(c.target), cams, div=wh, **kw)
            assert same_bits(_n(err), host_errors(pkg, c.X, c.target, c.cams, wh=wh, **s)), (c.tag, wh)


def test_loss_equals_host(pkg):
    for n, c in enumerate(cases("scene")):
        cams, kw = device_scene(pkg, c)
        for k, kind in enumerate(orc.KINDS):
            wh = DIVS[(n + k) % 2]
            X = _t(c.X).requires_grad_(True)
            t = None if c.t is None else _t(c.t).requires_grad_(True)
            loss = pkg.reprojection_loss(X, _t(c.target), cams, kw["cam_ids"], translation=t, weights=_t(c.w), kind=kind,
                                         denorm=kw["denorm"], div=wh)
            loss.backward()
            want = host_loss(pkg, c.X, c.target, c.cams, w=c.w, kind=kind, wh=wh, **c.scene())
            tag = (c.tag, kind, wh)
            assert same_bits(_n(loss), want[0]), tag                  # (the host replays the device's summation order)
            assert same_bits(_n(X.grad), want[1]), tag
            if t is not None:
                assert same_bits(_n(t.grad), want[2]), tag
            if c.w is not None and c.bad is None:
                assert not X.grad[_t(c.w) == 0].any(), tag            # a zero-weight joint: exactly zero for finite inputs


def test_fit_equals_host(pkg):
    for n, c in enumerate(cases("fit")):
        cams, kw = device_scene(pkg, c)
        X, exact, noisy = c.rel()
        for iters, tgt in (((3, 0, 1, 8)[n % 4], noisy), (3, exact.astype(F))):
            t, rms = pkg.fit_translation(_t(X), _t(tgt), cams, kw["cam_ids"], weights=_t(c.w), denorm=kw["denorm"], iters=iters)
            want = host_fit(pkg, X, tgt, c.cams, c.ids, c.w, c.sub, c.div, iters)
            assert same_bits(_n(t), want[0]) and same_bits(_n(rms), want[1]), (c.tag, iters)


def test_degenerate_and_non_finite_poses_equal_host(pkg):
    c = Scene(65, 17, ids="mixed", weights="random", seed=9)
    cams, kw = device_scene(pkg, c)
    X, _, noisy = c.rel()
    Xn, w = X.copy(), np.ones((65, 17), F)
    Xn[40, 6, 1] = np.nan
    w[2], w[5] = 0.0, 0.0
    w[5, 3] = 0.7
    Xn[7], noisy[7] = Xn[7, 4], noisy[7, 4]
    t, rms = pkg.fit_translation(_t(Xn), _t(noisy), cams, kw["cam_ids"], weights=_t(w))
    want = host_fit(pkg, Xn, noisy, c.cams, c.ids, w)
    assert same_bits(_n(t), want[0]) and same_bits(_n(rms), want[1])
    assert sorted(np.flatnonzero(np.isnan(_n(rms))).tolist()) == [2, 5, 7, 40]
    s = c.scene()
    uv = pkg.project_poses(_t(Xn), cams, **kw)
    assert same_bits(_n(uv), host_project(pkg, Xn, c.cams, **s)) and int(torch.isnan(uv).any(-1).sum()) == 1
    wz = c.w.copy()
    wz[40, 6] = 0.0                                                      # a zero weight does not hide the NaN
    loss = pkg.reprojection_loss(_t(Xn), _t(c.target), cams, weights=_t(wz), **kw)
    assert torch.isnan(loss)


# ---- alignment and what outputs and scratch held --------------------------------------------------------------------------------
def test_offset_pointers_and_dirty_outputs_give_the_same_bits(pkg):
    L = pkg.lib()
    c = Scene(257, 17, ids="mixed", denorm=True, weights="random", seed=11)
    B, J, s = c.B, c.J, c.scene()
    Xr, _, noisy = c.rel()
    want_uv = host_project(pkg, c.X, c.cams, **s)
    want_bwd = host_project_bwd(pkg, c.X, c.duv, c.cams, **s)
    want_err = host_errors(pkg, c.X, c.target, c.cams, wh=DIVS[1], **s)
    want_loss = host_loss(pkg, c.X, c.target, c.cams, w=c.w, kind="l2", wh=DIVS[1], **s)
    want_fit = host_fit(pkg, Xr, noisy, c.cams, c.ids, c.w, c.sub, c.div, 3)
    stream = torch.cuda.current_stream().cuda_stream
    X, tgt, duv, cams, ids, t, sub, div, w, nz = (off16(a) for a in (c.X, c.target, c.duv, c.cams, c.ids, c.t, c.sub, c.div, c.w, noisy))
    scene = (cams.data_ptr(), 4, ids.data_ptr())
    nscratch = L.pl_camera_reproj_loss_scratch_bytes(B, J)
    for fill in (float("nan"), 0xFF):
        uv = off16(want_uv, fill)
        assert L.pl_camera_project(X.data_ptr(), B, J, *scene, t.data_ptr(), sub.data_ptr(), div.data_ptr(), uv.data_ptr(), stream) == 0
        assert same_bits(_n(uv), want_uv)
        dX, dT = off16(want_bwd[0], fill), off16(want_bwd[1], fill)
        assert L.pl_camera_project_bwd(X.data_ptr(), duv.data_ptr(), B, J, *scene, t.data_ptr(), sub.data_ptr(), div.data_ptr(),
                                       dX.data_ptr(), dT.data_ptr(), stream) == 0
        assert same_bits(_n(dX), want_bwd[0]) and same_bits(_n(dT), want_bwd[1])
        err = off16(want_err, fill)
        assert L.pl_camera_reproj_errors(X.data_ptr(), tgt.data_ptr(), B, J, *scene, t.data_ptr(), sub.data_ptr(), div.data_ptr(),
                                         DIVS[1][0], DIVS[1][1], err.data_ptr(), stream) == 0
        assert same_bits(_n(err), want_err)
        dX, dT, loss = off16(want_loss[1], fill), off16(want_loss[2], fill), off16(np.zeros(1, F), fill)
        scratch = torch.empty(nscratch, dtype=torch.uint8, device=DEV)                       # fp64 partials: 8-byte aligned
        scratch.fill_(0xFF) if isinstance(fill, int) else scratch.view(torch.float64).fill_(fill)
        assert L.pl_camera_reproj_loss_fwd_bwd(X.data_ptr(), tgt.data_ptr(), B, J, *scene, t.data_ptr(), sub.data_ptr(),
                                               div.data_ptr(), w.data_ptr(), KIND["l2"], DIVS[1][0], DIVS[1][1], 1.0, dX.data_ptr(),
                                               dT.data_ptr(), loss.data_ptr(), scratch.data_ptr(), stream) == 0
        assert same_bits(_n(loss)[0], want_loss[0]) and same_bits(_n(dX), want_loss[1]) and same_bits(_n(dT), want_loss[2])
        ft, frms = off16(want_fit[0], fill), off16(want_fit[1], fill)
        assert L.pl_camera_fit_translation(X.data_ptr(), nz.data_ptr(), B, J, *scene, w.data_ptr(), sub.data_ptr(), div.data_ptr(), 3,
                                           ft.data_ptr(), frms.data_ptr(), stream) == 0
        assert same_bits(_n(ft), want_fit[0]) and same_bits(_n(frms), want_fit[1])
    assert L.pl_camera_reproj_loss_fwd_bwd(X.data_ptr(), tgt.data_ptr(), B, J, *scene, t.data_ptr(), sub.data_ptr(), div.data_ptr(),
                                           None, 0, 1.0, 1.0, 1.0, None, None, loss.data_ptr(), scratch.data_ptr() + 4, stream) == -1


def _scratch_case(pkg):
    """The camera launches as a case of tests/test_gpu_scratch_independence.py: run(empty) -> the record of what they return."""
    c = Scene(130, 17, ids="mixed", denorm=True, weights="random", seed=12)
    cams, kw = device_scene(pkg, c)
    X, tgt, w, duv = _t(c.X), _t(c.target), _t(c.w), _t(c.duv)
    Xr, _, noisy = c.rel()
    noisy = _t(noisy)

    def run(empty):
        Xg, tg = X.clone().requires_grad_(True), kw["translation"].clone().requires_grad_(True)
        k = dict(kw, translation=tg)
        uv = pkg.project_poses(Xg, cams, **k)
        gx, gt = torch.autograd.grad(uv, (Xg, tg), duv)
        loss = pkg.reprojection_loss(Xg, tgt, cams, k["cam_ids"], translation=tg, weights=w, kind="l2", denorm=k["denorm"])
        lx, lt = torch.autograd.grad(loss, (Xg, tg))
        t, rms = pkg.fit_translation(X, noisy, cams, k["cam_ids"], weights=w, denorm=k["denorm"])
        return {"uv": uv.detach(), "dX": gx, "dT": gt, "err": pkg.reprojection_errors(X, tgt, cams, **kw), "loss": loss.detach(),
                "loss dX": lx, "loss dT": lt, "t": t, "rms": rms}
    return run


# tests/test_gpu_scratch_independence.py::test_every_kernel_has_a_case wants a case there for every __global__ function of
# csrc/: the kernels of camera.hip get theirs here (the registry is that module's, filled when this one is imported)
tsi.REG["cameras"] = _scratch_case


def test_results_do_not_depend_on_what_the_outputs_held(pkg, monkeypatch):
    ran, _ = tsi._independent(pkg, monkeypatch, "cameras", tsi.REG["cameras"](pkg))
    assert {"camera_project_kernel", "camera_reproj_errors_kernel", "camera_bwd_tile_kernel", "camera_loss_final_kernel",
            "camera_fit_kernel"} <= ran, sorted(ran)


# ---- autograd -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("denorm", [False, True])
def test_autograd_gives_the_oracle_gradients(pkg, denorm):
    c = Scene(257, 17, ids="mixed", denorm=denorm, weights="random", seed=13)
    cams, kw = device_scene(pkg, c)
    X, t = _t(c.X).requires_grad_(True), _t(c.t).requires_grad_(True)
    pkg.project_poses(X, cams, kw["cam_ids"], translation=t, denorm=kw["denorm"]).backward(_t(c.duv))
    args = (c.X, c.duv, c.cams, c.ids, c.t, c.sub, c.div)
    lo, hi = orc.project_bwd(*args, dtype=F32), orc.project_bwd(*args)
    for got, l, h in ((X.grad, lo[0], hi[0]), (t.grad, lo[1], hi[1])):
        assert np.abs(_n(got).astype(np.float64) - h).max() <= orc.bound(l, h, h)
    for kind in orc.KINDS:
        X.grad = t.grad = None
        pkg.reprojection_loss(X, _t(c.target), cams, kw["cam_ids"], translation=t, weights=_t(c.w), kind=kind,
                              denorm=kw["denorm"]).backward()
        args = (c.X, c.target, c.cams, c.ids, c.t, c.sub, c.div, c.w, kind)
        lo, hi = orc.loss(*args, dtype=F32), orc.loss(*args)
        for got, l, h in ((X.grad, lo[1], hi[1]), (t.grad, lo[2], hi[2])):
            assert np.abs(_n(got).astype(np.float64) - h).max() <= orc.bound(l, h, h), kind
        assert not X.grad[_t(c.w) == 0].any()                            # a zero-weight joint: exactly zero
    Xd = _t(c.X)                                                         # no gradient asked for: the value alone, the same bits
    a = pkg.reprojection_loss(Xd, _t(c.target), cams, kw["cam_ids"], translation=_t(c.t), weights=_t(c.w), kind="l2",
                              denorm=kw["denorm"])
    assert not a.requires_grad and same_bits(_n(a), host_loss(pkg, c.X, c.target, c.cams, w=c.w, kind="l2", **c.scene())[0])


def test_loss_composes_with_a_criterion_under_a_model(pkg):
    """One autograd step of a lifter at B = 65 with loss = crit(y, y3d) + 0.1 reprojection_loss(y as poses): the gradient
    reaching y is the criterion's own plus 0.1 times the _host reprojection gradient, within one fp32 ulp of the larger."""
    B = 65
    torch.manual_seed(5)
    model = pkg.LinearModel(34, 51, linear_size=64).to(DEV).train()
    c = Scene(B, 17, ids="mixed", denorm=True, seed=14)
    cams, kw = device_scene(pkg, c)
    x, _ = pkg.synth.synthetic_batch(B, 77, DEV)
    y3d = _t(c.X.reshape(B, 51))
    root = _t(c.t).requires_grad_(True)
    crit = pkg.PoseCriterion("mpjpe", coords=3).to(DEV)
    y = model(x.reshape(B, 34))
    y.retain_grad()
    rep = pkg.reprojection_loss(y.view(-1, 17, 3), _t(c.target), cams, kw["cam_ids"], translation=root, denorm=kw["denorm"])
    (crit(y, y3d) + 0.1 * rep).backward()
    yd = y.detach().clone().requires_grad_(True)
    crit(yd, y3d).backward()
    gc = _n(yd.grad).reshape(B, 17, 3)
    _, gr, gt = host_loss(pkg, _n(y).reshape(B, 17, 3), c.target, c.cams, **c.scene())
    part = F(0.1) * gr
    ulp = np.spacing(np.maximum(np.abs(gc), np.abs(part)).astype(F))
    got = _n(y.grad).reshape(B, 17, 3)
    assert np.all(np.abs(got.astype(np.float64) - (gc.astype(np.float64) + part.astype(np.float64))) <= ulp)
    assert np.abs(part).max() > 0 and np.abs(gc).max() > 0
    assert same_bits(_n(root.grad), F(0.1) * gt)
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)


# ---- SequenceLifter.locate --------------------------------------------------------------------------------------------------------
DIV = (1000.0, 1002.0)


def test_locate_is_the_composition_of_the_public_pieces(pkg):
    g15, g17 = load_golden("g15_video_tracks.npz"), load_golden("g17_cameras.npz")
    det = _t(g15["det"])
    cams = pkg.CameraTable.from_table(g17["cameras"])
    ids = _t(np.full(256, 2, np.int32))
    torch.manual_seed(3)
    model = pkg.LinearModel(34, 51, linear_size=64, compute_dtype="fp32").to(DEV).eval()
    rs = np.random.RandomState(1)
    s3, d3 = rs.uniform(-0.3, 0.3, (17, 3)).astype(F), rs.uniform(0.05, 0.6, (17, 3)).astype(F)
    s3[0], d3[0] = 0.0, 0.0
    t2, dn = pkg.PoseTransform.normalize_2d(), pkg.PoseTransform(s3, d3)
    f2, f3, ft = pkg.TemporalFilter.gaussian(1.0), pkg.TemporalFilter.box(5), pkg.TemporalFilter.gaussian(2.0)
    lifter = pkg.SequenceLifter(model, layout="h36m17", div=DIV, transform_2d=t2, denorm=dn, filter_2d=f2, filter_3d=f3)
    # lift(): the bits it returned before locate() existed -- the hand composition of tests/test_gpu_track.py
    poses, w, state = lifter.lift(det)
    xy, w0, s0 = pkg.prepare_tracks(det, "h36m17", DIV, 0.1, 8, 0.5)
    with torch.no_grad():
        y = model(t2.apply(pkg.filter_tracks(xy, f2, w0))).reshape(-1, 17, 3)
    hand = pkg.filter_tracks(dn.invert(y), f3, w0)
    assert same_bits_t(poses, hand) and same_bits_t(w, w0) and torch.equal(state, s0)
    px = xy * torch.tensor(DIV, device=DEV)
    for filt in (None, ft):
        p2, t, rms, w2, st2 = lifter.locate(det, cams, cam_ids=ids, iters=3, filter_t=filt)
        assert same_bits_t(p2, poses) and same_bits_t(w2, w) and torch.equal(st2, state)
        ht, hrms = pkg.fit_translation(poses, px, cams, cam_ids=ids, weights=w, iters=3)
        if filt is not None:
            ht = pkg.filter_tracks(ht.reshape(-1, 1, 3), filt, torch.isfinite(hrms).float().reshape(-1, 1)).reshape(-1, 3)
        assert same_bits_t(t, ht) and same_bits_t(rms, hrms)
        assert tuple(t.shape) == (256, 3) and tuple(rms.shape) == (256,)
    # two copies as two sequences: each half the bits of the track alone
    two, seq = torch.cat([det, det]), _t(np.repeat(np.array([7, 3], np.int32), 256))
    t2s = lifter.locate(two, cams, cam_ids=torch.cat([ids, ids]), seq_ids=seq, filter_t=ft)[1]
    assert same_bits_t(t2s[:256], t) and same_bits_t(t2s[256:], t)


def test_recorded_track_on_the_device(pkg):
    X, gt, cam = recorded_track()
    cams = pkg.CameraTable.from_table(cam)
    t0, _ = pkg.fit_translation(_t(X), _t(gt), cams, iters=0)
    t3, rms = pkg.fit_translation(_t(X), _t(gt), cams, iters=3)
    e0 = float(pkg.reprojection_errors(_t(X), _t(gt), cams, translation=t0).double().mean())
    e3 = float(pkg.reprojection_errors(_t(X), _t(gt), cams, translation=t3).double().mean())
    assert torch.isfinite(t3).all() and torch.isfinite(rms).all() and e3 <= e0
    assert 4.0 < float(t3[:, 2].min()) and float(t3[:, 2].max()) < 7.0


# ---- graph capture ------------------------------------------------------------------------------------------------------------------
def test_loss_forward_and_backward_in_a_captured_graph(pkg):
    a, b = Scene(257, 17, ids="mixed", weights="random", seed=15), Scene(257, 17, ids="mixed", weights="random", seed=16)
    cams, kw = device_scene(pkg, a)                                      # (both scenes: the same cameras)
    cams.to(DEV)

    def eager(c):
        X, t = _t(c.X).requires_grad_(True), _t(c.t).requires_grad_(True)
        loss = pkg.reprojection_loss(X, _t(c.target), cams, _t(c.ids), translation=t, weights=_t(c.w), kind="l2", denorm=kw["denorm"])
        gx, gt = torch.autograd.grad(loss, (X, t))
        return loss.detach().clone(), gx.clone(), gt.clone()
    want = {id(c): eager(c) for c in (a, b)}
    sX, st, suv, sids, sw = (_t(v) for v in (a.X, a.t, a.target, a.ids, a.w))
    sX.requires_grad_(True)
    st.requires_grad_(True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = pkg.reprojection_loss(sX, suv, cams, sids, translation=st, weights=sw, kind="l2", denorm=kw["denorm"])
        gx, gt = torch.autograd.grad(loss, (sX, st))
    for c in (b, a, b):
        with torch.no_grad():
            for dst, src in ((sX, c.X), (st, c.t), (suv, c.target), (sids, c.ids), (sw, c.w)):
                dst.copy_(_t(src))
        graph.replay()
        torch.cuda.synchronize()
        for got, ref in zip((loss, gx, gt), want[id(c)]):
            assert same_bits_t(got.detach(), ref), c.tag
