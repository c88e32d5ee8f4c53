"""GPU tests of the video tracks: the remap, prepare, filter and velocity kernels against their _host forms, bit for bit (the
same inline text, contraction off, correctly rounded division and square root), on every case list of test_track_host.py;
inputs and outputs off 16-byte alignment and outputs that held NaN or garbage; SequenceLifter on the recorded track
g15_video_tracks.npz against the hand composition of the public pieces."""
import numpy as np
import pytest
import torch

import test_gpu_scratch_independence as tsi
import track_oracle as orc
from conftest import load_golden
from test_track_host import (F, filter_cases, filter_taps, gap_track, host_filter, host_prepare, host_remap, host_velocity, make_det,
                             make_seq, make_w, make_x, prepare_cases, same_bits, velocity_cases)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUT = {orc.COCO17: "coco17", orc.H36M17: "h36m17"}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.build()
    assert torch.cuda.is_available()
    return p


@pytest.fixture(scope="module")
def g15():
    return load_golden("g15_video_tracks.npz")


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.cpu().numpy()


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


# ---- device == host on every case list ------------------------------------------------------------------------------------------
def test_remap_equals_host(pkg):
    rs = np.random.RandomState(1)
    for T in (1, 67, 4101):
        det = np.concatenate([rs.uniform(0, 1000, (T, 17, 2)), rs.uniform(0, 1, (T, 17, 1))], axis=-1).astype(F)
        det[T // 2, 5] = (np.nan, np.inf, np.nan)
        got = _n(pkg.coco_to_h36m(_t(det)))
        want = host_remap(pkg, det)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_prepare_equals_host(pkg):
    cases = prepare_cases() + [(gap_track(G)[0], orc.H36M17, (1.0, 1.0), 0.1, G, 0.5, None) for G in (0, 1, 8, 64)]
    big = make_det(4101, 5)
    big[2000:2003, :, 0] = np.nan
    cases.append((big, orc.COCO17, (1000.0, 1002.0), 0.1, 8, 0.5, make_seq(4101, "runs")))
    for det, layout, div, thr, G, fc, seq in cases:
        want = host_prepare(pkg, det, layout, div, thr, G, fc, seq)
        got = pkg.prepare_tracks(_t(det), LAYOUT[layout], div, thr, G, fc, _t(seq))
        tag = (det.shape[0], layout, G)
        assert np.array_equal(_n(got[2]), want[2]), tag
        assert same_bits(_n(got[0]), want[0]) and same_bits(_n(got[1]), want[1]), tag
    with pytest.raises(pkg.PoseliftError):
        pkg.prepare_tracks(_t(det), max_gap=65)
    with pytest.raises(ValueError):
        pkg.prepare_tracks(_t(det), seq_ids=_t(np.zeros(3, np.int32)))


def test_prepare_non_finite_values_equal_host(pkg):
    T, G = 130, 8
    det = make_det(T, 58)
    rs = np.random.RandomState(T)
    vals = np.array([np.nan, np.inf, -np.inf], F)
    hit = rs.rand(T, 17) < 0.3                                         # in invalid and in valid-confidence samples alike
    det[..., 0][hit] = vals[rs.randint(0, 3, int(hit.sum()))]
    det[..., 2][rs.rand(T, 17) < 0.05] = np.nan
    for layout in (orc.COCO17, orc.H36M17):
        seq = make_seq(T, "halves")
        want = host_prepare(pkg, det, layout, (1000.0, 1002.0), 0.1, G, 0.5, seq)
        got = pkg.prepare_tracks(_t(det), LAYOUT[layout], (1000.0, 1002.0), 0.1, G, 0.5, _t(seq))
        assert np.array_equal(_n(got[2]), want[2]) and same_bits(_n(got[0]), want[0]) and same_bits(_n(got[1]), want[1])
        assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()


def test_filter_equals_host(pkg):
    for x, taps, w, seq in filter_cases(pkg):
        want = host_filter(pkg, x, taps, w, seq)
        got = _n(pkg.filter_tracks(_t(x), pkg.TemporalFilter(taps), _t(w), _t(seq)))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (x.shape, len(taps), w is None, seq is None)


def test_filter_zero_weights_and_nans_equal_host(pkg):
    T, J, D, K = 129, 17, 3, 7
    x, w, taps = make_x(T, J, D, 2), make_w(T, J, 2, zeros=0.0), filter_taps(pkg, K, 1)
    seq = make_seq(T, "halves")
    w[40:50, 3], w[:, 5], w[70, 8], w[20, 1] = 0.0, 0.0, 0.0, np.nan
    x[44, 3, 1], x[10, 5, :], x[70, 8, 0] = np.nan, np.inf, np.nan
    filt = pkg.TemporalFilter(taps)
    got = _n(pkg.filter_tracks(_t(x), filt, _t(w), _t(seq)))
    assert np.array_equal(got.view(np.uint32), host_filter(pkg, x, taps, w, seq).view(np.uint32))
    assert same_bits(got[43:47, 3], x[43:47, 3]) and same_bits(got[:, 5], x[:, 5]) and np.isfinite(got[70, 8]).all()
    xm = make_x(T, J, D, 2)
    xm[64, 2, 1] = np.nan
    ym = _n(pkg.filter_tracks(_t(xm), filt, None, _t(seq)))
    want = np.zeros(xm.shape, bool)
    want[61:65, 2, 1] = True
    assert np.array_equal(np.isnan(ym), want)
    assert np.array_equal(ym.view(np.uint32), host_filter(pkg, xm, taps, None, seq).view(np.uint32))
    x1 = make_x(T, J, D, 9)
    x1[0, 0, 0] = -0.0
    assert same_bits(_n(pkg.filter_tracks(_t(x1), pkg.TemporalFilter([1.0]))), x1)        # one unit tap: the identity
    t = np.array([0.5, -0.25, 0.5], F)
    y = torch.empty(T, J, D, device=DEV)
    assert pkg.lib().pl_track_filter(_t(x).data_ptr(), T, J, D, None, None, t.ctypes.data, 3, y.data_ptr(), None) == -1
    assert pkg.lib().pl_track_filter(_t(x).data_ptr(), T, J, D, None, None, t.ctypes.data, 2, y.data_ptr(), None) == -1


def test_velocity_equals_host(pkg):
    for p, g, seq, order, sub, div in velocity_cases():
        want = host_velocity(pkg, p, g, seq, order, sub, div)
        dn = None if sub is None else pkg.PoseTransform(sub, div)
        err, cnt = pkg.velocity_errors(_t(p), _t(g), _t(seq), order, dn)
        assert np.array_equal(_n(cnt), want[1]), (p.shape, order)
        assert np.array_equal(_n(err).view(np.uint32), want[0].view(np.uint32)), (p.shape, order, sub is None)


# ---- alignment and what the outputs held ------------------------------------------------------------------------------------------
def test_offset_pointers_and_dirty_outputs_give_the_same_bits(pkg):
    L = pkg.lib()
    T, G = 130, 8
    det, seq = make_det(T, 3), make_seq(T, "runs")
    want = host_prepare(pkg, det, orc.COCO17, (1000.0, 1002.0), 0.1, G, 0.5, seq)
    x, w, taps = make_x(T, 17, 3, 4), make_w(T, 17, 4), filter_taps(pkg, 7, 1)
    want_f = host_filter(pkg, x, taps, w, seq)
    p, g = make_x(T, 17, 3, 5), make_x(T, 17, 3, 6)
    want_v = host_velocity(pkg, p, g, seq, 2)
    stream = torch.cuda.current_stream().cuda_stream
    det_o, seq_o, x_o, w_o, p_o, g_o = (off16(a) for a in (det, seq, x, w, p, g))             # kept alive across the launches
    for fill in (float("nan"), 0xA5):
        xy, ww, st = off16(want[0], fill), off16(want[1], fill), off16(want[2], 0xA5)
        assert L.pl_track_prepare(det_o.data_ptr(), T, 0, 1000.0, 1002.0, 0.1, G, 0.5, seq_o.data_ptr(), xy.data_ptr(),
                                  ww.data_ptr(), st.data_ptr(), stream) == 0
        assert same_bits(_n(xy), want[0]) and same_bits(_n(ww), want[1]) and np.array_equal(_n(st), want[2])
        y = off16(want_f, fill)
        assert L.pl_track_filter(x_o.data_ptr(), T, 17, 3, w_o.data_ptr(), seq_o.data_ptr(), taps.ctypes.data, 7,
                                 y.data_ptr(), stream) == 0
        assert np.array_equal(_n(y).view(np.uint32), want_f.view(np.uint32))
        e, c = off16(want_v[0], fill), off16(want_v[1], 0xA5)
        assert L.pl_track_velocity_errors(p_o.data_ptr(), g_o.data_ptr(), T, 17, seq_o.data_ptr(), 2, None, None,
                                          e.data_ptr(), c.data_ptr(), stream) == 0
        assert np.array_equal(_n(e).view(np.uint32), want_v[0].view(np.uint32)) and np.array_equal(_n(c), want_v[1])
        r = off16(det, fill)
        assert L.pl_track_remap(det_o.data_ptr(), T, 0, r.data_ptr(), stream) == 0
        assert same_bits(_n(r), host_remap(pkg, det))


def _scratch_case(pkg):
    """The four track launches (both filter instantiations, weights and sequence ids on) as a case of
    tests/test_gpu_scratch_independence.py: run(empty) -> the record of everything they return."""
    T = 130
    det, seq = _t(make_det(T, 3)), _t(make_seq(T, "runs"))
    pose, tgt = _t(make_x(T, 17, 3, 5)), _t(make_x(T, 17, 3, 6))

    def run(empty):
        xy, w, state = pkg.prepare_tracks(det, "coco17", (1000.0, 1002.0), 0.1, 8, 0.5, seq)
        filt = pkg.TemporalFilter.gaussian(1.0)
        err, count = pkg.velocity_errors(pose, tgt, seq, 2)
        return {"remap": pkg.coco_to_h36m(det), "xy": xy, "w": w, "state": state, "xy filtered": pkg.filter_tracks(xy, filt, w, seq),
                "pose filtered": pkg.filter_tracks(pose, pkg.TemporalFilter.box(65), w, seq), "err": err, "count": count}
    return run


# tests/test_gpu_scratch_independence.py::test_every_kernel_has_a_case wants a case there for every __global__ function of
# csrc/: the kernels of track.hip get theirs here (the registry is that module's, filled when this one is imported)
tsi.REG["video tracks"] = _scratch_case


def test_results_do_not_depend_on_what_the_outputs_held(pkg, monkeypatch):
    """Under the three fill patterns of every package allocation (tests/scratch_guard.py, the protocol of
    tests/test_gpu_scratch_independence.py): the same bits, all finite, and no write outside the bytes asked for."""
    ran, _ = tsi._independent(pkg, monkeypatch, "video tracks", tsi.REG["video tracks"](pkg))
    assert {"track_remap_kernel", "track_prepare_kernel", "track_filter_kernel", "track_velocity_kernel"} <= ran, sorted(ran)


# ---- SequenceLifter -----------------------------------------------------------------------------------------------------------------
def _model(pkg, dtype, seed=3):
    torch.manual_seed(seed)
    return pkg.LinearModel(34, 51, linear_size=64, compute_dtype=dtype).to(DEV).eval()


def _transforms(pkg):
    rs = np.random.RandomState(1)
    s3, d3 = rs.uniform(-0.3, 0.3, (17, 3)).astype(F), rs.uniform(0.05, 0.6, (17, 3)).astype(F)
    s3[0], d3[0] = 0.0, 0.0
    return pkg.PoseTransform.normalize_2d(), pkg.PoseTransform(s3, d3)


DIV = (1000.0, 1002.0)


@pytest.mark.parametrize("dtype", ["f16x3", "fp32"])
def test_lift_is_the_composition_of_the_public_pieces(pkg, g15, dtype):
    det = _t(g15["det"])
    model = _model(pkg, dtype)
    t2, dn = _transforms(pkg)
    f2, f3 = pkg.TemporalFilter.gaussian(1.0), pkg.TemporalFilter.box(5)
    kw = dict(layout="h36m17", div=DIV, transform_2d=t2, denorm=dn, filter_2d=f2, filter_3d=f3)
    poses, w, state = pkg.SequenceLifter(model, **kw).lift(det)
    xy, w0, s0 = pkg.prepare_tracks(det, "h36m17", DIV, 0.1, 8, 0.5)
    with torch.no_grad():
        y = model(t2.apply(pkg.filter_tracks(xy, f2, w0))).reshape(-1, 17, 3)
    hand = pkg.filter_tracks(dn.invert(y), f3, w0)
    assert same_bits_t(poses, hand) and same_bits_t(w, w0) and torch.equal(state, s0)
    assert tuple(poses.shape) == (256, 17, 3) and torch.isfinite(poses).all()
    small = pkg.SequenceLifter(model, chunk=64, **kw).lift(det)[0]
    assert same_bits_t(small, poses)                                               # chunk = 64 == chunk = 4096
    # flip test-time augmentation: predict_flip_tta on the prepared rows
    tta = pkg.SequenceLifter(model, flip_tta=True, **kw).lift(det)[0]
    y = pkg.predict_flip_tta(model, t2.apply(pkg.filter_tracks(xy, f2, w0)))
    assert same_bits_t(tta, pkg.filter_tracks(dn.invert(y), f3, w0))
    # two copies of the track as two sequences of one call
    two = torch.cat([det, det])
    seq = _t(np.repeat(np.array([7, 3], np.int32), 256))
    p2, w2, s2 = pkg.SequenceLifter(model, **kw).lift(two, seq)
    for half in (slice(0, 256), slice(256, 512)):
        assert same_bits_t(p2[half], poses) and same_bits_t(w2[half], w) and torch.equal(s2[half], state)
    p1 = pkg.SequenceLifter(model, **kw).lift(two)[0]                              # one sequence: the seam is filtered across
    assert not same_bits_t(p1[250:262], p2[250:262])
    model.train()
    with pytest.raises(ValueError):
        pkg.SequenceLifter(model, **kw).lift(det)


def test_track_weights_feed_a_train_step(pkg, g15):
    det = _t(g15["det"])
    xy, w, _ = pkg.prepare_tracks(det, "h36m17", DIV)
    torch.manual_seed(4)
    model = pkg.LinearModel(34, 51, linear_size=64, compute_dtype="f16x3").to(DEV).train()
    opt = pkg.FlatAdamW(model, lr=1e-4)
    crit = pkg.PoseCriterion("mpjpe", coords=3).to(DEV)
    loss, pred = pkg.train_step(model, opt, xy, _t(g15["mb3d"]), criterion=crit, row_weights=pkg.normalize_row_weights(w))
    assert torch.isfinite(loss).all() and tuple(pred.reshape(-1, 17, 3).shape) == (256, 17, 3)


def test_velocity_on_the_recorded_track(pkg, g15):
    mb = _t(g15["mb3d"])
    filt = pkg.TemporalFilter.gaussian(1.0)
    jit = mb + _t(np.random.RandomState(15).randn(*g15["mb3d"].shape).astype(F) * F(0.01))

    def mpjve(a):
        e, c = pkg.velocity_errors(a, mb)
        return float(e.double().sum() / (c.sum() * 17))
    v_smooth, v_jit_f, v_jit = mpjve(pkg.filter_tracks(mb, filt)), mpjve(pkg.filter_tracks(jit, filt)), mpjve(jit)
    assert np.isfinite(v_smooth) and v_smooth < v_jit_f < v_jit
