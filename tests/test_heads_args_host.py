"""CPU tests of the argument checks of the soft-argmax entry points (csrc/softargmax.hip): every invalid call below is turned
away before the first HIP call, so no device is needed and the pointers are host buffers that nobody reads (the law array,
which the host does read, aside).  Each answers the status the entry point has always answered, and pl_last_error() starts
with the name of the entry point that was called."""
import ctypes

import numpy as np
import pytest

EINVAL, ESHAPE = -1, -2
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    return ge.build().lib()


_buf = np.zeros(256, np.float32)
PTR = (_buf.ctypes.data + 63) & ~63               # 64-byte aligned, inside the buffer
LAW = (ctypes.c_float * 6)(4.0, 2.0, 4.0, 1.0, 1.0, 1.0)
NCHW = dict(BJ=6, D=8, H=4, W=8, ncoord=3, centred=1)
NHWC = dict(B=2, J=3, H=3, W=5)
HM = dict(target=PTR, sigma=0.5, law=LAW)
PLANES = dict(dlogits=PTR, dl_planes=PTR, planes_mode=3, dl_scale=PTR)

# entry point -> (its parameters in order, a valid call's values); "stream" is not a device stream here and never used
ENTRIES = {
    "pl_softargmax_fwd": ("logits BJ D H W ncoord centred coords stats stream", dict(NCHW)),
    "pl_softargmax_bwd": ("logits stats gcoords BJ D H W ncoord centred dlogits stream", dict(NCHW)),
    "pl_softargmax_hm_fwd": ("logits target BJ D H W ncoord centred sigma law coords sq stats stream", dict(NCHW, **HM)),
    "pl_softargmax_hm_bwd": ("logits target stats gcoords gsq BJ D H W ncoord centred sigma law dlogits stream", dict(NCHW, **HM)),
    "pl_softargmax3d_nhwc_fwd": ("logits B J H W coords stats stream", dict(NHWC)),
    "pl_softargmax3d_nhwc_hm_fwd": ("logits target B J H W sigma law coords sq stats stream", dict(NHWC, **HM)),
    "pl_softargmax3d_nhwc_bwd": ("logits stats gcoords B J H W dlogits stream", dict(NHWC)),
    "pl_softargmax3d_nhwc_bwd_ex": ("logits stats gcoords B J H W dlogits dl_planes planes_mode dl_scale stream",
                                    dict(NHWC, **PLANES)),
    "pl_softargmax3d_nhwc_hm_bwd_ex": ("logits target stats gcoords gsq B J H W sigma law dlogits dl_planes planes_mode dl_scale "
                                       "stream", dict(NHWC, **HM, **PLANES)),
    "pl_softargmax_dl_scale": ("gcoords rows ncoord scale2 stream", dict(rows=6, ncoord=3)),
    "pl_softargmax_hm_dl_scale": ("gcoords gsq rows ncoord scale2 stream", dict(rows=6, ncoord=3)),
    "pl_heatmap_gaussian": ("target BJ D H W ncoord sigma law out stream", dict(NCHW, **HM)),
    "pl_heatmap_gaussian_host": ("target BJ D H W ncoord sigma law out", dict(NCHW, **HM)),
}
POINTERS = {"logits", "target", "stats", "gcoords", "gsq", "coords", "sq", "dlogits", "dl_planes", "dl_scale", "scale2", "out", "law"}
NCHW_SOFTARGMAX = [n for n in ENTRIES if n.startswith("pl_softargmax_") and "dl_scale" not in n]
HM_ENTRIES = [n for n, (p, _) in ENTRIES.items() if "sigma" in p.split()]
PLANES_ENTRIES = [n for n, (p, _) in ENTRIES.items() if "dl_planes" in p.split()]
NAN_LAW = (ctypes.c_float * 6)(4.0, 2.0, NAN, 1.0, 1.0, 1.0)


def _cases():
    """(entry point, what is wrong, the arguments to replace, status, a text the message holds)"""
    out = []
    for name, (params, _) in ENTRIES.items():
        params = params.split()
        for p in params:
            optional = p == "dl_scale" or (p in ("dlogits", "dl_planes") and "dl_planes" in params)
            if p in POINTERS and not optional:
                out.append((name, f"null {p}", {p: None}, EINVAL, "null"))
        # alignment is asked of the float4 kernels only (the NHWC forward reads scalars)
        if "logits" in params and name != "pl_softargmax3d_nhwc_fwd" and name != "pl_softargmax3d_nhwc_hm_fwd":
            out.append((name, "logits at a 4-byte offset", {"logits": PTR + 4}, EINVAL, "16-byte aligned"))
        if name in NCHW_SOFTARGMAX:
            out.append((name, "W = 6", {"W": 6}, ESHAPE, "W % 4 == 0"))
        if "ncoord" in params and "D" in params:
            out.append((name, "ncoord = 2 with D = 2", {"ncoord": 2, "D": 2}, ESHAPE, "2 coordinates need depth 1"))
        if "ncoord" in params:
            out.append((name, "ncoord = 4", {"ncoord": 4}, ESHAPE, "ncoord=4" if "D" in params else "bad dims"))
        if name in ("pl_softargmax_bwd", "pl_softargmax_hm_bwd"):
            out.append((name, "BJ = 65536", {"BJ": 65536}, ESHAPE, "65535 (split the batch)"))
        if name in HM_ENTRIES:
            out.append((name, "sigma = 0", {"sigma": 0.0}, EINVAL, "not a positive finite number"))
            out.append((name, "sigma = 3.0", {"sigma": 3.0}, ESHAPE, "half-width 9"))
            out.append((name, "a NaN in law", {"law": NAN_LAW}, EINVAL, "law[2] is not finite"))
        if name in PLANES_ENTRIES:
            out.append((name, "mode 3 planes without dl_scale", {"dl_scale": None}, EINVAL, "fp16 planes need dl_scale"))
            out.append((name, "both outputs NULL", {"dlogits": None, "dl_planes": None}, EINVAL, "null pointer"))
    return out


CASES = _cases()


def test_the_cases_cover_every_entry_point_of_the_file():
    assert len(ENTRIES) == 13 and {c[0] for c in CASES} == set(ENTRIES)
    assert sum(c[1] == "sigma = 3.0" for c in CASES) == 6 and sum(c[1] == "BJ = 65536" for c in CASES) == 2


@pytest.mark.parametrize("name,what,wrong,status,text", CASES, ids=[f"{c[0]}-{c[1].replace(' ', '_')}" for c in CASES])
def test_invalid_call_answers_its_status_under_the_called_name(L, name, what, wrong, status, text):
    params, valid = ENTRIES[name]
    args = dict({p: PTR for p in params.split() if p in POINTERS}, stream=None, **valid)
    args.update(wrong)
    rc = getattr(L, name)(*[args[p] for p in params.split()])
    msg = L.pl_last_error().decode()
    print(f"{name}, {what}: status {rc}, {msg!r}")
    assert rc == status
    assert msg.startswith(name + ": ") and text in msg
