"""The "f16x3" range guard's host side: the message builder on hand-made records, the error type, and the C entry in
both the header and the ctypes table.  No GPU."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()


def _record(**slots):
    rec = np.zeros(16, dtype=np.int32)
    for s, mag in slots.items():
        rec[int(s[1:])] = np.float32(mag).view(np.int32)
    return rec


def test_describe_clean_record_is_none(pkg):
    rg = pkg.range_guard
    assert rg.describe(np.zeros(16, dtype=np.int32)) is None
    assert rg.flagged(np.zeros(16, dtype=np.uint32)) == []
    with pytest.raises(ValueError):
        rg.describe(np.zeros(8, dtype=np.int32))


def test_describe_one_site_names_layer_magnitude_limit_and_remedy(pkg):
    rg = pkg.range_guard
    msg = rg.describe(_record(s3=70000.0))
    assert "hidden activation of layer 3" in msg
    assert "70000" in msg and "65504" in msg
    assert 'compute_dtype="bf16x6"' in msg and '"fp32"' in msg
    assert rg.flagged(_record(s3=70000.0)) == [(3, 70000.0)]


def test_describe_several_sites_with_their_own_limits(pkg):
    rg = pkg.range_guard
    msg = rg.describe(_record(s0=1e5, s8=5000.0, s9=5e6, s10=4100.0, s11=123456.0))
    assert "hidden activation of layer 0" in msg and "100000" in msg
    assert "weight planes of the lifter" in msg and "5000" in msg and "4094" in msg          # 65504 / 16
    assert "conv-path feature map" in msg and "5e+06" in msg and "4.19226e+06" in msg         # 65504 * 64
    assert "conv-path weight planes" in msg and "4100" in msg
    assert "caller-chosen scale" in msg and "123456" in msg and "65504 / scale" in msg
    assert [s for s, _ in rg.flagged(_record(s0=1e5, s8=5000.0, s9=5e6))] == [0, 8, 9]
    assert rg.site_limit(8) == 65504.0 / 16 and rg.site_limit(9) == 65504.0 * 64 and rg.site_limit(11) is None


def test_describe_clamped_layer_index(pkg):
    rg = pkg.range_guard
    msg = rg.describe(_record(s7=80000.0))
    assert "layer 7 or above" in msg and "80000" in msg
    assert "layer 6" in rg.describe(_record(s6=80000.0))


def test_range_error_is_a_poselift_error(pkg):
    assert issubclass(pkg.PoseliftRangeError, pkg.PoseliftError)
    assert pkg.range_guard.PoseliftRangeError is pkg.PoseliftRangeError
    e = pkg.PoseliftRangeError("m", [(3, 7e4)])
    assert isinstance(e, RuntimeError) and e.sites == [(3, 7e4)]


def test_entry_in_header_and_ctypes_table(pkg):
    header = open(os.path.join(ROOT, "include", "poselift.h")).read()
    assert re.search(r"\bint\s+pl_range_monitor\s*\(\s*void\s*\*", header)
    assert int(re.search(r"#define PL_RANGE_SITES (\d+)", header).group(1)) == pkg.range_guard.SITES == 16
    assert "pl_range_monitor" in pkg._lib.SIGNATURES
    L = pkg.lib()
    assert L.pl_range_monitor(None) == 0                  # the initial state again: host only, nothing is launched
    assert L.pl_range_monitor(2) != 0                     # a misaligned record is refused
    assert L.pl_range_monitor(None) == 0
    for name, val in (("LIFTER_ACT", 0), ("LIFTER_WEIGHT", 8), ("CONV_ACT", 9), ("CONV_WEIGHT", 10), ("SPLIT", 11)):
        assert int(re.search(rf"#define PL_RANGE_SITE_{name} (\d+)", header).group(1)) == getattr(pkg.range_guard, "SITE_" + name) == val
