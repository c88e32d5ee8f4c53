"""Host-only model of the chained backward pair's hand-off (csrc/gemm_planes16.h HAND-OFF, csrc/gemm_planes.hip ChainHand):
the step schedule of the two wave roles, the vmcnt arithmetic of the loader's steps and the LDS layout of the hand-off block.
No GPU: a mismatched barrier count hangs a workgroup, and that must not be found out on a device.

The constants are read from the header, so the model follows the code; the schedules below are the loops of
planes_run16_chain written out as lists of events."""
import os
import re

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "3d_poseestimation_amd", "csrc")


def _consts():
    text = open(os.path.join(CSRC, "gemm_planes16.h")).read()
    env = {}
    for name in ("kChainChunks", "kChainAhead", "kChainFirst", "kChainMinNk1", "kHandBytes"):
        expr = re.search(r"constexpr int %s = ([^;]+);" % name, text).group(1)
        env[name] = int(eval(expr, {}, env))
    return env


C = _consts()
NCH, AHEAD, FIRST, MIN_NK1 = C["kChainChunks"], C["kChainAhead"], C["kChainFirst"], C["kChainMinNk1"]
NDMA = {1: 4, 2: 8}                      # LDS-DMA instructions per loader wave and k-tile: one bf16 plane, two fp16 planes


def vm_ops(j, add, bnr):
    """ChainHand::vm_ops: the loads of row-quad j (addend; saved z and two bitmap loads), the g store of row-quad j - AHEAD"""
    return ((1 if add else 0) + (3 if bnr else 0) if 0 <= j < NCH else 0) + (1 if 0 <= j - AHEAD < NCH else 0)


def computing_schedule(nk0, nk1):
    """Events of a computing wave: ('barrier', i) in order; ('put',) = the hand-off block written (after item 0's last step);
    ('epi1',) = dW's epilogue (stages through the hand-off blocks)."""
    ev = [("barrier", "first")]
    for kt in range(nk0):
        ev.append(("barrier", kt))                     # the mid-step barrier of stream step kt
    ev.append(("put",))
    for kt in range(nk1):
        ev.append(("barrier", nk0 + kt))
    ev.append(("epi1",))
    return ev


def loader_schedule(nk0, nk1, hand, add=True, bnr=True, npl=2):
    """Events of a loader wave: ('dma', tile), ('vm', n, what), ('lds_read', row_quad), ('wait', N), ('barrier', i)."""
    nd = NDMA[npl]
    ev = [("dma", 0), ("dma", 1), ("wait", nd), ("barrier", "first")]
    for g in range(nk0 - 2):
        ev += [("dma", g + 2), ("wait", nd), ("barrier", g)]
    step = nk0 - 2                                       # barrier index of item-1 iteration kt = nk0 - 2 + kt

    def plain(kt):
        return [("dma", nk0 + kt), ("wait", nd), ("barrier", step + kt)]
    if not hand:
        for kt in range(nk1):
            ev += plain(kt)
    else:
        for kt in range(FIRST):
            ev += plain(kt)
        for j in range(NCH + AHEAD):
            kt = FIRST + j
            store = 1 if 0 <= j - AHEAD < NCH else 0
            ev.append(("dma", nk0 + kt))
            if j < NCH:
                ev.append(("vm", vm_ops(j, add, bnr) - store, "loads"))
            if store:
                ev += [("lds_read", j - AHEAD), ("vm", 1, "store")]
            ev += [("wait", vm_ops(j - 1, add, bnr) + nd + vm_ops(j, add, bnr)), ("barrier", step + kt)]
        for kt in range(FIRST + NCH + AHEAD, nk1):       # (a range that is empty or negative issues nothing, like the for loop)
            ev += plain(kt)
    ev += [("wait", 0), ("barrier", nk0 + nk1 - 2), ("wait", 0), ("barrier", nk0 + nk1 - 1)]
    return ev


def barriers(ev):
    return [e[1] for e in ev if e[0] == "barrier"]


GRID = [(nk0, nk1) for nk0 in (2, 3, 4, 20, 32) for nk1 in range(MIN_NK1 - 3, MIN_NK1 + 4)]


def test_constants():
    assert NCH == 16 and MIN_NK1 == FIRST + NCH + AHEAD + 1 and FIRST + AHEAD >= 3
    assert C["kHandBytes"] == 4 * 64 * 64 * 4 and 3 * 32768 + C["kHandBytes"] <= 160 * 1024
    src = open(os.path.join(CSRC, "gemm_planes.hip")).read()
    assert "nk1 >= plp::kChainMinNk1" in src              # the host check states the bound


@pytest.mark.parametrize("nk0,nk1", GRID)
def test_roles_execute_the_same_barriers(nk0, nk1):
    """Whatever the host routes (hand-off from kChainMinNk1 on, the epilogue on the computing waves below), both roles run
    the same barriers in the same order: one per stream step, plus the first."""
    hand = nk1 >= MIN_NK1
    want = ["first"] + list(range(nk0 + nk1))
    assert barriers(computing_schedule(nk0, nk1)) == want
    assert barriers(loader_schedule(nk0, nk1, hand)) == want
    # the bound is not decorative: two steps below it the hand-off schedule would run more barriers than the computing waves
    if nk1 < FIRST + NCH + AHEAD:
        assert barriers(loader_schedule(nk0, nk1, True)) != want


@pytest.mark.parametrize("nk0,nk1", [g for g in GRID if g[1] >= MIN_NK1])
def test_epilogue_sits_between_put_and_the_last_step(nk0, nk1):
    ev = loader_schedule(nk0, nk1, True)
    passed = []                                           # barriers the loader has passed so far
    reads = {}
    for e in ev:
        if e[0] == "barrier":
            passed.append(e[1])
        if e[0] == "lds_read":
            reads[e[1]] = passed[-1]
    assert sorted(reads) == list(range(NCH))              # every row-quad, once
    # the block is written between the barriers of steps nk0 - 1 and nk0: the first read comes after the barrier of step nk0
    assert min(reads.values()) >= nk0
    # the last row-quad leaves in an iteration whose own barrier is before the loop's last step; dW's epilogue (which stages
    # through the hand-off blocks) starts after the last barrier
    assert max(reads.values()) + 1 < nk0 + nk1 - 1
    comp = computing_schedule(nk0, nk1)
    assert comp.index(("epi1",)) > comp.index(("barrier", nk0 + nk1 - 1))
    assert comp.index(("barrier", nk0 - 1)) < comp.index(("put",)) < comp.index(("barrier", nk0))


@pytest.mark.parametrize("npl", [1, 2])
@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("bnr", [False, True])
def test_vmcnt_of_every_step_lands_the_next_tile(npl, add, bnr):
    """vmcnt counts loads, stores and LDS-DMA in issue order.  At the barrier of step g k-tile g + 1 must have landed: the wait's
    N may be at most the number of operations issued after that tile's last DMA (fewer waits for more: safe; more would let
    the barrier pass with the tile in flight), it must fit the 6-bit counter, and inside the epilogue steps it is exact."""
    nk0, nk1 = 4, MIN_NK1 + 1
    nd = NDMA[npl]
    queue, last_dma = [], {}                              # issue order; index in `queue` of each tile's last DMA
    for e in loader_schedule(nk0, nk1, True, add, bnr, npl):
        if e[0] == "dma":
            queue += [("dma", e[1])] * nd
            last_dma[e[1]] = len(queue) - 1
        elif e[0] == "vm":
            queue += [e[2]] * e[1]
        elif e[0] == "wait":
            pending_wait = e[1]
        elif e[0] == "barrier":
            g = -1 if e[1] == "first" else e[1]
            if g + 1 in last_dma:
                after = len(queue) - 1 - last_dma[g + 1]
                assert pending_wait <= after and pending_wait <= 63, (e, pending_wait, after)
                in_epilogue = nk0 - 2 + FIRST <= g < nk0 - 2 + FIRST + NCH + AHEAD
                if in_epilogue:
                    assert pending_wait == after, (e, pending_wait, after)


def hand_idx(row, col):
    """plp::hand_idx: float index of element (row, col) of a 64 x 64 hand-off block"""
    return row * 64 + (col ^ (((row >> 2) & 3) << 4))


def test_hand_off_layout_is_a_bijection_with_16_byte_rows():
    assert sorted(hand_idx(r, c) for r in range(64) for c in range(64)) == list(range(64 * 64))
    for r in range(64):
        for c in range(0, 64, 4):                         # the loader's float4: four consecutive columns stay together
            assert [hand_idx(r, c + i) for i in range(4)] == [hand_idx(r, c) + i for i in range(4)] and hand_idx(r, c) % 4 == 0


def test_hand_off_layout_bank_conflicts():
    """ds_write_b32 of the accumulator layout: lane groups are the two 32-lane halves, 32 banks of 4 bytes -- at most 2-way
    (here: none).  ds_read_b128 of the epilogue layout: four 16-lane groups, 64 banks -- the 16 lanes of a group on 16
    distinct 16-byte slots of the 256-byte bank row."""
    for rt in range(4):
        for ct in range(4):
            for r in range(4):
                for half in (range(0, 32), range(32, 64)):
                    banks = [hand_idx(rt * 16 + 4 * (l >> 4) + r, ct * 16 + (l & 15)) % 32 for l in half]
                    assert max(banks.count(b) for b in set(banks)) <= 2
                    assert len(set(banks)) == 32
    groups = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
              list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
              list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
              list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]
    assert sorted(sum(groups, [])) == list(range(64))
    for it in range(16):
        for grp in groups:
            slots = [(hand_idx(4 * it + (l >> 4), 4 * (l & 15)) // 4) % 16 for l in grp]
            assert len(set(slots)) == 16
