"""Host-only model of the slab ride in the chained backward pair (csrc/gemm_planes16.h SLAB RIDE): in dX's half of the launch
the loader waves sum the four split-K slabs of the layer above, a chunk per k-step, between their DMA issue and the barrier.
No GPU: a mismatched barrier count hangs a workgroup and a wrong vmcnt lets a barrier pass with a k-tile in flight; neither
must be found out on a device.

The constants are read from the header, so the model follows the code; the schedules below are the two loader loops of
planes_run16_chain's dX phase written out as lists of events, and the predicate is gemm_planes.hip's pair_carries_slab_sum
on top of pair_route, in the lifter's terms."""
import os
import re

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "3d_poseestimation_amd", "csrc")


def _consts():
    text = open(os.path.join(CSRC, "gemm_planes16.h")).read()
    env = {}
    for name in ("kChainChunks", "kChainAhead", "kChainFirst", "kChainMinNk1", "kRideSlabs", "kRideChunks", "kRideFirst",
                 "kRideMinNk0"):
        expr = re.search(r"constexpr int %s = ([^;]+);" % name, text).group(1)
        env[name] = int(eval(expr, {}, env))
    return env


C = _consts()
R, Q, A, FIRST, MIN_NK0, MIN_NK1 = (C["kRideSlabs"], C["kRideChunks"], C["kChainAhead"], C["kRideFirst"], C["kRideMinNk0"],
                                    C["kChainMinNk1"])
NDMA = {1: 4, 2: 8}                      # LDS-DMA instructions per loader wave and k-tile: one bf16 plane, two fp16 planes


def vm_ops(j):
    """SlabRider::vm_ops: the R slab loads of chunk j, the store of chunk j - A"""
    return (R if 0 <= j < Q else 0) + (1 if 0 <= j - A < Q else 0)


def computing_dx(nk0):
    """Barriers of a computing wave up to the end of item 0: the first, then the mid-step barrier of every stream step."""
    return ["first"] + list(range(nk0))


def loader_dx(nk0, ride, npl=2, first=FIRST):
    """Events of a loader wave in dX's phase: ('dma', tile), ('load', chunk), ('store', chunk), ('wait', N), ('barrier', i).
    Iteration g issues k-tile g + 2 and runs the barrier of step g; the barriers of steps nk0 - 2 and nk0 - 1 belong to item
    1's first two iterations (plain in their DMA count as far as item 0's waits go: appended here as such)."""
    nd = NDMA[npl]
    ev = [("dma", 0), ("dma", 1), ("wait", nd), ("barrier", "first")]

    def plain(g):
        return [("dma", g + 2), ("wait", nd), ("barrier", g)]
    if not ride:
        for g in range(nk0 - 2):
            ev += plain(g)
    else:
        for g in range(first):
            ev += plain(g)
        for j in range(Q + A):
            ev.append(("dma", first + j + 2))
            if j < Q:
                ev.append(("load", j))
            if 0 <= j - A < Q:
                ev.append(("store", j - A))
            ev += [("wait", vm_ops(j - 1) + nd + vm_ops(j)), ("barrier", first + j)]
        for g in range(first + Q + A, nk0 - 2):          # (a range that is empty or negative issues nothing, like the for loop)
            ev += plain(g)
    ev += plain(nk0 - 2) + plain(nk0 - 1)                # item 1's first two iterations close dX's last two steps
    return ev


def barriers(ev):
    return [e[1] for e in ev if e[0] == "barrier"]


def tn_splits(M, N, K):
    """api.hip tn_splits"""
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    return max(1, min(256 // tiles, (K + 127) // 128))


def carries(H, B, splits):
    """pair_carries_slab_sum for the lifter's pair (dX: M = B, N = K = H; dW: M = N = H, K = B in `splits` slices) and the
    slabs of an equal layer above: the hand-off route, four slabs, the float4s dealt exactly, dX long enough."""
    grid_nn, grid_tn = (B // 128) * (H // 128), (H // 128) ** 2 * splits
    chain = grid_nn == grid_tn and H % 32 == 0 and H >= 64 and B % (32 * splits) == 0 and B >= 32 * splits
    hand = chain and B // (32 * splits) >= MIN_NK1
    return hand and splits == R and H * H == Q * 4 * 64 * 4 * grid_nn and H // 32 >= MIN_NK0


def test_constants():
    assert R == 4 and Q * R == 16 and A == 3
    assert MIN_NK0 == FIRST + Q + A + 2                  # nk0 - 2 >= kRideFirst + q + A
    assert max(vm_ops(j - 1) + 8 + vm_ops(j) for j in range(Q + A)) <= 63          # the 6-bit counter
    src = open(os.path.join(CSRC, "gemm_planes.hip")).read()
    assert "nk0 >= plp::kRideMinNk0" in src               # the host check states the bound
    assert "nk1 >= plp::kChainMinNk1" in src


NK0S = [Q + A + 1, Q + A + 2, Q + A + 3, 20, 32]


@pytest.mark.parametrize("nk0", NK0S)
def test_roles_execute_the_same_barriers(nk0):
    """Whatever the host routes (the ride from kRideMinNk0 on, the plain loop below), both roles run the same barriers in
    the same order: one per stream step, plus the first."""
    ride = nk0 >= MIN_NK0
    want = computing_dx(nk0)
    assert barriers(loader_dx(nk0, ride)) == want
    assert barriers(loader_dx(nk0, False)) == want


@pytest.mark.parametrize("first", sorted({0, FIRST}))
def test_the_bound_is_the_real_one(first):
    """At the bound the ride's last step is dX's last loader iteration; one step below it the ride loop would run a barrier
    more than the computing waves do.  (first = 0: nk0 - 2 >= q + A, the ride's own length.)"""
    bound = first + Q + A + 2
    assert barriers(loader_dx(bound, True, first=first)) == computing_dx(bound)
    assert barriers(loader_dx(bound - 1, True, first=first)) != computing_dx(bound - 1)
    if first == FIRST:
        assert bound == MIN_NK0


@pytest.mark.parametrize("npl", [1, 2])
@pytest.mark.parametrize("nk0", [n for n in NK0S + [MIN_NK0, MIN_NK0 + 1] if n >= MIN_NK0])
def test_vmcnt_of_every_step_lands_the_next_tile(npl, nk0):
    """vmcnt counts loads, stores and LDS-DMA in issue order.  At the barrier of step g k-tile g + 1 must have landed: every
    wait's N equals the number of operations issued after that tile's last DMA."""
    nd = NDMA[npl]
    queue, last_dma, pending = [], {}, None
    for e in loader_dx(nk0, True, npl):
        if e[0] == "dma":
            queue += [("dma", e[1])] * nd
            last_dma[e[1]] = len(queue) - 1
        elif e[0] == "load":
            queue += [e] * R
        elif e[0] == "store":
            queue.append(e)
        elif e[0] == "wait":
            pending = e[1]
        elif e[0] == "barrier":
            g = -1 if e[1] == "first" else e[1]
            after = len(queue) - 1 - last_dma[g + 1]
            # equal in the ride's steps; the plain step right behind it waits for the last store as well (fewer: safe)
            assert pending <= after and pending <= 63, (e, pending, after)
            if g < FIRST + Q + A:
                assert pending == after, (e, pending, after)


@pytest.mark.parametrize("nk0", [n for n in NK0S + [MIN_NK0] if n >= MIN_NK0])
def test_stores_follow_their_loads_and_end_inside_dx(nk0):
    ev = loader_dx(nk0, True)
    step, loads, stores = -1, {}, {}                      # step = index of the next barrier
    for e in ev:
        if e[0] == "barrier":
            step = 0 if e[1] == "first" else e[1] + 1
        elif e[0] == "load":
            assert e[1] not in loads
            loads[e[1]] = step
        elif e[0] == "store":
            assert e[1] not in stores
            stores[e[1]] = step
    assert sorted(loads) == sorted(stores) == list(range(Q))
    for j in range(Q):
        assert stores[j] - loads[j] >= A
    # the last store is issued before the barrier of step nk0 - 3, the last one of item 0's own iterations -- before dX's last
    # barrier (step nk0 - 1) -- and the first hand-off step (iteration 0 of item 1) sees a plain step in front of it or waits
    # for that store too
    assert max(stores.values()) <= nk0 - 3 < nk0 - 1


def ride_indices(H, B, splits):
    """float4 index of (workgroup, loader wave, lane, chunk): wave-global index wv = 4 workgroup + loader wave."""
    grid = (B // 128) * (H // 128)
    nwaves = 4 * grid
    for wg in range(grid):
        for lw in range(4):
            wv = 4 * wg + lw
            for j in range(Q):
                base = (j * nwaves + wv) * 64
                yield base                                 # lanes base .. base + 63: one contiguous KB per instruction


def test_coverage_at_the_bench_shape():
    H, B = 1024, 4096
    splits = tn_splits(H, H, B)
    assert splits == 4 and carries(H, B, splits)
    n4 = H * H // 4
    bases = sorted(ride_indices(H, B, splits))
    assert bases == list(range(0, n4, 64))                # every float4 of [0, n4) exactly once, none beyond


def test_predicate_refuses_other_slab_counts():
    H, B = 640, 6400
    splits = tn_splits(H, H, B)
    assert splits == 10 and B // (32 * splits) >= MIN_NK1  # the hand-off route, but ten slabs
    assert not carries(H, B, splits)
    for H in (768, 896, 1152, 1280):                      # 7, 5, 3, 2 slabs
        s = tn_splits(H, H, H * tn_splits(H, H, 1 << 20))
        assert s != R and not carries(H, H * s, s)
    assert not carries(256, 1024, 4)                      # four slabs, chained, but not the hand-off form: no ride
