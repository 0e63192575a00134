"""The order of the decode task lists on the CPU (csrc/need.h: dcl_group_pos and dcl_place_round through the host-only lic360_dcl_order_layout, no
GPU work) against the restatement of tests/dc_order_cases.py: grouped emission, the placement pass, and the load of the workgroups that walk the list."""
import ctypes as C

import numpy as np
import pytest

import dc_order_cases as cases

W_VALUES = (31, 32)


def lib_layout(g0, nrec, G, nb, place, W):
    from lic360 import _lib, _chk
    n = 3 * int(sum(nrec))
    a, b = np.array(list(g0) + [0], np.int32), np.array(list(nrec) + [0], np.int32)
    emit, slot = np.full(n + 1, -7, np.int32), np.full(n + 1, -7, np.int32)
    _chk(_lib.lic360_dcl_order_layout(len(g0), a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), G, nb, int(place), W,
                                      emit.ctypes.data_as(C.c_void_p), slot.ctypes.data_as(C.c_void_p)))
    assert emit[n] == -7 and slot[n] == -7
    return emit[:n].astype(np.int64), slot[:n].astype(np.int64)


def test_the_workgroups_of_an_xcd():
    """(D6_GRID - xcd + 7) >> 3 at the launcher's grid of 256: 32 on every XCD; 31 occurs on a grid that is no multiple of 8 (250: XCDs 2..7)"""
    assert {cases.wgs_of_xcd(x) for x in range(8)} == {32}
    assert [cases.wgs_of_xcd(x, 250) for x in range(8)] == [32, 32, 31, 31, 31, 31, 31, 31]


@pytest.mark.parametrize("W", W_VALUES)
def test_layout_matches_the_restatement(W):
    sizes = set()
    for g0, nrec, G in cases.count_cases():
        n = 3 * sum(nrec)
        sizes.add(n)
        cost = cases.costs_by_id(g0, nrec, G)
        ratio = {}
        for name, (nb, place) in cases.ORDERS.items():
            for pl in sorted({place, False}):
                emit, slot = lib_layout(g0, nrec, G, nb, pl, W)
                we, ws = cases.layout(g0, nrec, G, nb, pl, W)
                assert np.array_equal(emit, we) and np.array_equal(slot, ws), (g0, nrec, G, name, pl)
                assert sorted(emit.tolist()) == list(range(n)) and sorted(slot.tolist()) == list(range(n)), "a permutation"
                assert np.array_equal(slot // W, emit // W), "every record stays in its round"
                if nb == 1:
                    assert np.array_equal(emit, np.arange(n))
                    if not pl:
                        assert np.array_equal(slot, np.arange(n)), "NB = 1 without placement is the identity"
                if not pl:
                    assert np.array_equal(slot, emit)
                load = cases.walk_loads(slot, cost, W)
                assert load.sum() == cost.sum()
                ratio[nb, pl] = cases.max_over_mean([load])
        for nb in (1, 2, 4, 8):
            assert ratio[nb, True] <= ratio[nb, False] + 1e-12, (g0, nrec, G, nb, ratio)
    assert {0, 3, 30, 33, 63, 96} <= sizes, "empty, single-block, shorter than a round, one past a round, one short of two rounds, three rounds"


def test_round_sizes_around_w():
    """lists of exactly W and of W + 1 records.  A list as built holds three nets' records, a multiple of 3: exactly W is 30 records at W = 30,
    W + 1 is 33 at W = 32; W = 31 takes 30 (one short) and 33 (two past)."""
    for W in (30,) + W_VALUES:
        for g0, nrec, G in (([45, 42, 39], [10, 0, 0], 48), ([45, 42], [10, 1], 48), ([45, 42, 39], [5, 5, 1], 48), ([9, 6, 3, 0], [3, 3, 3, 2], 12)):
            n = 3 * sum(nrec)
            assert n in (30, 33)
            for nb in (1, 2, 4, 8):
                emit, slot = lib_layout(g0, nrec, G, nb, True, W)
                assert sorted(slot.tolist()) == list(range(n)) and np.array_equal(slot // W, emit // W)
                assert np.array_equal(slot, cases.layout(g0, nrec, G, nb, True, W)[1])


def test_group_positions_put_equal_record_indices_side_by_side():
    """inside a group of NB blocks: net, then record index, then block -- record r of the group's blocks, one net, are neighbours"""
    g0, nrec, G = [45, 42, 39, 36, 33], [3, 1, 0, 2, 2], 48
    ids = cases.ids_of(nrec)
    emit, _ = lib_layout(g0, nrec, G, 4, False, 32)
    seq = [ids[i] for i in np.argsort(emit)]
    want = []
    for net in range(3):
        want += [(0, net, 0), (1, net, 0), (3, net, 0), (0, net, 1), (3, net, 1), (0, net, 2)]
    want += [(4, net, r) for net in range(3) for r in range(2)]
    assert seq == want


def test_fixture_is_what_the_cases_file_records():
    rows = np.load(cases.os.path.join(cases.os.path.dirname(cases.os.path.abspath(__file__)), "golden", cases.GOLDEN))["rows"]
    assert np.array_equal(rows, cases.smooth_mask_counts())


def test_grouped_order_keeps_the_balance_on_smooth_masks():
    """The recorded smooth-mask lists (XCD 0 of 64 images at 48 x 64 x 128; layers 2, 6, 10, 11; every plane), W = 32.  A plane's launch waits for its
    most loaded workgroup, so a layer's figure is sum of the planes' maxima over sum of their means.  The margin comes from today's order (NB = 1, no
    placement) alone: no layer may be worse balanced under NB = 4 with placement than the worst-balanced recorded layer is today -- and placement must
    not lose against the same emission without it.

    The figures (max / mean; today, NB = 4 as emitted, NB = 4 placed): layer 2: 1.0239, 1.0608, 1.0197; layer 6: 1.0292, 1.0967, 1.0219; layer 10:
    1.0515, 1.1320, 1.0339; layer 11: 1.0718, 1.1604, 1.0399.  (With the rounds taken strictly in list order the placed figures were 1.0324, 1.0374,
    1.0668 and 1.0792 -- layer 11 above the margin: a short last round landed on whatever its workgroups carried by then.  It is charged first now.)"""
    W = 32
    G = cases.GOLDEN_SHAPE[0]
    today, naive, placed = {}, {}, {}
    for l, lists in cases.golden_lists().items():
        loads = {k: [] for k in ("today", "naive", "placed")}
        for g0, nrec in lists:
            cost = cases.costs_by_id(g0, nrec, G)
            loads["today"].append(cases.walk_loads(lib_layout(g0, nrec, G, 1, False, W)[1], cost, W))
            loads["naive"].append(cases.walk_loads(lib_layout(g0, nrec, G, 4, False, W)[1], cost, W))
            loads["placed"].append(cases.walk_loads(lib_layout(g0, nrec, G, 4, True, W)[1], cost, W))
        today[l], naive[l], placed[l] = (cases.max_over_mean(loads[k]) for k in ("today", "naive", "placed"))
        print("layer %2d: max / mean load today %.4f, NB = 4 as emitted %.4f, NB = 4 placed %.4f" % (l, today[l], naive[l], placed[l]))
    margin = max(today.values())
    for l in today:
        assert placed[l] <= margin, (l, placed[l], margin)
        assert placed[l] <= naive[l]
