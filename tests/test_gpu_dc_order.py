"""The order of the decode task lists on the GPU (LIC360_DC_ORDER, read when a codec is created: csrc/need.h, need_kernels.hip: k_dc_tasks' grouped
emission and k_dc_place).  The order decides which workgroup runs which record when and nothing else, so under every order -- 1, 1p, 2, 4, 8 -- on the
shapes of tests/dc_order_cases.py, with 1e10 in every activation cell beforehand and again in a second pass over other masks in the same buffers:
  * the bitstreams are the CPU oracle's (the fixture tests/golden/dc_order_streams.npz), the decode of the oracle's bytes gives the symbols, err is 0;
  * per (layer, plane) the records of the eight lists are, as a multiset, those of order 1;
  * order 1 gives the lists of the commit before the switch existed, position for position (their digests, recorded from that commit's library, are
    the fixture tests/golden/dc_order_parent_lists.npz), and a grouped order really is another order."""
import hashlib
import os

import numpy as np
import pytest

import dc_order_cases as cases
from util import make_main_params
from gpu_support import codec_under, dev  # noqa: F401

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POISON = 1.0e10


def lists_of(fc, shape):
    """[(counts [8], records of list x up to its count)] per (layer 1..11, plane)"""
    G, H, W, B = shape
    P = H + W + G - 2
    cnt, cap = fc.debug_lists(3)
    cnt = cnt.reshape(12, P, 8)
    rec = fc.debug_lists(4)[0].reshape(12, P, 8, cap, 4)
    assert (cnt[1:] >= 0).all() and (cnt[1:] <= cap).all()                 # (the first layer keeps its full task list: no counts of layer 0)
    return cnt, rec


def digest(cnt, rec):
    h = hashlib.sha256(np.ascontiguousarray(cnt[1:]).astype(np.int32).tobytes())
    for l in range(1, 12):
        for p in range(cnt.shape[1]):
            for x in range(8):
                h.update(np.ascontiguousarray(rec[l, p, x, :cnt[l, p, x]]).astype(np.uint32).tobytes())
    return h.hexdigest()


def multisets(cnt, rec):
    out = {}
    for l in range(1, 12):
        for p in range(cnt.shape[1]):
            out[l, p] = sorted(tuple(r) for x in range(8) for r in rec[l, p, x, :cnt[l, p, x]].tolist())
    return out


_first = {}


def order_one(shape):
    """order 1 on the shape: its lists of both passes, shared by the other orders' checks"""
    if shape not in _first:
        _first[shape] = run(shape, "1")
    return _first[shape]


def run(shape, order):
    G, H, W, B = shape
    layers = make_main_params(cases.weight_seed(shape), G)
    fc = codec_under(G, H, W, B, layers, LIC360_DC_ORDER=order)
    assert fc.skip_active() == 2
    got = []
    for second in (False, True):
        code, mask = cases.batch(shape, second)
        want = cases.golden_streams(shape, second, code, mask)
        fc.debug_fill(POISON)
        streams = fc.encode(dev(code), dev(mask))
        for i in range(B):
            assert streams[i] == want[i], "image %d, pass %d" % (i, second)
        fc.debug_fill(-POISON)
        out = fc.decode(want, dev(mask)).cpu().numpy()                      # (raises unless err is 0 for every image)
        assert int(fc.err[:B].abs().sum().item()) == 0
        assert np.array_equal(out, code * mask), "pass %d" % second
        got.append(lists_of(fc, shape))
    return got


@pytest.mark.parametrize("order", list(cases.ORDERS), ids=lambda o: "order" + o)
@pytest.mark.parametrize("shape", cases.GPU_SHAPES, ids=cases.shape_id)
def test_every_order_gives_the_oracles_bytes_and_the_same_records(shape, order):
    first = order_one(shape)
    got = first if order == "1" else run(shape, order)
    moved = 0
    for second in (0, 1):
        want, have = multisets(*first[second]), multisets(*got[second])
        assert sum(len(v) for v in want.values()) > 0
        for k in want:
            assert have[k] == want[k], (k, second)
        moved += digest(*got[second]) != digest(*first[second])
    nb, place = cases.ORDERS[order]
    rounds = max(int(c.max()) for c, _ in first) > cases.wgs_of_xcd(0)
    if nb > 1 and rounds:
        assert moved, "a grouped order of lists longer than a round is another order"


@pytest.mark.parametrize("shape", cases.GPU_SHAPES, ids=cases.shape_id)
def test_order_one_is_the_order_of_the_commit_before_the_switch(shape):
    g = np.load(os.path.join(GOLD, "dc_order_parent_lists.npz"))
    first = order_one(shape)
    for second in (0, 1):
        assert digest(*first[second]) == str(g[cases.stream_key(shape, bool(second))]), "pass %d" % second


def test_unset_is_the_default_and_a_wrong_value_is_refused():
    from lic360 import Lic360Error
    shape = cases.GPU_SHAPES[2]
    G, H, W, B = shape
    layers = make_main_params(cases.weight_seed(shape), G)
    code, mask = cases.batch(shape)
    fc = codec_under(G, H, W, B, layers)
    fc.decode(fc.encode(dev(code), dev(mask)), dev(mask))
    fd = codec_under(G, H, W, B, layers, LIC360_DC_ORDER=cases.DEFAULT_ORDER)
    fd.decode(fd.encode(dev(code), dev(mask)), dev(mask))
    assert digest(*lists_of(fc, shape)) == digest(*lists_of(fd, shape))
    for bad in ("3", "0", "16", "4p", "p", ""):
        with pytest.raises(Lic360Error):
            codec_under(G, H, W, B, layers, LIC360_DC_ORDER=bad)


def test_the_balancing_pass_belongs_to_the_codec():
    """LIC360_NOBALANCE is read when a codec is created and is that codec's: a default codec and then, in the same process, one under LIC360_NOBALANCE=1, both
    at order 1 (no placement).  Images 3 and 11 -- the home list of XCD 3 -- are fully masked, so that list starts empty and the balancing pass fills it
    from the others: the default codec holds records away from their home list n % 8, the other codec none; the records are the same multisets and both
    decode the first codec's streams exactly."""
    shape = cases.GPU_SHAPES[0]
    G, H, W, B = shape
    layers = make_main_params(cases.weight_seed(shape), G)
    code, mask = cases.batch(shape)
    mask = mask.copy()
    mask[3] = mask[11] = 0.0
    got = []
    streams = None
    for switches in ({}, {"LIC360_NOBALANCE": 1}):
        fc = codec_under(G, H, W, B, layers, LIC360_DC_ORDER="1", **switches)
        assert fc.skip_active() == 2
        if streams is None:
            streams = fc.encode(dev(code), dev(mask))
        out = fc.decode(streams, dev(mask)).cpu().numpy()                   # (raises unless err is 0 for every image)
        assert int(fc.err[:B].abs().sum().item()) == 0
        assert np.array_equal(out, code * mask)
        cnt, rec = lists_of(fc, shape)
        away = sum(int(((rec[l, p, x, :cnt[l, p, x], 0] >> 10) % 8 != x).sum()) for l in range(1, 12) for p in range(cnt.shape[1]) for x in range(8))
        got.append((multisets(cnt, rec), away, int(cnt[1:].sum())))
    (balanced, moved, n), (plain, stayed, m) = got
    assert moved > 0, "the masks load the XCDs unevenly: the balancing pass of the default codec moves records"
    assert stayed == 0, "without the balancing pass every record is in its home list"
    assert n == m > 0 and balanced == plain
