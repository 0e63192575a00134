"""The decode-order dead-cone lists on latents of 65..128 rows (csrc/need.h, need_kernels.hip, k_cconv4v6lt of csrc/cconv4v6_dc.inc).

A FusedCodec of such a latent builds its decode lists (skip_active() == 2) and runs the hidden and last layers over them: every sample's row window
trimmed to the hull of its live rows, a window of up to 128 rows cut over two or three waves.  Checked on the shapes of tests/dc_tall_cases.py, each
the smallest at which one class of failure can occur, with 1e10 in every activation cell beforehand:
  * bitstreams == the CPU oracle's (the fixture tests/golden/dc_tall_lists.npz), decode of the oracle's bytes == the symbols, for every image of
    the batch -- at (48, 128, 24, 16), where the oracle needs a quarter of a minute per image, images 0..7 (one per XCD list) against the oracle
    and the other eight against a LIC360_NOSKIP codec, whose row-segment kernels existing tests pin to the oracle;
  * the records, decoded with the restatement of tests/dc_tall_cases.py: every live cell of the need maps stored exactly once, no row outside its
    sample's hull, and the records themselves equal to the restated builder's;
  * the decode counters of skip_stats == the cells the restated records store;
  * the 48 x 128 x 256 golden of 1024 x 2048 ERPs inside a batch of 16; the A/B switch LIC360_DC_NOTALL."""
import hashlib
import os
import time

import numpy as np
import pytest

import dc_tall_cases as cases
from util import latent_smooth, make_main_params
from gpu_support import codec_under, dev  # noqa: F401

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POISON = 1.0e10


class Run(object):
    pass


_runs = {}


def run_of(shape):
    """one encode + decode per shape, shared by the tests: oracle bytes, the codec's bytes and symbols, its need maps, records and counters"""
    if shape in _runs:
        return _runs[shape]
    G, H, W, B = shape
    r = Run()
    r.code, r.mask = cases.batch(G, H, W, B, cases.batch_seed(shape))
    layers = make_main_params(cases.weight_seed(shape), G)
    r.want = cases.golden_streams(shape, r.code, r.mask)                    # the CPU oracle's bytes (tools/gen_golden_dc_tall.py)
    n_or = len(r.want)
    if n_or < B:                                                            # the other images: today's row-segment kernels, which existing tests pin to the oracle
        ref = codec_under(G, H, W, B, layers, LIC360_NOSKIP=1)
        assert ref.skip_active() == 0
        rest = ref.encode(dev(r.code), dev(r.mask))
        assert rest[:n_or] == r.want
        r.want = r.want + rest[n_or:]
        del ref
    fc = codec_under(G, H, W, B, layers)
    r.active = fc.skip_active()
    fc.debug_fill(POISON)
    r.streams = fc.encode(dev(r.code), dev(r.mask))
    fc.debug_fill(-POISON)
    fc.skip_stats(True)
    r.out = fc.decode(r.want, dev(r.mask)).cpu().numpy()
    r.dec_stats = fc.skip_stats(False, read=True)[1].astype(np.int64)
    P = H + W + G - 2
    if r.active == 2:
        r.need = fc.debug_lists(0)[0].reshape(B, 12, H, W).astype(np.int64)
        cnt, r.cap = fc.debug_lists(3)
        r.cnt = cnt.reshape(12, P, 8)
        r.rec = fc.debug_lists(4)[0].reshape(12, P, 8, r.cap, 4)
    _runs[shape] = r
    return r


@pytest.mark.parametrize("shape", cases.GPU_SHAPES, ids=cases.shape_id)
def test_tall_codec_skips_in_decode_order_and_matches_the_oracle(shape):
    G, H, W, B = shape
    r = run_of(shape)
    assert r.active == 2
    for i in range(B):
        assert r.streams[i] == r.want[i], "image %d" % i
    assert np.array_equal(r.out, r.code * r.mask)


@pytest.mark.parametrize("shape", cases.LIST_SHAPES, ids=cases.shape_id)
def test_tall_records_cover_the_live_cells_exactly_once(shape):
    G, H, W, B = shape
    r = run_of(shape)
    assert r.active == 2 and r.cap == cases.list_cap(G, B, H)
    need = cases.need_maps(r.mask)
    assert np.array_equal(r.need, need)
    P = H + W + G - 2
    stored = np.zeros((12, 3 * B, G, H, W), np.int32)
    cut = 0
    for p in range(P):
        want = cases.build_records(need, G, H, W, B, p)
        hulls = {}
        for l in range(1, 12):
            got = []
            for x in range(8):
                assert r.cnt[l, p, x] <= r.cap
                for q in r.rec[l, p, x, :r.cnt[l, p, x]].tolist():
                    g0, packed, n, gm = q[0] & 127, (q[0] >> 7) & 7, q[0] >> 10, (q[1] >> 22) & 7
                    assert packed == 4 and gm and g0 % 3 == 0 and n < 3 * B, "every record of a tall latent is packed"
                    if g0 not in hulls:
                        hulls[g0] = cases.block_hulls(need, G, H, W, p, g0)
                    lo, hi = hulls[g0][0][:, l], hulls[g0][1][:, l]
                    pieces, last = [], None
                    for w in (q[1] & ~(7 << 22), q[2], q[3]):
                        if not w >> 21:
                            continue
                        k, slo, shi, a0 = cases.piece_fields(w)
                        smp = n + 8 * k
                        assert smp // B == n // B, "one net per record: its waves' weights are uniform"
                        assert lo[smp % B] <= slo <= shi <= hi[smp % B], "no row outside the sample's hull"
                        assert (a0 - slo) % 4 == 0 and a0 + shi - slo <= (63 if shi == H - 1 else 61) and (a0 >= 2 or slo == 0)
                        if last is not None:
                            assert a0 >= ((last + 4) // 4 + 1) * 4
                        last = a0 + shi - slo
                        cut += shi < hi[smp % B]
                        pieces.append((smp, slo, shi, a0))
                        for g, s, ya, yb in cases.stored_rows(G, H, W, p, g0, gm, slo, shi):
                            ys = np.arange(ya, yb + 1)
                            stored[l, smp, g, ys, s - ys] += 1
                    assert pieces
                    got.append((n % 8, g0, n, gm, pieces))                  # (n % 8: the record's home list; the balancing pass may have moved it)
            assert sorted(got) == sorted(want[l]), (l, p)
    assert (cut > 0) == (shape in cases.CUT_SHAPES)
    assert stored.max() <= 1
    live = np.arange(G)[None, None, :, None, None] <= need.transpose(1, 0, 2, 3)[:, :, None]      # [12, B, G, H, W]
    for net in range(3):
        assert not (live[1:] & (stored[1:, net * B:(net + 1) * B] == 0)).any()


def restated_counts(mask, shape):
    """[12, 64] cells per (layer, group) that the restated records store"""
    G, H, W, B = shape
    want = np.zeros((12, 64), np.int64)
    need = cases.need_maps(mask)
    for p in range(H + W + G - 2):
        for l, recs in cases.build_records(need, G, H, W, B, p, nets=(0,)).items():
            for (_x, g0, _n, gm, pieces) in recs:
                for (_smp, slo, shi, _a0) in pieces:
                    for g, _s, ya, yb in cases.stored_rows(G, H, W, p, g0, gm, slo, shi):
                        want[l, g] += 3 * (yb - ya + 1)                     # (the three nets' records differ in their samples only)
    return want


@pytest.mark.parametrize("shape", cases.GPU_SHAPES, ids=cases.shape_id)
def test_decode_counters_equal_the_restated_hull_cells(shape):
    G, H, W, B = shape
    r = run_of(shape)
    assert r.active == 2
    want = restated_counts(r.mask, shape)
    assert want[1:].sum() > 0 and np.array_equal(r.dec_stats, want)
    full = 3 * B * H * W                                                    # cells of a (layer, group) without the skip
    assert (want[1:, :G] <= full).all() and want[1:, :G].sum() < 11 * G * full, "something was skipped"


def test_full_size_tall_golden_with_poisoned_buffers():
    """cfg5s (oracle bytes of a 48 x 128 x 256 latent with SURVEY 8d's smooth mask: 1024 x 2048 ERPs) as images 0 and 9 of a batch of 16 -- the home
    lists of XCDs 0 and 1, second sample of the latter: encode == the oracle's bytes, decode of them == the symbols, in list mode, 1e10 in every
    activation cell beforehand.  Time: the bench record's config 5 (48 such images, both streams, 47.2 Mpixel/s = 2.1 s) puts one encode + decode of
    16 at under a second; creating the codec (25 GB of activation buffers to clear) and the 100 MB host arrays take about as long again."""
    g = np.load(os.path.join(GOLD, "full_cfg5s.npz"))
    G, H, W = int(g["G"]), int(g["H"]), int(g["W"])
    assert (G, H, W) == (48, 128, 256)
    code, mask, _ = latent_smooth(np.random.default_rng(int(g["latent_seed"])), G, H, W)
    assert hashlib.sha256(code.tobytes()).hexdigest() == str(g["code_sha256"]) and hashlib.sha256(mask.tobytes()).hexdigest() == str(g["mask_sha256"])
    layers = make_main_params(int(g["weight_seed"]), G)
    c14, m14 = cases.batch(G, H, W, 14, 555)
    code16 = np.concatenate([code, c14[:8], code, c14[8:]], 0)
    mask16 = np.concatenate([mask, m14[:8], mask, m14[8:]], 0)
    fc = codec_under(G, H, W, 16, layers)
    assert fc.skip_active() == 2
    fc.debug_fill(POISON)
    t0 = time.time()
    streams = fc.encode(dev(code16), dev(mask16))
    gold = g["bytes"].tobytes()
    assert streams[0] == gold and streams[9] == gold
    fc.debug_fill(-POISON)
    out = fc.decode([gold] + streams[1:9] + [gold] + streams[10:], dev(mask16)).cpu().numpy()
    print("encode + decode of 16 latents of 48 x 128 x 256: %.2f s" % (time.time() - t0))
    assert np.array_equal(out, code16 * mask16)


def test_the_switch_keeps_tall_latents_on_the_row_segment_kernels():
    shape = cases.GPU_SHAPES[0]
    G, H, W, B = shape
    r = run_of(shape)
    layers = make_main_params(cases.weight_seed(shape), G)
    fc = codec_under(G, H, W, B, layers, LIC360_DC_NOTALL=1)
    assert fc.skip_active() == 1
    assert fc.encode(dev(r.code), dev(r.mask)) == r.want
    assert np.array_equal(fc.decode(r.want, dev(r.mask)).cpu().numpy(), r.code * r.mask)
    short = codec_under(G, 64, W, B, layers, LIC360_DC_NOTALL=1)
    assert short.skip_active() == 2, "the switch is about latents taller than 64 rows only"
    assert codec_under(G, 130, W, B, layers).skip_active() == 1, "past 128 rows: row segments, as before"
