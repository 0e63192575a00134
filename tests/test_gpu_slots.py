"""The bitstream slots at their edges on every coder path (cases, reference and checker: tests/slot_cases.py; the contract: DESIGN.md 4.4).

Every encode of this file targets a view into a slot_layout allocation -- canary-filled guards wide enough for an encoder with no
capacity check at all -- so no outcome depends on memory the test did not allocate; every true stream and length is the CPU oracle's.

  * raw hooks lic360_devcoder_encode / _decode (k_ac_encode's DevBitSink; k_dec_init, k_dec_plane and k_imp_dec_plane's DevBits): every case
    at every capacity; decodes from slots whose bytes past the stream hold 0xFF;
  * FusedCodec with the coder on the device and on host threads, FusedImpCodec: two of the images overflow their slots, the exact fit, a
    decode straight from the slots an encode filled (clamped lengths are flagged with bit 32), shorter streams encoded over longer ones
    with no clearing in between, and one codec decoding from slots of four pitches in turn.

Latent shape (G, H, W) = (12, 8, 12): the oracle's streams of (6, 8, 12) stay under 260 bytes (232 at a full mask; (8, 6, 10): 166), here the
four images of the overflow batch have 321, 287, 1 and 151 bytes -- more than one 256-byte window in the longest."""
import numpy as np
import pytest
import torch

import ref_codec as rc
import slot_cases as sc
from util import latent
from gpu_support import dev, lic  # noqa: F401

pytestmark = pytest.mark.gpu
CASES = sc.raw_cases()
G, H, W, B = 12, 8, 12, 4


def i32(n=1, v=0):
    return torch.full((n,), v, dtype=torch.int32, device="cuda:0")


# ---------------------------------------------------------------------------------------------------- raw hooks
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_device_encoder_at_every_capacity(lic, case):
    """k_ac_encode into slots of every capacity class, one after the other in one allocation (the slots behind the one being written are
    still all canary, so a spill shows): nbytes is the true length, bit 16 exactly on overflow, the oracle's bytes up to the capacity and not
    one byte elsewhere."""
    caps = sorted(set(sc.capacities(case.L).values()))
    buf, lay = sc.slot_layout(caps, None, case.L)
    d = dev(buf)
    t, l = dev(case.tables), dev(case.labels)
    m = None if case.mask is None else dev(case.mask)
    for i, cap in enumerate(caps):
        nb, er = i32(1, -7), i32(1, -7)
        lic._chk(lic._lib.lic360_devcoder_encode(lic._stream(0), lic._p(t), case.ncode, lic._p(l), lic._p(m), case.n,
                                                 lic._p(d[lay.offsets[i]:]), cap, lic._p(nb), lic._p(er)))
        sc.check_slot(d.cpu().numpy(), lay, i, case.stream, nb.item(), er.item())


def _hook_decode(lic, case, slot, cap, nbytes, chunk):
    t = dev(case.tables)
    m = None if case.mask is None else dev(case.mask)
    out = torch.full((case.n,), -1.0, dtype=torch.float32, device="cuda:0")
    nb, er = i32(1, nbytes), i32(1, -7)
    lic._chk(lic._lib.lic360_devcoder_decode(lic._stream(0), lic._p(t), case.ncode, lic._p(m), case.n, chunk, lic._p(slot), cap,
                                             lic._p(nb), lic._p(out), lic._p(er)))
    return out.cpu().numpy(), int(er.item())


def _ff_slot(stream, cap, keep=None):
    """a slot of cap bytes behind and in front of a window of 0xFF: the stream's first `keep` bytes, 0xFF after them"""
    a = np.full(256 + cap + 512, 0xFF, np.uint8)
    s = np.frombuffer(stream, np.uint8)[:keep]
    a[256:256 + len(s)] = s
    return dev(a)[256:]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_device_decoder_ignores_what_follows_the_stream(lic, case):
    """the oracle's stream from a slot that fits it exactly and from a roomy one, 0xFF in every byte past the stream (in the slot and behind
    it), in chunks of 64 symbols and in one chunk: every coded symbol comes back, masked ones are 0, no error.  The reference's finish
    writes a single 1, so the last symbols are right only if what follows the stream reads as zeros."""
    keep = sc.keep_of(case)
    for cap in (sc.up4(case.L), sc.up4(case.L) + 1024):
        slot = _ff_slot(case.stream, cap)
        for chunk in (64, case.n + 1):
            got, err = _hook_decode(lic, case, slot, cap, case.L, chunk)
            assert err == 0, (cap, chunk, err)
            assert np.array_equal(got[keep].astype(np.int32), case.labels[keep]) and np.all(got[~keep] == 0), (cap, chunk)


@pytest.mark.parametrize("case", [c for c in CASES if c.L > 4], ids=[c.name for c in CASES if c.L > 4])
def test_device_decoder_flags_a_length_above_the_capacity(lic, case):
    """what an overflowed encode leaves: the slot holds the stream's first cap bytes, nbytes the true length -- the decoder clamps and says so"""
    cap = (case.L - 1) // 4 * 4
    got, err = _hook_decode(lic, case, _ff_slot(case.stream, cap, cap), cap, case.L, 64)
    assert err & 32
    assert got.min() >= 0 and got.max() <= case.ncode - 1


# ---------------------------------------------------------------------------------------------------- the fused codecs
def _codec(coder, cap_bytes):
    from lic360_fused import FusedCodec
    fc = FusedCodec(G, H, W, max_batch=B, cap_bytes=cap_bytes)
    fc.load_layers(rc.make_main_params(2051, G))
    fc.set_coder(coder)
    return fc


def _slots(fc, max_len):
    """fc.bytes <- a [maxB, cap] view into a slot_layout allocation -> (the whole allocation on the device, its Layout)"""
    buf, lay = sc.slot_layout(fc.cap, fc.maxB, max_len)
    d = dev(buf)
    fc.bytes = d[lay.front:lay.end].view(fc.maxB, fc.cap)
    assert fc.bytes.data_ptr() == d.data_ptr() + lay.front and fc.bytes.data_ptr() % 4 == 0
    return d, lay


def _check_all(d, lay, fc, streams):
    host, nb, er = d.cpu().numpy(), fc.nbytes.cpu().numpy(), fc.err.cpu().numpy()
    for i, s in enumerate(streams):
        lay.expect(i, len(s))
    for i, s in enumerate(streams):
        sc.check_slot(host, lay, i, s, nb[i], er[i])


@pytest.fixture(scope="module")
def latents():
    """two batches of four latents with the oracle's streams: `mixed` (mask densities 0.82, 0.74, 0 and 0.40: 321, 287, 1 and 151 bytes) and
    `long` (every mask full: 410, 415, 400 and 414 bytes)"""
    layers = rc.make_main_params(2051, G)
    rng = np.random.default_rng(51)
    out = {}
    for name, dens in (("mixed", (0.9, 0.7, 0.0, 0.45)), ("long", (1.0, 1.0, 1.0, 1.0))):
        items = [latent(rng, G, H, W, mean=m) for m in dens]
        code = np.concatenate([it[0] for it in items], 0)
        mask = np.concatenate([it[1] for it in items], 0)
        for i, m in enumerate(dens):
            if m in (0.0, 1.0):
                mask[i] = m
        streams = [rc.encode_main(code[i:i + 1], mask[i:i + 1], layers, G) for i in range(B)]
        out[name] = (code, mask, streams)
    assert max(len(s) for s in out["mixed"][2]) > 260 and out["mixed"][2][2] == b"\x80"
    return out


def _two_overflow(lengths):
    """the capacity at which exactly the two longest of the streams overflow"""
    s = sorted(lengths)
    cap = sc.up4(s[-3])
    assert s[-3] <= cap < s[-2]
    return cap


@pytest.mark.parametrize("coder", ["device", "host"])
def test_fused_codec_overflow_is_reported_never_written(coder, latents):
    from lic360 import Lic360Error
    code, mask, streams = latents["mixed"]
    lens = np.array([len(s) for s in streams])
    fc = _codec(coder, _two_overflow(lens))
    over = lens > fc.cap
    assert over.sum() == 2
    d, lay = _slots(fc, lens.max())
    fc.encode_async(dev(code), dev(mask))
    _check_all(d, lay, fc, streams)
    assert np.array_equal((fc.err.cpu().numpy() & 16) != 0, over) and np.array_equal(fc.nbytes.cpu().numpy(), lens)
    # decode straight from those slots: the streams that fit decode, the clamped lengths are flagged
    out = fc.decode_async(dev(mask)).cpu().numpy()
    err = fc.err.cpu().numpy()
    assert np.array_equal((err & 32) != 0, over), err
    assert np.all(err[~over] == 0), err
    assert np.array_equal(out[~over], (code * mask)[~over])
    with pytest.raises(Lic360Error):
        fc.encode(dev(code), dev(mask))
    _check_all(d, lay, fc, streams)


@pytest.mark.parametrize("coder", ["device", "host"])
def test_fused_codec_exact_fit_of_the_longest_stream(coder, latents):
    code, mask, streams = latents["mixed"]
    longest = max(len(s) for s in streams)
    fc = _codec(coder, sc.up4(longest))
    assert fc.cap - 4 < longest <= fc.cap
    d, lay = _slots(fc, longest)
    fc.encode_async(dev(code), dev(mask))
    _check_all(d, lay, fc, streams)
    assert np.array_equal(fc.decode_async(dev(mask)).cpu().numpy(), code * mask)
    assert not fc.err.cpu().numpy().any()


@pytest.mark.parametrize("coder", ["device", "host"])
def test_fused_codec_decodes_short_streams_over_stale_tails(coder, latents):
    """the production order: encode, encode shorter streams into the same slots, decode from them -- what the first encode left behind a
    second stream is not part of it"""
    code1, mask1, first = latents["long"]
    code2, mask2, second = latents["mixed"]
    assert all(len(b) < len(a) for a, b in zip(first, second)), ([len(s) for s in first], [len(s) for s in second])
    fc = _codec(coder, sc.up4(max(len(s) for s in first)) + 4)
    d, lay = _slots(fc, fc.cap)
    fc.encode_async(dev(code1), dev(mask1))
    _check_all(d, lay, fc, first)
    fc.encode_async(dev(code2), dev(mask2))
    _check_all(d, lay, fc, second)
    host = d.cpu().numpy()
    for i in range(B):                                                 # the tails ARE stale: the first stream's bytes, not zeros
        a = np.frombuffer(first[i], np.uint8)
        assert np.array_equal(lay.slot(host, i)[len(second[i]):len(a)], a[len(second[i]):]), i
    assert np.array_equal(fc.decode_async(dev(mask2)).cpu().numpy(), code2 * mask2)
    assert not fc.err.cpu().numpy().any()


def _staged(streams, pitch):
    """[B, pitch] device slots holding the streams, 0xFF everywhere else"""
    a = np.full((len(streams), pitch), 0xFF, np.uint8)
    for i, s in enumerate(streams):
        a[i, :len(s)] = np.frombuffer(s, np.uint8)
    return dev(a)


@pytest.mark.parametrize("coder", ["device", "host"])
def test_fused_codec_decodes_from_slots_of_any_pitch(coder, latents):
    """one codec, four decodes: its own slots, slots three times as wide, its own again, slots half as wide (the host leg grows its pinned
    slots for the second and copies between two pitches for the third and fourth)"""
    code, mask, streams = latents["mixed"]
    longest = max(len(s) for s in streams)
    fc = _codec(coder, 2 * (sc.up4(longest) + 4))
    nb = dev(np.array([len(s) for s in streams], np.int32))
    fc.nbytes.copy_(nb)
    fc.bytes.copy_(_staged(streams, fc.cap))
    m = dev(mask)
    for pitch in (None, 3 * fc.cap, None, fc.cap // 2):
        assert pitch is None or (pitch % 4 == 0 and pitch >= longest)
        fc.code_out.fill_(-3.0)
        out = fc.decode_async(m) if pitch is None else fc.decode_async(m, bytes_dev=_staged(streams, pitch), nbytes_dev=nb)
        assert np.array_equal(out.cpu().numpy(), code * mask), pitch
        assert not fc.err.cpu().numpy().any(), pitch


# ---------------------------------------------------------------------------------------------------- the importance-map codec
IH, IW, IB, CPG, NSYM = 8, 12, 3, 8, 49


@pytest.fixture(scope="module")
def maps():
    """a pool of twelve random level maps under the weights of test_fused_importance_codec_matches_oracle's first case, by the length of the
    oracle's stream (68 .. 74 bytes: every cell of a map is coded, so the lengths differ by a few bytes only) -> the weights and three
    batches (levels, streams): the three longest, the three shortest, and the shortest with the two longest"""
    layers = rc.make_imp_params(4031, CPG, NSYM)
    levels = np.random.default_rng(31).integers(0, NSYM, (12, 1, IH, IW)).astype(np.float32)
    streams = rc.encode_imp_batch(levels, layers, NSYM)
    order = np.argsort([len(s) for s in streams], kind="stable")
    pick = lambda idx: (np.ascontiguousarray(levels[idx]), [streams[i] for i in idx])
    return layers, pick(order[-IB:]), pick(order[:IB]), pick(order[[-1, 0, -2]])


def _imp_codec(layers, cap_bytes):
    from lic360_fused import FusedImpCodec
    fc = FusedImpCodec(IH, IW, max_batch=IB, hidden_channels=CPG, nsym=NSYM, cap_bytes=cap_bytes)
    fc.load_layers(layers)
    return fc


def test_fused_importance_codec_overflow_is_reported_never_written(maps):
    from lic360 import Lic360Error
    layers, _, _, (levels, streams) = maps
    lens = np.array([len(s) for s in streams])
    fc = _imp_codec(layers, _two_overflow(lens))
    over = lens > fc.cap
    assert over.sum() == 2
    d, lay = _slots(fc, lens.max())
    fc.encode_async(dev(levels))
    _check_all(d, lay, fc, streams)
    out = fc.decode_async(IB).cpu().numpy()
    err = fc.err.cpu().numpy()
    assert np.array_equal((err & 32) != 0, over) and np.all(err[~over] == 0), err
    assert np.array_equal(out[~over], levels[~over])
    with pytest.raises(Lic360Error):
        fc.encode(dev(levels))
    _check_all(d, lay, fc, streams)


def test_fused_importance_codec_decodes_short_streams_over_stale_tails(maps):
    layers, (levels1, first), (levels2, second), _ = maps
    assert all(len(b) < len(a) for a, b in zip(first, second)), ([len(s) for s in first], [len(s) for s in second])
    fc = _imp_codec(layers, sc.up4(max(len(s) for s in first)) + 4)
    d, lay = _slots(fc, fc.cap)
    fc.encode_async(dev(levels1))
    _check_all(d, lay, fc, first)
    fc.encode_async(dev(levels2))
    _check_all(d, lay, fc, second)
    host = d.cpu().numpy()
    for i in range(IB):
        a = np.frombuffer(first[i], np.uint8)
        assert np.array_equal(lay.slot(host, i)[len(second[i]):len(a)], a[len(second[i]):]), i
    assert np.array_equal(fc.decode_async(IB).cpu().numpy(), levels2)
    assert not fc.err.cpu().numpy().any()
