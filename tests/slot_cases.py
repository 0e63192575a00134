"""Bitstream slots at their edges: cases, reference and checker (numpy + the CPU oracle only; no torch, no GPU).

Every stream of both fused codecs lives in a slot of `cap` bytes at bytes + image * cap (csrc/codec_fused.hip).  The slot contract
(DESIGN.md 4.4):
  * an encoder writes bytes [0, min(L, cap)) of its slot and nothing else, reports nbytes = L -- the TRUE length, also when L > cap --
    and sets error bit 16 exactly when L > cap;
  * a decoder reads nbytes clamped to cap (error bit 32 flags the clamp) and treats everything past it as zeros, whatever the slot holds
    there; the pitch of the slots is the caller's, any multiple of 4.

The reference is the CPU oracle's coder (oracle.Encoder / Decoder, pinned to the reference project's coder by tests/test_oracle_ac.py):
the true stream and its true length L always come from it, never from the code under test.

Raw cases (tables [n, ncode + 1] int32, labels, mask or None).  A prefix scan over the oracle picks the stream lengths that pin the
states of the device sink DevBitSink (64 big-endian words per 256-byte window):
  * L % 256 == 0: the terminating 1 bit itself fills the window, the flush empties it, finish() runs with wpos == 0;
  * L % 256 in {1, 2, 3}: a tail of 1, 2, 3 bytes in the first word of a fresh window; 4: one whole word and no tail;
  * L % 256 in {252, 253, 254, 255}: the last word of a window whole (252) and as a tail of 1, 2, 3 bytes;
  * L < 4 (every symbol masked: the lone terminator byte 0x80) and 4 < L < 8;
  * underflow: 1199 times symbol 1 of [0, 32767, 32769, 40000, ...] keeps low = 01.., high = 10.. (two underflow bits per symbol), one
    closing symbol on a uniform table resolves them: L = 2249 with a constant run of 2247 bytes, i.e. one put_run call that spans
    8 windows.  The bit of the run is the complement of the closing symbol's first bit: closing symbol 1 gives a run of 0xFF, the
    mirrored table closed by symbol 6 a run of 0x00;
  * freq1: 4000 frequency-1 symbols of [0, 1, ..., 7, 65536], 16 bits each.  MEASURED on the oracle: 8001 bytes = 2.00025 bytes per
    symbol, the worst case of this coder (16-bit tables, frequency >= 1: at most 16 bits per symbol + the terminator byte); the default
    slot of 1 byte per symbol (lic360_fused.py) does not hold it;
  * one stream of 49-symbol tables (the importance-map decoder's path).

Slot capacities of a case (all multiples of 4): 4; the largest multiple of 4 below L; L rounded up to 4 (exact fit); that plus 4; 256
and 260 where L > 260; one roomy value.
"""
import collections
import functools

import numpy as np

import oracle as orc

UNIFORM = np.arange(9, dtype=np.int32) * 8192
STRADDLE = np.array([0, 32767, 32769, 40000, 45000, 50000, 55000, 60000, 65536], np.int32)
STRADDLE_MIRROR = (65536 - STRADDLE[::-1]).astype(np.int32)         # [0, 5536, ..., 25536, 32767, 32769, 65536]: symbol 6 straddles the middle
FREQ1 = np.array([0, 1, 2, 3, 4, 5, 6, 7, 65536], np.int32)
RESIDUES = (0, 1, 2, 3, 4, 252, 253, 254, 255)
FREQ1_BYTES, FREQ1_SYMBOLS = 8001, 4000                              # measured on the oracle (test_slot_cases_cpu.py asserts it)

Case = collections.namedtuple("Case", "name tables ncode labels mask stream")
Case.L = property(lambda c: len(c.stream))
Case.n = property(lambda c: len(c.labels))


def oracle_stream(tables, ncode, labels, mask=None):
    e = orc.Encoder()
    e.encode(tables, ncode, labels, mask, len(labels))
    return e.finish()


def oracle_decode(stream, tables, ncode, mask, n):
    """the symbols the oracle reads back (0 where masked)"""
    d = orc.Decoder(stream)
    out = d.decode(tables, ncode, mask, n, 0.0)[:n]
    d.close()
    return out.astype(np.int32)


def keep_of(case):
    return np.ones(case.n, bool) if case.mask is None else case.mask > 0.5


def _case(name, tables, ncode, labels, mask=None):
    tables = np.ascontiguousarray(tables, np.int32)
    labels = np.ascontiguousarray(labels, np.int32)
    mask = None if mask is None else np.ascontiguousarray(mask, np.float32)
    return Case(name, tables, ncode, labels, mask, oracle_stream(tables, ncode, labels, mask))


def _random_tables(rng, n, ncode):
    """strictly increasing tables that total 65536, inner entries anywhere in 1..65535"""
    inner = np.sort(np.stack([rng.choice(np.arange(1, 65536), ncode - 1, replace=False) for _ in range(n)]), 1)
    return np.concatenate([np.zeros((n, 1), np.int64), inner, np.full((n, 1), 65536)], 1).astype(np.int32)


def _prefix_lengths(tables, ncode, labels, mask, lo, hi):
    """{prefix length: L} of the stream's prefixes lo..hi"""
    return {n: len(oracle_stream(tables[:n], ncode, labels[:n], None if mask is None else mask[:n])) for n in range(lo, hi + 1)}


@functools.lru_cache(maxsize=None)
def raw_cases():
    """the list of Case (built once; nothing in it may be modified)"""
    cases = []
    # the residues of L % 256, alternately from an unmasked and from a masked stream of random tables
    rng = np.random.default_rng(20240)
    n = 3000
    tab, lab = _random_tables(rng, n, 8), rng.integers(0, 8, n)
    masks = (None, (rng.random(n) > 0.3).astype(np.float32))
    scans = [_prefix_lengths(tab, 8, lab, m, 600, n) for m in masks]
    for k, res in enumerate(RESIDUES):
        for which in (k % 2, 1 - k % 2):
            hits = [p for p, L in scans[which].items() if L % 256 == res and L > 256]
            if hits:
                break
        p, m = hits[0], masks[which]
        cases.append(_case("res%d%s" % (res, "m" if m is not None else ""), tab[:p], 8, lab[:p], None if m is None else m[:p]))
    # L < 4: everything masked; 4 < L < 8: the first prefix that long
    cases.append(_case("allmasked", tab[:100], 8, lab[:100], np.zeros(100, np.float32)))
    p = next(p for p in range(1, 64) if 4 < len(oracle_stream(tab[:p], 8, lab[:p])) < 8)
    cases.append(_case("short", tab[:p], 8, lab[:p]))
    # one underflow run over 8 windows, of either bit
    for name, T, sym, last in (("underflow_ff", STRADDLE, 1, 1), ("underflow_00", STRADDLE_MIRROR, 6, 6)):
        t = np.tile(T, (1200, 1))
        t[-1] = UNIFORM
        l = np.full(1200, sym)
        l[-1] = last
        cases.append(_case(name, t, 8, l))
    # frequency-1 symbols only
    cases.append(_case("freq1", np.tile(FREQ1, (FREQ1_SYMBOLS, 1)), 8, np.random.default_rng(1).integers(0, 7, FREQ1_SYMBOLS)))
    # 49 symbols: the first prefix past one window whose tail is 3 bytes
    rng = np.random.default_rng(20249)
    tab49, lab49 = _random_tables(rng, 700, 49), rng.integers(0, 49, 700)
    p = next(p for p, L in _prefix_lengths(tab49, 49, lab49, None, 400, 700).items() if L > 260 and L % 4 == 3)
    cases.append(_case("rand49", tab49[:p], 49, lab49[:p]))
    return tuple(cases)


def constant_run(stream):
    """(length, byte value) of the longest run of equal bytes"""
    a = np.frombuffer(stream, np.uint8)
    edges = np.concatenate([[0], np.flatnonzero(np.diff(a) != 0) + 1, [len(a)]])
    k = int(np.argmax(np.diff(edges)))
    return int(edges[k + 1] - edges[k]), int(a[edges[k]])


def up4(n):
    return (n + 3) // 4 * 4


def capacities(L):
    """the slot capacities a stream of L bytes is encoded at: {name: cap}"""
    caps = {"four": 4, "below": (L - 1) // 4 * 4, "fit": up4(L), "fit+4": up4(L) + 4, "roomy": up4(L) + 1024}
    if L > 260:
        caps.update(window=256, window4=260)
    return {k: v for k, v in caps.items() if v >= 4}


# ---------------------------------------------------------------------------------------------------- layout and checker
def canary(n, start=0):
    """bytes start .. start + n of the canary pattern: never 0x00 or 0xFF (what padding and underflow runs write), never two equal
    neighbours"""
    k = np.arange(start, start + n, dtype=np.int64)
    return (1 + (131 * k + 17 * (k >> 8)) % 254).astype(np.uint8)


class Layout(object):
    """slots of caps[i] bytes, back to back from byte `front` of an allocation of `size` bytes; written[i]: the bytes of slot i that an
    encoder may have written so far -- the longest stream checked or expected there, cut at the capacity"""

    def __init__(self, caps, front, size):
        self.caps, self.front, self.size = list(caps), front, size
        self.offsets = [front + int(sum(self.caps[:i])) for i in range(len(self.caps))]
        self.end = front + int(sum(self.caps))
        self.written = [0] * len(self.caps)

    def expect(self, i, L):
        self.written[i] = max(self.written[i], min(int(L), self.caps[i]))

    def slot(self, buf, i):
        return buf[self.offsets[i]:self.offsets[i] + self.caps[i]]


def slot_layout(caps_or_cap, n_slots=None, max_len=0):
    """-> (flat uint8 buffer filled with the canary, Layout): the slots (n_slots of one capacity, or one per entry of a list) lie back to
    back at a 4-byte aligned offset behind a guard of 256 bytes; the guard after the last slot is max_len rounded up to 256, plus 256 --
    an encoder with no capacity check at all, writing a stream of max_len bytes (in whole 256-byte windows) into any slot, stays inside
    the allocation."""
    caps = [int(caps_or_cap)] * n_slots if np.isscalar(caps_or_cap) else [int(c) for c in caps_or_cap]
    assert caps and all(c > 0 and c % 4 == 0 for c in caps)
    front = 256
    back = (int(max_len) + 255) // 256 * 256 + 256
    lay = Layout(caps, front, front + sum(caps) + back)
    return canary(lay.size), lay


def lay_stream(buf, lay, i, stream):
    """what a correct encoder leaves of `stream` in slot i of buf -> (nbytes, err)"""
    a = np.frombuffer(stream, np.uint8)
    w = min(len(a), lay.caps[i])
    buf[lay.offsets[i]:lay.offsets[i] + w] = a[:w]
    return len(a), (16 if len(a) > lay.caps[i] else 0)


def check_slot(buffer_after, lay, i, want_stream, nbytes, err):
    """asserts the slot contract for slot i of the allocation `buffer_after` (flat uint8, as slot_layout made it and an encoder left it)"""
    buf = np.asarray(buffer_after)
    assert buf.dtype == np.uint8 and buf.shape == (lay.size,)
    want = np.frombuffer(want_stream, np.uint8)
    L, cap, off = len(want), lay.caps[i], lay.offsets[i]
    w = min(L, cap)
    lay.expect(i, L)
    assert int(nbytes) == L, "slot %d: nbytes %d, the stream has %d bytes (cap %d)" % (i, int(nbytes), L, cap)
    assert bool(int(err) & 16) == (L > cap), "slot %d: error %d, length %d, cap %d" % (i, int(err), L, cap)
    assert int(err) & ~16 == 0, "slot %d: error %d" % (i, int(err))
    bad = np.flatnonzero(buf[off:off + w] != want[:w])
    assert len(bad) == 0, "slot %d: %d of the first %d bytes differ, first at %d" % (i, len(bad), w, bad[0])
    clean = np.ones(lay.size, bool)                                   # every byte no encoder may have touched
    for j in range(len(lay.caps)):
        clean[lay.offsets[j]:lay.offsets[j] + lay.written[j]] = False
    bad = np.flatnonzero((buf != canary(lay.size)) & clean)
    assert len(bad) == 0, "%d bytes written outside the streams (slot %d: offset %d, cap %d, length %d), first at %d, last at %d" % (
        len(bad), i, off, cap, L, bad[0], bad[-1])


# ---------------------------------------------------------------------------------------------------- models of broken sinks
BROKEN = ("word_past_cap", "partial_word_dropped", "tail_reversed", "nbytes_clamped", "bit16_missing", "window_skipped", "final_word_whole")


def broken_sink(kind, buf, lay, i, stream):
    """a sink with one defect lays `stream` into slot i of buf -> (nbytes, err); where the defect does not show at this length and
    capacity the result is the correct one"""
    a = np.frombuffer(stream, np.uint8)
    L, cap, off = len(a), lay.caps[i], lay.offsets[i]
    nbytes, err = lay_stream(buf, lay, i, stream)
    if kind == "word_past_cap" and L > cap:                           # the guard is off by one word
        buf[off + cap:off + min(L, cap + 4)] = a[cap:cap + 4]
    elif kind == "partial_word_dropped" and L % 4 and L <= cap:
        buf[off + L - L % 4:off + L] = canary(L % 4, off + L - L % 4)
    elif kind == "tail_reversed" and L % 4 and L <= cap:
        buf[off + L - L % 4:off + L] = a[L - L % 4:][::-1]
    elif kind == "nbytes_clamped":
        nbytes = min(L, cap)
    elif kind == "bit16_missing":
        err = 0
    elif kind == "window_skipped" and L % 256 == 0 and 0 < L <= cap:   # the window that the terminator filled never leaves the registers
        buf[off + L - 256:off + L] = canary(256, off + L - 256)
    elif kind == "final_word_whole" and L % 4 and L < cap:            # the zero padding of the last word goes out with it
        buf[off + L:off + up4(L)] = 0
    return nbytes, err
