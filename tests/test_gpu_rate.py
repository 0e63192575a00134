"""Rate estimation on the GPU (csrc/rate_kernels.hip, k_rate_sum): the integer code length of the fused codecs' records equals the Python-integer
restatement over the oracle's tables (tests/rate_cases.py) -- bit for bit, whatever the order of the reduction -- per image, per group and per
latitude row; estimating disturbs nothing; and the real streams lie within the slack measured on the CPU."""
import ctypes as C

import pytest
import torch

import rate_cases as rt
from gpu_support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = -0x0123456789ABCDEF


def _sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int64, device="cuda:0")


@pytest.mark.parametrize("ncode", rt.RAW_NCODE)
@pytest.mark.parametrize("n,B", rt.RAW_CASES)
def test_rate_records_on_raw_tables(n, B, ncode):
    """lic360_rate_records: raw tables through the coder's record construction and k_rate_sum; f = 1, f = 65536, uncoded and random symbols in every case
    (one symbol: one kind), sizes around a wave and just past a workgroup's chunk, odd n: image bases on 8- and 16-byte boundaries in turn"""
    import lic360
    from lic360 import _lib, _p, _stream
    tabs, labels, mask = rt.raw_case(n, B, ncode)
    want_q, want_n = rt.raw_expected(tabs, labels, mask, n, B)
    q32, nsym = _sentinel(B), _sentinel(B)
    d_tabs, d_labels, d_mask = dev(tabs), dev(labels), dev(mask)
    lic360._chk(_lib.lic360_rate_records(_stream(0), _p(d_tabs), ncode, _p(d_labels), _p(d_mask), C.c_long(n), B, _p(q32), _p(nsym)))
    assert q32.cpu().tolist() == want_q
    assert nsym.cpu().tolist() == want_n


def _raw_breakdowns(fc, b):
    """the integer outputs of lic360_codec_rate_last, sentinel-filled before the call -> q32 [b], symbols [b], group [b][G], row [b][H] as Python ints"""
    import lic360
    from lic360 import _lib, _p, _stream
    q32, nsym, group, row = _sentinel(b), _sentinel(b), _sentinel(b, fc.G), _sentinel(b, fc.H)
    lic360._chk(_lib.lic360_codec_rate_last(_stream(0), fc._h, b, _p(q32), _p(nsym), _p(group), _p(row)))
    torch.cuda.synchronize()
    return q32.cpu().tolist(), nsym.cpu().tolist(), group.cpu().tolist(), row.cpu().tolist()


def _check_estimate(fc, case):
    """FusedCodec.estimate of the case on fc: every field against the restatement for the held images, the breakdowns' sums for all"""
    G, H, W, B, seed, held = case
    code, mask, _ = rt.main_case(G, H, W, B, seed)
    want = rt.main_expected(*case)
    est = fc.estimate(dev(code), dev(mask), groups=True, rows=True)
    q32, nsym, group, row = _raw_breakdowns(fc, B)
    assert est.q32.dtype == torch.int64 and est.symbols.dtype == torch.int64 and est.bits.dtype == torch.float64
    assert est.q32.tolist() == q32 and est.symbols.tolist() == nsym
    assert tuple(est.group_bits.shape) == (B, G) and tuple(est.row_bits.shape) == (B, H)
    # the float fields are exact multiples of 2^-32 (the cases' sums are far below 2^53)
    assert (est.bits * 2.0 ** 32).tolist() == [float(v) for v in q32]
    assert (est.group_bits * 2.0 ** 32).tolist() == [[float(v) for v in g] for g in group]
    assert (est.row_bits * 2.0 ** 32).tolist() == [[float(v) for v in r] for r in row]
    for i in range(B):
        assert sum(group[i]) == q32[i] and sum(row[i]) == q32[i], i
    for i in held:
        e = want[i]
        assert q32[i] == e["q32"] and nsym[i] == e["symbols"], i
        assert group[i] == e["group"] and row[i] == e["row"], i
    return q32, nsym


def _codec(case):
    from lic360_fused import FusedCodec
    G, H, W, B, seed, _ = case
    fc = FusedCodec(G, H, W, max_batch=B)
    fc.load_layers(rt.main_case(G, H, W, B, seed)[2])
    return fc


@pytest.mark.parametrize("state", ["skip", "noskip", "generic"])
@pytest.mark.parametrize("case", rt.MAIN_CASES, ids=lambda c: "x".join(map(str, c[:4])))
def test_fused_codec_estimate_matches_oracle(monkeypatch, case, state):
    """in all three codec states -- the dead-cone skip active, the skip off (LIC360_NOSKIP), the generic-kernel fall-back (LIC360_FUSED_CONV=16) -- the
    same integers"""
    if state == "noskip":
        monkeypatch.setenv("LIC360_NOSKIP", "1")
    elif state == "generic":
        monkeypatch.setenv("LIC360_FUSED_CONV", "16")
    fc = _codec(case)
    assert bool(fc.skip_active()) == (state == "skip")
    q32, nsym = _check_estimate(fc, case)
    if case[3] == 16:
        assert q32[1] == 0 and nsym[1] == 0                       # the fully masked image


@pytest.mark.parametrize("coder", ["device", "host"])
def test_estimate_disturbs_nothing(coder):
    """estimate, then encode of the same batch: the oracle's bytes; rate_last after that encode == the estimate; a smaller batch afterwards gives that
    batch's values; rate_last of more images than the last call held refuses"""
    import lic360
    case = rt.MAIN_CASES[3]
    G, H, W, B, seed, held = case
    code, mask, _ = rt.main_case(G, H, W, B, seed)
    want = rt.main_expected(*case)
    fc = _codec(case)
    fc.set_coder(coder)
    with pytest.raises(lic360.Lic360Error, match="bad argument"):
        fc.rate_last(1)
    est = fc.estimate(dev(code), dev(mask), groups=True, rows=True)
    streams = fc.encode(dev(code), dev(mask))
    for i in held:
        assert streams[i] == want[i]["stream"], i
    last = fc.rate_last(B, groups=True, rows=True)
    for a, b in zip(est, last):
        assert torch.equal(a, b)
    # three other images (the batch's last three) on the same codec
    small = fc.estimate(dev(code[B - 3:]), dev(mask[B - 3:]), groups=True)
    assert small.q32.tolist() == [want[i]["q32"] for i in range(B - 3, B)] and small.symbols.tolist() == [want[i]["symbols"] for i in range(B - 3, B)]
    assert small.row_bits is None and (small.group_bits * 2.0 ** 32).tolist() == [[float(v) for v in want[i]["group"]] for i in range(B - 3, B)]
    with pytest.raises(lic360.Lic360Error, match="bad argument"):
        fc.rate_last(4)
    assert fc.rate_last(3).q32.tolist() == small.q32.tolist()


@pytest.mark.parametrize("case", rt.MAIN_CASES, ids=lambda c: "x".join(map(str, c[:4])))
def test_estimate_against_the_real_streams(case):
    """|8 len(stream) - bits| <= the slack measured on the CPU against the oracle's coder (rate_cases.SLACK_BITS), for every image, streams from fc.encode"""
    G, H, W, B, seed, _ = case
    code, mask, _ = rt.main_case(G, H, W, B, seed)
    fc = _codec(case)
    est = fc.estimate(dev(code), dev(mask))
    streams = fc.encode(dev(code), dev(mask))
    for i in range(B):
        d = 8 * len(streams[i]) - float(est.bits[i])
        print("image %d: %d symbols, 8 len - bits = %+.3f" % (i, int(est.symbols[i]), d))
        assert abs(d) <= rt.slack(int(est.symbols[i])), i


@pytest.mark.parametrize("case", rt.IMP_CASES, ids=lambda c: "cpg%d" % c[0])
def test_fused_importance_codec_estimate_matches_restatement(case):
    """FusedImpCodec.estimate at 144 hidden channels and on the 8-channel generic path: q32, symbols and the row breakdown; encode afterwards gives the
    oracle's bytes and rate_last the same integers"""
    import lic360
    from lic360 import _lib, _p, _stream
    from lic360_fused import FusedImpCodec
    cpg, nsym, H, W, B, seed = case
    levels, layers = rt.imp_case(*case)
    want = rt.imp_expected(*case)
    fc = FusedImpCodec(H, W, max_batch=4, hidden_channels=cpg, nsym=nsym)
    fc.load_layers(layers)
    with pytest.raises(lic360.Lic360Error, match="bad argument"):
        fc.rate_last(1)
    est = fc.estimate(dev(levels), rows=True)
    assert est.group_bits is None
    assert est.q32.tolist() == [e["q32"] for e in want] and est.symbols.tolist() == [e["symbols"] for e in want] == [H * W] * B
    q32, cnt, row = _sentinel(B), _sentinel(B), _sentinel(B, H)
    lic360._chk(_lib.lic360_impcodec_rate_last(_stream(0), fc._h, B, _p(q32), _p(cnt), _p(row)))
    assert row.cpu().tolist() == [e["row"] for e in want] and q32.cpu().tolist() == est.q32.tolist() and cnt.cpu().tolist() == est.symbols.tolist()
    assert (est.row_bits * 2.0 ** 32).tolist() == [[float(v) for v in e["row"]] for e in want]
    assert fc.encode(dev(levels)) == [e["stream"] for e in want]
    assert fc.rate_last(B).q32.tolist() == est.q32.tolist()
    for i in range(B):
        assert abs(8 * len(want[i]["stream"]) - float(est.bits[i])) <= rt.slack(H * W)
