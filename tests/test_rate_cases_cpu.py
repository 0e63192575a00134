"""Rate estimation without a GPU: the library's cost table against the Python restatement, the restated coding order against the oracle's, and the
slack between the oracle coder's stream lengths and the ideal code length (tests/rate_cases.py holds the restatement and the cases)."""
import ctypes as C
import math

import numpy as np

import rate_cases as rt


def test_rate_table_is_the_definition():
    """lic360_rate_table (host-only): entry 0 is 0, every power of two is exact, every other entry within one unit of the restatement (float64 log2 may
    differ in the last place between the C library and Python, which moves a rounding only at a near-tie), non-increasing in f"""
    import lic360
    got = np.zeros(65537, np.uint64)
    lic360._chk(lic360._lib.lic360_rate_table(got.ctypes.data_as(C.c_void_p)))
    got = [int(v) for v in got]
    want = rt.table()
    assert got[0] == 0 and want[0] == 0
    for k in range(17):
        assert got[1 << k] == (16 - k) << 32 == want[1 << k], k
    assert got[65536] == 0
    assert max(abs(g - w) for g, w in zip(got, want)) <= 1
    assert all(got[f] >= got[f + 1] for f in range(1, 65536))
    assert want[3] == int(math.floor((16 - math.log2(3)) * 2 ** 32 + 0.5))


def test_bucket_rule_matches_the_oracles_coding_order():
    shapes = {(c[0], c[1], c[2]) for c in rt.MAIN_CASES} | {(1, c[2], c[3]) for c in rt.IMP_CASES}
    for G, H, W in sorted(shapes):
        b = rt.buckets(G, H, W)
        assert b == rt.buckets_from_oracle(G, H, W), (G, H, W)
        assert len(b) == G * H * W and len(set((g, th, k) for k, (g, th) in enumerate(b))) == len(b)
        assert sorted(g for g, _ in b) == sorted(list(range(G)) * (H * W)) and sorted(th for _, th in b) == sorted(list(range(H)) * (G * W))


def test_raw_cases_hold_every_kind_of_symbol():
    for n, B in rt.RAW_CASES:
        for ncode in rt.RAW_NCODE:
            tabs, labels, mask = rt.raw_case(n, B, ncode)
            f = tabs[np.arange(n * B), labels + 1] - tabs[np.arange(n * B), labels]
            if n * B >= 4:
                assert (f[mask > 0.5] == 1).any() and (f[mask > 0.5] == 65536).any() and (mask < 0.5).any() and ((f > 1) & (f < 65536) & (mask > 0.5)).any()
            q32, nsym = rt.raw_expected(tabs, labels, mask, n, B)
            assert len(q32) == B and sum(nsym) == int(((f != 0) & (mask > 0.5)).sum())
    assert any(n % 2 == 1 and n // rt.CHUNK == 1 and n % rt.CHUNK == 1 and B == 3 for n, B in rt.RAW_CASES)


def test_stream_length_slack():
    """8 len(oracle stream) - q32 / 2^32 for every image of the cases: inside the recorded range, and SLACK_BITS is the larger magnitude + 16.  Image 1 of the
    16-image case is fully masked: 0 bits, 0 symbols, the bare terminator byte."""
    rows = rt.slack_rows()
    for key, nsym, d in rows:
        print("%-28s symbols %6d   8 len - bits = %+8.3f" % (key, nsym, d))
    lo, hi = min(d for _, _, d in rows), max(d for _, _, d in rows)
    print("min %+.3f max %+.3f" % (lo, hi))
    e = rt.main_expected(*rt.MAIN_CASES[2])[1]
    assert e["q32"] == 0 and e["symbols"] == 0 and e["stream"] == b"\x80"
    assert rt.SLACK_MEASURED[0] <= lo and hi <= rt.SLACK_MEASURED[1]
    for _, nsym, d in rows:
        assert abs(d) <= rt.slack(nsym)
    assert rt.SLACK_BITS == math.ceil(max(abs(rt.SLACK_MEASURED[0]), abs(rt.SLACK_MEASURED[1]))) + 16
