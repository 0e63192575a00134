"""Rate estimation (include/lic360_hip.h, csrc/rate_kernels.hip): the case list, a Python-integer restatement of the definition, and the expected
values from the oracle.

Definition.  A coded symbol whose CDF record is (lo, hi) has frequency f = hi - lo in [1, 65536] and costs cost(f) = round(2^32 (16 - log2 f)) Q32
bits; a masked symbol (coder.cpp:79) or a record with hi == lo costs nothing and is not counted.  An image's code length is the Python-int sum of its
symbols' costs, and the breakdowns are the same sums by group and by latitude row."""
import functools
import math

import numpy as np

Q32 = 1 << 32


def cost(f):
    """Q32 bits of a symbol of frequency f of 65536 (f = 0: an uncoded record)"""
    return 0 if f == 0 else int(math.floor(Q32 * (16.0 - math.log2(f)) + 0.5))


@functools.lru_cache(None)
def table():
    return [cost(f) for f in range(65537)]


# ---- coding order, restated without the oracle: planes p = g + th + tw ascending; inside a plane the anti-diagonals s = th + tw ascending (so the
# group p - s descends); inside a diagonal the rows ascending (extension/code_contex_cuda.cu:19-31, tile_extract_cuda.cu:36-41)
def buckets(G, H, W):
    """[(group, row)] of every position of the latent's coding order (G = 1: the importance map's)"""
    out = []
    for p in range(G + H + W - 2):
        for s in range(max(0, p - G + 1), min(p, H + W - 2) + 1):
            out += [(p - s, th) for th in range(max(0, s - W + 1), min(s, H - 1) + 1)]
    return out


def buckets_from_oracle(G, H, W):
    """the same list from the oracle's scan order (orc.code_contex) and its plane windows"""
    import oracle as orc
    idx, pidx = orc.code_contex(H, W)
    out = []
    for p in range(G + H + W - 2):
        start, end = pidx[max(0, p - G + 1)], pidx[min(p, H + W - 2) + 1]
        assert end - start == orc.plane_len(p, G, H, W, pidx)
        out += [(p - int(idx[q]) - int(idx[q + H * W]), int(idx[q])) for q in range(start, end)]
    return out


def rate_of(planes, bkt, G, H):
    """planes: [(tables [n][ncode + 1], labels [n], mask [n] or None)] in coding order; bkt: buckets() of the same order
    -> dict(q32, symbols, group [G], row [H]) of Python ints"""
    t = table()
    q32, nsym, group, row, k = 0, 0, [0] * G, [0] * H, 0
    for tab, lab, mk in planes:
        for i in range(len(lab)):
            g, th = bkt[k]
            k += 1
            if mk is not None and mk[i] < 0.5:
                continue
            f = int(tab[i][lab[i] + 1]) - int(tab[i][lab[i]])
            if f == 0:
                continue
            c = t[f]
            q32, nsym = q32 + c, nsym + 1
            group[g] += c
            row[th] += c
    assert k == len(bkt)
    return dict(q32=q32, symbols=nsym, group=group, row=row)


# ---- 1. raw tables (lic360_rate_records).  (n, B): one symbol; sizes around a wave; 257; and one n just past a workgroup's chunk of 8192 records,
# odd: images 1 and 2 then start on an 8- and a 16-byte boundary in turn, and the second chunk is a tail of one record.
CHUNK = 8192
RAW_CASES = [(1, 1), (2, 3), (63, 2), (64, 1), (65, 3), (257, 5), (CHUNK + 1, 3)]
RAW_NCODE = [8, 49]


def raw_case(n, B, ncode):
    """tables [B n][ncode + 1] int32 (each totals 65536), labels [B n] int32, mask [B n] float32.  Symbol i of the flattened case is of kind
    (i + ncode) % 4: 0 -> f = 1, 1 -> f = 65536, 2 -> uncoded (mask 0), 3 -> a random table and label.  Every case of at least four symbols
    holds all four kinds; the one symbol of (1, 1) is f = 1 at ncode 8 and f = 65536 at ncode 49."""
    rng = np.random.default_rng([n, B, ncode])
    N = n * B
    cuts = np.sort(rng.integers(0, 65537, (N, ncode - 1)), axis=1)
    tabs = np.concatenate([np.zeros((N, 1), np.int64), cuts, np.full((N, 1), 65536, np.int64)], 1)
    labels = rng.integers(0, ncode, N)
    mask = np.ones(N, np.float32)
    for i in range(N):
        kind, s = (i + ncode) % 4, int(labels[i])
        if kind == 0:                                              # symbol s has frequency 1: the entries below it at some a, those above at a + 1
            a = int(rng.integers(0, 65536))
            tabs[i, 1:s + 1], tabs[i, s + 1:ncode] = a, a + 1
            if s == 0:
                tabs[i, 1:ncode] = 1
            elif s == ncode - 1:
                tabs[i, 1:ncode] = 65535
        elif kind == 1:                                            # all the mass on symbol s
            tabs[i, 1:s + 1], tabs[i, s + 1:ncode] = 0, 65536
        elif kind == 2:
            mask[i] = 0.0
    assert (np.diff(tabs, axis=1) >= 0).all() and (tabs[:, 0] == 0).all() and (tabs[:, -1] == 65536).all()
    return tabs.astype(np.int32), labels.astype(np.int32), mask


def raw_expected(tabs, labels, mask, n, B):
    """-> (q32 [B], symbols [B]) Python ints"""
    t = table()
    f = (tabs[np.arange(n * B), labels + 1].astype(np.int64) - tabs[np.arange(n * B), labels]) * (mask >= 0.5)
    f = f.reshape(B, n)
    return [sum(t[int(v)] for v in f[b]) for b in range(B)], [int((f[b] != 0).sum()) for b in range(B)]


# ---- 2. the latent codec against the oracle.  (G, H, W, B, seed, the images held against the oracle)
MAIN_CASES = [(3, 5, 3, 3, 61, (0, 1, 2)),             # odd n = 45: image 1 starts on an 8-byte boundary
              (4, 64, 6, 2, 62, (0, 1)),               # W < 7: the row-major encode kernel
              (6, 8, 12, 16, 63, (0, 1, 15)),          # every image through the kernel; image 1 fully masked: exactly 0 bits and 0 symbols
              (6, 28, 40, 8, 64, tuple(range(8)))]


@functools.lru_cache(None)
def main_case(G, H, W, B, seed):
    """-> code, mask [B, G, H, W] float32, layers (util.make_main_params).  Image 1 of the 16-image case is fully masked."""
    from util import latent, make_main_params
    rng = np.random.default_rng(seed)
    items = [latent(rng, G, H + H % 2, W + W % 2) for _ in range(B)]           # (util.latent takes even sizes: an odd one is cropped)
    code = np.ascontiguousarray(np.concatenate([it[0] for it in items], 0)[:, :, :H, :W])
    mask = np.ascontiguousarray(np.concatenate([it[1] for it in items], 0)[:, :, :H, :W])
    if B == 16:
        mask[1] = 0.0
    return code, mask, make_main_params(5000 + seed, G)


@functools.lru_cache(None)
def main_expected(G, H, W, B, seed, held):
    """-> {image: dict(q32, symbols, group, row, stream)}: the restatement over the oracle's per-plane tables, and the oracle coder's bytes"""
    import ref_codec as rc
    code, mask, layers = main_case(G, H, W, B, seed)
    bkt = buckets(G, H, W)
    out = {}
    for i in held:
        data, planes = rc.encode_main(code[i:i + 1], mask[i:i + 1], layers, G, want_tables=True)
        out[i] = dict(rate_of(planes, bkt, G, H), stream=data)
    return out


# ---- 5. the importance-map codec: nsym = 49 at 144 hidden channels and on the 8-channel generic path, the shapes of
# tests/test_gpu_codec.py::test_fused_importance_codec_matches_oracle.  (cpg, nsym, H, W, B, seed)
IMP_CASES = [(8, 49, 8, 12, 3, 31), (144, 49, 4, 6, 1, 32)]


@functools.lru_cache(None)
def imp_case(cpg, nsym, H, W, B, seed):
    from util import make_imp_params
    rng = np.random.default_rng(seed)
    return rng.integers(0, nsym, (B, 1, H, W)).astype(np.float32), make_imp_params(6000 + seed, cpg, nsym)


def imp_planes(y, levels, nsym, idx, pidx):
    """ref_codec._imp_coder with the tables kept: the net's output y [1, nsym, h, w] and the levels [1, 1, h, w] of ONE image
    -> (bytes, [(tables, labels, None)] per plane)"""
    import oracle as orc
    _, _, H, W = levels.shape
    enc = orc.Encoder()
    z = np.zeros(nsym * H * W, np.float32)
    lab = np.zeros(H * W, np.float32)
    planes = []
    for p in range(H + W - 1):
        tn = orc.tile_extract(y, z, 1, True, idx, pidx, p)
        tab = orc.entropy_table(z, tn, nsym).astype(np.int32)
        orc.tile_extract(levels, lab, 1, True, idx, pidx, p)
        enc.encode(tab, nsym, lab[:tn].astype(np.int32), None, tn)
        planes.append((tab, lab[:tn].astype(np.int32).copy(), None))
    return enc.finish(), planes


@functools.lru_cache(None)
def imp_expected(cpg, nsym, H, W, B, seed):
    """-> [dict(q32, symbols, group, row, stream)] per image"""
    import oracle as orc
    import ref_codec as rc
    levels, layers = imp_case(cpg, nsym, H, W, B, seed)
    idx, pidx = orc.code_contex(H, W)
    y = rc.net_ec(orc.scale(levels, -1.0, np.float32(2.0 / (nsym - 2))), layers, 1)
    bkt = buckets(1, H, W)
    out = []
    for i in range(B):
        data, planes = imp_planes(np.ascontiguousarray(y[i:i + 1]), levels[i:i + 1], nsym, idx, pidx)
        assert data == rc.encode_imp(levels[i:i + 1], layers, nsym)
        out.append(dict(rate_of(planes, bkt, 1, H), stream=data))
    return out


# ---- stream-length slack: 8 len(stream) - q32 / 2^32 over every image of MAIN_CASES (held images) and IMP_CASES, measured on the CPU against the
# oracle's coder (tests/test_rate_cases_cpu.py::test_stream_length_slack prints the table; see the comment at SLACK_BITS below)
def slack_rows():
    rows = []
    for G, H, W, B, seed, held in MAIN_CASES:
        for i, e in sorted(main_expected(G, H, W, B, seed, held).items()):
            rows.append((("main", G, H, W, i), e["symbols"], 8 * len(e["stream"]) - e["q32"] / Q32))
    for case in IMP_CASES:
        for i, e in enumerate(imp_expected(*case)):
            rows.append((("imp",) + case[:4] + (i,), e["symbols"], 8 * len(e["stream"]) - e["q32"] / Q32))
    return rows


# Measured with  python -m pytest tests/test_rate_cases_cpu.py -k slack -s  (20 images, 0 to 3468 coded symbols each):
#     minimum -0.477 bits (main 6 x 28 x 40, image 7, 3360 symbols), maximum +8.000 bits (the fully masked image: the bare terminator byte, 0 bits)
# Both signs, as expected: the coder ends with one terminating bit and zero padding to a byte (up to +8), and the decoder reads zeros past the end, so
# pending bits the stream never needed are not written (below 0).  The difference does not grow with the symbol count -- 18 symbols: -0.14 .. +4.8,
# 3256 .. 3468 symbols: -0.48 .. +6.7 -- so the slack is one constant, not a + b * symbols: the larger magnitude, rounded up, plus 16 (one byte of
# padding plus a terminator's worth).  The GPU test reuses it; it is not tuned to the GPU.
SLACK_MEASURED = (-0.48, 8.0)                   # (rounded outwards to two decimals)
SLACK_BITS = 8 + 16


def slack(symbols):
    """the bound on |8 len(stream) - bits| of an image with `symbols` coded symbols (constant: see above)"""
    return SLACK_BITS
