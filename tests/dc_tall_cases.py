"""Cases of the decode-order dead-cone lists on latents of 65..128 rows (csrc/need.h, need_kernels.hip, k_cconv4v6lt in csrc/cconv4v6_dc.inc), with the
record format, the cut rule and the list builder's arithmetic restated from DESIGN.md 4.6 ("Tall latents").  No GPU, no oracle and no call of the
library in here: tests/test_dc_tall_cpu.py checks this file against the library's host-only lic360_dcl_pack_layout, tests/test_gpu_dc_tall_lists.py
decodes the device-built lists with it.

The format.  A record is four 32-bit words: x = g0 | packed << 7 | n << 10 (g0: first group of the three-group block, n: first sample), y / z / w = up
to three PIECES.  A piece = k | (slo & 63) << 3 | (shi & 63) << 9 | a0 << 15 | 1 << 21 | (slo >> 6) << 25 | (shi >> 6) << 26: sample n + 8 k stores its
rows slo..shi in lanes a0..a0 + shi - slo of the wave; bits 22..24 of y say which of the block's groups are live somewhere in the record.  On a
latent of at most 64 rows bits 25 and 26 are zero and the word is what it always was.

The cut rule.  The live row windows lo[k]..hi[k] of a chunk of up to eight samples are laid end to end over waves of 64 lanes: (a0 - slo) % 4 == 0;
a piece that does not start with image row 0 leaves lanes 0, 1 free, one that does not end with the image's last row ends at lane 61 or earlier (a
stored lane takes shifted partial sums from the two lanes on either side of it); a window that does not fit is CUT there and goes on in the next
wave, which fetches the rows around the cut again as its halo; a cut piece must hold at least four rows and start at lane 57 or earlier; the next
piece starts in the band quad behind the previous piece's last column (last lane + 4); three pieces per wave at the most.  A 128-row window takes
three waves (rows 0..61, 62..121, 122..127), and the rest of the third wave goes to the next sample."""
import numpy as np

PS = 3                      # groups (staggered diagonals) of a task
CHUNK = 8                   # samples per packing chunk
LAYERS = 12
PACK_HEIGHTS = (65, 66, 72, 96, 126, 128)
# FusedCodec shapes (G, H, W, B), each the smallest at which one class of failure can occur
GPU_SHAPES = [
    (5, 66, 10, 16),        # one row past a wave
    (12, 72, 20, 16),       # a cut inside a block's hull
    (6, 128, 16, 16),       # full height: three waves per window
    (48, 128, 24, 16),      # all sixteen group blocks, and the live-group bits
    (6, 96, 8, 80),         # ten samples per XCD list: more than one chunk, and the balancing pass
    # A diagonal has at most min(H, W) rows, so the windows of the shapes above (W <= 24) never reach the end of a wave.  These two have diagonals
    # longer than a wave:
    (3, 72, 68, 16),        # windows CUT in mid-image, rows past 63 on either side of a cut
    (3, 128, 132, 16),      # full-height windows over three waves
]
LIST_SHAPES = [GPU_SHAPES[1], GPU_SHAPES[2], GPU_SHAPES[5]]       # where the records themselves are decoded
CUT_SHAPES = [GPU_SHAPES[5], GPU_SHAPES[6]]                       # where windows are cut between waves (tests/test_dc_tall_cpu.py checks that they are)


# The CPU oracle's bitstreams of these batches are a committed fixture (tests/golden/dc_tall_lists.npz, written by tools/gen_golden_dc_tall.py: the
# oracle takes 2..12 s per batch, and ~15 s per IMAGE at (48, 128, 24, 16) -- there images 0..7, one per XCD list, are pinned)
GOLDEN = "dc_tall_lists.npz"
GOLDEN_IMAGES = {s: (8 if s == (48, 128, 24, 16) else s[3]) for s in GPU_SHAPES}


def batch_seed(shape):
    return 8800 + shape[1] + shape[0]


def weight_seed(shape):
    return 300 + shape[0]


def batch(G, H, W, B, seed, n_iid=2):
    """code, mask [B, G, H, W] of a seeded batch: SURVEY 8d's smooth masks, the last n_iid images i.i.d. (as _batch of tests/test_gpu_need.py)"""
    from util import latent, latent_smooth
    cs, ms = [], []
    for i in range(B):
        c, m, _ = (latent if i >= B - n_iid else latent_smooth)(np.random.default_rng(seed + i), G, H, W)
        cs.append(c)
        ms.append(m)
    return np.concatenate(cs, 0), np.concatenate(ms, 0)


def golden_streams(shape, code, mask):
    """the oracle's bitstreams of the first GOLDEN_IMAGES[shape] images of the shape's batch, from the fixture; code / mask: the batch, whose digests
    must be the fixture's"""
    import hashlib
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN))
    k = shape_id(shape)
    assert [hashlib.sha256(code.tobytes()).hexdigest(), hashlib.sha256(mask.tobytes()).hexdigest()] == [str(v) for v in g[k + "_sha256"]], "the fixture is of another batch"
    ends = np.cumsum(g[k + "_lengths"])
    assert len(ends) == GOLDEN_IMAGES[shape]
    data = g[k + "_bytes"].tobytes()
    return [data[e - n:e] for e, n in zip(ends.tolist(), g[k + "_lengths"].tolist())]


def shape_id(s):
    return "g%d_%dx%d_b%d" % tuple(s)


def piece_word(k, slo, shi, a0, row_bits=7):
    w = k | (slo & 63) << 3 | (shi & 63) << 9 | a0 << 15 | 1 << 21
    if row_bits > 6:
        w |= (slo >> 6) << 25 | (shi >> 6) << 26
    return w


def piece_fields(w):
    """-> (k, slo, shi, a0) of a piece word (bits 22..24, the record's live groups, are not the piece's)"""
    return w & 7, (w >> 3) & 63 | (w >> 25 & 1) << 6, (w >> 9) & 63 | (w >> 26 & 1) << 6, (w >> 15) & 63


def wave_pieces(lo, hi, h, c, k, slo, halo=2, last_row=None):
    """the pieces (k, slo, shi, a0) of ONE wave and where the next wave starts.  halo / last_row: the mutations of tests/test_dc_tall_cpu.py
    (lanes kept free at a cut; the row that counts as the image's last)"""
    last_row = h - 1 if last_row is None else last_row
    out, pos = [], 0
    while len(out) < 3 and k < c:
        if hi[k] < lo[k]:                                                   # nothing of this sample is live
            k += 1
            if k < c:
                slo = lo[k]
            continue
        a0 = pos
        if slo != 0 and a0 < halo:
            a0 = halo
        a0 += (slo - a0) & 3
        top = 63 if hi[k] == last_row else 63 - halo
        shi = hi[k]
        if a0 + (hi[k] - slo) > top:
            shi = slo + (63 - halo - a0)                                    # cut
        if a0 > 63 - halo or (shi < hi[k] and (a0 > 57 or shi - slo + 1 < 4)):
            break
        out.append((k, slo, shi, a0))
        pos = ((a0 + (shi - slo) + 4) // 4 + 1) * 4
        slo = shi + 1
        if slo > hi[k]:
            k += 1
            if k < c:
                slo = lo[k]
    return out, k, slo


def pack_chunk(h, lo, hi, row_bits=7, halo=2, last_row=None):
    """the waves of one chunk of samples: a list of [word, word, word] (0 = no piece), as lic360_dcl_pack_layout reports them"""
    c, k, slo, waves = len(lo), 0, lo[0], []
    while k < c:
        pcs, k, slo = wave_pieces(lo, hi, h, c, k, slo, halo, last_row)
        if not pcs:
            break
        words = [piece_word(*p, row_bits=row_bits) for p in pcs]
        waves.append(words + [0] * (3 - len(words)))
    return waves


def waves_per_window(h):
    """the waves that can START with a piece of one window: every one but the last holds at least 57 of its rows (a0 <= 5, cut at lane 61)"""
    return 1 if h <= 64 else 1 + (h - 1) // 57


def list_cap(G, B, h):
    """records an XCD's list of one (layer, plane) has room for: group blocks x three nets x samples of the list x waves per window"""
    return (G + 2) // 3 * 3 * (B // 8) * waves_per_window(h)


def pack_cases(h):
    """(lo, hi) per case: the extremes (full, one-row and empty windows, rows 63 / 64 and the last row), then seeded random chunks"""
    full = (0, h - 1)
    cases = [
        ([0], [h - 1]),                                                     # one full window
        ([0] * 8, [h - 1] * 8),                                             # rows 0..h-1 of all eight samples
        ([h - 1], [h - 1]), ([0], [0]), ([63], [63]), ([64], [64]),         # single rows
        ([1, 0, 1], [0, h - 1, 0]),                                         # empty samples around a full one
        ([1] * 4, [0] * 4),                                                 # nothing live at all
        ([60, 63, 64, 40], [min(66, h - 1), 64, 64, h - 1]),                            # windows that straddle rows 63 / 64
        ([h - 2, h - 1, h - 3, 0], [h - 1, h - 1, h - 2, h - 2]),           # ... and end at, or one short of, the last row
        ([2, 3] * 4, [h - 1, h - 2] * 4),
        ([0, 5], [58, h - 1]), ([0, 5], [61, h - 1]), ([0, 5], [62, h - 1]),
    ]
    if h > 127:
        cases += [([120, 127, 126], [127, 127, 127]), ([0] * 3, [127, 126, 127])]
    rng = np.random.default_rng(h)
    for _ in range(300):
        c = int(rng.integers(1, CHUNK + 1))
        lo, hi = [], []
        for _k in range(c):
            kind = int(rng.integers(0, 7))
            if kind == 0:
                a, b = 1, 0
            elif kind == 1:
                a, b = full
            elif kind == 2:
                a = b = int(rng.integers(h))
            elif kind == 3:                                                 # short windows: three to a wave
                a = int(rng.integers(h))
                b = min(h - 1, a + int(rng.integers(0, 12)))
            else:
                a = int(rng.integers(h))
                b = int(rng.integers(a, h))
            lo.append(a)
            hi.append(b)
        cases.append((lo, hi))
    return cases


# ---- the list builder (need_kernels.hip: k_dc_tasks), from the need maps of a batch
def need_maps(mask):
    """mask [B, G, H, W] (>= 0.5: coded) -> need [B, 12, H, W]: need_11 = highest coded group (-1: none), need_l(q) = min(G - 1, max over p in
    q + [-2, 2]^2 with need_{l+1}(p) >= 0 of need_{l+1}(p) + (p_y - q_y) + (p_x - q_x)), -1 where that is negative or no such p exists"""
    B, G, H, W = mask.shape
    live = mask >= 0.5
    out = np.full((B, LAYERS, H, W), -1, np.int64)
    out[:, 11] = np.where(live, np.arange(G)[None, :, None, None], -1).max(1)
    NONE = -1000
    for l in range(10, -1, -1):
        up = np.full((B, H + 4, W + 4), NONE, np.int64)
        up[:, 2:-2, 2:-2] = np.where(out[:, l + 1] >= 0, out[:, l + 1], NONE)
        best = np.full((B, H, W), NONE, np.int64)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                best = np.maximum(best, up[:, 2 + dy:2 + dy + H, 2 + dx:2 + dx + W] + dy + dx)
        out[:, l] = np.where(best < 0, -1, np.minimum(best, G - 1))
    return out


def block_hulls(need, G, H, W, p, g0):
    """need [..., H, W] (any leading axes: images, layers) -> per leading index the hull (lo, hi) of the rows that need one of the groups g0..g0+2 on
    plane p ((1, 0): none) and the mask of the groups that are live there"""
    lead, S = need.shape[:-2], H + W - 1
    lo, hi, gm = np.full(lead, 1 << 20), np.full(lead, -1), np.zeros(lead, np.int64)
    for q in range(PS):
        g, s = g0 + q, p - g0 - q
        if g >= G or s < 0 or s >= S:
            continue
        ya, yb = max(0, s - W + 1), min(s, H - 1)
        ys = np.arange(ya, yb + 1)
        lv = need[..., ys, s - ys] >= g                                     # [..., rows of the diagonal]
        anyl = lv.any(-1)
        first, last = ya + lv.argmax(-1), yb - lv[..., ::-1].argmax(-1)
        lo = np.where(anyl, np.minimum(lo, first), lo)
        hi = np.where(anyl, np.maximum(hi, last), hi)
        gm |= anyl.astype(np.int64) << q
    return np.where(hi < 0, 1, lo), np.where(hi < 0, 0, hi), gm


def visible_blocks(G, H, W, p):
    """first groups of the plane's group blocks, in list order (heaviest first): every block between the first and the last one that has a
    diagonal on the plane"""
    S = H + W - 1
    vis = [gb for gb in range((G + 2) // 3) if not (p - gb * 3 - 2 >= S or p - gb * 3 < 0)]
    return [gb * 3 for gb in range(vis[-1], vis[0] - 1, -1)] if vis else []


def build_records(need, G, H, W, B, p, nets=(0, 1, 2)):
    """need [B, 12, H, W] -> {layer 1..11: the records of plane p before the balancing pass}, for H > 64 (every live block is packed): a record is
    (home XCD, g0, n, gm, [(sample, slo, shi, a0)]).  Per XCD list: group block major, then net, then chunk of eight samples; the three nets'
    records differ in their samples only (net k: + k B)."""
    out = {l: [] for l in range(1, LAYERS)}
    m = B // 8
    for g0 in visible_blocks(G, H, W, p):
        lo, hi, gm = block_hulls(need, G, H, W, p, g0)                      # [B, 12]
        for l in range(1, LAYERS):
            if not (hi[:, l] >= lo[:, l]).any():
                continue
            llo, lhi, lgm = lo[:, l].tolist(), hi[:, l].tolist(), gm[:, l].tolist()
            for xcd in range(8):
                for c0 in range(0, m, CHUNK):
                    ch = [xcd + 8 * k for k in range(c0, min(m, c0 + CHUNK))]
                    clo, chi = [llo[i] for i in ch], [lhi[i] for i in ch]
                    k, slo, waves = 0, clo[0], []
                    while k < len(ch):
                        pcs, k, slo = wave_pieces(clo, chi, H, len(ch), k, slo)
                        if not pcs:
                            break
                        g = 0
                        for pc in pcs:
                            g |= lgm[ch[pc[0]]]
                        waves.append((g, pcs))
                    for net in nets:
                        nb = xcd + 8 * (net * m + c0)
                        out[l] += [(xcd, g0, nb, g, [(nb + 8 * kk, a, b, a0) for (kk, a, b, a0) in pcs]) for (g, pcs) in waves]
    return out


def stored_rows(G, H, W, p, g0, gm, slo, shi):
    """what a piece stores: [(group, diagonal s, first row, last row)] -- its rows that lie on the diagonals of the groups the record computes"""
    out = []
    for q in range(PS):
        g, s = g0 + q, p - g0 - q
        if g >= G or s < 0 or s >= H + W - 1 or not gm >> q & 1:
            continue
        ya, yb = max(slo, s - W + 1, 0), min(shi, s, H - 1)
        if yb >= ya:
            out.append((g, s, ya, yb))
    return out
