"""Cases, float64 references and the kernel's geometry restated for the native backward of the group-causal convolution
(csrc/cconv_wgrad_kernels.hip, lic360.cconv_wgrad / cconv_dgrad, MaskConv2(route="fused")).  A plain module, imported by
tests/test_maskconv_grad_cases_cpu.py (which checks it against autograd and against the kernel source) and tests/test_gpu_maskconv_grad.py.

The mask rule (oracle.mask_constrain): weight [oc, ic, th, tw] is kept iff th + tw + ic // cin <= oc // cout + 4, strictly less for constrain 5.
The weight gradient: gw[oc, ic, th, tw] = sum_{n, y, x} gy[n, oc, y, x] * x[n, ic, y + th - 2, x + tw - 2], x zero outside the map, at kept taps; +0.0 at
the others.  Integer operands in -3 .. 3 keep every sum below 2^24 (at most 9 * n * h * w <= 9 * 1024), so its fp32 value is the same in any order."""
import collections
import functools

import numpy as np

F = np.float32
KSZ, TAPS = 5, 25
# the kernel's constants (test_maskconv_grad_cases_cpu.py reads them out of the source)
TILE = 16                     # CW_TILE: output channels per row block, input channels per column block
KW = 32                       # CW_KW: positions of one image row per staged chunk
KSTEP = 4                     # positions per MFMA
SPLIT_ROWS = 1                # CW_SPLIT_ROWS: least image rows (of n * h) per split
MAX_SPLITS = 32               # CW_MAX_SPLITS
THREADS = 64                  # CW_THREADS

Case = collections.namedtuple("Case", "id G cin cout constrain n h w")


def split_geometry(rows):
    """-> (rows per split, number of splits, rows of the last split) for n * h = rows"""
    rps = max(SPLIT_ROWS, -(-rows // MAX_SPLITS))
    nsplit = -(-rows // rps)
    return rps, nsplit, rows - (nsplit - 1) * rps


def _split_case():
    """the smallest n * h * w with more than one split and a last split shorter than the rest: the first such row count, rows of one cell"""
    rows = next(r for r in range(1, 4 * MAX_SPLITS * SPLIT_ROWS + 4) if split_geometry(r)[1] > 1 and split_geometry(r)[2] < split_geometry(r)[0])
    return Case("split_tail", 6, 4, 4, 6, 1, rows, 1)


CASES = (
    Case("g6_4x4", 6, 4, 4, 6, 2, 7, 9),
    Case("g17_1x4_first", 17, 1, 4, 5, 1, 5, 19),          # a column block of one channel
    Case("g6_4x3_straddle", 6, 4, 3, 6, 3, 9, 35),         # row blocks that straddle groups; w % 4 == 3
    Case("g1_20x7_imp", 1, 20, 7, 6, 2, 6, 33),            # the importance net's one-group form
    Case("g48_4x4_classes", 48, 4, 4, 6, 1, 8, 16),        # every class of block pair
    Case("short_map", 6, 4, 4, 6, 2, 3, 4),                # map shorter than the window
    _split_case(),
    Case("split_over_images", 6, 4, 3, 5, 3, 11, 6),       # 33 rows: splits of two rows that cross image boundaries, the last of one
    Case("g9_4x3_one_tap", 9, 4, 3, 5, 1, 4, 5),           # pair (0, 2) keeps tap (0, 0) alone: 15 // 3 - 32 // 4 + 4 - 1 = 0
)
BY_ID = {c.id: c for c in CASES}
MODULE_CASES = CASES[:3]
IDENTITY_SHAPES = ((6, 4, 4, False), (6, 1, 4, True), (5, 4, 3, False), (7, 2, 3, True))      # (G, cin, cout, strict) on 2 x . x 7 x 9


def channels(case):
    return case.G * case.cin, case.G * case.cout                           # (channel, nout)


# ---------------------------------------------------------------------------------------------------- the mask rule
def keep_mask(G, cin, cout, constrain, group_in=None, group_out=None):
    """[nout, channel, 5, 5] bool; group_in / group_out: (channel index -> group), the rule's own divisors by default"""
    channel, nout = G * cin, G * cout
    gi = np.arange(channel) // cin if group_in is None else group_in(np.arange(channel))
    go = np.arange(nout) // cout if group_out is None else group_out(np.arange(nout))
    s = np.arange(KSZ)[:, None] + np.arange(KSZ)[None, :]
    lhs = s[None, None] + gi[None, :, None, None]
    rhs = go[:, None, None, None] + KSZ - 1
    return lhs < rhs if constrain == 5 else lhs <= rhs


# ---------------------------------------------------------------------------------------------------- geometry of the kernel
def blocks(case):
    channel, nout = channels(case)
    return (nout + TILE - 1) // TILE, (channel + TILE - 1) // TILE          # (row blocks, column blocks)


def reach(case, rb, cb):
    """d of a pair: its live taps are th + tw <= d (cw_reach)"""
    channel, nout = channels(case)
    oc_hi = min(rb * TILE + TILE - 1, nout - 1)
    d = oc_hi // case.cout - (cb * TILE) // case.cin + KSZ - 1 - (1 if case.constrain == 5 else 0)
    return min(d, 2 * (KSZ - 1))


def live_taps(case, rb, cb):
    d = reach(case, rb, cb)
    return [(th, tw) for th in range(KSZ) for tw in range(KSZ) if th + tw <= d]


def splits(case):
    """-> (rows per split, number of splits, rows of the last split)"""
    return split_geometry(case.n * case.h)


def pair_classes(case):
    """{(rb, cb): set of classes}: what the geometry does with each block pair"""
    channel, nout = channels(case)
    keep = keep_mask(case.G, case.cin, case.cout, case.constrain)
    nrb, ncb = blocks(case)
    out = {}
    for rb in range(nrb):
        for cb in range(ncb):
            sub = keep[rb * TILE:(rb + 1) * TILE, cb * TILE:(cb + 1) * TILE]
            live = live_taps(case, rb, cb)
            cls = set()
            assert {(th, tw) for th in range(KSZ) for tw in range(KSZ) if sub[:, :, th, tw].any()} == set(live)      # live == some weight kept
            if not live:
                cls.add("dead")
            elif sub.all():
                cls.add("dense")
            else:
                cls.add("partially_masked")
            if len(live) == 1:
                cls.add("one_live_tap")
            if sub.shape[0] < TILE:
                cls.add("partial_row_block")
            if sub.shape[1] < TILE:
                cls.add("partial_column_block")
            rows = np.arange(rb * TILE, rb * TILE + sub.shape[0]) // case.cout
            cols = np.arange(cb * TILE, cb * TILE + sub.shape[1]) // case.cin
            if (TILE % case.cout and len(set(rows)) > 1) or (TILE % case.cin and len(set(cols)) > 1 and case.cin > 1):
                cls.add("straddling")
            out[(rb, cb)] = cls
    return out


def reaches(case):
    """every class of the geometry this case exercises"""
    got = set().union(*pair_classes(case).values())
    if case.w % KSTEP:
        got.add("k_tail")
    if case.w % KW and case.w > KW:
        got.add("ragged_chunk")
    rps, nsplit, last = splits(case)
    if nsplit > 1 and last < rps:
        got.add("multi_split_short_tail")
    return got


REACH = ("partial_row_block", "partial_column_block", "straddling", "dead", "partially_masked", "one_live_tap", "dense", "k_tail", "ragged_chunk",
         "multi_split_short_tail")


def scratch_bytes(case):
    """what lic360_cconv_wgrad_scratch_bytes returns: the pair table (12 bytes a pair, rounded to 16) and one 16 x 16 fp32 tile per live (pair, tap)
    and split, the splits counted by their bound min(ceil(rows / SPLIT_ROWS), MAX_SPLITS)"""
    nrb, ncb = blocks(case)
    tiles = sum(len(live_taps(case, rb, cb)) for rb in range(nrb) for cb in range(ncb))
    bound = min(-(-case.n * case.h // SPLIT_ROWS), MAX_SPLITS)
    return (nrb * ncb * 12 + 15) // 16 * 16 + bound * tiles * TILE * TILE * 4


# ---------------------------------------------------------------------------------------------------- operands
@functools.lru_cache(maxsize=None)
def inputs(case):
    """integer-valued x, gy in -3 .. 3 (fp32) and a masked, trained-scale weight and bias"""
    rng = np.random.default_rng(sum(ord(ch) for ch in case.id) * 7 + 1)
    channel, nout = channels(case)
    x = rng.integers(-3, 4, (case.n, channel, case.h, case.w)).astype(F)
    gy = rng.integers(-3, 4, (case.n, nout, case.h, case.w)).astype(F)
    w = (rng.standard_normal((nout, channel, KSZ, KSZ)) * 0.1).astype(F) * keep_mask(case.G, case.cin, case.cout, case.constrain)
    b = (rng.standard_normal(nout) * 0.1).astype(F)
    for a in (x, gy, w, b):
        a.setflags(write=False)
    return dict(x=x, gy=gy, weight=w.astype(F), bias=b)


@functools.lru_cache(maxsize=None)
def real_inputs(case):
    """trained-scale real-valued x and gy"""
    rng = np.random.default_rng(sum(ord(ch) for ch in case.id) * 11 + 5)
    channel, nout = channels(case)
    x = rng.standard_normal((case.n, channel, case.h, case.w)).astype(F)
    gy = (rng.standard_normal((case.n, nout, case.h, case.w)) * 0.05).astype(F)
    for a in (x, gy):
        a.setflags(write=False)
    return dict(x=x, gy=gy)


# ---------------------------------------------------------------------------------------------------- the weight gradient in float64
BROKEN = ("taps_swapped", "shift_sign", "other_strictness", "wrong_divisor", "halo_wrapped", "last_split_dropped", "tile_transposed")


def wgrad_f64(case, x, gy, broken=None, absolute=False):
    """the contract in float64, [nout, channel, 5, 5]; absolute: the sum of |gy * x| instead (for the fp32 bound).
    broken: one of BROKEN, a model of a kernel that gets that one thing wrong"""
    assert broken is None or broken in BROKEN
    channel, nout = channels(case)
    x, gy = np.asarray(x, np.float64), np.asarray(gy, np.float64)
    if absolute:
        x, gy = np.abs(x), np.abs(gy)
    n, h, w = case.n, case.h, case.w
    if broken == "last_split_dropped":
        rps, nsplit, _ = splits(case)
        rows = np.arange(n * h).reshape(n, h) < (nsplit - 1) * rps if nsplit > 1 else np.ones((n, h), bool)
        gy = gy * rows[:, None, :, None]
    pad = np.pad(x, ((0, 0), (0, 0), (2, 2), (2, 2)), mode="wrap" if broken == "halo_wrapped" else "constant")
    gw = np.zeros((nout, channel, KSZ, KSZ))
    for th in range(KSZ):
        for tw in range(KSZ):
            sh, sw = (KSZ - 1 - th, KSZ - 1 - tw) if broken == "shift_sign" else (th, tw)
            gw[:, :, th, tw] = np.einsum("nohw,nihw->oi", gy, pad[:, :, sh:sh + h, sw:sw + w])
    if broken == "taps_swapped":
        gw = gw.transpose(0, 1, 3, 2)
    if broken == "tile_transposed":
        out = gw.copy()
        for r0 in range(0, nout, TILE):
            for c0 in range(0, channel, TILE):
                m = min(TILE, nout - r0, channel - c0)
                out[r0:r0 + m, c0:c0 + m] = gw[r0:r0 + m, c0:c0 + m].transpose(1, 0, 2, 3)
        gw = out
    if broken == "other_strictness":
        keep = keep_mask(case.G, case.cin, case.cout, 11 - case.constrain)
    elif broken == "wrong_divisor":
        keep = keep_mask(case.G, case.cin, case.cout, case.constrain, lambda c: c // case.cout, lambda c: c // case.cin)
    else:
        keep = keep_mask(case.G, case.cin, case.cout, case.constrain)
    return np.where(keep, gw, 0.0)


@functools.lru_cache(maxsize=None)
def wgrad_reference(case):
    """the integer case's gradient as fp32 (exact: the float64 sums are integers below 2^24); shared, left unchanged"""
    t = inputs(case)
    want64 = wgrad_f64(case, t["x"], t["gy"])
    want = want64.astype(F)
    assert np.array_equal(want, want64) and float(np.abs(want64).max()) < 2.0 ** 24
    want.setflags(write=False)
    return want


def gamma(k):
    """the fp32 bound of a sum of k products in any order: |computed - exact| <= gamma_k * sum |products|"""
    u = 2.0 ** -24
    return k * u / (1.0 - k * u)


# ---------------------------------------------------------------------------------------------------- the data-gradient identity, index by index
def group_flip_np(t, G):
    """R F with indices only: out[n, a c + i, y, x] = t[n, (G - 1 - a) c + i, h - 1 - y, w - 1 - x]"""
    n, ch, h, w = t.shape
    c = ch // G
    out = np.empty_like(t)
    for a in range(G):
        for i in range(c):
            out[:, a * c + i] = t[:, (G - 1 - a) * c + i, ::-1, ::-1]
    return out


def transpose_weight_np(wt, G):
    """w'[a cin + ci, b cout + co] = w[(G - 1 - b) cout + co, (G - 1 - a) cin + ci], taps unchanged"""
    nout, channel = wt.shape[:2]
    cout, cin = nout // G, channel // G
    out = np.empty((channel, nout) + wt.shape[2:], wt.dtype)
    for a in range(G):
        for ci in range(cin):
            for b in range(G):
                for co in range(cout):
                    out[a * cin + ci, b * cout + co] = wt[(G - 1 - b) * cout + co, (G - 1 - a) * cin + ci]
    return out


def dgrad_oracle(case, gy, weight):
    """R F oracle.cconv_ec(R F gy, w', 0, None, G, constrain): the bits lic360.cconv_dgrad must return"""
    import oracle
    channel, nout = channels(case)
    y = oracle.cconv_ec(group_flip_np(np.asarray(gy, F), case.G), transpose_weight_np(np.asarray(weight, F), case.G), np.zeros(channel, F), None, case.G,
                        case.constrain)
    return np.ascontiguousarray(group_flip_np(y, case.G))


# ---------------------------------------------------------------------------------------------------- layers and nets in float64 (torch, CPU)
def conv_f64(x, weight, bias, G, cin, cout, constrain):
    """the layer as mathematics: a dense convolution over the masked weight; float64 torch tensors"""
    import torch
    keep = torch.from_numpy(keep_mask(G, cin, cout, constrain))
    return torch.nn.functional.conv2d(x, torch.where(keep, weight, torch.zeros_like(weight)), bias, padding=2)


def entropy_net_f64(params, x, G, cpn, nlast, prefix):
    """lic360_models' entropy net (first layer, PReLU, five residual blocks, last layer) on float64 parameters named as its state dict"""
    import torch.nn.functional as fn
    p = lambda name: params[prefix + name]
    t = fn.prelu(conv_f64(x, p("0.weight"), p("0.bias"), G, 1, cpn, 5), p("1.weight"))
    for blk in range(2, 7):
        u = fn.prelu(conv_f64(t, p("%d.net.0.weight" % blk), p("%d.net.0.bias" % blk), G, cpn, cpn, 6), p("%d.net.1.weight" % blk))
        u = fn.prelu(conv_f64(u, p("%d.net.2.weight" % blk), p("%d.net.2.bias" % blk), G, cpn, cpn, 6), p("%d.net.3.weight" % blk))
        t = u + t
    return conv_f64(t, p("7.weight"), p("7.bias"), G, cpn, nlast, 6)
