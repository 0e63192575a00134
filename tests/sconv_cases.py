"""Exact-data cases of the transforms' own kernels -- the sphere convolutions (csrc/conv3x3_kernels.hip, csrc/sconv_bf16x3.inc) and the one-pass
GDN (csrc/gdn_kernels.hip) -- with their data, their references and the launch geometry the native code will pick.  No GPU and nothing of `lic360`
in here: tests/test_sconv_cases_cpu.py checks this file by itself (coverage of the case list, the exactness condition, that the references tell
a wrong kernel from a right one), tests/test_gpu_sconv_exact.py and tests/test_gpu_gdn_exact.py compare the kernels with it.

The method.  v_mfma_f32_16x16x4_f32 is a chain of fmaf.  When every input, weight, bias and residual is a small integer and every PReLU slope is one
of 1, 1/2, 1/4, 0, every partial sum of every summation order is an integer below 2^24: the convolution has ONE fp32 result, and a kernel either
returns it bit for bit or is wrong.  The split-bf16 form (hi = bf16(v), lo = bf16(v - hi), products w_hi x_hi + w_hi x_lo + w_lo x_hi) is exact in the
same sense as long as hi + lo holds each operand exactly and the dropped w_lo x_lo is zero, which three tiers of data arrange:

    tier   |x| <=   |w| <=   proves
    fp32        8        4   (the fp32 form's data)
    hi        255        7   both operands fit bf16's 8 significant bits: w_hi x_hi alone; loader, epilogue, pack order
    xlo      2047        2   x needs 9 .. 11 bits: the w_hi x_lo term is computed, once, from the right cell
    wlo         4     1023   w needs 9 .. 10 bits: the w_lo x_hi term and the pack's lo planes

The condition (assert_exact_domain) is asserted per case from the case's own data, in float64:
    max over outputs of |b| + 4 |res| + sum |w| |x|  <  2^24,
with |v| read as |hi| + |lo| in the bf16x3 tiers.  (4 |res|, not |res|: a negative sum y times the slope 1/4 is a multiple of 1/4, and
y / 4 + res = (y + 4 res) / 4 is exact when |y| + 4 |res| < 2^24.)  The bound is taken per output channel as sum_ci (sum_taps |w|) max_cells |x[ci]|,
which is never below the true maximum and costs nothing at the production sizes.

GDN: x in -15 .. 15, gamma in 0 .. 3, beta in 1 .. 16, all integers: beta + sum_j gamma[i][j] x[j]^2 < 2^24 is exact on the same MFMA, and what is left
is one correctly rounded fp32 square root and one correctly rounded fp32 division (or product): numpy's float32 `sqrt`, `/` and `*`."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

from util import _stable

SENTINEL = 7.0
EXACT_BELOW = float(1 << 24)
TIERS = {"fp32": (8, 4), "hi": (255, 7), "xlo": (2047, 2), "wlo": (4, 1023)}        # tier -> (max |x|, max |w|)
B3_TIERS = ("hi", "xlo", "wlo")
SLOPES = (1.0, 0.5, 0.25, 0.0)

Case = collections.namedtuple("Case", "name ks cin cout n hp wp pad sphere ring ring_w crop shuffle slope res prod")
Branch = collections.namedtuple("Branch", "b3 nq rw rw_last ks blocks_y tiles_y tiles_x rem full tall chunks")


def _c(name, ks, cin, cout, n, hp, wp, pad=2, sphere=1, ring=2, ring_w=None, crop=0, shuffle=False, slope=True, res=False, prod=False):
    if ks == 1:
        pad, sphere = 0, 0                                                 # the 1x1 entry points take neither
    return Case(name, ks, cin, cout, n, hp, wp, pad, sphere, ring, ring if ring_w is None else ring_w, crop, shuffle, slope, res, prod)


# ---- the branch matrix on small maps.  Window rows nr = hp - 2 ring, columns nc = wp - 2 ring_w; a tile is 16 x 16; nrg = 8 / NQ row groups
SMALL = [
    # 3x3, NQ = 4 (cout a multiple of 192), nrg = 2: tall last row at rem 1 and 2, the extra tile row at rem 3
    _c("s3_q4_rem1", 3, 32, 192, 1, 19, 36, ring=1, ring_w=2),                                           # nr 17, nc 32 (exact)
    _c("s3_q4_rem2_wrap", 3, 32, 192, 3, 22, 25, sphere=2, res=True),                                    # nr 18, nc 21 (ragged)
    _c("s3_q4_rem3_plain", 3, 32, 192, 1, 21, 23, pad=1, sphere=0, ring=1, slope=False),                 # nr 19: two tile rows, the second mostly dead
    _c("s3_q4_low_pad3", 3, 192, 192, 1, 13, 24, pad=3),                                                 # nr 9: full = 0; six bf16x3 chunks
    _c("s3_q4_3rows_tall_pad1", 3, 32, 192, 1, 51, 20, pad=1, ring=1),                                   # nr 49: three tile rows, the last one tall
    _c("s3_q4_3rows", 3, 192, 192, 3, 52, 20, res=True),                                                 # nr 48: three ordinary tile rows, n = 3
    _c("s3_q4_crop", 3, 32, 192, 1, 22, 24, crop=1),                                                     # crop without shuffle
    _c("s3_q4_shuffle_768", 3, 192, 768, 1, 14, 22, crop=1, shuffle=True),                               # blockIdx.y 0 .. 3
    _c("s3_q4_shuffle_res", 3, 32, 384, 3, 22, 22, crop=1, shuffle=True, res=True),                      # shuffle + residual on a 3x3, tall row
    _c("s3_q4_wrap_pad3", 3, 64, 192, 1, 23, 36, pad=3, sphere=2, ring=3, slope=False, res=True),        # nr 17
    # 3x3, NQ = 2 (cout = 96), nrg = 4: tall last row at rem 1 .. 4, the extra tile row at rem 5
    _c("s3_q2_rem1_cin16", 3, 16, 96, 1, 19, 24, ring=1, ring_w=2),                                      # one fp32 chunk (the bf16x3 form does not take 16)
    _c("s3_q2_rem1", 3, 32, 96, 1, 21, 22),                                                              # nr 17
    _c("s3_q2_rem2", 3, 32, 96, 1, 38, 36, sphere=2, res=True),                                          # nr 34
    _c("s3_q2_rem3", 3, 64, 96, 3, 23, 25),                                                              # nr 19
    _c("s3_q2_rem4", 3, 96, 96, 1, 24, 20, pad=1, ring=2, slope=False),                                  # nr 20; six fp32 chunks
    _c("s3_q2_rem5_plain", 3, 32, 96, 3, 23, 22, sphere=0, ring=1, ring_w=3),                            # nr 21: two tile rows
    _c("s3_q2_low", 3, 32, 96, 1, 13, 36, pad=3, ring=2),                                                # nr 9: full = 0
    _c("s3_q2_3rows_tall", 3, 192, 96, 1, 54, 20, ring=1),                                               # nr 52: three tile rows, the last one tall (rem 4)
    _c("s3_q2_shuffle_res", 3, 32, 96, 1, 20, 24, shuffle=True, res=True),                               # shuffle at crop 0
    # 1x1
    _c("s1_q4", 1, 32, 192, 1, 20, 36, res=True),                                                        # nr 16, nc 32 (exact)
    _c("s1_q4_3rows", 1, 96, 192, 1, 44, 24, slope=False, res=True),                                     # nr 40
    _c("s1_q4_low_crop", 1, 32, 192, 1, 11, 23, ring=1, crop=1),                                         # nr 9: full = 0
    _c("s1_q4_shuffle_768", 1, 192, 768, 1, 14, 22, crop=1, shuffle=True, slope=False, res=True),        # the up-sampling block's shortcut
    _c("s1_q4_n3", 1, 192, 384, 3, 20, 22, ring=1, ring_w=3),
    _c("s1_q2", 1, 192, 96, 3, 21, 37, ring=1, ring_w=3, slope=False),                                   # nr 19, nc 31 (ragged)
    _c("s1_q2_low", 1, 32, 96, 1, 9, 36),                                                                # nr 5: full = 0
    _c("s1_q2_shuffle", 1, 32, 96, 1, 20, 24, crop=1, shuffle=True),                                     # shuffle without residual
    _c("s1_q2_3rows", 1, 64, 96, 1, 40, 20, ring=1, res=True),                                           # nr 38
]

# ---- the calls lic360_models makes at the reference width (C = 192) for a 512 x 1024 image, as (shape, window, flags), read off its blocks
# and confirmed by wrapping lic360.sconv* with a recording function during CMP_Encoder / CMP_Decoder (the `_counting` wrapper of
# tests/test_gpu_sconv_bf16x3.py, keeping the arguments): ResidualBlockV2.conv1 (sphere 1, ring 1, ring_w 2) and .conv2 (sphere 2, ring 2, + x);
# ResidualBlockDown / Up.conv2 (sphere 1, ring 2, no PReLU: GDN follows); the AttentionBlock's bottleneck (1x1 192 -> 96, 3x3 96 -> 96, 1x1 96 -> 192 + x);
# ResidualBlockUp.conv1 (192 -> 768, crop 1, shuffled store) and its shortcut (1x1 192 -> 768, crop 1, shuffled store, + the shuffled branch).
# Maps: 36 x 68 (latent), 68 x 132, 132 x 260, 260 x 516; the models go fused from 256 workgroups per launch: recorded at batch 1, the 260 x 516
# layers and the 192 -> 768 pair at 132 x 260; at batch 8 (tools/transform_bench.py's chunk) every row below except those at 516 x 1028 and the
# 192 -> 768 pair at 260 x 516 and the bottleneck's 1x1 layers at 260 x 516, which are the same layers one up-sampling further (the sizes at which
# an image's activations pass 2^28 bytes).  The bottleneck (AttentionBlock) sits at 132 x 260 only.  Batch 1 here;
# tests/test_gpu_sconv_exact.py::test_past_4gib runs 22 images.
_MAPS = ((68, 132), (132, 260), (260, 516), (516, 1028))
_UP_MAPS = ((36, 68), (68, 132), (132, 260), (260, 516))                   # inputs of the 192 -> 768 layers (the last one: one up-sampling further, as 516 x 1028 above)
PRODUCTION = (
    [_c("v2_conv1_%dx%d" % m, 3, 192, 192, 1, m[0], m[1], ring=1, ring_w=2, prod=True) for m in _MAPS]
    + [_c("v2_conv2_%dx%d" % m, 3, 192, 192, 1, m[0], m[1], sphere=2, res=True, prod=True) for m in _MAPS]
    + [_c("gdn_conv2_%dx%d" % m, 3, 192, 192, 1, m[0], m[1], slope=False, prod=True) for m in _MAPS[:3]]
    + [_c("bottleneck_3x3_132x260", 3, 96, 96, 1, 132, 260, prod=True)]
    + [_c("up_conv1_%dx%d" % m, 3, 192, 768, 1, m[0], m[1], crop=1, shuffle=True, prod=True) for m in _UP_MAPS]
    + [_c("up_shortcut_%dx%d" % m, 1, 192, 768, 1, m[0], m[1], crop=1, shuffle=True, slope=False, res=True, prod=True) for m in _UP_MAPS]
    + [_c("bottleneck_in_%dx%d" % m, 1, 192, 96, 1, m[0], m[1], prod=True) for m in _MAPS[1:3]]
    + [_c("bottleneck_out_%dx%d" % m, 1, 96, 192, 1, m[0], m[1], slope=False, res=True, prod=True) for m in _MAPS[1:3]])
CASES = SMALL + PRODUCTION
PAST_4GIB = _c("v2_conv1_516x1028_n22", 3, 192, 192, 22, 516, 1028, ring=1, ring_w=2, prod=True)


# ---- the launch geometry, restated from sconv_ok / sconv_launch / sconv_workgroup (csrc/conv3x3_kernels.hip)
def chunk_of(b3, ks):
    return 32 if b3 or ks == 1 else 16


def supported(b3, cin, cout, ks):
    ck = chunk_of(b3, ks)
    return ks in (1, 3) and cin >= ck and cin % ck == 0 and cout >= 96 and (cout % 192 == 0 or cout == 96)


def tile_rows(nr, nq, ks=3):
    """(tile rows, tall last row?) of a window of nr rows: a remainder of at most 8 / NQ rows rides on the last tile row of a 3x3"""
    nrg, full, rem = 8 // nq, nr // 16, nr % 16
    tall = ks == 3 and 0 < rem <= nrg and full > 0
    return (full if tall else (nr + 15) // 16), tall


def branch_of(case, b3):
    c = case
    assert supported(b3, c.cin, c.cout, c.ks), (c.name, b3)
    nq = 4 if c.cout % 192 == 0 else 2
    nr = c.hp - 2 * c.ring
    tiles_y, tall = tile_rows(nr, nq, c.ks)
    rw = 16 // (8 // nq)
    return Branch(b3, nq, rw, rw + 1 if tall else rw, c.ks, c.cout // 192 if nq == 4 else 1, tiles_y, (c.wp - 2 * c.ring_w + 15) // 16,
                  nr % 16, nr // 16, tall, c.cin // chunk_of(b3, c.ks))


def forms_of(case):
    """(b3, tier) pairs a case runs in: the fp32 form on its own data, the bf16x3 form on each of its three tiers"""
    out = [(False, "fp32")] if supported(False, case.cin, case.cout, case.ks) else []
    if supported(True, case.cin, case.cout, case.ks):
        out += [(True, t) for t in B3_TIERS]
    return out


def out_shape(c):
    oh, ow = c.hp - 2 * c.crop, c.wp - 2 * c.crop
    return (c.n, c.cout // 4, 2 * oh, 2 * ow) if c.shuffle else (c.n, c.cout, oh, ow)


# ---- data
def _ints(rng, bound, shape):
    return rng.integers(-bound, bound + 1, shape, dtype=np.int32).astype(np.float32)


def make_case(case, tier):
    """integer-valued x, w, b, slope, res of a case in a tier, seeded by (case, tier).  Uniform random integers everywhere: every image, channel
    and cell differs from its neighbours, and the apron cells of x hold values of their own -- not what the sphere rule would put there -- so a
    loader that reads a stored apron cell where it must read the interior (or the other way round) changes the result."""
    c, (xm, wm) = case, TIERS[tier]
    rng = np.random.default_rng(_stable((case.name, tier)))
    return dict(x=_ints(rng, xm, (c.n, c.cin, c.hp, c.wp)), w=_ints(rng, wm, (c.cout, c.cin, c.ks, c.ks)), b=_ints(rng, 8, (c.cout,)),
                slope=rng.choice(np.array(SLOPES, np.float32), c.cout) if c.slope else None,
                res=_ints(rng, 8, out_shape(c)) if c.res else None)


def bf16_hi(v):
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).bfloat16().float().numpy()


def bf16_split(v):
    hi = bf16_hi(v)
    return hi, bf16_hi(v - hi)


def assert_exact_domain(case, data, tier):
    """max over outputs of |b| + 4 |res| + sum |w| |x| < 2^24 (module docstring), from the case's own data in float64"""
    mag = (lambda v: np.abs(v).astype(np.float64)) if tier == "fp32" else (lambda v: sum(np.abs(p).astype(np.float64) for p in bf16_split(v)))
    xmax = mag(data["x"]).max(axis=(0, 2, 3))                               # [cin]
    wsum = mag(data["w"]).sum(axis=(2, 3))                                  # [cout][cin]
    bound = float((wsum @ xmax + np.abs(data["b"])).max()) + (4.0 * float(np.abs(data["res"]).max()) if data["res"] is not None else 0.0)
    assert bound < EXACT_BELOW, "%s / %s: |b| + 4 |res| + sum |w||x| can reach %g >= 2^24" % (case.name, tier, bound)
    for k in ("x", "w", "b", "res"):
        assert data[k] is None or np.array_equal(data[k], np.rint(data[k])), k
    assert data["slope"] is None or np.isin(data["slope"], SLOPES).all()
    return bound


# ---- the reference
def source_cells(hp, wp, pad, sphere, mut=None):
    """the cell whose stored value a convolution reads for padded cell (ph, pw).  sphere 1: the interior cell the sphere puts there -- longitude
    wraps; across a pole the row reflects and the longitude turns by half a circle, which on the wrapped grid is the mirrored column; sphere 2:
    longitude wrap only, rows as stored; sphere 0: every cell as stored"""
    ph, pw = np.meshgrid(np.arange(hp), np.arange(wp), indexing="ij")
    if sphere == 0:
        return ph, pw
    H, W, th, tw = hp - 2 * pad, wp - 2 * pad, ph - pad, pw - pad
    off = 1 if mut == "wrap_off_by_one" else 0
    tw = np.where(tw < 0, tw + W - off, np.where(tw >= W, tw - W + off, tw))
    if sphere == 1 or mut == "sphere2_as_1":
        pole = (th < 0) | (th >= H)
        th = np.where(th < 0, -1 - th, np.where(th >= H, 2 * H - 1 - th, th))
        if mut != "pole_no_mirror":
            tw = np.where(pole, W - 1 - tw, tw)
    return th + pad, tw + pad


def shuffle2(y):
    """Dtow(2): channel 4 p + v of cell (r, c) -> channel p, cell (2 r + v / 2, 2 c + v % 2)"""
    n, c4, h, w = y.shape
    return np.ascontiguousarray(y.reshape(n, c4 // 4, 2, 2, h, w).transpose(0, 1, 4, 2, 5, 3)).reshape(n, c4 // 4, 2 * h, 2 * w)


def reference(case, data, mut=None):
    """the whole expected `out` of one call in float64, the untouched frame (SENTINEL) included.  `mut`: one of MUTATIONS -- the same computation
    with one bug a kernel could have (tests/test_sconv_cases_cpu.py: each must change the result)"""
    c = case
    x, w, b, slope, res = data["x"], data["w"], data["b"], data["slope"], data["res"]
    if mut == "x_lo_dropped":
        x = bf16_hi(x)
    if mut == "w_lo_dropped":
        w = bf16_hi(w)
    if mut == "prev_image":
        x = np.roll(x, 1, 0)
    if mut == "chunk_twice":
        x = x.copy()
        x[:, 32:64] = x[:, :32]
    if mut == "tap_dropped":
        w = w.copy()
        w[:, c.cin - 1, c.ks - 1, 0] = 0
    if mut == "kh_kw_swapped":
        w = np.ascontiguousarray(w.transpose(0, 1, 3, 2))
    if c.sphere:
        sh, sw = source_cells(c.hp, c.wp, c.pad, c.sphere, mut)
        x = x[:, :, sh, sw]
    y = F.conv2d(torch.from_numpy(np.ascontiguousarray(x)).double(), torch.from_numpy(w).double(), None, 1, c.ks // 2).numpy()    # the input grid
    y += (2.0 if mut == "bias_twice" else 1.0) * b.astype(np.float64)[None, :, None, None]
    if slope is not None:
        s = np.roll(slope, -4) if mut == "slope_co_plus_4" else slope
        y = np.where(y > 0, y, y * s.astype(np.float64)[None, :, None, None])
    oh, ow = c.hp - 2 * c.crop, c.wp - 2 * c.crop
    if res is not None and (not c.shuffle or mut == "res_unshuffled"):
        y[:, :, c.crop:c.hp - c.crop, c.crop:c.wp - c.crop] += res.reshape(c.n, c.cout, oh, ow)
    nq = 4 if c.cout % 192 == 0 else 2
    tiles_y, tall = tile_rows(c.hp - 2 * c.ring, nq, c.ks)
    if mut == "tile_row_shift":                                            # the last tile row computes the rows one below its own
        t0 = c.ring + (tiles_y - 1) * 16
        y[:, :, t0:] = np.roll(y[:, :, t0:], -1, 2)
    ring_w = c.ring if mut == "ring_for_ring_w" else c.ring_w
    if mut == "tile_col_shift":
        t0 = c.ring_w + ((c.wp - 2 * c.ring_w + 15) // 16 - 1) * 16
        y[:, :, :, t0:] = np.roll(y[:, :, :, t0:], -1, 3)
    y = y[:, :, c.crop:c.hp - c.crop, c.crop:c.wp - c.crop]
    r0, r1, c0, c1 = c.ring - c.crop, c.hp - c.ring - c.crop, ring_w - c.crop, c.wp - ring_w - c.crop
    if mut == "tall_last_row_missing":
        r1 -= 1
    if c.shuffle:
        y = shuffle2(y)
        r0, r1, c0, c1 = 2 * r0, 2 * r1, 2 * c0, 2 * c1
        if res is not None and mut != "res_unshuffled":
            y = y + res
    out = np.full(out_shape(c), SENTINEL, np.float64)
    out[:, :, r0:r1, c0:c1] = y[:, :, r0:r1, c0:c1]
    return out


# mutation -> does it apply to (case, tier)?  (window row `ring` reads row ring - 1: an apron row iff ring <= pad; likewise the columns)
MUTATIONS = {
    "pole_no_mirror": lambda c, t: c.ks == 3 and c.sphere == 1 and c.ring <= c.pad,           # pole rows reflected but not mirrored in longitude
    "wrap_off_by_one": lambda c, t: c.ks == 3 and c.sphere in (1, 2) and c.ring_w <= c.pad,    # longitude wrap off by one column
    "sphere2_as_1": lambda c, t: c.ks == 3 and c.sphere == 2 and c.ring <= c.pad,              # the wrap-only mode read through the full sphere rule
    "tall_last_row_missing": lambda c, t: tile_rows(c.hp - 2 * c.ring, 4 if c.cout % 192 == 0 else 2, c.ks)[1],
    "tile_row_shift": lambda c, t: True,
    "tile_col_shift": lambda c, t: True,
    "ring_for_ring_w": lambda c, t: c.ring != c.ring_w,                                        # the window test with ring where ring_w belongs
    "slope_co_plus_4": lambda c, t: c.slope,
    "res_unshuffled": lambda c, t: c.shuffle and c.res,                                        # the residual read with the unshuffled index
    "bias_twice": lambda c, t: True,
    "tap_dropped": lambda c, t: True,
    "kh_kw_swapped": lambda c, t: c.ks == 3,
    "chunk_twice": lambda c, t: c.cin >= 64,                                                   # channels 32 .. 63 read from chunk 0
    "x_lo_dropped": lambda c, t: t == "xlo",
    "w_lo_dropped": lambda c, t: t == "wlo",
    "prev_image": lambda c, t: c.n >= 2,                                                       # image n reads image n - 1
}


def describe_mismatch(case, b3, got, want):
    """where a wrong output sits in the kernel's own terms: these kernels fail by tile"""
    c, br = case, branch_of(case, b3)
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return "equal"
    def grid(idx):
        n, ch, row, col = (int(v) for v in idx)
        if c.shuffle:
            return n, 4 * ch + 2 * (row % 2) + col % 2, row // 2 + c.crop, col // 2 + c.crop
        return n, ch, row + c.crop, col + c.crop
    n, co, ph, pw = grid(bad[0])
    msg = "%s %s: %d of %d cells differ; first at out%s = %r, expected %r" % (
        c.name, "bf16x3" if b3 else "fp32", len(bad), got.size, tuple(int(v) for v in bad[0]), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))
    rows = bad[:, 2] // 2 + c.crop if c.shuffle else bad[:, 2] + c.crop
    ty_all = np.clip((rows - c.ring) // 16, 0, br.tiles_y - 1)
    inside = c.ring <= ph < c.hp - c.ring and c.ring_w <= pw < c.wp - c.ring_w
    if inside:
        ty = min((ph - c.ring) // 16, br.tiles_y - 1)
        local, rwb = ph - c.ring - 16 * ty, (br.rw_last if ty == br.tiles_y - 1 else br.rw)
        msg += "; (n, co, row, col) = (%d, %d, %d, %d): tile (ty, tx) = (%d, %d), blockIdx.y %d, wave (mq, nh) = (%d, %d), accumulator m %d row %d (kq %d, v %d)" % (
            n, co, ph, pw, ty, (pw - c.ring_w) // 16, co // (br.nq * 48), co % (br.nq * 48) // 48, local // rwb, co % 48 // 16, local % rwb, co % 16 // 4, co % 4)
    else:
        msg += "; (n, co, row, col) = (%d, %d, %d, %d) lies OUTSIDE the window (a frame cell was written)" % (n, co, ph, pw)
    return msg + "; wrong cells per tile row: %s" % dict(zip(*(v.tolist() for v in np.unique(ty_all, return_counts=True))))


# ==== GDN
GdnCase = collections.namedtuple("GdnCase", "name c n h w inverse misaligned prod")
GDN_SMALL = [
    GdnCase("g16_odd_small", 16, 1, 5, 7, False, False, False),            # P = 35: odd, below one tile
    GdnCase("g16_one_tile", 16, 1, 8, 8, True, False, False),              # P = 64
    GdnCase("g32_p66", 32, 3, 6, 11, False, False, False),                 # P % 4 == 2
    GdnCase("g32_two_tiles", 32, 1, 8, 16, True, False, False),            # P = 128
    GdnCase("g48_p65", 48, 1, 5, 13, True, False, False),                  # P = 64 + 1
    GdnCase("g48_vec", 48, 1, 12, 16, False, False, False),
    GdnCase("g64_misaligned", 64, 1, 8, 8, False, True, False),            # P % 4 == 0 through a view 4 bytes past a 16-byte boundary
    GdnCase("g64_vec_n3", 64, 3, 4, 20, True, False, False),
    GdnCase("g96_odd", 96, 1, 9, 15, True, False, False),
    GdnCase("g96_vec", 96, 1, 16, 20, False, False, False),                # P = 320 = 5 * 64
    GdnCase("g128_p130", 128, 1, 10, 13, False, False, False),
    GdnCase("g128_vec", 128, 1, 16, 16, True, False, False),
    GdnCase("g192_odd_n3", 192, 3, 21, 37, False, False, False),           # P = 777
    GdnCase("g192_vec", 192, 1, 12, 20, False, False, False),
    GdnCase("g192_misaligned", 192, 1, 12, 20, True, True, False),
]
# lic360_operator.GDN calls gdn_forward behind ResidualBlockDown.conv2 (forward; analysis side) and ResidualBlockUp.conv2 (inverse; synthesis side),
# on the whole padded map; 516 x 1028 as in PRODUCTION
GDN_PRODUCTION = [GdnCase("down_%dx%d" % m, 192, 1, m[0], m[1], False, False, True) for m in _MAPS[:3][::-1]] + \
                 [GdnCase("up_%dx%d" % m, 192, 1, m[0], m[1], True, False, True) for m in _MAPS]
GDN_CASES = GDN_SMALL + GDN_PRODUCTION
GDN_CHANNELS = (16, 32, 48, 64, 96, 128, 192)


def gdn_branch_of(case):
    """(CT, VEC) of k_gdn<CT, VEC>: lic360_gdn takes the 16-byte form iff P % 4 == 0 and x and out sit on 16-byte boundaries"""
    p = case.h * case.w
    return case.c // 16, p % 4 == 0 and not case.misaligned


def gdn_make(case, n=None):
    rng = np.random.default_rng(_stable(("gdn", case.name)))
    c = case.c
    return dict(x=_ints(rng, 15, (case.n if n is None else n, c, case.h, case.w)), gamma=rng.integers(0, 4, (c, c)).astype(np.float32),
                beta=rng.integers(1, 17, (c,)).astype(np.float32))


def gdn_sums(data, mut=None):
    """beta[i] + sum_j gamma[i][j] x[j]^2 in float64 (exact: integers far below 2^53)"""
    x, gamma, beta = data["x"].astype(np.float64), data["gamma"].astype(np.float64), data["beta"].astype(np.float64)
    n, c, h, w = x.shape
    sq = (x if mut == "x_not_squared" else x * x).reshape(n, c, h * w)
    if mut == "last_tile_zeroed":
        sq[:, :, (h * w) // 64 * 64:] = 0
    if mut == "slab_twice":
        sq[:, 16:32] = sq[:, :16]
    if mut == "gamma_transposed":
        gamma = gamma.T
    if mut == "beta_plus_4":
        beta = np.roll(beta, -4)
    return (np.matmul(gamma[None], sq) + beta[None, :, None]).reshape(n, c, h, w)


def gdn_assert_exact_domain(case, data):
    xmax = (data["x"].astype(np.float64) ** 2).max(axis=(0, 2, 3))
    bound = float((data["gamma"].astype(np.float64) @ xmax + data["beta"]).max())
    assert bound < EXACT_BELOW and float(data["beta"].min()) >= 1 and float(data["gamma"].min()) >= 0, (case.name, bound)
    return bound


def gdn_reference(case, data, mut=None):
    """float32: x / sqrt(s) (x * sqrt(s) for the inverse), s the exact integer sum; numpy's float32 sqrt, / and * are correctly rounded"""
    x = data["x"]
    with np.errstate(invalid="ignore", divide="ignore"):                   # (only a mutation takes the root of a negative sum)
        norm = np.sqrt(gdn_sums(data, mut).astype(np.float32))
        return x * norm if (case.inverse and mut != "inverse_ignored") else x / norm


def gdn_perfect_squares(data):
    """cells whose sum is a perfect square: norm is an integer there, and equality must hold even under an approximate square root"""
    s = gdn_sums(data)
    r = np.rint(np.sqrt(s))
    return r * r == s


GDN_MUTATIONS = {
    "gamma_transposed": lambda c: True,
    "x_not_squared": lambda c: True,
    "beta_plus_4": lambda c: True,
    "last_tile_zeroed": lambda c: (c.h * c.w) % 64 != 0,
    "slab_twice": lambda c: c.c >= 32,
    "inverse_ignored": lambda c: c.inverse,
}
