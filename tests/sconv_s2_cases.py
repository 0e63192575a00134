"""Exact-data cases of the stride-2 sphere convolutions (lic360_sconv3x3s2 / lic360_sconv1x1s2, the stride-2 forms of the body in
csrc/conv3x3_kernels.hip): data, float64 references and the launch geometry the native code will pick.  No GPU and nothing of `lic360` in here;
the method, the data makers, the sentinel, the sphere rule and the exactness condition are those of tests/sconv_cases.py (integer data: one fp32
result whatever the summation order, so a kernel returns the reference bit for bit or is wrong).  tests/test_sconv_s2_cases_cpu.py checks this file
by itself, tests/test_gpu_sconv_s2_exact.py compares the kernels with it.

The operation.  x [n][cin][hp][wp] carries a `pad`-cell apron around an even interior H x W; X(r, c) is the value at interior coordinates (r, c)
after the sphere rule (sphere 1: apron cells come from the interior -- longitude wrap, pole rows reflected and mirrored; sphere 0: as stored).
out [n][cout][H / 2 + 2 oring][W / 2 + 2 oring]; its interior window is
    3x3:  bias + sum w[kh][kw] X(2 i + kh - 1, 2 j + kw - 1)      (Conv2d(cin, c, 3, stride 2, padding 3) behind SpherePad(2))
    1x1:  bias + w X(2 i, 2 j)                                    (Conv2d(cin, c, 1, stride 2, padding 2))
then PReLU, then + residual (the OUTPUT's geometry); every other cell of out keeps what it held (SENTINEL)."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

from sconv_cases import SENTINEL, SLOPES, TIERS, _ints, assert_exact_domain, source_cells          # noqa: F401  (re-exported for the tests)
from util import _stable

Case = collections.namedtuple("Case", "name ks cin cout n hp wp pad sphere oring slope res prod")
Branch = collections.namedtuple("Branch", "nq rw ks blocks_y tiles_y tiles_x rem full chunks")


def _c(name, ks, cin, cout, n, oh, ow, pad=2, sphere=1, oring=2, slope=True, res=False, prod=False):
    """a case by its OUTPUT window oh x ow: the input map is (2 oh + 2 pad) x (2 ow + 2 pad)"""
    if ks == 1:
        sphere = 0                                                         # the 1x1 entry point reads the interior only and takes no sphere flag
    return Case(name, ks, cin, cout, n, 2 * oh + 2 * pad, 2 * ow + 2 * pad, pad, sphere, oring, slope, res, prod)


# ---- the branch matrix on small maps.  A tile is 16 x 16 outputs; there is no tall last tile row at stride 2: a remainder takes an extra tile row
SMALL = [
    # 3x3, NQ = 4 (cout a multiple of 192)
    _c("d3_q4_one_tile", 3, 32, 192, 1, 16, 16),                                                        # exactly one tile
    _c("d3_q4_rows_n3", 3, 32, 192, 3, 21, 16, res=True),                                               # ragged rows: the extra tile row holds 5; n = 3
    _c("d3_q4_cols_plain_pad3", 3, 16, 192, 1, 16, 21, pad=3, sphere=0, slope=False),                   # ragged columns; one chunk; apron as stored
    _c("d3_q4_low_192", 3, 192, 192, 1, 5, 24, res=True),                                               # full = 0; twelve chunks
    _c("d3_q4_384_rem1", 3, 32, 384, 1, 17, 18, oring=1),                                               # blockIdx.y 0 .. 1; an extra tile row of one row
    _c("d3_q4_pad3_sphere", 3, 64, 192, 1, 18, 16, pad=3, oring=0, slope=False, res=True),              # pad 3 under the sphere rule; no frame at all
    # 3x3, NQ = 2 (cout = 96)
    _c("d3_q2_one_tile_cin16", 3, 16, 96, 1, 16, 16),
    _c("d3_q2_rem_n3_pad3", 3, 32, 96, 3, 19, 33, pad=3, slope=False, res=True),
    _c("d3_q2_low_192_plain", 3, 192, 96, 1, 7, 16, sphere=0),
    # 1x1
    _c("d1_q4_one_tile", 1, 32, 192, 1, 16, 16, slope=False, res=True),
    _c("d1_q4_ragged_n3", 1, 192, 384, 3, 21, 19, pad=3),
    _c("d1_q4_low", 1, 32, 192, 1, 6, 32, oring=0),
    _c("d1_q2_ragged", 1, 64, 96, 1, 18, 21, res=True),
    _c("d1_q2_low_192", 1, 192, 96, 1, 3, 16, slope=False),
    _c("d1_q2_one_tile_pad3_n3", 1, 32, 96, 3, 16, 16, pad=3),
]

# ---- the calls lic360_models makes at the reference width (C = 192) for a 512 x 1024 image: ResidualBlockDown.conv1 (+ PReLU) and .short_cut (+ the
# GDN branch as residual) of stages 2 and 3, and SphereConv2 (no PReLU); input maps 260 x 516, 132 x 260, 68 x 132
PRODUCTION = [
    _c("down_conv1_260x516", 3, 192, 192, 1, 128, 256, prod=True),
    _c("down_conv1_132x260", 3, 192, 192, 1, 64, 128, prod=True),
    _c("sphereconv2_68x132", 3, 192, 192, 1, 32, 64, slope=False, prod=True),
    _c("down_shortcut_260x516", 1, 192, 192, 1, 128, 256, slope=False, res=True, prod=True),
    _c("down_shortcut_132x260", 1, 192, 192, 1, 64, 128, slope=False, res=True, prod=True),
]
CASES = SMALL + PRODUCTION


# ---- the launch geometry, restated from sconv_ok / sconv_plan's stride-2 branch (csrc/conv3x3_kernels.hip)
def chunk_of(ks):
    return 32 if ks == 1 else 16


def supported(cin, cout, ks):
    ck = chunk_of(ks)
    return ks in (1, 3) and cin >= ck and cin % ck == 0 and cout >= 96 and (cout % 192 == 0 or cout == 96)


def out_hw(c):
    return (c.hp - 2 * c.pad) // 2, (c.wp - 2 * c.pad) // 2


def out_shape(c):
    oh, ow = out_hw(c)
    return (c.n, c.cout, oh + 2 * c.oring, ow + 2 * c.oring)


def branch_of(case):
    c = case
    assert supported(c.cin, c.cout, c.ks), c.name
    nq = 4 if c.cout % 192 == 0 else 2
    oh, ow = out_hw(c)
    return Branch(nq, 16 // (8 // nq), c.ks, c.cout // 192 if nq == 4 else 1, (oh + 15) // 16, (ow + 15) // 16, oh % 16, oh // 16, c.cin // chunk_of(c.ks))


def make_case(case):
    """integer-valued operands in the fp32 tier of sconv_cases (|x| <= 8, |w| <= 4, |b|, |res| <= 8, slopes 1, 1/2, 1/4, 0), seeded by the case; the
    apron cells of x hold values of their own, so reading a stored apron cell where the sphere rule applies (or the reverse) changes the result"""
    c, (xm, wm) = case, TIERS["fp32"]
    rng = np.random.default_rng(_stable((case.name, "s2")))
    return dict(x=_ints(rng, xm, (c.n, c.cin, c.hp, c.wp)), w=_ints(rng, wm, (c.cout, c.cin, c.ks, c.ks)), b=_ints(rng, 8, (c.cout,)),
                slope=rng.choice(np.array(SLOPES, np.float32), c.cout) if c.slope else None,
                res=_ints(rng, 8, out_shape(c)) if c.res else None)


# ---- the reference
def reference(case, data, mut=None):
    """the whole expected `out` of one call in float64, the untouched frame (SENTINEL) included.  `mut`: one of MUTATIONS -- the same computation with
    one bug a stride-2 kernel could have (tests/test_sconv_s2_cases_cpu.py: each must change the result)"""
    c = case
    x, w, b, slope, res = data["x"], data["w"], data["b"], data["slope"], data["res"]
    oh, ow = out_hw(c)
    H, W = 2 * oh, 2 * ow
    assert c.pad >= 2                                                      # (the shifted-tile mutations look one output row / column past the window)
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
    # X(-k/2 .. H + 1, -k/2 .. W + 1): the cells the window's taps reach, and those of one more output row and column
    o = c.pad - c.ks // 2 + (1 if mut == "taps_on_2i_plus_1" else 0)
    xs = torch.from_numpy(np.ascontiguousarray(x[:, :, o:o + H + 2 + 2 * (c.ks // 2) - (1 if mut == "taps_on_2i_plus_1" else 0),
                                                 o:o + W + 2 + 2 * (c.ks // 2) - (1 if mut == "taps_on_2i_plus_1" else 0)])).double()
    stride = {"stride_rows_only": (2, 1), "stride_cols_only": (1, 2), "stride_1_read": (1, 1)}.get(mut, (2, 2))
    y = F.conv2d(xs, torch.from_numpy(w).double(), None, stride, 0).numpy()
    if mut == "taps_on_2i_plus_1":                                         # (one row / column short of the extended grid: repeat the last, it is not read below)
        y = np.pad(y, ((0, 0), (0, 0), (0, 1), (0, 1)), mode="edge")
    y = np.ascontiguousarray(y[:, :, :oh + 1, :ow + 1])                    # output (i, j), i <= oh, j <= ow: the window and one row / column past it
    y += (2.0 if mut == "bias_twice" else 1.0) * b.astype(np.float64)[None, :, None, None]
    if slope is not None:
        s = np.roll(slope, -4) if mut == "slope_co_plus_4" else slope
        y = np.where(y > 0, y, y * s.astype(np.float64)[None, :, None, None])
    if mut == "tile_row_shift":                                            # the last tile row computes the rows one below its own
        t0 = ((oh + 15) // 16 - 1) * 16
        y[:, :, t0:oh] = y[:, :, t0 + 1:oh + 1].copy()
    if mut == "tile_col_shift":
        t0 = ((ow + 15) // 16 - 1) * 16
        y[:, :, :, t0:ow] = y[:, :, :, t0 + 1:ow + 1].copy()
    y = y[:, :, :oh, :ow]
    r = c.oring
    if res is not None:
        if mut == "res_on_input_grid":                                     # the residual of window cell (i, j) read at the input grid's pitch and plane size
            n_, co_, i_, j_ = np.meshgrid(np.arange(c.n), np.arange(c.cout), np.arange(oh), np.arange(ow), indexing="ij")
            flat = ((n_ * c.cout + co_) * (c.hp * c.wp) + (r + i_) * c.wp + (r + j_)) % res.size
            y = y + res.ravel()[flat]
        else:
            y = y + res[:, :, r:r + oh, r:r + ow]
    out = np.full(out_shape(c), SENTINEL, np.float64)
    out[:, :, r:r + oh, r:r + ow] = y
    return out


# mutation -> does it apply to a case?
MUTATIONS = {
    # the stride's own
    "taps_on_2i_plus_1": lambda c: True,                                    # taps centred on 2 i + 1 (the other parity of the interior)
    "stride_rows_only": lambda c: True,                                     # columns read at stride 1
    "stride_cols_only": lambda c: True,                                     # rows read at stride 1
    "stride_1_read": lambda c: True,                                        # the top-left quarter of the stride-1 result
    "res_on_input_grid": lambda c: c.res,                                   # the residual indexed with the input's geometry
    # shared with the stride-1 cases (row -1 and column -1 of X are always read by a 3x3: a pole row, a wrapped column)
    "pole_no_mirror": lambda c: c.ks == 3 and c.sphere == 1,
    "wrap_off_by_one": lambda c: c.ks == 3 and c.sphere == 1,
    "tile_row_shift": lambda c: True,
    "tile_col_shift": lambda c: True,
    "bias_twice": lambda c: True,
    "tap_dropped": lambda c: True,
    "kh_kw_swapped": lambda c: c.ks == 3,
    "chunk_twice": lambda c: c.cin >= 64,
    "prev_image": lambda c: c.n >= 2,
    "slope_co_plus_4": lambda c: c.slope,
}


def describe_mismatch(case, got, want):
    """where a wrong output sits in the kernel's own terms: tile, wave, accumulator"""
    c, br = case, branch_of(case)
    oh, ow = out_hw(c)
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return "equal"
    n, co, row, col = (int(v) for v in bad[0])
    msg = "%s stride 2: %d of %d cells differ; first at out%s = %r, expected %r" % (
        c.name, len(bad), got.size, (n, co, row, col), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))
    i, j = row - c.oring, col - c.oring
    if 0 <= i < oh and 0 <= j < ow:
        local = i % 16
        msg += "; output (i, j) = (%d, %d): tile (ty, tx) = (%d, %d), blockIdx.y %d, wave (mq, nh) = (%d, %d), accumulator m %d row %d (kq %d, v %d)" % (
            i, j, i // 16, j // 16, co // (br.nq * 48), co % (br.nq * 48) // 48, local // br.rw, co % 48 // 16, local % br.rw, co % 16 // 4, co % 4)
    else:
        msg += "; (row, col) = (%d, %d) lies OUTSIDE the window (a frame cell was written)" % (row, col)
    ty_all = np.clip((bad[:, 2] - c.oring) // 16, 0, br.tiles_y - 1)
    return msg + "; wrong cells per tile row: %s" % dict(zip(*(v.tolist() for v in np.unique(ty_all, return_counts=True))))
