"""Cases of the split-bf16 ("bf16x3") one-pass GDN (csrc/gdn_bf16x3.inc, kernels k_gdn_b3<C, VEC>, lic360.gdn_bf16x3_forward): the case list, the
launch geometry, integer data on which the kernel has ONE right answer, the reference that restates its arithmetic, and the real-valued data and the
float64 GDN of the parity test.  No GPU and nothing of `lic360` in here: tests/test_gdn_bf16x3_cases_cpu.py checks this file by itself,
tests/test_gpu_gdn_bf16x3_exact.py and tests/test_gpu_gdn_bf16x3.py compare the kernel with it.

The contract.  sq = x * x in fp32; sq and the effective gamma are each split into hi = bf16(v) and lo = bf16(v - hi), round to nearest even (written at
bit level in tests/sconv_bf16x1_cases.py: `bf16_rne`); s = beta + sum_j (g_hi sq_hi + g_hi sq_lo + g_lo sq_hi) accumulated in fp32, g_lo sq_lo dropped;
then one correctly rounded fp32 square root and one correctly rounded fp32 division (or product) on the unrounded x.

The method is sconv_cases.py's: on integer data whose every partial sum stays below 2^24 the three kept products add to one fp32 number whatever the
order, so the output must EQUAL numpy's float32 x / sqrt(s).  Three tiers:

    tier   |x| <=   gamma                               proves
    hi         15   0 .. 3                              nothing splits (x^2 <= 225 is a bf16 number): loader, pack order, position order, epilogue
    xsq       255   0, 1                                x^2 needs hi + lo, both exact integers: the g_hi sq_lo term, computed once, from the right cell
    both       20   0 .. 3, a few per row 257 .. 511    both operands have lo parts: the g_lo sq_hi term, the pack's lo planes, and that lo lo is DROPPED

In tier `both` the reference differs from the plain sum by exactly the dropped terms.  beta is drawn from 1 .. 1023 in every tier: most such values are
not bf16 numbers, so an epilogue that rounds beta changes the result.  What rounding does to the split operands: every odd integer of 256 .. 512 is a tie
(the `both` tier's large gammas: ties to both sides); squares up to 255^2 round up, round down and tie -- a square that ties always ties DOWN (it is 4^k
times an odd square of nine bits, 289 .. 484, and odd squares are 1 mod 8).  |x| <= 255 is itself a bf16
number, so "x rounded before squaring" cannot show on integers; it is told apart on the real-valued data, where it breaks the bound (emulate)."""
import numpy as np

import sconv_cases as sc
from sconv_cases import GdnCase, _MAPS, SENTINEL, EXACT_BELOW, GDN_MUTATIONS  # noqa: F401
from sconv_bf16x1_cases import bf16_rne, bf16_truncate, rounding_classes
from util import _stable

PT = 64                                                                     # GB3_PT: positions per workgroup, the tile of k_gdn's cases too
CHANNELS = (32, 64, 96, 128, 192)
TIERS = ("hi", "xsq", "both")
BOUND = 2.0 ** -15                                                          # relative, per element, against the float64 GDN (gamma >= 0)

SMALL = [
    GdnCase("b32_odd_small", 32, 1, 5, 7, False, False, False),             # P = 35: odd, below one tile
    GdnCase("b32_one_tile", 32, 1, 8, 8, True, False, False),               # P = 64
    GdnCase("b32_p66_n3", 32, 3, 6, 11, False, False, False),               # P % 4 == 2, n = 3
    GdnCase("b64_p65", 64, 1, 5, 13, True, False, False),                   # one tile + 1
    GdnCase("b64_misaligned", 64, 1, 8, 8, False, True, False),             # P % 4 == 0 through a view 4 bytes past a 16-byte boundary
    GdnCase("b64_vec_n3", 64, 3, 4, 20, True, False, False),
    GdnCase("b96_odd", 96, 1, 9, 15, True, False, False),                   # P = 135
    GdnCase("b96_vec", 96, 1, 16, 20, False, False, False),                 # P = 320 = 5 tiles
    GdnCase("b128_p130", 128, 1, 10, 13, False, False, False),              # P % 4 == 2, two tiles + 2
    GdnCase("b128_vec", 128, 1, 16, 16, True, False, False),                # four tiles
    GdnCase("b192_odd_n3", 192, 3, 21, 37, False, False, False),            # P = 777
    GdnCase("b192_vec", 192, 1, 12, 20, False, False, False),               # P = 240
    GdnCase("b192_misaligned", 192, 1, 12, 20, True, True, False),
]
# the six GDN calls of one image pair: ResidualBlockDown (forward, analysis) and ResidualBlockUp (inverse, synthesis) on the whole padded map
PRODUCTION = [GdnCase("down_%dx%d" % m, 192, 1, m[0], m[1], False, False, True) for m in _MAPS[:3][::-1]] + \
             [GdnCase("up_%dx%d" % m, 192, 1, m[0], m[1], True, False, True) for m in _MAPS[:3]]
CASES = SMALL + PRODUCTION
INSTANTIATIONS = {(c, v) for c in CHANNELS for v in (True, False)}          # every k_gdn_b3<C, VEC>


# ---- the launch geometry, restated from lic360_gdn_bf16x3 / k_gdn_b3 (csrc/gdn_bf16x3.inc)
def supported(c):
    return c in CHANNELS


def branch_of(case):
    """(C, VEC) of k_gdn_b3<C, VEC>: the 16-byte form iff P % 4 == 0 and x and out sit on 16-byte boundaries"""
    return case.c, (case.h * case.w) % 4 == 0 and not case.misaligned


def wave_split(c):
    """(channel groups, position groups, row tiles per wave, position tiles per wave) of the four waves"""
    ncg = 4 if c // 16 % 4 == 0 else 2
    return ncg, 4 // ncg, c // 16 // ncg, ncg


def packed_layout(gamma):
    """the pack restated: [cg][s < C / 32][m < MT][hl][lane = 16 kq + i][j < 8] = part hl of gamma[16 (cg MT + m) + i][32 s + 8 kq + j], as float32 values"""
    c = gamma.shape[0]
    ncg, _, mt, _ = wave_split(c)
    hi = bf16_rne(gamma)
    parts = np.stack([hi, bf16_rne(gamma - hi)])                            # [hl][row][col]
    v = parts.reshape(2, ncg, mt, 16, c // 32, 4, 8)                        # hl, cg, m, i, s, kq, j
    return np.ascontiguousarray(v.transpose(1, 4, 2, 0, 5, 3, 6)).reshape(-1)   # cg, s, m, hl, kq, i, j


# ---- integer data
def make(case, tier, n=None):
    rng = np.random.default_rng(_stable(("gdn_b3", case.name, tier)))
    c, shape = case.c, (case.n if n is None else n, case.c, case.h, case.w)
    beta = rng.integers(1, 1024, (c,)).astype(np.float32)
    if tier == "hi":
        return dict(x=sc._ints(rng, 15, shape), gamma=rng.integers(0, 4, (c, c)).astype(np.float32), beta=beta)
    if tier == "xsq":
        return dict(x=sc._ints(rng, 255, shape), gamma=rng.integers(0, 2, (c, c)).astype(np.float32), beta=beta)
    gamma = rng.integers(0, 4, (c, c)).astype(np.float32)
    for i in range(c):                                                      # three large entries per row, at least one tie to each side
        cols = rng.choice(c, 3, replace=False)
        gamma[i, cols] = (257 + 4 * rng.integers(0, 64), 259 + 4 * rng.integers(0, 64), rng.integers(257, 512))
    return dict(x=sc._ints(rng, 20, shape), gamma=gamma, beta=beta)


def split(v, rnd=bf16_rne):
    hi = rnd(v)
    return hi, rnd((np.asarray(v, np.float32) - hi).astype(np.float32))


def assert_exact_domain(case, data):
    """beta + sum |gamma parts| |x^2 parts| < 2^24 for every output (x^2 by its per-channel maximum of |hi| + |lo|), all values integers, gamma >= 0, beta >= 1"""
    x = data["x"]
    sq = (x * x).astype(np.float32)
    mag = lambda v: sum(np.abs(p).astype(np.float64) for p in split(v))
    bound = float((mag(data["gamma"]) @ mag(sq).max(axis=(0, 2, 3)) + data["beta"]).max())
    assert bound < EXACT_BELOW, (case.name, bound)
    assert float(data["beta"].min()) >= 1 and float(data["gamma"].min()) >= 0
    for k in ("x", "gamma", "beta"):
        assert np.array_equal(data[k], np.rint(data[k])), k
    return bound


def sums(data, mut=None):
    """beta[i] + sum_j of the three kept products in float64 (exact: integers far below 2^53).  `mut`: one of MUTATIONS"""
    x, gamma, beta = data["x"], data["gamma"], data["beta"].astype(np.float64)
    n, c, h, w = x.shape
    rnd = bf16_truncate if mut == "truncation" else bf16_rne
    sq = (x if mut == "x_not_squared" else (x * x).astype(np.float32)).reshape(n, c, h * w).copy()
    if mut == "last_tile_zeroed":
        sq[:, :, (h * w) // PT * PT:] = 0
    if mut == "slab_twice":
        sq[:, 16:32] = sq[:, :16]
    if mut == "gamma_transposed":
        gamma = np.ascontiguousarray(gamma.T)
    if mut == "beta_plus_4":
        beta = np.roll(beta, -4)
    if mut == "beta_rounded":
        beta = bf16_rne(data["beta"]).astype(np.float64)
    (gh, gl), (sh, sl) = (tuple(p.astype(np.float64) for p in split(v, rnd)) for v in (gamma, sq))
    if mut == "lo_dropped":
        gl, sl = 0 * gl, 0 * sl
    s = np.matmul(gh[None], sh) + np.matmul(gh[None], sl) + np.matmul(gl[None], sh)
    if mut == "lo_lo_added":
        s = s + np.matmul(gl[None], sl)
    return (s + beta[None, :, None]).reshape(n, c, h, w)


def reference(case, data, mut=None):
    """float32: x / sqrt(s) (x * sqrt(s) for the inverse) with numpy's correctly rounded float32 sqrt, / and *"""
    x = data["x"]
    with np.errstate(invalid="ignore", divide="ignore"):                   # (only a mutation takes the root of a negative sum)
        norm = np.sqrt(sums(data, mut).astype(np.float32))
        return x * norm if (case.inverse and mut != "inverse_ignored") else x / norm


def perfect_squares(data):
    s = sums(data)
    r = np.rint(np.sqrt(s))
    return r * r == s


# mutation -> does it apply to (case, tier)?  sconv_cases.GDN_MUTATIONS' six, and this form's arithmetic
MUTATIONS = dict({m: (lambda c, t, f=f: f(c)) for m, f in GDN_MUTATIONS.items()}, **{
    "lo_dropped": lambda c, t: t in ("xsq", "both"),                       # hi parts only: the single-pass form
    "lo_lo_added": lambda c, t: t == "both",                               # the fourth product
    "truncation": lambda c, t: t == "both",                                # parts chopped, not rounded (xsq: gamma has no lo and hi + lo = x^2 either way)
    "beta_rounded": lambda c, t: True,
})


# ---- real-valued data: the parity test's
def real_params(c, seed):
    """RAW parameters of a GDN module (lic360_operator.GDN's `gamma`, `beta`) with a dense non-negative effective gamma: the initial 0.1 I plus
    |N(0, 0.02)| everywhere, beta 1 +- 0.5, each behind the module's square-root reparametrisation"""
    rng = np.random.default_rng(_stable(("gdn_b3_params", c, seed)))
    ped = (2.0 ** -18) ** 2
    gamma = 0.1 * np.eye(c) + np.abs(rng.normal(0, 0.02, (c, c)))
    beta = 1.0 + rng.uniform(-0.5, 0.5, (c,))
    return np.sqrt(gamma + ped).astype(np.float32), np.sqrt(beta + ped).astype(np.float32)


def effective(raw_gamma, raw_beta, beta_min=1e-6, reparam_offset=2.0 ** -18):
    """GDN.forward's reparametrisation in float32 numpy: max(p, bound)^2 - pedestal"""
    ped = np.float32(reparam_offset ** 2)
    gb, bb = np.float32(reparam_offset), np.float32(np.sqrt(beta_min + reparam_offset ** 2))
    return np.maximum(raw_gamma, gb) ** 2 - ped, np.maximum(raw_beta, bb) ** 2 - ped


def real_x(c, scale, n=2, h=9, w=15):
    rng = np.random.default_rng(_stable(("gdn_b3_x", c, scale)))
    return (scale * rng.standard_normal((n, c, h, w))).astype(np.float32)


def gdn_float64(x, gamma, beta, inverse):
    """the GDN of the fp32 operands in float64: what the bound is stated against"""
    n, c = x.shape[:2]
    xd = x.astype(np.float64).reshape(n, c, -1)
    norm = np.sqrt(np.matmul(gamma.astype(np.float64)[None], xd * xd) + beta.astype(np.float64)[None, :, None])
    return (xd * norm if inverse else xd / norm).reshape(x.shape)


def emulate(x, gamma, beta, inverse, mode="bf16x3"):
    """the kernel's operand arithmetic with float64 sums: "bf16x3" (the three kept products), "hi_only" (no lo parts: a single-pass form) or
    "x_rounded" (bf16x3 with x rounded to bf16 BEFORE squaring); square root and division in float64 on the unrounded x"""
    n, c = x.shape[:2]
    xs = bf16_rne(x) if mode == "x_rounded" else x
    sq = (xs * xs).astype(np.float32).reshape(n, c, -1)
    (gh, gl), (sh, sl) = (tuple(p.astype(np.float64) for p in split(v)) for v in (gamma, sq))
    s = np.matmul(gh[None], sh)
    if mode != "hi_only":
        s = s + np.matmul(gh[None], sl) + np.matmul(gl[None], sh)
    norm = np.sqrt(s + beta.astype(np.float64)[None, :, None])
    xd = x.astype(np.float64).reshape(n, c, -1)
    return (xd * norm if inverse else xd / norm).reshape(x.shape)


def max_rel_err(got, want):
    """max over elements of |got - want| / |want| (elements with want == 0 must be 0 in got)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    zero = want == 0
    assert np.array_equal(got[zero], want[zero])
    return float((np.abs(got - want)[~zero] / np.abs(want[~zero])).max())
