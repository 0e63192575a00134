"""Exact-data cases of the single-pass bf16 ("bf16x1") form of the sphere convolutions (csrc/sconv_bf16x3.inc with NT = 1, kernels k_sconv_b1): the
case list, launch geometry, sphere rule and float64 reference of tests/sconv_cases.py (the geometry is the bf16x3 form's: `branch_of(case, True)`), with
this form's own arithmetic in front.  No GPU and nothing of `lic360` in here: tests/test_sconv_bf16x1_cases_cpu.py checks this file by itself,
tests/test_gpu_sconv_bf16x1_exact.py compares the kernels with it.

The contract.  Every input value and every weight is rounded once to bf16, round to nearest even; each product is one v_mfma_f32_16x16x32_bf16 with fp32
accumulation; bias, PReLU and residual are applied in fp32, unrounded.  The reference is therefore the float64 convolution of the ROUNDED operands, and
the rounding is written here at bit level in numpy (`bf16_rne`), not borrowed from a library.

The method is sconv_cases.py's: on integer data whose every partial sum stays below 2^24 the result is one fp32 number whatever the summation order (the
bf16 MFMA adds such integers exactly: tests/test_gpu_sconv_exact.py), and a kernel either returns it bit for bit or is wrong.  Three tiers:

    tier   |x| <=   |w| <=   proves
    hi        255        7   nothing rounds: loader, pack order, epilogue
    xrnd     2047        2   x is rounded, once, to nearest even: values that round up, values that round down, ties to both sides
    wrnd        4     1023   the same for w (the pack kernel's rounding)

In the rounding tiers a quarter of the operand's values come from a list that holds each rounding class at each binade in reach (257 -> 256, 259 -> 260,
261 -> 260, 263 -> 264, 513 -> 512, 2047 -> 2048, ... and their negatives), the rest are uniform; `rounding_classes` names the classes a tensor holds and
the CPU test requires all four in every case.  Bias and residual are drawn up to 1023 in every tier -- most such values are NOT bf16 numbers, so an
epilogue that rounds them changes the result.  The exactness condition is sconv_cases.assert_exact_domain's, computed on the rounded operands:
for every output |b| + 4 |res| + sum |w~||x~| < 2^24."""
import numpy as np

import sconv_cases as sc
from sconv_cases import CASES, PAST_4GIB, Case, branch_of, out_shape, supported, describe_mismatch, SENTINEL, EXACT_BELOW, SLOPES  # noqa: F401
from util import _stable

TIERS = {"hi": (255, 7), "xrnd": (2047, 2), "wrnd": (4, 1023)}             # tier -> (max |x|, max |w|)
EPILOGUE_MAX = 1023                                                         # |b|, |res| <= this, in every tier
# magnitudes that need rounding, by what happens to them (bf16 keeps 8 significant bits: steps of 2 from 256, 4 from 512, 8 from 1024)
# (every odd integer of 256 .. 512 is a tie)
ROUNDS = {"down": (513, 517, 1025, 1027, 1035), "up": (515, 519, 1023, 1029, 1031, 2047),
          "tie_down": (257, 261, 265, 514, 522, 1028, 1044), "tie_up": (259, 263, 267, 511, 518, 526, 1036, 1052)}
CASES_B1 = [c for c in CASES if supported(True, c.cin, c.cout, c.ks)]
BODIES = {(4, 8, 3), (4, 9, 3), (2, 4, 3), (2, 5, 3), (4, 8, 1), (2, 4, 1)}   # (NQ, RW, KS) of every b3_body<.., 1> instantiation


# ---- the rounding, at bit level
def _bits(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32)


def bf16_rne(v):
    """float32 -> the nearest bf16 number (as float32), ties to the even bf16: add 0x7fff plus the kept part's last bit to the magnitude bits, drop 16"""
    u = _bits(v)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)


def bf16_truncate(v):
    return (_bits(v) & np.uint32(0xFFFF0000)).view(np.float32)


def bf16_half_away(v):
    """ties away from zero (sign-magnitude bits: adding half a step to the magnitude)"""
    return ((_bits(v) + np.uint32(0x8000)) & np.uint32(0xFFFF0000)).view(np.float32)


def rounding_classes(v):
    """which of "exact", "down", "up", "tie_down", "tie_up" (in magnitude) the values of v fall in under bf16_rne"""
    a = np.abs(np.asarray(v, np.float32))
    r, t, h = np.abs(bf16_rne(a)), bf16_truncate(a), bf16_half_away(a)
    tie = (a != t) & (h - a == a - t)
    out = set()
    for name, m in (("exact", r == a), ("down", (r < a) & ~tie), ("up", (r > a) & ~tie), ("tie_down", (r < a) & tie), ("tie_up", (r > a) & tie)):
        if m.any():
            out.add(name)
    return out


# ---- data
def _rounding_ints(rng, bound, shape):
    """uniform integers in [-bound, bound], a quarter of them replaced by values from ROUNDS (those within the bound) with random signs"""
    pool = np.array(sorted({m for ms in ROUNDS.values() for m in ms if m <= bound}), np.float32)
    v = sc._ints(rng, bound, shape)
    planted = rng.choice(pool, shape) * rng.choice(np.array((-1.0, 1.0), np.float32), shape)
    return np.where(rng.random(shape) < 0.25, planted, v).astype(np.float32)


def make_case(case, tier):
    """integer-valued x, w, b, slope, res of a case in a tier, seeded by (case, tier); apron cells of x hold values of their own, as in sconv_cases"""
    c, (xm, wm) = case, TIERS[tier]
    rng = np.random.default_rng(_stable(("bf16x1", case.name, tier)))
    draw = lambda on, bound, shape: _rounding_ints(rng, bound, shape) if on else sc._ints(rng, bound, shape)
    return dict(x=draw(tier == "xrnd", xm, (c.n, c.cin, c.hp, c.wp)), w=draw(tier == "wrnd", wm, (c.cout, c.cin, c.ks, c.ks)),
                b=sc._ints(rng, EPILOGUE_MAX, (c.cout,)), slope=rng.choice(np.array(SLOPES, np.float32), c.cout) if c.slope else None,
                res=sc._ints(rng, EPILOGUE_MAX, out_shape(c)) if c.res else None)


def rounded(data, fx=bf16_rne, fw=bf16_rne):
    return dict(data, x=fx(data["x"]), w=fw(data["w"]))


def assert_exact_domain(case, data):
    """sconv_cases.assert_exact_domain on the ROUNDED operands (its plain-magnitude rule): |b| + 4 |res| + sum |w~||x~| < 2^24 for every output"""
    return sc.assert_exact_domain(case, rounded(data), "fp32")


# ---- the reference
ARITHMETIC_MUTATIONS = {                                                   # mutation -> does it apply to (case, tier)?
    "truncation": lambda c, t: t in ("xrnd", "wrnd"),                      # operands chopped to bf16, not rounded
    "half_away": lambda c, t: t in ("xrnd", "wrnd"),                       # ties away from zero, not to even
    "x_not_rounded": lambda c, t: t == "xrnd",
    "w_not_rounded": lambda c, t: t == "wrnd",
    "lo_added": lambda c, t: t in ("xrnd", "wrnd"),                        # the bf16x3 result: hi + lo of both operands
    "bias_rounded": lambda c, t: True,
    "res_rounded": lambda c, t: c.res,
}
MUTATIONS = dict(ARITHMETIC_MUTATIONS, **{m: f for m, f in sc.MUTATIONS.items() if not m.endswith("_lo_dropped")})


def reference(case, data, mut=None):
    """the whole expected `out` of one bf16x1 call in float64, untouched frame (SENTINEL) included: sconv_cases.reference of the rounded operands.
    `mut`: one of MUTATIONS -- an arithmetic bug of this form, or one of sconv_cases' geometry bugs applied behind the rounding"""
    f = {"truncation": bf16_truncate, "half_away": bf16_half_away}.get(mut, bf16_rne)
    same = lambda v: v
    d = rounded(data, same if mut in ("x_not_rounded", "lo_added") else f, same if mut in ("w_not_rounded", "lo_added") else f)
    if mut == "bias_rounded":
        d["b"] = bf16_rne(d["b"])
    if mut == "res_rounded":
        d["res"] = bf16_rne(d["res"])
    return sc.reference(case, d, mut if mut in sc.MUTATIONS else None)
