"""Exact-data cases of the single-pass bf16 ("bf16x1") forms of the stride-2 sphere convolutions (lic360_sconv3x3s2_bf16x1 / lic360_sconv1x1s2_bf16x1;
kernels k_sconv_b1s2: csrc/sconv_b1s2.inc for the 3x3, b3_body at stride 2 for the 1x1).  No GPU and nothing of `lic360` in here: the geometry, the sphere
rule and the float64 reference are tests/sconv_s2_cases.py's, the arithmetic in front of them (bit-level round to nearest even, the three tiers, the data
makers, the exactness condition on the rounded operands) tests/sconv_bf16x1_cases.py's.  tests/test_sconv_s2_bf16x1_cases_cpu.py checks this file by
itself, tests/test_gpu_sconv_s2_bf16x1_exact.py compares the kernels with it.

The contract.  Every input value and every weight is rounded once to bf16 (nearest even), each product is one v_mfma_f32_16x16x32_bf16 with fp32
accumulation, bias / PReLU / residual are fp32: the reference is sconv_s2_cases.reference of the ROUNDED operands.  On integer data with
|b| + 4 |res| + sum |w~||x~| < 2^24 that is one fp32 number whatever the summation order: a kernel returns it bit for bit or is wrong.

The chunk is 32 input channels at BOTH kernel sizes (the K of one bf16 MFMA), so the cases are those of sconv_s2_cases with cin % 32 == 0 -- plus cases of an
odd chunk count above 1: the bodies alternate their ring sets by chunk parity (b3_body's operand set, b1s2_body's loader and operand sets)."""
import numpy as np

import sconv_bf16x1_cases as b1
import sconv_s2_cases as s2
from sconv_bf16x1_cases import ARITHMETIC_MUTATIONS, EPILOGUE_MAX, TIERS, bf16_rne, rounded, rounding_classes   # noqa: F401  (re-exported for the tests)
from sconv_s2_cases import SENTINEL, Branch, Case, describe_mismatch, out_hw, out_shape                         # noqa: F401
from util import _stable

CHUNK = 32
ODD_CHUNKS = [
    s2._c("b3_q4_96_res", 3, 96, 192, 1, 16, 17, res=True),                 # three chunks; ragged columns; a residual
    s2._c("b3_q2_96_rows", 3, 96, 96, 1, 17, 16),                           # three chunks at NQ = 2; an extra tile row of one row
    s2._c("b1_q2_96_rows", 1, 96, 96, 1, 17, 16),                           # the 1x1 likewise
    s2._c("b1_q4_160", 1, 160, 192, 1, 16, 16, slope=False, res=True),      # five chunks at NQ = 4
]
CASES = [c for c in s2.CASES if c.cin % CHUNK == 0] + ODD_CHUNKS
SMALL = [c for c in CASES if not c.prod]
PRODUCTION = [c for c in CASES if c.prod]
BODIES = {(4, 8, 3), (2, 4, 3), (4, 8, 1), (2, 4, 1)}                      # (NQ, RW, KS) of every k_sconv_b1s2 instantiation


# ---- the launch geometry, restated from sconv_ok(1, ..) / sconv_plan's stride-2 branch (csrc/conv3x3_kernels.hip)
def supported(cin, cout, ks):
    return ks in (1, 3) and cin >= CHUNK and cin % CHUNK == 0 and cout >= 96 and (cout % 192 == 0 or cout == 96)


def branch_of(case):
    c = case
    assert supported(c.cin, c.cout, c.ks), c.name
    nq = 4 if c.cout % 192 == 0 else 2
    oh, ow = out_hw(c)
    return Branch(nq, 16 // (8 // nq), c.ks, c.cout // 192 if nq == 4 else 1, (oh + 15) // 16, (ow + 15) // 16, oh % 16, oh // 16, c.cin // CHUNK)


# ---- data: the tiers of sconv_bf16x1_cases on the stride-2 shapes
def make_case(case, tier):
    """integer-valued x, w, b, slope, res of a case in a tier, seeded by (case, tier); bias and residual up to 1023 in every tier (most are not bf16
    numbers); apron cells of x hold values of their own"""
    c, (xm, wm) = case, TIERS[tier]
    rng = np.random.default_rng(_stable(("s2_bf16x1", case.name, tier)))
    draw = lambda on, bound, shape: b1._rounding_ints(rng, bound, shape) if on else s2._ints(rng, bound, shape)
    return dict(x=draw(tier == "xrnd", xm, (c.n, c.cin, c.hp, c.wp)), w=draw(tier == "wrnd", wm, (c.cout, c.cin, c.ks, c.ks)),
                b=s2._ints(rng, EPILOGUE_MAX, (c.cout,)), slope=rng.choice(np.array(s2.SLOPES, np.float32), c.cout) if c.slope else None,
                res=s2._ints(rng, EPILOGUE_MAX, out_shape(c)) if c.res else None)


def assert_exact_domain(case, data):
    """|b| + 4 |res| + sum |w~||x~| < 2^24 for every output, on the ROUNDED operands"""
    return s2.assert_exact_domain(case, rounded(data), "fp32")


# ---- the reference
MUTATIONS_ARITHMETIC = ARITHMETIC_MUTATIONS                                 # (case, tier) -> applies?
MUTATIONS_GEOMETRY = s2.MUTATIONS                                           # case -> applies?


def reference(case, data, mut=None):
    """the whole expected `out` of one call in float64, untouched frame (SENTINEL) included: sconv_s2_cases.reference of the rounded operands.  `mut`: an
    arithmetic bug of the form (ARITHMETIC_MUTATIONS) or a geometry bug of sconv_s2_cases.MUTATIONS applied behind the rounding"""
    f = {"truncation": b1.bf16_truncate, "half_away": b1.bf16_half_away}.get(mut, bf16_rne)
    same = lambda v: v
    d = rounded(data, same if mut in ("x_not_rounded", "lo_added") else f, same if mut in ("w_not_rounded", "lo_added") else f)
    if mut == "bias_rounded":
        d["b"] = bf16_rne(d["b"])
    if mut == "res_rounded":
        d["res"] = bf16_rne(d["res"])
    return s2.reference(case, d, mut if mut in s2.MUTATIONS else None)
