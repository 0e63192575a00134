"""Exact-data cases of the attention blocks' fused gate (lic360.sconv1x1_gate / _bf16x3 / _bf16x1; kernels k_gate_sconv / k_gate_sconv_b3 / k_gate_sconv_b1 of
csrc/conv3x3_kernels.hip): on rows [ring, hp - ring) x columns [ring_w, wp - ring_w)

    y = conv1x1(x) + bias          g = 1.0f / (1.0f + lic360_expf(-y))          out = residual + trunk * g

with one fp32 rounding per operation and no fused multiply-add.  No GPU and nothing of `lic360` in here: tests/test_sconv_gate_cases_cpu.py checks this file
by itself, tests/test_gpu_sconv_gate_exact.py compares the kernels with it; case type, launch geometry and the convolution's float64 reference are those of
tests/sconv_cases.py (fp32, bf16x3) and tests/sconv_bf16x1_cases.py (bf16x1), by import.

The method.  The integer x, w and b of a form's tier come from that tier's generator; w and b are then multiplied by 2^-s,
    s = max(0, ceil(log2(sqrt(cin xm (xm + 1) / 3 wm (wm + 1) / 3) / 4)))          for the tier's bounds (xm, wm)
-- a power of two changes neither a tier's bf16 splits nor exactness: y 2^s is the integer the existing references compute, below 2^24, so y has ONE fp32
value whatever the summation order, of a standard deviation of about 4: inside the sigmoid's working range.  lic360_expf is the project's host / device
bit-identical exponential (oracle.expf), fp32 `+`, `/` and `*` are correctly rounded on both sides: the whole output has one value, and a kernel returns it bit
for bit or is wrong.  trunk and residual are integers in [-8, 8].  The saturation case plants output channels with an all-zero weight row and bias +64 (g == 1),
-128 (lic360_expf overflows to +inf: g == 0) or 0 (g = the reference's value at 0)."""
import math

import numpy as np

import sconv_bf16x1_cases as b1
import sconv_cases as sc
from sconv_cases import SENTINEL, branch_of, describe_mismatch  # noqa: F401
from util import _stable

FORMS = ("fp32", "bf16x3", "bf16x1")
TIERS = {"fp32": ("fp32",), "bf16x3": tuple(sc.B3_TIERS), "bf16x1": tuple(b1.TIERS)}       # form -> the tiers of its existing exact file
BOUNDS = {"fp32": dict(fp32=sc.TIERS["fp32"]), "bf16x3": {t: sc.TIERS[t] for t in sc.B3_TIERS}, "bf16x1": dict(b1.TIERS)}
EPILOGUE_MAX = 8                                                            # |trunk|, |residual| <= this
SATURATE = {64.0: (5, 70, 133), -128.0: (17, 100, 190), 0.0: (40, 150)}     # bias -> output channels of g_saturate with an all-zero weight row


def _g(name, cin, cout, n, hp, wp, ring=2, ring_w=None, prod=False):
    return sc._c(name, 1, cin, cout, n, hp, wp, ring=ring, ring_w=ring_w, slope=False, res=False, prod=prod)


CASES = [
    _g("g_q4_one", 32, 192, 1, 20, 36),                                     # one chunk, exact tiles
    _g("g_q4_ragged_n3", 64, 192, 3, 21, 37, ring=1, ring_w=3),             # ragged window, two chunks, several images
    _g("g_q4_low", 32, 192, 1, 9, 36),                                      # window below one tile
    _g("g_q4_3rows", 192, 192, 1, 44, 24),                                  # three tile rows, six chunks
    _g("g_q4_blocks", 96, 384, 2, 20, 22, ring=1, ring_w=3),                # blockIdx.y = 1: the channel index of trunk / residual / out in the second block
    _g("g_q2", 192, 96, 3, 21, 37, ring=1, ring_w=3),
    _g("g_q2_low", 32, 96, 1, 9, 36),
    _g("g_q2_3rows", 64, 96, 1, 40, 20, ring=1),
    _g("g_saturate", 32, 192, 1, 20, 20),
    _g("g_prod_132x260", 192, 192, 1, 132, 260, prod=True),                 # the production map
]
SMALL = [c for c in CASES if not c.prod]
BY_NAME = {c.name: c for c in CASES}
PARAMS = [(c, f, t) for c in CASES for f in FORMS for t in TIERS[f]]


def ident(p):
    return "%s-%s-%s" % (p[0].name, p[1], p[2])


def instantiation(case, form):
    """(form, NQ) of the kernel a call runs: k_gate_sconv* <NQ, RW> with RW = 16 / (8 / NQ)"""
    return form, branch_of(case, form != "fp32").nq


def shift_of(case, form, tier):
    xm, wm = BOUNDS[form][tier]
    return max(0, int(math.ceil(math.log2(math.sqrt(case.cin * xm * (xm + 1) / 3.0 * wm * (wm + 1) / 3.0) / 4.0))))


def window(case):
    return (Ellipsis, slice(case.ring, case.hp - case.ring), slice(case.ring_w, case.wp - case.ring_w))


def make_case(case, form, tier):
    """x, w, b (w and b scaled by 2^-s; `ints`: the tier generator's unscaled data), trunk, res of a case in a form's tier, seeded by (case, form, tier)"""
    ints = (b1 if form == "bf16x1" else sc).make_case(case, tier)
    s = shift_of(case, form, tier)
    scale = np.float32(2.0 ** -s)
    w, b = ints["w"] * scale, ints["b"] * scale
    if case.name == "g_saturate":
        for bias, chans in SATURATE.items():
            w[list(chans)] = 0.0
            b[list(chans)] = bias
    rng = np.random.default_rng(_stable(("gate", case.name, form, tier)))
    shape = (case.n, case.cout, case.hp, case.wp)
    return dict(x=ints["x"], w=w, b=b, s=s, ints=ints, trunk=sc._ints(rng, EPILOGUE_MAX, shape), res=sc._ints(rng, EPILOGUE_MAX, shape))


def assert_exact_domain(case, form, tier, data):
    """the convolution's condition of the form's own file on the generator's integers (no slope, no residual: |b| + sum |w||x| < 2^24, with the tier's
    magnitude rule), so that y 2^s is an integer below 2^24 in every summation order; the scale is a power of two; trunk and residual are small integers"""
    ints = dict(data["ints"], slope=None, res=None)
    bound = b1.assert_exact_domain(case, ints) if form == "bf16x1" else sc.assert_exact_domain(case, ints, tier)
    normal = np.ones(case.cout, bool)
    if case.name == "g_saturate":
        normal[[c for chans in SATURATE.values() for c in chans]] = False
    scale = np.float32(2.0 ** -data["s"])
    assert np.array_equal(data["w"][normal], data["ints"]["w"][normal] * scale) and np.array_equal(data["b"][normal], data["ints"]["b"][normal] * scale)
    for k in ("trunk", "res"):
        assert np.array_equal(data[k], np.rint(data[k])) and float(np.abs(data[k]).max()) <= EPILOGUE_MAX
    return bound


def conv_y(case, form, data):
    """the window's y = conv1x1(x) + bias as float32, from the float64 convolution of the form's kept products (sconv_cases.reference; for bf16x1 the
    rounded operands' through sconv_bf16x1_cases.reference); the cast must be exact"""
    d = dict(x=data["x"], w=data["w"], b=data["b"], slope=None, res=None)
    y64 = (b1.reference(case, d) if form == "bf16x1" else sc.reference(case, d))[window(case)]
    y = y64.astype(np.float32)
    assert np.array_equal(y, y64), "%s / %s: y is not an fp32 number" % (case.name, form)
    return y


def sigmoid32(y, mut=None):
    import oracle as orc
    one = np.float32(1.0)
    with np.errstate(over="ignore", divide="ignore"):
        e = orc.expf(np.ascontiguousarray(y if mut == "exp_plus" else -y, np.float32)).reshape(y.shape)
        g = one / (one + e)
    assert g.dtype == np.float32
    return b1.bf16_rne(g) if mut == "g_bf16" else g


MUTATIONS = {                                                               # mutation -> does it apply to the case?
    "trunk_res_swapped": lambda c: True,
    "exp_plus": lambda c: True,                                             # expf(+y) in place of expf(-y)
    "bias_after_sigmoid": lambda c: True,
    "fma": lambda c: True,                                                  # fmaf(trunk, g, residual) in place of the two roundings
    "block_trunk": lambda c: c.cout > 192,                                  # the second output block reads the first block's trunk channels
    "row_shift": lambda c: True,                                            # the window shifted by one row
    "col_shift": lambda c: True,
    "g_bf16": lambda c: True,                                               # g rounded to bf16
}


def reference(case, form, data, mut=None):
    """the whole expected `out` in float32, untouched frame (SENTINEL) included.  `mut`: one of MUTATIONS"""
    win = window(case)
    trunk, res = data["trunk"][win], data["res"][win]
    if mut == "trunk_res_swapped":
        trunk, res = res, trunk
    if mut == "block_trunk":
        trunk = np.concatenate([trunk[:, :192]] * (case.cout // 192), 1)
    if mut == "bias_after_sigmoid":
        y = conv_y(case, form, dict(data, b=np.zeros_like(data["b"])))
        g = sigmoid32(y) + data["b"][None, :, None, None]
    else:
        g = sigmoid32(conv_y(case, form, data), mut)
    if mut == "fma":
        o = (trunk.astype(np.float64) * g.astype(np.float64) + res.astype(np.float64)).astype(np.float32)      # (the product of two fp32 numbers is exact in float64)
    else:
        tg = trunk * g
        o = res + tg
    assert o.dtype == np.float32
    out = np.full((case.n, case.cout, case.hp, case.wp), SENTINEL, np.float32)
    out[win] = o
    if mut == "row_shift":
        out = np.roll(out, 1, 2)
    if mut == "col_shift":
        out = np.roll(out, 1, 3)
    return out


_REFS = {}


def shared(case, form, tier):
    """(data, reference) of a case, computed once per process and shared among the tests that need it; callers leave both unchanged"""
    key = (case.name, form, tier)
    if key not in _REFS:
        data = make_case(case, form, tier)
        _REFS[key] = (data, reference(case, form, data))
    return _REFS[key]


# ---- real-valued data: the parity bound of tests/test_gpu_sconv_gate.py
REAL_CASES = ("g_q4_ragged_n3", "g_prod_132x260")


def real_data(case, seed=0):
    """x ~ N(0, 1), w ~ N(0, 1 / cin), b ~ N(0, 1) / 4, trunk and residual ~ N(0, 1)"""
    rng = np.random.default_rng(_stable(("gate-real", case.name, seed)))
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    shape = (case.n, case.cout, case.hp, case.wp)
    return dict(x=f(case.n, case.cin, case.hp, case.wp), w=f(case.cout, case.cin, 1, 1) / np.float32(math.sqrt(case.cin)), b=f(case.cout) / np.float32(4.0),
                trunk=f(*shape), res=f(*shape))


def gate64(x, w, b, trunk, res, form="fp32"):
    """the float64 gate of the operands as a form rounds them (unrounded for fp32 and bf16x3, x and w rounded to bf16 for bf16x1), on the whole map"""
    if form == "bf16x1":
        x, w = b1.bf16_rne(x), b1.bf16_rne(w)
    y = np.einsum("oc,nchw->nohw", w.reshape(w.shape[0], -1).astype(np.float64), x.astype(np.float64), optimize=True) + b.astype(np.float64)[None, :, None, None]
    return res.astype(np.float64) + trunk.astype(np.float64) / (1.0 + np.exp(-y))


def parity_excess(got, want64, trunk, res):
    """max over cells of |got - ref| - (1e-4 |trunk| + 1e-6 (1 + |residual|)): the bound holds iff this is <= 0.  From the project's criterion for an
    fp32-accumulated kernel, |y - y64| <= 1e-4 (1 + |y|): sigmoid'(y) (1 + |y|) < 0.48, so |g - g64| < 0.5e-4 -- a margin of two in the first term; the
    epilogue's roundings add at most 2^-22 (|residual| + |trunk|) -- a margin of about four in the second"""
    err = np.abs(got.astype(np.float64) - want64)
    return float((err - (1e-4 * np.abs(trunk.astype(np.float64)) + 1e-6 * (1.0 + np.abs(res.astype(np.float64))))).max())


def emulate32(x, w, b, trunk, res, form="fp32", mut=None):
    """the kernel's arithmetic on real data, on the host: y rounded once to fp32 from the float64 sum, the fp32 sigmoid on oracle.expf, two fp32 roundings"""
    if form == "bf16x1":
        x, w = b1.bf16_rne(x), b1.bf16_rne(w)
    y = (np.einsum("oc,nchw->nohw", w.reshape(w.shape[0], -1).astype(np.float64), x.astype(np.float64), optimize=True)
         + b.astype(np.float64)[None, :, None, None]).astype(np.float32)
    tg = trunk * sigmoid32(y, mut)
    return res + tg
