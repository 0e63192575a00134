"""Exact-data cases of the narrow-workgroup sphere convolutions (lic360.sconv3x3_narrow / sconv1x1_narrow / sconv1x1_gate_narrow; kernels k_narrow_conv /
k_narrow_gate of csrc/conv3x3_kernels.hip): the wide kernels' operation with `cpw` = 96 or 48 output channels per workgroup instead of a whole pack block.
No GPU and nothing of `lic360` in here: tests/test_sconv_narrow_cases_cpu.py checks this file by itself, tests/test_gpu_sconv_narrow_exact.py compares the
kernels with it.  Case type, data tiers, exactness condition and float64 references are those of tests/sconv_cases.py (fp32, bf16x3), tests/sconv_bf16x1_cases.py
(bf16x1) and tests/sconv_gate_cases.py (the gate), by import: a narrow launch computes what the wide launch of the same arguments computes, so its reference IS the
wide one's.  What is this file's own is the narrow launch geometry, restated from sconv_plan / sconv_workgroup / s3_body, and the bugs only a narrow kernel can have.

The narrow geometry.  The pack's channel block is PB = 192 where cout % 192 == 0, else 96 (cout = 96): PQ = PB / 48 slots of 48 channels.  A narrow workgroup
takes NQ = cpw / 48 of them (cpw < PB): blockIdx.y = nb counts blocks of cpw channels, nb < cout / cpw; it reads pack block nb / (PQ / NQ) at the mq slots
(nb % (PQ / NQ)) * NQ + mq, mq < NQ, and writes channels nb * cpw + 48 mq + ...  Its 8 waves form 8 / NQ row groups of 16 / (8 / NQ) rows: RW = 4 at cpw 96, 2 at
cpw 48.  The tile rule: a 3x3 window's remainder of 1 .. 8 / NQ rows rides on the last tile row (RW + 1 rows per wave: 20-row tiles at cpw 96, 24-row tiles at
cpw 48) -- except in the split-bf16 form at cpw 48, whose 24-row tile does not fit the LDS (183 KB): there every remainder takes a tile row of its own."""
import collections

import numpy as np

import sconv_bf16x1_cases as b1
import sconv_cases as sc
import sconv_gate_cases as gc
from sconv_cases import SENTINEL, describe_mismatch  # noqa: F401
from util import _stable

FORMS = ("fp32", "bf16x3", "bf16x1")
FORM_NUMBER = {"fp32": 0, "bf16x3": 3, "bf16x1": 1}                          # the C entry points' `form`
TIERS = {"fp32": ("fp32",), "bf16x3": tuple(sc.B3_TIERS), "bf16x1": tuple(b1.TIERS)}
CPWS = (96, 48)

NCase = collections.namedtuple("NCase", "case cpws")                       # a sconv_cases.Case and the cpw values it runs at
NBranch = collections.namedtuple("NBranch", "form nq pq rw rw_last ks blocks_y tiles_y tiles_x rem full tall chunks")


def _n(cpws, *a, **k):
    return NCase(sc._c(*a, **k), (cpws,) if isinstance(cpws, int) else tuple(cpws))


SMALL = [
    # 3x3, 192 channels at cpw 96 (NQ = 2, 4 row groups: tall last row at rem 1 .. 4, the extra tile row at rem 5)
    _n(96, "n3_96_rem1_cin32", 3, 32, 192, 1, 21, 36),                                                   # nr 17, nc 32 (exact)
    _n(96, "n3_96_rem4_wrap", 3, 32, 192, 1, 24, 25, sphere=2, res=True),                                # nr 20 (tall), ragged columns
    _n(96, "n3_96_rem5_plain", 3, 32, 192, 1, 23, 23, pad=1, sphere=0, ring=1, slope=False),             # nr 21: two tile rows
    _n(96, "n3_96_low", 3, 64, 192, 1, 13, 24, pad=3),                                                   # nr 9: full = 0
    _n(96, "n3_96_3rows_n3", 3, 32, 192, 3, 52, 20, res=True),                                           # nr 48: three tile rows, n = 3
    _n(96, "n3_96_384", 3, 32, 384, 1, 21, 22, ring=2),                                                  # the second pack block
    _n((96, 48), "n3_shuffle_768", 3, 192, 768, 1, 14, 22, crop=1, shuffle=True),                        # blockIdx.y 0 .. 7 / 0 .. 15; six bf16 chunks
    # 3x3, 192 channels at cpw 48 (NQ = 1, 8 row groups: tall last row at rem 1 .. 8, the extra tile row at rem 9)
    _n(48, "n3_48_rem1", 3, 32, 192, 1, 19, 36, ring=1, ring_w=2),                                       # nr 17
    _n(48, "n3_48_rem8", 3, 32, 192, 3, 28, 25, sphere=2, res=True),                                     # nr 24 (tall), n = 3
    _n(48, "n3_48_rem9", 3, 32, 192, 1, 29, 20),                                                         # nr 25: two tile rows
    _n(48, "n3_48_low", 3, 32, 192, 1, 13, 24, pad=3),                                                   # nr 9: full = 0
    _n(48, "n3_48_384", 3, 32, 384, 1, 24, 22),                                                          # the second pack block, tall (rem 4)
    _n(48, "n3_48_shuffle_res", 3, 32, 384, 3, 22, 22, crop=1, shuffle=True, res=True),                  # shuffle + residual, nr 18
    # 3x3, 96 channels at cpw 48 (the 96-block pack: PQ = 2)
    _n(48, "n3_q2_cin16", 3, 16, 96, 1, 19, 24, ring=1, ring_w=2),                                       # one fp32 chunk (the bf16 forms do not take 16)
    _n(48, "n3_q2_cin96_rem8", 3, 96, 96, 1, 28, 20, pad=1, slope=False),                                # six fp32 chunks, three bf16 ones; nr 24 (tall)
    _n(48, "n3_q2_rem1_wrap", 3, 32, 96, 1, 21, 22, sphere=2, res=True),                                 # nr 17, sphere 2
    _n(48, "n3_q2_rem9_plain", 3, 32, 96, 3, 27, 22, sphere=0, ring=1, ring_w=3),                        # nr 25: two tile rows, sphere 0
    _n(48, "n3_q2_exact", 3, 32, 96, 1, 36, 36),                                                         # nr 32, nc 32: no remainder, sphere 1
    _n(48, "n3_q2_low", 3, 32, 96, 1, 13, 36, pad=3),                                                    # nr 9: full = 0
    # 1x1: the three combinations, a ragged window, n = 3, the shuffled shortcut, 192 -> 96
    _n((96, 48), "n1_192", 1, 32, 192, 1, 20, 36, res=True),                                             # exact tiles
    _n((96, 48), "n1_192_ragged_n3", 1, 64, 384, 3, 21, 37, ring=1, ring_w=3),                           # nr 19, nc 31; two pack blocks
    _n((96, 48), "n1_shuffle_768", 1, 192, 768, 1, 14, 22, crop=1, shuffle=True, slope=False, res=True),
    _n(48, "n1_192_to_96", 1, 192, 96, 3, 21, 37, ring=1, ring_w=3, slope=False),
    _n(48, "n1_96_low", 1, 32, 96, 1, 9, 36),                                                            # nr 5: full = 0
]
# the layers lic360_models routes narrow with set_conv_precision(.., small="narrow") after measurement (NARROW_* there, DESIGN 7c, profiles/sconv_narrow_probe.json),
# once each at their batch, at the cpw the count rule picks (tests/test_gpu_sconv_narrow.py records the calls): the 132 x 260 stage and the 192 -> 768 pair on
# 68 x 132 at batch 1, the 192-channel 3x3 layers of the 36 x 68 maps at batch 8.  (p_v2_conv1_132x260 is routed narrow in bf16x3 and bf16x1 only: in fp32 the
# measurement sends it back to the library, NARROW_ROUTED_BACK; the kernel is checked in all three forms all the same.)
PRODUCTION = [
    _n(96, "p_v2_conv1_132x260", 3, 192, 192, 1, 132, 260, ring=1, ring_w=2, prod=True),
    _n(96, "p_v2_conv2_132x260", 3, 192, 192, 1, 132, 260, sphere=2, res=True, prod=True),
    _n(96, "p_gdn_conv2_132x260", 3, 192, 192, 1, 132, 260, slope=False, prod=True),
    _n(48, "p_bottleneck_in_132x260", 1, 192, 96, 1, 132, 260, prod=True),
    _n(48, "p_bottleneck_3x3_132x260", 3, 96, 96, 1, 132, 260, prod=True),
    _n(96, "p_bottleneck_out_132x260", 1, 96, 192, 1, 132, 260, slope=False, res=True, prod=True),
    _n(48, "p_v2_conv1_36x68_n8", 3, 192, 192, 8, 36, 68, ring=1, ring_w=2, prod=True),
    _n(48, "p_v2_conv2_36x68_n8", 3, 192, 192, 8, 36, 68, sphere=2, res=True, prod=True),
    _n(48, "p_gdn_conv2_36x68_n8", 3, 192, 192, 8, 36, 68, slope=False, prod=True),
    _n(96, "p_up_conv1_68x132", 3, 192, 768, 1, 68, 132, crop=1, shuffle=True, prod=True),
    _n(96, "p_up_shortcut_68x132", 1, 192, 768, 1, 68, 132, crop=1, shuffle=True, slope=False, res=True, prod=True),
]
CASES = SMALL + PRODUCTION
BY_NAME = {nc.case.name: nc for nc in CASES}

# the gate (cout % 192 == 0 only), on the cases and helpers of tests/sconv_gate_cases.py: one exact tile, a ragged window with several images, the second pack
# block, the saturated channels, the production map -- each at cpw 96 and 48
GATE_CASES = [gc.BY_NAME[n] for n in ("g_q4_one", "g_q4_ragged_n3", "g_q4_blocks", "g_saturate", "g_prod_132x260")]


# ---- the narrow launch geometry, restated from sconv_narrow_ok / sconv_plan / sconv_tall (csrc/conv3x3_kernels.hip)
def pack_block(cout):
    return 192 if cout % 192 == 0 else 96


def supported(form, ks, cin, cout, cpw):
    return form in FORMS and cpw in CPWS and sc.supported(form != "fp32", cin, cout, ks) and cpw < pack_block(cout)


def has_tall(form, nq, ks):
    return ks == 3 and not (form == "bf16x3" and nq == 1)


def tile_rows(nr, nq, ks, form):
    """(tile rows, tall last row?): a remainder of at most 8 / NQ rows -- the NARROW form's NQ -- rides on the last tile row of a 3x3 where the form has one"""
    nrg, full, rem = 8 // nq, nr // 16, nr % 16
    tall = has_tall(form, nq, ks) and 0 < rem <= nrg and full > 0
    return (full if tall else (nr + 15) // 16), tall


def branch_of(case, form, cpw):
    c = case
    assert supported(form, c.ks, c.cin, c.cout, cpw), (c.name, form, cpw)
    nq, pq, nr = cpw // 48, pack_block(c.cout) // 48, c.hp - 2 * c.ring
    tiles_y, tall = tile_rows(nr, nq, c.ks, form)
    rw = 16 // (8 // nq)
    return NBranch(form, nq, pq, rw, rw + 1 if tall else rw, c.ks, c.cout // cpw, tiles_y, (c.wp - 2 * c.ring_w + 15) // 16, nr % 16, nr // 16, tall,
                   c.cin // sc.chunk_of(form != "fp32", c.ks))


def slots_of(case, cpw):
    """(pack block, first mq slot) of every blockIdx.y of a launch"""
    nq, pq = cpw // 48, pack_block(case.cout) // 48
    return [(nb // (pq // nq), nb % (pq // nq) * nq) for nb in range(case.cout // cpw)]


def bodies_of(case, form, cpw):
    """the (form, NQ, RW, KS, PQ) body instantiations a launch runs: the ordinary tile rows' and, with a tall last row, that row's"""
    br = branch_of(case, form, cpw)
    out = {(form, br.nq, br.rw_last, br.ks, br.pq)}
    if br.tiles_y > 1 or not br.tall:
        out.add((form, br.nq, br.rw, br.ks, br.pq))
    return out


# every body the narrow kernels instantiate: k_narrow_conv<NT, 2, 4, KS, 4>, <NT, 1, 2, KS, 4>, <NT, 1, 2, KS, 2> with their tall bodies (RW + 1 at KS = 3)
BODIES = {(f, nq, rw, ks, pq) for f in FORMS for (nq, rw0, pq) in ((2, 4, 4), (1, 2, 4), (1, 2, 2)) for ks in (3, 1)
          for rw in ((rw0, rw0 + 1) if has_tall(f, nq, ks) else (rw0,))}
GATE_KERNELS = {(f, nq) for f in FORMS for nq in (2, 1)}                    # k_narrow_gate<NT, NQ, 16 / (8 / NQ), 4>


def params():
    """(NCase, form, tier, cpw) of every run; a production case runs its form's last tier only"""
    out = []
    for nc in CASES:
        for form in FORMS:
            for cpw in nc.cpws:
                if supported(form, nc.case.ks, nc.case.cin, nc.case.cout, cpw):
                    out += [(nc, form, t, cpw) for t in (TIERS[form][-1:] if nc.case.prod else TIERS[form])]
    return out


def gate_params():
    return [(c, f, (gc.TIERS[f][-1:] if c.prod else gc.TIERS[f])[i], cpw) for c in GATE_CASES for f in FORMS for i in range(1 if c.prod else len(gc.TIERS[f]))
            for cpw in CPWS]


def ident(p):
    return "%s-%s-%s-cpw%d" % (getattr(p[0], "case", p[0]).name, p[1], p[2], p[3])


# ---- data and references: the wide forms'
def make_case(case, form, tier):
    return b1.make_case(case, tier) if form == "bf16x1" else sc.make_case(case, tier)


def assert_exact_domain(case, form, tier, data):
    return b1.assert_exact_domain(case, data) if form == "bf16x1" else sc.assert_exact_domain(case, data, tier)


def _wide_reference(case, form, data):
    return b1.reference(case, data) if form == "bf16x1" else sc.reference(case, data)


# bugs of a narrow kernel: mutation -> does it apply to (case, form, cpw)?
MUTATIONS = {
    "slot_0": lambda c, f, cpw: True,                                       # every narrow block reads mq slot 0 of its pack block
    "offset_from_pack_block": lambda c, f, cpw: True,                       # the channel offset is blockIdx.y times the PACK's block size
    "wide_tall_threshold": lambda c, f, cpw: tile_rows(c.hp - 2 * c.ring, cpw // 48, c.ks, f)[1]       # the kernel's tall test with 8 / PQ where 8 / NQ belongs:
    and not (0 < (c.hp - 2 * c.ring) % 16 <= 8 // (pack_block(c.cout) // 48)),                          # the remainder rows beyond it are not computed
    "shuffle_block_dropped": lambda c, f, cpw: c.shuffle,                   # the shuffled store with the block's channel offset dropped
}


def reference(case, form, data, cpw, mut=None):
    """the whole expected `out` of a narrow call in float64, untouched frame (SENTINEL) included: the wide reference -- or, with `mut`, what a narrow kernel with
    that bug writes"""
    c = case
    pb = pack_block(c.cout)
    if mut == "slot_0":                                                     # channel co takes the weights of slot 0's channels of its pack block, the epilogue is its own
        co = np.arange(c.cout)
        return _wide_reference(c, form, dict(data, w=data["w"][co // pb * pb + co % cpw]))
    if mut == "offset_from_pack_block":                                     # block nb's results land at channels nb * PB + j (with that channel's epilogue), those in range
        src = np.full(c.cout, -1)
        for nb in range(c.cout // cpw):
            if nb * pb + cpw <= c.cout:
                src[nb * pb:nb * pb + cpw] = np.arange(nb * cpw, (nb + 1) * cpw)
        ref = _wide_reference(c, form, dict(data, w=data["w"][np.maximum(src, 0)]))
        written = src >= 0
        if c.shuffle:
            ref[:, ~written.reshape(-1, 4).all(1)] = SENTINEL
        else:
            ref[:, ~written] = SENTINEL
        return ref
    ref = _wide_reference(c, form, data)
    if mut == "wide_tall_threshold":                                        # tiles_y = full, but the last tile row is not run tall: the remainder rows stay untouched
        rows = c.ring - c.crop + (c.hp - 2 * c.ring) // 16 * 16
        k = 2 if c.shuffle else 1
        ref[:, :, k * rows:] = SENTINEL
    if mut == "shuffle_block_dropped":                                      # every block stores at shuffled channels 0 .. cpw / 4: the last block's values survive
        out = np.full_like(ref, SENTINEL)
        out[:, :cpw // 4] = ref[:, (c.cout - cpw) // 4:]
        return out
    return ref


_REFS = {}


def shared(case, form, tier, cpw=None):
    """(data, reference) of a case, computed once per process and shared among the tests that need it (the reference does not depend on cpw); callers leave both unchanged"""
    key = (case.name, form, tier)
    if key not in _REFS:
        data = make_case(case, form, tier)
        _REFS[key] = (data, _wide_reference(case, form, data))
    return _REFS[key]


def real_data(case, seed=0):
    """N(0, 1) data of a case: the narrow output must equal the wide kernel's bit for bit (an output's sequence of K steps is the same in both)"""
    rng = np.random.default_rng(_stable(("narrow-real", case.name, seed)))
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    return dict(x=f(case.n, case.cin, case.hp, case.wp), w=f(case.cout, case.cin, case.ks, case.ks) / np.float32(np.sqrt(case.cin * case.ks * case.ks)), b=f(case.cout),
                slope=np.abs(f(case.cout)) if case.slope else None, res=f(*sc.out_shape(case)) if case.res else None)
