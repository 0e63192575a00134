"""The fused cross-entropy rate loss (csrc/ce_rate_kernels.hip, DESIGN.md "Fused cross-entropy rate loss"): cases, the launch geometry restated,
the reference and models of broken kernels (numpy, torch on the CPU and the CPU oracle only; no GPU, and nothing of the unit under test).

The arithmetic contract, restated.  Inputs fp32 contiguous: logit [N, G*K, H, W] (the net's raw output), label [N, G, H, W] holding class indices.
Symbol (n, g, y, x) reads channel g*K + i, i < K -- the element ContextReshape puts in row ((n G + g) H + y) W + x, column i -- and is valid iff
label > -1 and label < K (so NaN is invalid); its class is c = (int)label, truncated: -0.5 -> 0, 3.7 -> 3.  For a valid symbol, every operation
rounded once in fp32:
    m     = l_0; for i = 1..K-1: if (m < l_i) m = l_i                      (lic360_softmax_inplace's order)
    e_i   = lic360_expf(l_i - m);  s = 0; s = s + e_i in index order
    loss  = lic360_logf(s) - (l_c - m)
    backward with t = grad_nats[n]:  p_i = e_i / s;  d_logit_i = (i == c ? p_i - 1 : p_i) * t
An invalid symbol costs 0, is counted in invalid[n] and not in symbols[n], and gets exact zeros in d_logit, whatever its logits hold.  nats[n]
(float64) is the sum of the valid symbols' fp32 losses added in double in some fixed order: within symbols * 2^-53 * sum|loss| of math.fsum.  map
is the per-symbol loss (0 where invalid).

The reference is built from pieces that do not come from the new unit: oracle.expf, an fp32 numpy restatement of lic360_logf
(csrc/lic360_exact_math.h:79-103; tests/test_ce_rate_cases_cpu.py holds it bit for bit against the header, compiled on the host) on
gmm_rate_cases.fmaf, plain fp32 numpy for the rest, math.fsum.  `head_f64` states the head in float64 torch autograd.
"""
import collections
import functools
import math

import numpy as np

import oracle as orc
from gmm_rate_cases import fmaf
from ops_edge_cases import _rng

F = np.float32

# ---------------------------------------------------------------------------------------------------- the launch geometry, restated
THREADS = 128                 # CE_THREADS
PER_THREAD = 2                # CE_PER_THREAD: cells of a plane per thread
CHUNK = THREADS * PER_THREAD  # CE_CHUNK: cells of one (n, g) plane per workgroup
WAVE = 64
MAX_K = 64                    # CE_MAX_K
STATIC_K = 49                 # CE_STATIC_K: the instantiation with the class count at compile time (logits in registers)
VEC_BYTES = 8                 # the vector form moves a thread's two consecutive cells in one access

Case = collections.namedtuple("Case", "id N G H W K labels family offset")
LABEL_KINDS = ("classes", "mixed", "image")     # every class; + fractional and invalid labels; + an image all of whose labels are invalid


def _c(N, G, H, W, K, labels, family="regular", offset=0):
    return Case("%s_%dx%dx%dx%d_k%d_%s%s" % (family[0], N, G, H, W, K, labels, "_off%d" % offset if offset else ""), N, G, H, W, K, labels, family, offset)


CASES = (
    _c(1, 1, 1, 1, 49, "classes"),
    _c(1, 1, 1, 1, 3, "classes"),
    _c(3, 5, 3, 5, 49, "image"),               # N and H W odd, G > 1: image and plane bases on 4-byte boundaries only -> the scalar form
    _c(3, 5, 3, 5, 3, "mixed"),
    _c(2, 2, 6, 8, 49, "mixed"),               # the vector form, K = 49 at G = 2
    _c(2, 2, 6, 8, 2, "classes"),
    _c(3, 4, 6, 8, 48, "image"),
    _c(2, 3, 4, 12, 49, "mixed", offset=1),    # W % 4 == 0, every tensor 4 bytes off a 16-byte boundary: the scalar form must be chosen; K = 49 at G = 3
    _c(2, 3, 4, 12, 50, "mixed", offset=1),
    _c(2, 1, 4, 12, 49, "classes", offset=2),  # 8 bytes off a 16-byte boundary: the vector form still holds
    _c(1, 1, 16, 32, 49, "mixed"),             # a plane of exactly two chunks, vector form
    _c(1, 2, 16, 32, 64, "mixed"),
    _c(2, 1, 15, 19, 49, "mixed"),             # 285 cells: a second, ragged chunk of 29, scalar form
    _c(1, 2, 15, 19, 1, "mixed"),
    _c(1, 1, 10, 30, 49, "mixed"),             # 300 cells: a ragged second chunk of 44 in the vector form
    _c(1, 2, 10, 30, 50, "classes"),
    _c(3, 2, 6, 8, 49, "image", "edge"),
    _c(3, 5, 3, 5, 49, "image", "edge"),
    _c(2, 2, 6, 8, 3, "mixed", "edge"),
    _c(2, 1, 15, 19, 50, "mixed", "edge"),
    _c(2, 129, 2, 4, 3, "mixed", "slots"),     # 129 slots per image: the finish kernel's second pass (THREADS + 1), vector form, generic K
    _c(2, 129, 3, 5, 49, "mixed", "slots"),    # the same in the scalar form, K = 49
)
REGULAR = tuple(c for c in CASES if c.family == "regular")
EDGE = tuple(c for c in CASES if c.family == "edge")
SLOTS = tuple(c for c in CASES if c.family == "slots")       # kernels only: bit for bit and within nats_bound, no recorded float64 figures
BY_ID = {c.id: c for c in CASES}


def valid_variant(case):
    """the regular case with every invalid label replaced by class 0: what the library route takes (torch raises on any other label), so what the
    two routes of the module are compared on.  Its inputs are the case's own otherwise; it is no case of the kernels' list."""
    assert case.family == "regular"
    return case._replace(id=case.id + "_valid", family="valid")


VALID = tuple(valid_variant(c) for c in REGULAR)
BASE_OF = {v.id: c for v, c in zip(VALID, REGULAR)}
EDGE_KINDS = ("equal", "max_first", "max_last", "max_tied", "spread_past_104", "magnitude_1e30", "subnormal_spread")


def form(case):
    """the launcher's choice: 8-byte accesses when W % 2 == 0 and every base is 8-byte aligned (offset: floats past a 16-byte aligned start)"""
    return "vec" if case.W % 2 == 0 and case.offset % 2 == 0 else "scalar"


def instantiation(case):
    return "static" if case.K == STATIC_K else "generic"


def chunks(case):
    return -(-(case.H * case.W) // CHUNK)


def valid_of(label, K, clamped=False):
    """the kernel's rule, on an fp32 array: label > -1 and label < K (NaN: neither holds)"""
    with np.errstate(invalid="ignore"):
        v = (label > F(-1.0)) & (label < F(K))
    return np.ones(label.shape, bool) if clamped else v


def reach(case):
    """names of the code paths and edges a case reaches, derived from the restated geometry and the case's own inputs"""
    d = inputs(case)
    names = {form(case), instantiation(case), form(case) + "_" + instantiation(case), "labels_" + case.labels, "family_" + case.family, "K%d" % case.K}
    hw = case.H * case.W
    if chunks(case) > 1:
        names.add("multi_chunk")
    if hw == 2 * CHUNK:
        names.add("exactly_two_chunks")
    if hw % CHUNK and chunks(case) > 1:
        names.add("ragged_chunk_" + form(case))
    if case.W % 4 == 0 and case.offset % 4:
        names.add("misaligned_w4_" + form(case))
    if hw % 2 and case.N * case.G > 1:
        names.add("plane_base_4_byte")
    if case.K == STATIC_K and case.G > 1:
        names.add("K49_G%d" % case.G)
    lab, valid = d["label"], valid_of(d["label"], case.K)
    cls = lab[valid].astype(np.int64)
    if case.K > 1 and (cls == 0).any() and (cls == case.K - 1).any() and len(set(cls.tolist())) == case.K:
        names.add("every_class")
    if (lab == F(-0.5)).any():
        names.add("label_minus_half")
    if (valid & (lab != np.trunc(lab)) & (lab > 0)).any():
        names.add("label_fractional")
    for name, hit in (("label_minus_1", lab == F(-1)), ("label_K", lab == F(case.K)), ("label_1e9", lab == F(1e9)), ("label_nan", np.isnan(lab))):
        if hit.any():
            names.add(name)
    per_image = valid.reshape(case.N, -1)
    if case.N > 1 and (~per_image.any(1)).any() and per_image.any():
        names.add("invalid_image_among_valid")
    names |= {"edge_" + k for k in d["edges"]}
    if case.G * chunks(case) > THREADS:                                 # slots per image: the finish kernel adds them in passes of THREADS
        names.add("finish_second_pass")
    return names


REACH = ("vec_static", "vec_generic", "scalar_static", "scalar_generic", "multi_chunk", "exactly_two_chunks", "ragged_chunk_vec", "ragged_chunk_scalar",
         "misaligned_w4_scalar", "misaligned_w4_vec", "plane_base_4_byte", "K49_G2", "K49_G3", "every_class", "label_minus_half", "label_fractional",
         "label_minus_1", "label_K", "label_1e9", "label_nan", "invalid_image_among_valid", "family_regular", "family_edge", "finish_second_pass") + \
    tuple("K%d" % k for k in (1, 2, 3, 48, 49, 50, 64)) + tuple("labels_" + k for k in LABEL_KINDS) + tuple("edge_" + k for k in EDGE_KINDS)

# MEASURED here on the CPU: the reference's own distance from the float64 statement -- max |reference - float64 autograd| over the elements of d_logit
# and of the per-symbol loss, and max over the images of |nats - float64 nats|; logits are N(0, 2), so losses lie around log K + 2, and the
# gradient scale is max |grad| <= 1.5 (tests/test_ce_rate_cases_cpu.py::test_reference_against_float64 re-measures, prints and holds each recorded
# figure within a factor 2 of the measurement).  Filled in from that run: measured (3 digits) -> recorded (rounded up).  The "_valid" rows are the
# same cases with the invalid labels replaced by class 0 (valid_variant): the inputs on which the module's two routes are compared, measured on
# those inputs.  GPU assertions get twice the figure.
F64_TOL = {                                                              # (elements of d_logit and of the map, nats)
    "r_1x1x1x1_k49_classes":                (3.0e-7, 3.0e-7),    # 2.94e-07, nats 2.94e-07 at nats up to 13
    "r_1x1x1x1_k3_classes":                 (5.4e-8, 5.4e-8),    # 5.32e-08, nats 5.32e-08 at nats up to 3.01
    "r_3x5x3x5_k49_image":                  (7.8e-7, 3.0e-6),    # 7.76e-07, nats 2.98e-06 at nats up to 429
    "r_3x5x3x5_k3_mixed":                   (4.5e-7, 1.5e-6),    # 4.46e-07, nats 1.44e-06 at nats up to 143
    "r_2x2x6x8_k49_mixed":                  (1.1e-6, 3.7e-6),    # 1.03e-06, nats 3.63e-06 at nats up to 536
    "r_2x2x6x8_k2_classes":                 (3.9e-7, 1.9e-7),    # 3.86e-07, nats 1.83e-07 at nats up to 125
    "r_3x4x6x8_k48_image":                  (9.9e-7, 5.4e-6),    # 9.86e-07, nats 5.38e-06 at nats up to 1.09e+03
    "r_2x3x4x12_k49_mixed_off1":            (9.3e-7, 8.7e-7),    # 9.28e-07, nats 8.61e-07 at nats up to 790
    "r_2x3x4x12_k50_mixed_off1":            (9.4e-7, 2.1e-6),    # 9.31e-07, nats 2.03e-06 at nats up to 769
    "r_2x1x4x12_k49_classes_off2":          (7.8e-7, 2.7e-6),    # 7.78e-07, nats 2.7e-06 at nats up to 274
    "r_1x1x16x32_k49_mixed":                (1.1e-6, 1.6e-6),    # 1.01e-06, nats 1.59e-06 at nats up to 2.8e+03
    "r_1x2x16x32_k64_mixed":                (9.3e-7, 5.7e-6),    # 9.29e-07, nats 5.69e-06 at nats up to 5.93e+03
    "r_2x1x15x19_k49_mixed":                (8.6e-7, 7.5e-6),    # 8.58e-07, nats 7.48e-06 at nats up to 1.62e+03
    "r_1x2x15x19_k1_mixed":                 (0.0, 0.0),    # 0, nats 0 at nats up to 0
    "r_1x1x10x30_k49_mixed":                (8.5e-7, 2.6e-6),    # 8.45e-07, nats 2.6e-06 at nats up to 1.63e+03
    "r_1x2x10x30_k50_classes":              (9.0e-7, 9.2e-6),    # 8.98e-07, nats 9.13e-06 at nats up to 3.57e+03
    "r_1x1x1x1_k49_classes_valid":          (3.0e-7, 3.0e-7),    # 2.94e-07, nats 2.94e-07 at nats up to 13
    "r_1x1x1x1_k3_classes_valid":           (5.4e-8, 5.4e-8),    # 5.32e-08, nats 5.32e-08 at nats up to 3.01
    "r_3x5x3x5_k49_image_valid":            (7.8e-7, 3.1e-6),    # 7.76e-07, nats 3.09e-06 at nats up to 439
    "r_3x5x3x5_k3_mixed_valid":             (4.5e-7, 1.5e-6),    # 4.46e-07, nats 1.45e-06 at nats up to 147
    "r_2x2x6x8_k49_mixed_valid":            (1.1e-6, 4.2e-6),    # 1.03e-06, nats 4.15e-06 at nats up to 548
    "r_2x2x6x8_k2_classes_valid":           (3.9e-7, 1.9e-7),    # 3.86e-07, nats 1.83e-07 at nats up to 125
    "r_3x4x6x8_k48_image_valid":            (9.9e-7, 6.9e-6),    # 9.86e-07, nats 6.81e-06 at nats up to 1.13e+03
    "r_2x3x4x12_k49_mixed_off1_valid":      (9.3e-7, 9.3e-7),    # 9.28e-07, nats 9.25e-07 at nats up to 818
    "r_2x3x4x12_k50_mixed_off1_valid":      (9.4e-7, 2.9e-6),    # 9.31e-07, nats 2.87e-06 at nats up to 800
    "r_2x1x4x12_k49_classes_off2_valid":    (7.8e-7, 2.7e-6),    # 7.78e-07, nats 2.7e-06 at nats up to 274
    "r_1x1x16x32_k49_mixed_valid":          (1.1e-6, 3.3e-6),    # 1.01e-06, nats 3.26e-06 at nats up to 2.91e+03
    "r_1x2x16x32_k64_mixed_valid":          (9.3e-7, 7.8e-6),    # 9.29e-07, nats 7.76e-06 at nats up to 6.11e+03
    "r_2x1x15x19_k49_mixed_valid":          (8.6e-7, 7.3e-6),    # 8.58e-07, nats 7.23e-06 at nats up to 1.69e+03
    "r_1x2x15x19_k1_mixed_valid":           (0.0, 0.0),    # 0, nats 0 at nats up to 0
    "r_1x1x10x30_k49_mixed_valid":          (8.5e-7, 2.6e-6),    # 8.45e-07, nats 2.54e-06 at nats up to 1.67e+03
    "r_1x2x10x30_k50_classes_valid":        (9.0e-7, 9.2e-6),    # 8.98e-07, nats 9.13e-06 at nats up to 3.57e+03
}
# MEASURED on an MI355X: the library route of lic360_operator.CeRateLoss (ContextReshape, torch's cross_entropy in fp32, a float64 sum per image)
# against the float64 statement, max over the images of |nats - float64 nats|, on the "_valid" inputs (tests/test_gpu_ce_rate.py::
# test_module_routes_against_float64 prints it again).  A figure of its own, because the route does NOT meet twice the reference's: a sum of
# hundreds of per-symbol roundings is a random walk, and where it ends for the reference's roundings says little about where it ends for torch's
# log-softmax -- the library's sums lie up to 10 x further from float64 than the reference's (DESIGN.md "Fused cross-entropy rate loss").  Per element
# the library route does meet twice F64_TOL, and is held to it.  Recorded rounded up; the GPU assertion gets twice the figure.
LIBRARY_NATS_TOL = {
    "r_1x1x1x1_k49_classes_valid":          3.0e-7,    # 2.94e-07 (per element 2.94e-07)
    "r_1x1x1x1_k3_classes_valid":           5.4e-8,    # 5.32e-08 (per element 5.32e-08)
    "r_3x5x3x5_k49_image_valid":            4.0e-6,    # 3.97e-06 (per element 7.76e-07)
    "r_3x5x3x5_k3_mixed_valid":             2.1e-6,    # 2.07e-06 (per element 4.46e-07)
    "r_2x2x6x8_k49_mixed_valid":            7.7e-6,    # 7.67e-06 (per element 7.6e-07)
    "r_2x2x6x8_k2_classes_valid":           5.7e-7,    # 5.65e-07 (per element 3.86e-07)
    "r_3x4x6x8_k48_image_valid":            8.8e-6,    # 8.78e-06 (per element 8.75e-07)
    "r_2x3x4x12_k49_mixed_off1_valid":      9.5e-6,    # 9.45e-06 (per element 8.96e-07)
    "r_2x3x4x12_k50_mixed_off1_valid":      6.5e-6,    # 6.45e-06 (per element 7.35e-07)
    "r_2x1x4x12_k49_classes_off2_valid":    3.3e-6,    # 3.26e-06 (per element 6.17e-07)
    "r_1x1x16x32_k49_mixed_valid":          2.4e-5,    # 2.4e-05 (per element 9.57e-07)
    "r_1x2x16x32_k64_mixed_valid":          4.6e-5,    # 4.51e-05 (per element 1.17e-06)
    "r_2x1x15x19_k49_mixed_valid":          1.2e-5,    # 1.14e-05 (per element 8.58e-07)
    "r_1x2x15x19_k1_mixed_valid":           0.0,    # 0 (per element 0)
    "r_1x1x10x30_k49_mixed_valid":          1.3e-5,    # 1.27e-05 (per element 8.45e-07)
    "r_1x2x10x30_k50_classes_valid":        2.4e-5,    # 2.32e-05 (per element 9.76e-07)
}

# ---------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> dict(logit [N, G*K, H, W], label [N, G, H, W], grad [N], read-only fp32; edges: the names of the edge rows planted)"""
    if case.family == "valid":
        base = inputs(BASE_OF[case.id])
        label = np.array(base["label"])
        label[~valid_of(label, case.K)] = 0
        label.setflags(write=False)
        return dict(base, label=label)
    rng = _rng("ce_rate", case.id)
    N, G, H, W, K = case.N, case.G, case.H, case.W, case.K
    M = N * G * H * W
    logit = rng.normal(0, 2, (N, G * K, H, W)).astype(F)
    lab = np.resize(np.arange(K), M)                                    # every class, 0 and K - 1 included, when there are K symbols or more
    label = rng.permutation(lab).astype(F).reshape(N, G, H, W)
    flat = label.reshape(-1)
    if case.labels in ("mixed", "image") and M >= 12:
        pick = rng.permutation(M)[:max(8, M // 16)]
        for k, j in enumerate(pick):
            kind = k % 8
            if kind == 0: flat[j] = -0.5                                # valid: class 0
            if kind == 1: flat[j] = flat[j] + F(0.7)                    # valid: class c of c + 0.7, truncated, not rounded
            if kind == 2: flat[j] = -1.0                                # invalid from here on
            if kind == 3: flat[j] = K
            if kind == 4: flat[j] = 1e9
            if kind == 5: flat[j] = np.nan
            if kind == 6: flat[j] = np.nextafter(F(K), F(0))            # the largest valid label: class K - 1
            if kind == 7: flat[j] = np.nextafter(F(-1), F(0))           # the smallest valid label: class 0
    if case.labels == "image":
        label[1] = np.resize(np.array([-1.0, K, 1e9, np.nan, -7.0, K + 0.5], F), G * H * W).reshape(G, H, W)
    grad = (rng.uniform(0.5, 1.5, N) * np.where(np.arange(N) % 2, -1.0, 1.0)).astype(F)
    edges = []
    if case.family == "edge":
        valid = valid_of(label, K)
        where = np.argwhere(valid)
        assert len(where) >= len(EDGE_KINDS) and K >= 3, case.id
        pick = where[rng.permutation(len(where))[:len(EDGE_KINDS)]]
        for kind, (n, g, y, x) in zip(EDGE_KINDS, pick):
            row = logit[n, g * K:(g + 1) * K, y, x]                     # a view: the symbol's K logits
            if kind == "equal": row[:] = 0.625
            if kind == "max_first": row[0] = 9.5
            if kind == "max_last": row[K - 1] = 9.5
            if kind == "max_tied": row[0] = row[K - 1] = 9.5
            if kind == "spread_past_104":                               # lic360_expf gives 0 beyond -104: p is exactly 0 off the maximum
                row[:] = -60.0
                row[K // 2] = 50.0
            if kind == "magnitude_1e30":
                row[:] = np.where(np.arange(K) % 2, F(-1e30), F(1e30))
                row[0] = F(0.9e30)
            if kind == "subnormal_spread":
                row[:] = (np.arange(K) % 7).astype(F) * F(1.4e-45)
            edges.append(kind)
        dead = np.argwhere(~valid)
        assert len(dead) >= 3, case.id
        for k, (n, g, y, x) in enumerate(dead[rng.permutation(len(dead))[:3]]):
            logit[n, g * K + k % K, y, x] = (1e30, -1e30, 3e38)[k]      # huge logits under invalid symbols
        grad = np.array([0.0, -1.5, 0.75], F)[:N]
    out = dict(logit=logit, label=label, grad=grad)
    for v in out.values():
        v.setflags(write=False)
    out["edges"] = tuple(edges)
    return out


# ---------------------------------------------------------------------------------------------------- the reference
def rows(t, case, g_for_gk=False):
    """[N, G*K, H, W] -> [N*G*H*W, K]: ContextReshape's rows.  g_for_gk: the broken channel index g + i (clipped to the tensor)"""
    N, G, H, W, K = case.N, case.G, case.H, case.W, case.K
    if g_for_gk:
        ch = np.minimum(np.arange(G)[:, None] + np.arange(K)[None, :], G * K - 1)             # [G, K]
        return np.ascontiguousarray(t[:, ch].transpose(0, 1, 3, 4, 2)).reshape(-1, K)
    return np.ascontiguousarray(t.reshape(N, G, K, H, W).transpose(0, 1, 3, 4, 2)).reshape(-1, K)


def planes(r, case):
    """the inverse of rows"""
    N, G, H, W, K = case.N, case.G, case.H, case.W, case.K
    return np.ascontiguousarray(r.reshape(N, G, H, W, K).transpose(0, 1, 4, 2, 3)).reshape(N, G * K, H, W)


LN2_HI, LN2_LO, SQRT2 = F(float.fromhex("0x1.62e400p-1")), F(float.fromhex("0x1.7f7d1cp-20")), F(float.fromhex("0x1.6a09e6p+0"))
LOG_COEFFS = tuple(F(float.fromhex(h)) for h in ("0x1.745d18p-4", "0x1.c71c72p-4", "0x1.24924ap-3", "0x1.99999ap-3", "0x1.555556p-2"))


def logf(x):
    """lic360_logf (csrc/lic360_exact_math.h:79-103) on an fp32 array, operation by operation: x <= 0 (and NaN) -> -inf"""
    x = np.ascontiguousarray(x, F).reshape(-1)
    with np.errstate(all="ignore"):
        pos = x > 0
        x1 = np.where(pos, x, F(1.0))
        u = x1.view(np.uint32)
        sub = u < np.uint32(0x00800000)
        x1 = np.where(sub, x1 * F(16777216.0), x1).astype(F)
        u = x1.view(np.uint32)
        e = np.where(sub, -24, 0) + (u >> np.uint32(23)).astype(np.int64) - 127
        f = ((u & np.uint32(0x007fffff)) | np.uint32(0x3f800000)).view(F)
        big = f > SQRT2
        f = np.where(big, f * F(0.5), f).astype(F)
        e = e + big
        s = ((f - F(1.0)).astype(F) / (f + F(1.0)).astype(F)).astype(F)
        z = (s * s).astype(F)
        p = np.full(x.shape, LOG_COEFFS[0], F)
        for c in LOG_COEFFS[1:] + (F(1.0),):
            p = fmaf(p, z, np.full(x.shape, c, F))
        lm = ((F(2.0) * s).astype(F) * p).astype(F)
        ef = e.astype(F)
        out = fmaf(ef, np.full(x.shape, LN2_HI, F), fmaf(ef, np.full(x.shape, LN2_LO, F), lm))
        return np.where(pos, out, F(-np.inf)).astype(F)


BROKEN = ("no_max_subtraction", "sum_reversed", "label_rounded", "invalid_clamped", "minus_one_on_wrong_class", "gk_taken_as_g", "ragged_tail_written",
          "t_of_image_0", "finish_first_pass_only")
UNWRITTEN = F(7.7701e33)


@functools.lru_cache(maxsize=None)
def reference(case, broken=None):
    """-> dict(map [N,G,H,W] f32, symbols, invalid [N] int64, nats [N] float (math.fsum of the valid fp32 losses), abs [N] float (fsum of their
    magnitudes), d_logit [N,G*K,H,W] f32, valid [N,G,H,W] bool).  broken: one of BROKEN, a model of a plausible bug, for the test that the cases
    would notice it."""
    assert broken is None or broken in BROKEN
    d = inputs(case)
    N, G, H, W, K = case.N, case.G, case.H, case.W, case.K
    label = d["label"]
    clamped = broken == "invalid_clamped"
    valid = valid_of(label, K, clamped)
    with np.errstate(invalid="ignore"):
        if clamped:
            cls_all = np.clip(np.nan_to_num(label, nan=0.0), 0, K - 1).astype(np.int64)
        elif broken == "label_rounded":
            cls_all = np.clip(np.rint(np.where(valid, label, 0)), 0, K - 1).astype(np.int64)
        else:
            cls_all = np.where(valid, label, 0).astype(np.int64)        # astype truncates toward zero, as (int) does
    sel = np.flatnonzero(valid.reshape(-1))
    L = rows(d["logit"], case, broken == "gk_taken_as_g")[sel]
    c = cls_all.reshape(-1)[sel]
    t = np.repeat(d["grad"] if broken != "t_of_image_0" else np.full(N, d["grad"][0], F), G * H * W)[sel][:, None]
    idx = np.arange(len(sel))
    with np.errstate(all="ignore"):
        m = L[:, 0].copy() if len(sel) else np.zeros(0, F)
        for i in range(1, K):
            m = np.where(m < L[:, i], L[:, i], m)
        if broken == "no_max_subtraction":
            m = np.zeros_like(m)
        dlt = (L - m[:, None]).astype(F)
        e = orc.expf(dlt).reshape(dlt.shape) if len(sel) else np.zeros((0, K), F)
        s = np.zeros(len(sel), F)
        for i in (range(K - 1, -1, -1) if broken == "sum_reversed" else range(K)):
            s = (s + e[:, i]).astype(F)
        loss = (logf(s) - dlt[idx, c]).astype(F)
        p = (e / s[:, None]).astype(F)
        hot = np.zeros((len(sel), K), bool)
        hot[idx, (c + 1) % K if broken == "minus_one_on_wrong_class" else c] = True
        dl = (np.where(hot, (p - F(1.0)).astype(F), p) * t).astype(F)
    full = np.zeros((N * G * H * W, K), F)
    full[sel] = dl
    out = dict(d_logit=planes(full, case), valid=valid)
    mp = np.zeros(N * G * H * W, F)
    mp[sel] = loss
    out["map"] = mp.reshape(N, G, H, W)
    out["symbols"] = valid.reshape(N, -1).sum(1).astype(np.int64)
    out["invalid"] = (~valid).reshape(N, -1).sum(1).astype(np.int64)
    summed = valid.reshape(N, -1)
    if broken == "finish_first_pass_only":
        # slot j = g * chunks + chunk of an image; the slots past the first THREADS never reach nats and the counts
        slot = (np.arange(G)[:, None] * chunks(case) + np.arange(H * W)[None, :] // CHUNK).reshape(-1)
        summed = summed & (slot < THREADS)
        out["symbols"] = summed.sum(1).astype(np.int64)
        out["invalid"] = (~valid.reshape(N, -1) & (slot < THREADS)).sum(1).astype(np.int64)
    per = [list(map(float, mp.reshape(N, -1)[n][summed[n]])) for n in range(N)]
    if broken == "ragged_tail_written" and (H * W) % CHUNK:
        # the cells past the plane's end in its last chunk load zeros: label 0, K equal logits -- valid symbols of class 0 that cost log K
        tail = chunks(case) * CHUNK - H * W
        cost = float(logf(np.array([K], F))[0])
        out["symbols"] = out["symbols"] + G * tail
        per = [v + [cost] * (G * tail) for v in per]
    out["nats"] = np.array([math.fsum(v) for v in per], np.float64)
    out["abs"] = np.array([math.fsum(abs(x) for x in v) for v in per], np.float64)
    for v in out.values():
        v.setflags(write=False)
    return out


def nats_bound(ref):
    """how far a double sum of the fp32 losses in any fixed order can be from their exact sum: symbols * 2^-53 * sum|loss|, per image"""
    return ref["symbols"].astype(np.float64) * 2.0 ** -53 * ref["abs"]


# ---------------------------------------------------------------------------------------------------- the whole head in float64
def head_f64_torch(logit, label, G, K):
    """float64 logit (requires_grad where a gradient is wanted), float64 label -> (nats [N], loss [N,G,H,W]); the head as mathematics:
    -log softmax over a symbol's K logits at the truncated label, the valid symbols summed per image"""
    import torch
    N, _, H, W = logit.shape
    valid = (label > -1.0) & (label < float(K))
    cls = torch.where(valid, label, torch.zeros_like(label)).to(torch.int64)
    logp = torch.log_softmax(logit.reshape(N, G, K, H, W), dim=2)
    loss = -logp.gather(2, cls.reshape(N, G, 1, H, W)).reshape(N, G, H, W)
    loss = torch.where(valid, loss, torch.zeros_like(loss))
    return loss.reshape(N, -1).sum(1), loss


@functools.lru_cache(maxsize=None)
def head_f64(case):
    """-> dict(nats [N], map [N,G,H,W], d_logit) in float64: autograd of sum_n grad[n] nats[n]"""
    import torch
    d = inputs(case)
    logit = torch.tensor(d["logit"].astype(np.float64), requires_grad=True)
    nats, loss = head_f64_torch(logit, torch.tensor(d["label"].astype(np.float64)), case.G, case.K)
    (nats * torch.tensor(d["grad"].astype(np.float64))).sum().backward()
    return dict(nats=nats.detach().numpy(), map=loss.detach().numpy(), d_logit=logit.grad.numpy())


def f64_distance(case, got):
    """(max |got - float64| over d_logit and, where given, the map; max over the images of |nats - float64 nats|, where given)"""
    f = head_f64(case)
    worst = 0.0
    for k in ("d_logit", "map"):
        if got.get(k) is not None:
            worst = max(worst, float(np.abs(got[k].astype(np.float64) - f[k]).max()))
    dn = float(np.abs(np.asarray(got["nats"], np.float64) - f["nats"]).max()) if got.get("nats") is not None else 0.0
    return worst, dn
