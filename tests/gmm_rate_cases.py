"""The fused GMM rate loss (csrc/gmm_rate_kernels.hip, DESIGN.md "Fused GMM rate loss"): cases, the launch geometry restated, the reference
and models of broken kernels (numpy, torch on the CPU and the CPU oracle only; no GPU, and nothing of the unit under test).

The arithmetic contract, restated.  Inputs fp32 contiguous: logit, sigma, mean [N, G*ng, H, W] (the raw outputs of the three nets), label
[N, G, H, W], mask [N, G, H, W] or absent (every symbol coded).  Symbol (n, g, y, x) reads channel g*ng + i of each net, i < ng -- the element
ContextReshape puts in row ((n G + g) H + y) W + x, column i -- and is coded iff mask >= 0.5.  For a coded symbol, every operation rounded once
in fp32:
    w       = lic360_softmax_inplace(logit[0..ng)): the max, lic360_expf(l_i - max), the sum in index order from 0, the division
    s_i     = sigma_i > 0 ? sigma_i + 1e-5f : 1e-5f
    loss, wd_i, dd_i, md_i, ld = what k_entropy_gmm computes from (w, s, mean, label)                       (here: the CPU oracle)
    backward with t = grad_nats[n]:  gw_i = wd_i t,  d_mean_i = md_i t,  d_sigma_i = sigma_i > 0 ? dd_i t : 0,  d_label = ld t,
                                     dot = sum_i fmaf(gw_i, w_i, dot) in index order,  d_logit_i = w_i (gw_i - dot)
An uncoded symbol costs 0, counts as no symbol and gets exact zeros in every gradient, whatever its parameters hold.  nats[n] (float64) is the
sum of the coded symbols' fp32 losses added in double in some fixed order: within symbols * 2^-53 * sum|loss| of math.fsum.  symbols[n] is
the count, map the per-symbol loss (0 where uncoded).

The reference is built from pieces that do not come from the new unit: the softmax from oracle.expf in fp32 numpy, oracle.entropy_gmm, the
chain rule in fp32 numpy (the fused multiply-add by an exact product in double and one rounding to odd), math.fsum.  `head_f64` states the whole
head in float64 torch autograd, in the style of ops_edge_cases.gmm_loss_f64.
"""
import collections
import functools
import math

import numpy as np

import oracle as orc
from ops_edge_cases import GMM_MIN_P, GMM_MIN_KEPT, GMM_UNDERFLOW_LOSS, _rng      # the conditions of the GMM-loss cases, kept

F = np.float32

# ---------------------------------------------------------------------------------------------------- the launch geometry, restated
THREADS = 256                 # GR_THREADS
PER_THREAD = 4                # GR_PER_THREAD: cells of a plane per thread
CHUNK = THREADS * PER_THREAD  # GR_CHUNK: cells of one (n, g) plane per workgroup
WAVE = 64
MAX_NG = 16                   # GR_MAX_NG
STATIC_NG = 3                 # the instantiation with the mixture size at compile time
SIGMA_FLOOR = F(0.00001)

Case = collections.namedtuple("Case", "id N G H W ng mask family offset")


def _c(N, G, H, W, ng, mask, family="regular", offset=0):
    return Case("%s_%dx%dx%dx%d_ng%d_%s%s" % (family[0], N, G, H, W, ng, mask, "_off%d" % offset if offset else ""), N, G, H, W, ng, mask, family, offset)


MASK_KINDS = ("absent", "ones", "zeros", "image", "stair", "runs64", "runs256")
CASES = (
    _c(1, 1, 1, 1, 3, "absent"),
    _c(1, 1, 1, 1, 5, "ones"),
    _c(3, 5, 3, 5, 3, "stair"),              # N and H W odd: image and plane bases on 4-byte boundaries only -> the scalar form
    _c(3, 5, 3, 5, 1, "image"),
    _c(3, 5, 3, 5, 5, "absent"),
    _c(2, 4, 6, 8, 3, "ones"),               # the vector form
    _c(2, 4, 6, 8, 3, "zeros"),
    _c(2, 4, 6, 8, 5, "stair"),
    _c(2, 4, 6, 8, 1, "absent"),
    _c(3, 4, 6, 8, 3, "image"),
    _c(2, 3, 4, 12, 3, "stair", offset=1),   # W % 4 == 0, every tensor 4 bytes off a 16-byte boundary: the scalar form must be chosen
    _c(2, 3, 4, 12, 5, "absent", offset=1),
    _c(1, 2, 32, 64, 3, "runs256"),          # planes of exactly two chunks, vector form; whole waves uncoded next to coded ones
    _c(1, 2, 32, 64, 1, "stair"),
    _c(2, 2, 25, 45, 3, "runs64"),           # 1125 cells: a second, ragged chunk of 101, scalar form; whole waves uncoded
    _c(1, 2, 25, 45, 5, "stair"),
    _c(1, 1, 33, 36, 3, "absent"),           # 1188 cells: a ragged second chunk in the vector form
    _c(1, 1, 33, 36, 5, "runs256"),
    _c(3, 5, 3, 5, 3, "stair", "edge"),
    _c(3, 5, 3, 5, 5, "stair", "edge"),
    _c(2, 4, 6, 8, 3, "stair", "edge"),
    _c(2, 4, 6, 8, 1, "stair", "edge"),
    _c(3, 2, 25, 45, 3, "runs64", "edge"),
    _c(1, 2, 32, 64, 5, "runs256", "edge"),
    _c(2, 257, 2, 4, 3, "stair", "slots"),   # 257 slots per image: the finish kernel's second pass (THREADS + 1), vector form, ng = 3
    _c(2, 257, 3, 5, 5, "stair", "slots"),   # the same in the scalar form, ng at run time
)
REGULAR = tuple(c for c in CASES if c.family == "regular")
EDGE = tuple(c for c in CASES if c.family == "edge")
SLOTS = tuple(c for c in CASES if c.family == "slots")       # kernels only: bit for bit and within nats_bound, no recorded float64 figures
BY_ID = {c.id: c for c in CASES}


def form(case):
    """the launcher's choice: 16-byte accesses when W % 4 == 0 and every base is 16-byte aligned (offset: floats past an aligned start)"""
    return "vec" if case.W % 4 == 0 and case.offset % 4 == 0 else "scalar"


def instantiation(case):
    return "static" if case.ng == STATIC_NG else "generic"


def chunks(case):
    return -(-(case.H * case.W) // CHUNK)


def wave_of(case):
    """-> int array [H*W]: the wave (workgroup-wide index: chunk * 4 + wave in the workgroup) that holds each cell of a plane"""
    cell = np.arange(case.H * case.W)
    local = cell % CHUNK
    tid = local // PER_THREAD if form(case) == "vec" else local % THREADS
    return (cell // CHUNK) * (THREADS // WAVE) + tid // WAVE


def reach(case):
    """names of the code paths and edges a case reaches, derived from the restated geometry and the case's own mask"""
    d = inputs(case)
    names = {form(case), instantiation(case), form(case) + "_" + instantiation(case), "mask_" + case.mask, "family_" + case.family}
    hw = case.H * case.W
    if chunks(case) > 1:
        names.add("multi_chunk")
    if hw % CHUNK:
        names.add("ragged_chunk_" + form(case))
    if case.W % 4 == 0 and case.offset % 4:
        names.add("misaligned_w4")
    if hw % 4 and case.N * case.G > 1:
        names.add("plane_base_4_byte")
    coded = coded_of(d["mask"], case).reshape(case.N * case.G, hw)
    wv = wave_of(case)
    live = np.array([[coded[p, wv == k].any() for k in range(wv.max() + 1)] for p in range(coded.shape[0])])
    if (~live).any() and live.any() and any((~row).any() and row.any() for row in live):
        names.add("dead_wave_beside_live_" + form(case))
    if case.N > 1 and any(not coded.reshape(case.N, -1)[n].any() for n in range(case.N)) and coded.any():
        names.add("dead_image_among_live")
    if case.G * chunks(case) > THREADS:                                  # slots per image: the finish kernel adds them in passes of THREADS
        names.add("finish_second_pass")
    return names


REACH = ("vec_static", "vec_generic", "scalar_static", "scalar_generic", "multi_chunk", "ragged_chunk_vec", "ragged_chunk_scalar", "misaligned_w4",
         "plane_base_4_byte", "dead_wave_beside_live_vec", "dead_wave_beside_live_scalar", "dead_image_among_live", "family_regular", "family_edge", "finish_second_pass") + \
    tuple("mask_" + k for k in MASK_KINDS)

# MEASURED: max |reference - float64 autograd| on the rows with p >= GMM_MIN_P, (over the four gradients and the loss, of nats[n]); gradient scales
# reach ~15 at sigma = 0.3 (tests/test_gmm_rate_cases_cpu.py::test_reference_against_float64 re-measures, prints and holds the recorded figure
# within a factor 2 of the measurement).  Filled in from that run: measured (3 digits) -> recorded (rounded up).
F64_TOL = {                                                              # (gradients and loss, nats)
    "r_1x1x1x1_ng3_absent":                (1.8e-7, 1.8e-7),    # 1.7e-07 at gradient scale 0.58, nats 1.7e-07, 100.0 % kept
    "r_1x1x1x1_ng5_ones":                  (5.1e-8, 4.2e-8),    # 5.04e-08 at gradient scale 0.243, nats 4.14e-08, 100.0 % kept
    "r_3x5x3x5_ng3_stair":                 (3.0e-7, 1.9e-6),    # 2.93e-07 at gradient scale 1.24, nats 1.88e-06, 100.0 % kept
    "r_3x5x3x5_ng1_image":                 (1.4e-6, 2.0e-6),    # 1.38e-06 at gradient scale 5.71, nats 1.96e-06, 100.0 % kept
    "r_3x5x3x5_ng5_absent":                (2.9e-7, 2.7e-6),    # 2.89e-07 at gradient scale 2, nats 2.65e-06, 100.0 % kept
    "r_2x4x6x8_ng3_ones":                  (4.8e-7, 3.6e-6),    # 4.72e-07 at gradient scale 4.26, nats 3.54e-06, 100.0 % kept
    "r_2x4x6x8_ng3_zeros":                 (0.0, 0.0),    # 0 at gradient scale 0, nats 0, 100.0 % kept
    "r_2x4x6x8_ng5_stair":                 (3.5e-7, 3.8e-6),    # 3.49e-07 at gradient scale 2.31, nats 3.75e-06, 100.0 % kept
    "r_2x4x6x8_ng1_absent":                (4.2e-6, 9.0e-6),    # 4.14e-06 at gradient scale 15.7, nats 8.96e-06, 99.7 % kept
    "r_3x4x6x8_ng3_image":                 (5.2e-7, 2.6e-6),    # 5.12e-07 at gradient scale 3.29, nats 2.59e-06, 100.0 % kept
    "r_2x3x4x12_ng3_stair_off1":           (2.0e-7, 1.5e-6),    # 1.96e-07 at gradient scale 1.2, nats 1.5e-06, 100.0 % kept
    "r_2x3x4x12_ng5_absent_off1":          (4.2e-7, 4.1e-6),    # 4.15e-07 at gradient scale 1.78, nats 4.08e-06, 100.0 % kept
    "r_1x2x32x64_ng3_runs256":             (3.8e-6, 4.9e-5),    # 3.77e-06 at gradient scale 6.16, nats 4.81e-05, 100.0 % kept
    "r_1x2x32x64_ng1_stair":               (2.4e-5, 2.0e-5),    # 2.3e-05 at gradient scale 15.5, nats 1.96e-05, 99.7 % kept
    "r_2x2x25x45_ng3_runs64":              (2.4e-6, 2.4e-5),    # 2.36e-06 at gradient scale 5.65, nats 2.31e-05, 100.0 % kept
    "r_1x2x25x45_ng5_stair":               (1.5e-6, 3.2e-5),    # 1.44e-06 at gradient scale 4.84, nats 3.16e-05, 100.0 % kept
    "r_1x1x33x36_ng3_absent":              (2.2e-6, 3.1e-5),    # 2.17e-06 at gradient scale 5.01, nats 3.06e-05, 99.9 % kept
    "r_1x1x33x36_ng5_runs256":             (3.7e-7, 1.8e-5),    # 3.64e-07 at gradient scale 2.22, nats 1.75e-05, 100.0 % kept
}


# ---------------------------------------------------------------------------------------------------- inputs
def _mask(case, rng):
    N, G, H, W = case.N, case.G, case.H, case.W
    cell = np.arange(H * W)
    if case.mask == "absent":
        return None
    if case.mask == "ones":
        return np.ones((N, G, H, W), F)
    if case.mask == "zeros":
        return np.zeros((N, G, H, W), F)
    if case.mask == "image":                                            # one fully masked image among coded ones
        m = np.ones((N, G, H, W), F)
        m[1] = 0
        return m
    if case.mask == "stair":                                            # g < L[y, x], the importance map's staircase
        L = rng.integers(0, G + 1, (N, 1, H, W))
        L[:, :, 0, 0] = G                                               # one column fully coded, so every plane has a coded cell
        return (np.arange(G)[None, :, None, None] < L).astype(F)
    if case.mask == "runs64":                                           # runs of 64 cells: every second run of a 256-cell stretch uncoded
        keep = ((cell % THREADS) // WAVE) % 2 == 0
    else:                                                               # runs of 256 cells
        keep = (cell // THREADS) % 2 == 0
    return np.broadcast_to(keep.reshape(1, 1, H, W), (N, G, H, W)).astype(F).copy()


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> dict(logit, sigma, mean [N, G*ng, H, W], label [N, G, H, W], mask or None, grad [N]), read-only fp32"""
    rng = _rng("gmm_rate", case.id)
    N, G, H, W, ng = case.N, case.G, case.H, case.W, case.ng
    label = (rng.integers(0, 8, (N, G, H, W)) - 3.5).astype(F)
    lab_c = np.repeat(label, ng, 1)                                     # channel g*ng + i <- group g
    logit = rng.normal(0, 1, (N, G * ng, H, W)).astype(F)
    sigma = rng.uniform(0.3, 2.0, (N, G * ng, H, W)).astype(F)
    mean = (lab_c + rng.normal(0, 0.6, (N, G * ng, H, W))).astype(F)
    mask = _mask(case, rng)
    grad = (rng.uniform(0.5, 1.5, N) * np.where(np.arange(N) % 2, -1.0, 1.0)).astype(F)
    if case.family == "edge":
        coded = coded_of(mask, case)
        where = np.argwhere(coded)                                      # coded symbols (n, g, y, x), in index order
        assert len(where) >= 12, case.id
        pick = where[rng.permutation(len(where))[:12]]
        ch = lambda g, i: g * ng + i
        for k, (n, g, y, x) in enumerate(pick):
            i = k % ng
            if k == 0: sigma[n, ch(g, i), y, x] = 0.0                   # raw sigma exactly 0 ...
            if k == 1: sigma[n, ch(g, i), y, x] = -0.75                 # ... negative ...
            if k == 2: sigma[n, ch(g, i), y, x] = -0.0                  # ... and the negative zero
            if k == 3:                                                  # negative, but positive once the floor is added; the upper
                sigma[n, ch(g, i), y, x] = -4e-6                        # bin edge 8e-6 from the mean, so that the floor's size shows
                mean[n, ch(g, i), y, x] = F(label[n, g, y, x] + F(0.5)) - F(8e-6)
            if k == 4: logit[n, ch(g, 0):ch(g, 0) + ng, y, x] = 0.625   # equal logits
            if k == 5:                                                  # a gap beyond 104: lic360_expf gives 0, the weight is exactly 0
                logit[n, ch(g, 0):ch(g, 0) + ng, y, x] = -60.0
                logit[n, ch(g, ng - 1), y, x] = 50.0
            if k == 6:                                                  # p underflows: every component narrow and 3 away
                sigma[n, ch(g, 0):ch(g, 0) + ng, y, x] = 0.01
                mean[n, ch(g, 0):ch(g, 0) + ng, y, x] = label[n, g, y, x] + (3.0 if label[n, g, y, x] < 0 else -3.0)
            if k == 7: label[n, g, y, x] = -3.5
            if k == 8: label[n, g, y, x] = 3.5
            if k == 9: mask[n, g, y, x] = 0.5                           # coded: the rule is >=
            if k == 10: mask[n, g, y, x] = 0.75
            if k == 11: mask[n, g, y, x] = 2.0
        dead = np.argwhere(~coded)
        assert len(dead) >= 6, case.id
        bad = (np.inf, -np.inf, np.nan)
        for k, (n, g, y, x) in enumerate(dead[rng.permutation(len(dead))[:6]]):
            t = (logit, sigma, mean)[k % 3]
            t[n, ch(g, k % ng), y, x] = bad[(k // 3 + k) % 3]           # Inf / NaN parameters under uncoded symbols only
            if k == 4: mask[n, g, y, x] = np.nextafter(F(0.5), F(0))    # the largest uncoded value
            if k == 5: label[n, g, y, x] = np.nan
        grad = np.array([0.0, -1.5, 0.75], F)[:N] if N > 1 else np.array([-1.25], F)
        if N == 2:
            grad = np.array([0.0, -1.5], F)
    out = dict(logit=logit, sigma=sigma, mean=mean, label=label, mask=mask, grad=grad)
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


def coded_of(mask, case, rule=np.greater_equal):
    return np.ones((case.N, case.G, case.H, case.W), bool) if mask is None else rule(mask, F(0.5))


# ---------------------------------------------------------------------------------------------------- the reference
def rows(t, case, swapped=False):
    """[N, G*ng, H, W] -> [N*G*H*W, ng]: ContextReshape's rows.  swapped: the broken channel index i*G + g"""
    N, G, H, W, ng = case.N, case.G, case.H, case.W, case.ng
    if swapped:
        return np.ascontiguousarray(t.reshape(N, ng, G, H, W).transpose(0, 2, 3, 4, 1)).reshape(-1, ng)
    return np.ascontiguousarray(t.reshape(N, G, ng, H, W).transpose(0, 1, 3, 4, 2)).reshape(-1, ng)


def planes(r, case, swapped=False):
    """the inverse of rows"""
    N, G, H, W, ng = case.N, case.G, case.H, case.W, case.ng
    if swapped:
        return np.ascontiguousarray(r.reshape(N, G, H, W, ng).transpose(0, 4, 1, 2, 3)).reshape(N, G * ng, H, W)
    return np.ascontiguousarray(r.reshape(N, G, H, W, ng).transpose(0, 1, 4, 2, 3)).reshape(N, G * ng, H, W)


def fmaf(a, b, c):
    """fp32 fused multiply-add of arrays: the product is exact in double, the sum is rounded to odd there, so the rounding to fp32 is the only one"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    odd = (s.view(np.int64) & 1) != 0
    fix = (err != 0) & ~odd & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F)


def softmax_rows(l, no_max=False):
    """lic360_softmax_inplace on [M, ng] fp32: max, lic360_expf (the oracle's), the sum in index order from 0, the division"""
    m = l[:, 0].copy()
    for i in range(1, l.shape[1]):
        m = np.where(m < l[:, i], l[:, i], m)
    with np.errstate(all="ignore"):
        e = orc.expf(l if no_max else (l - m[:, None]).astype(F)).reshape(l.shape)
        s = np.zeros(l.shape[0], F)
        for i in range(l.shape[1]):
            s = (s + e[:, i]).astype(F)
        return (e / s[:, None]).astype(F)


BROKEN = ("channel_i_major", "mask_rule_gt", "relu_gradient_kept", "floor_before_sign", "softmax_without_max", "dot_reversed", "uncoded_unwritten",
          "last_chunk_dropped", "d_label_scaled_twice", "finish_first_pass_only")
UNWRITTEN = F(7.7701e33)


@functools.lru_cache(maxsize=None)
def reference(case, broken=None):
    """-> dict(map [N,G,H,W] f32, symbols [N] int64, nats [N] float (math.fsum of the coded fp32 losses), abs [N] float (fsum of their
    magnitudes), d_logit, d_sigma, d_mean [N,G*ng,H,W] f32, d_label [N,G,H,W] f32, coded [N,G,H,W] bool).  broken: one of BROKEN, a model of a
    plausible bug, for the test that the cases would notice it."""
    assert broken is None or broken in BROKEN
    d = inputs(case)
    N, G, H, W, ng = case.N, case.G, case.H, case.W, case.ng
    swapped = broken == "channel_i_major"
    coded = coded_of(d["mask"], case, np.greater if broken == "mask_rule_gt" else np.greater_equal)
    written = np.ones((N, G, H, W), bool)
    if broken == "last_chunk_dropped" and (H * W) % CHUNK:
        written.reshape(N, G, -1)[:, :, (chunks(case) - 1) * CHUNK:] = False
        coded = coded & written
    sel = np.flatnonzero(coded.reshape(-1))
    L, S, M = (rows(d[k], case, swapped)[sel] for k in ("logit", "sigma", "mean"))
    lab = d["label"].reshape(-1, 1)[sel]
    t = np.repeat(d["grad"], G * H * W)[sel][:, None]
    w = softmax_rows(L, no_max=broken == "softmax_without_max")
    with np.errstate(all="ignore"):
        if broken == "floor_before_sign":
            s = np.where((S + SIGMA_FLOOR).astype(F) > 0, (S + SIGMA_FLOOR).astype(F), SIGMA_FLOOR).astype(F)
        else:
            s = np.where(S > 0, (S + SIGMA_FLOOR).astype(F), SIGMA_FLOOR).astype(F)
        if len(sel):
            loss, wd, dd, md, ld = orc.entropy_gmm(w, s, M, lab)
        else:
            loss, wd, dd, md, ld = np.zeros(0, F), np.zeros((0, ng), F), np.zeros((0, ng), F), np.zeros((0, ng), F), np.zeros((0, 1), F)
        gw = (wd * t).astype(F)
        dmean = (md * t).astype(F)
        dsigma = (dd * t).astype(F) if broken == "relu_gradient_kept" else np.where(S > 0, (dd * t).astype(F), F(0)).astype(F)
        dlabel = (ld * t).astype(F)
        if broken == "d_label_scaled_twice":
            dlabel = (dlabel * t).astype(F)
        dot = np.zeros(len(sel), F)
        for i in (range(ng - 1, -1, -1) if broken == "dot_reversed" else range(ng)):
            dot = fmaf(gw[:, i], w[:, i], dot)
        dlogit = (w * (gw - dot[:, None]).astype(F)).astype(F)
    fill = UNWRITTEN if broken == "uncoded_unwritten" else F(0)

    def scatter(v, width):
        full = np.full((N * G * H * W, width), fill, F)
        full[sel] = v.reshape(len(sel), width)
        if broken == "last_chunk_dropped":
            full[~written.reshape(-1)] = UNWRITTEN
        return full
    out = dict(d_logit=planes(scatter(dlogit, ng), case, swapped), d_sigma=planes(scatter(dsigma, ng), case, swapped),
               d_mean=planes(scatter(dmean, ng), case, swapped), d_label=scatter(dlabel, 1).reshape(N, G, H, W), coded=coded)
    m = np.zeros(N * G * H * W, F)
    m[sel] = loss
    out["map"] = m.reshape(N, G, H, W)
    out["symbols"] = coded.reshape(N, -1).sum(1).astype(np.int64)
    summed = coded.reshape(N, -1)
    if broken == "finish_first_pass_only":
        # slot j = g * chunks + chunk of an image; the slots past the first THREADS never reach nats and the count
        slot = (np.arange(G)[:, None] * chunks(case) + np.arange(H * W)[None, :] // CHUNK).reshape(-1)
        summed = summed & (slot < THREADS)
        out["symbols"] = summed.sum(1).astype(np.int64)
    per = [m.reshape(N, -1)[n][summed[n]] for n in range(N)]
    out["nats"] = np.array([math.fsum(float(v) for v in p) for p in per], np.float64)
    out["abs"] = np.array([math.fsum(abs(float(v)) for v in p) for p in per], np.float64)
    for v in out.values():
        v.setflags(write=False)
    return out


def nats_bound(ref):
    """how far a double sum of the fp32 losses in any fixed order can be from their exact sum: symbols * 2^-53 * sum|loss|, per image"""
    return ref["symbols"].astype(np.float64) * 2.0 ** -53 * ref["abs"]


# ---------------------------------------------------------------------------------------------------- the whole head in float64
def head_f64_torch(logit, sigma, mean, label, mask, grad, G, ng):
    """float64 torch tensors (requires_grad where a gradient is wanted) -> (nats [N], loss [N,G,H,W], p [N,G,H,W]); the head as mathematics:
    softmax over a symbol's ng logits, relu(sigma) + 1e-5, -log(sum w (Phi_b - Phi_a) + 1e-7), the coded symbols summed per image"""
    import torch
    N, _, H, W = logit.shape
    r = lambda t: t.reshape(N, G, ng, H, W)
    w = torch.softmax(r(logit), dim=2)
    s = torch.relu(r(sigma)) + 1e-5
    phi = lambda z: 0.5 + 0.5 * torch.erf(z / math.sqrt(2.0))
    lab = label.reshape(N, G, 1, H, W)
    p = (w * (phi((lab + 0.5 - r(mean)) / s) - phi((lab - 0.5 - r(mean)) / s))).sum(2)
    loss = -torch.log(p + 1e-7)
    coded = torch.ones_like(loss, dtype=torch.bool) if mask is None else mask >= 0.5
    loss = torch.where(coded, loss, torch.zeros_like(loss))
    return loss.reshape(N, -1).sum(1), loss, p


@functools.lru_cache(maxsize=None)
def head_f64(case):
    """-> dict(nats [N], map, p [N,G,H,W], d_logit, d_sigma, d_mean, d_label, kept [N,G,H,W] bool: coded symbols with p >= GMM_MIN_P) in float64:
    autograd of sum_n grad[n] nats[n]"""
    import torch
    d = inputs(case)
    t = {k: torch.tensor(d[k].astype(np.float64), requires_grad=True) for k in ("logit", "sigma", "mean", "label")}
    mask = None if d["mask"] is None else torch.tensor(d["mask"].astype(np.float64))
    nats, loss, p = head_f64_torch(t["logit"], t["sigma"], t["mean"], t["label"], mask, None, case.G, case.ng)
    (nats * torch.tensor(d["grad"].astype(np.float64))).sum().backward()
    out = dict(nats=nats.detach().numpy(), map=loss.detach().numpy(), p=p.detach().numpy(), d_logit=t["logit"].grad.numpy(), d_sigma=t["sigma"].grad.numpy(),
               d_mean=t["mean"].grad.numpy(), d_label=t["label"].grad.numpy())
    out["kept"] = coded_of(d["mask"], case) & (out["p"] >= GMM_MIN_P)
    return out


def kept_channels(kept, case):
    """the kept symbols' mask over the [N, G*ng, H, W] tensors"""
    return np.repeat(kept, case.ng, 1)


def f64_distance(case, got):
    """(max |got - float64| over the four gradients and the map on the kept rows, max over the images of |nats - float64 nats|, kept share of the
    coded symbols, the largest gradient magnitude).  got: dict with d_logit, d_sigma, d_mean, d_label and optionally map, nats"""
    f = head_f64(case)
    kept, kc = f["kept"], kept_channels(f["kept"], case)
    worst = 0.0
    for k, sel in (("d_logit", kc), ("d_sigma", kc), ("d_mean", kc), ("d_label", kept), ("map", kept)):
        if k in got and got[k] is not None and sel.any():
            worst = max(worst, float(np.abs(got[k].astype(np.float64) - f[k])[sel].max()))
    scale = max(float(np.abs(f[k][sel]).max()) if sel.any() else 0.0 for k, sel in (("d_logit", kc), ("d_sigma", kc), ("d_mean", kc), ("d_label", kept)))
    ncoded = int(coded_of(inputs(case)["mask"], case).sum())
    share = float(kept.sum()) / ncoded if ncoded else 1.0
    dn = float(np.abs(np.asarray(got["nats"], np.float64) - f["nats"]).max()) if "nats" in got else 0.0
    return worst, dn, share, scale
