"""The pointwise, table and projection ops on every dispatch path: cases, the launchers' dispatch predicates restated, references and
models of broken kernels (numpy, torch on the CPU and the CPU oracle only; no GPU).

csrc/pointwise_kernels.hip, csrc/tile_table_kernels.hip and csrc/project_kernels.hip choose among two or three kernels per op by
alignment, alphabet size, plane count and stride.  `which_kernel(op, case)` restates each launcher's choice and names the in-kernel
edges a case reaches; tests/test_ops_edge_cases_cpu.py requires every name of REACH to be reached, the restated constants to be the
source's, the oracle to agree with the float64 / numpy statements below and every model of BROKEN to change a reference;
tests/test_gpu_ops_edges.py runs the cases through the drop-in ops.

References.  The CPU oracle stays the bit-exact standard for quant forward, dquant, dtow, the sphere ops, both tables, update_weight
and the quantiser's data gradient.  Beside it, statements that do not call it: `count` as an integer histogram of the indices, dtow as
reshape / transpose, the sphere pad as roll / flip and its backward as the float64 adjoint (a scatter-add over the forward's index
map), the quantiser's weight gradient as a float64 sum of the same selected terms, the GMM loss and its four gradients by float64
autograd of -log(sum w (Phi_b - Phi_a) + 1e-7), the viewport view by float64 bilinear sampling with the wrap and the clamp written
out, at the coordinates rebuilt from the returned angles.

MEASURED tolerances (GMM_F64_TOL, VIEWPORT_F64_TOL below): the oracle against the float64 statement on the CPU, maximum over the
case; the CPU test re-measures each and requires the recorded figure to hold and to be within a factor 2 of the measurement; the
kernel is allowed twice the recorded figure (kernel and oracle differ only in the last bits of the operands of lic360_expf and, for
the viewport, in the device's libm).
"""
import collections
import functools
import math

import numpy as np

import oracle as orc

# ---------------------------------------------------------------------------------------------------- restated constants
SLAB4_MAX_LEVELS = 8          # k_quant_slab4, k_quant_weight_diff8: levels <= 8
SLAB_MAX_LEVELS = 64          # k_quant_slab: levels <= 64
MAX_GRID_Y = 65535            # planes / groups on blockIdx.y
BIG30 = 1 << 30
BIG28 = 1 << 28
FLUSH_AFTER = 250             # k_quant_slab4: flush() once `since > 250`
BETA_MIN = 0.001              # k_quant_data_diff: beta clamp
BETA_INF = 10000.0            # k_quant_data_diff: the two sentinels
WG = 256

F = np.float32


def _rng(*key):
    import zlib
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ==================================================================================================== quantiser, forward
QuantCase = collections.namedtuple("QuantCase", "id shape levels offset")
QUANT_CASES = (
    QuantCase("slab4_256x256_L8", (1, 2, 256, 256), 8, 0),      # 64 iterations: one after the in-loop flush
    QuantCase("slab4_256x256_L5", (1, 2, 256, 256), 5, 0),
    QuantCase("slab4_252x260_L8", (1, 2, 252, 260), 8, 0),      # 16380 quads: 63 full iterations + a ragged one
    QuantCase("slab4_252x260_L5", (1, 2, 252, 260), 5, 0),
    QuantCase("slab_unaligned_256x256_L8", (1, 2, 256, 256), 8, 1),
    QuantCase("slab_unaligned_252x260_L5", (1, 2, 252, 260), 5, 1),
    QuantCase("slab_7x9_L8", (2, 3, 7, 9), 8, 0),               # inner % 4 != 0
    QuantCase("generic_L65_5x13", (2, 3, 5, 13), 65, 0),
    QuantCase("generic_L65_1x70", (1, 1, 1, 70), 65, 0),        # second wave: 6 live lanes
)


def quant_inputs(case):
    """-> x [N,C,H,W], weight_b [C, levels].  Channel 0 falls entirely into ONE level (level 2; 0 when there are fewer): with 16-byte
    lanes every thread of k_quant_slab4 adds 4 per iteration to a single 8-bit field, which reaches 252 right before the flush."""
    rng = _rng("quant", case.id)
    N, C, H, W = case.shape
    L = case.levels
    wb = np.concatenate([rng.uniform(-1, 0, (C, 1)), rng.uniform(-2, 0.3, (C, L - 1)) if L <= 12 else rng.uniform(-3, -2, (C, L - 1))], 1).astype(F)
    span = float(np.exp(wb[:, 1:]).sum(1).max()) + 2.0
    x = rng.uniform(-2.0, span, case.shape).astype(F)
    if H * W >= 63 * 4 * WG:
        wq = quant_weights(wb)
        j = min(2, L - 1)
        x[:, 0] = wq[0, 0] + wq[0, 1:j + 1].sum()               # the centre of level j (up to rounding: well inside its cell)
    return x, wb


def quant_weights(wb):
    """k_quant_weight: the first centre and the level increments exp(w) (lic360_expf through the oracle's elementwise view)"""
    wq = orc.expf(wb).reshape(wb.shape)
    wq[:, 0] = wb[:, 0]
    return wq


def count_histogram(qidx, levels):
    """count[c][j] = -(number of elements of channel c with index j): integers, no floating-point sum"""
    N, C = qidx.shape[:2]
    q = qidx.astype(np.int64).transpose(1, 0, 2, 3).reshape(C, -1)
    return -np.stack([np.bincount(q[c], minlength=levels) for c in range(C)]).astype(F)


def slab4_count_model(qidx, levels, flush_after=FLUSH_AFTER, in_loop_flush=True):
    """k_quant_slab4's counting restated: per thread eight 8-bit fields in one 64-bit word (a field that passes 255 carries into the next
    one, the top one out of the word), flushed into the histogram once `since > flush_after` and after the loop"""
    N, C, H, W = qidx.shape
    inner4 = H * W // 4
    iters = -(-inner4 // WG)
    count = np.zeros((C, levels), np.int64)
    fields = lambda pk: np.stack([(pk >> np.uint64(8 * b)) & np.uint64(0xff) for b in range(8)], 1).astype(np.int64)
    for n in range(N):
        for c in range(C):
            q = np.full((iters * WG, 4), -1, np.int64)
            q[:inner4] = qidx[n, c].reshape(inner4, 4).astype(np.int64)
            q = q.reshape(iters, WG, 4)
            pk, since, hist = np.zeros(WG, np.uint64), 0, np.zeros(8, np.int64)
            for it in range(iters):
                for k in range(4):
                    live = q[it, :, k] >= 0
                    pk = pk + np.where(live, np.uint64(1) << (np.uint64(8) * q[it, :, k].clip(0).astype(np.uint64)), np.uint64(0))
                since += 4
                if in_loop_flush and since > flush_after:
                    hist += fields(pk).sum(0)
                    pk, since = np.zeros(WG, np.uint64), 0
            hist += fields(pk).sum(0)
            count[c] += hist[:levels]
    return -count.astype(F)


# ==================================================================================================== dquant
DquantCase = collections.namedtuple("DquantCase", "id shape levels offset")
DQUANT_CASES = (
    DquantCase("inner35", (2, 3, 5, 7), 8, 0),
    DquantCase("unaligned", (1, 2, 4, 8), 8, 1),
    DquantCase("planes65536", (1, 65536, 2, 2), 3, 0),
    DquantCase("plane4", (2, 3, 4, 8), 8, 0),                   # the fast path, for contrast
)


def dquant_inputs(case):
    rng = _rng("dquant", case.id)
    N, C, H, W = case.shape
    wb = np.concatenate([rng.uniform(-1, 0, (C, 1)), rng.uniform(-2, 0.3, (C, case.levels - 1))], 1).astype(F)
    q = rng.integers(0, case.levels, case.shape).astype(F)
    mask = (rng.random(case.shape) > 0.3).astype(F)
    return q, mask, wb


# ==================================================================================================== quantiser, backward
QuantBwdCase = collections.namedtuple("QuantBwdCase", "id levels ntop shape")
QUANT_BWD_CASES = tuple(QuantBwdCase("L%d_ntop%d" % (L, nt), L, nt, (3, 3, 15, 20)) for L in (3, 5, 8, 9, 12) for nt in (1, 2))
QUANT_ALPHA = F(0.1)


@functools.lru_cache(maxsize=None)
def quant_bwd_inputs(case):
    """-> dict(x, wb, top, qidx, g0, g1): x holds exact centres of the first, a middle and the last level, values below the first
    centre and beyond the last one; weight column 2 has exp(w) < 0.001 (the beta clamp).  top / qidx are the oracle's forward."""
    rng = _rng("quant_bwd", case.levels)                       # ntop 1 and 2 share the draw
    N, C, H, W = case.shape
    L = case.levels
    wb = np.concatenate([rng.uniform(-1, 0, (C, 1)), rng.uniform(-2, -0.5, (C, L - 1))], 1).astype(F)
    wb[:, 2] = -8.0                                             # exp(-8) = 3.4e-4
    span = float(np.exp(wb[:, 1:]).sum(1).max()) + 1.5
    x = rng.uniform(-2.5, span, case.shape).astype(F)
    # channel 0: dyadic increments (0.25, 2^-12, 0.5, ...) from -0.5, so that every centre and every step of the quantiser's subtraction
    # chain is exact and x = centre gives top == bottom bit for bit; 30 elements each on the first, a middle and the last centre
    wb[0, 0] = -0.5
    wb[0, 1:] = [_log_of_dyadic(DYADIC[(k - 1) % len(DYADIC)]) if k != 2 else _log_of_dyadic(2.0 ** -12) for k in range(1, L)]
    wq = quant_weights(wb)
    centres = np.cumsum(wq[0].astype(np.float64)).astype(F)
    flat = x[:, 0].reshape(-1)
    slots = rng.permutation(flat.size)
    for k, level in enumerate((0, L // 2 if L > 3 else 1, L - 1)):
        flat[slots[k * 30:(k + 1) * 30]] = centres[level]
    x[:, 0] = flat.reshape(N, H, W)
    for c in range(C):                                          # 30 elements per channel inside the tiny cell between centres 1 and 2:
        flat = x[:, c].reshape(-1)                              # index 1 from below, beta = exp(w2) < 0.001
        flat[rng.permutation(flat.size)[:30] if c else slots[90:120]] = F(wq[c, 0] + wq[c, 1]) + F(0.3) * wq[c, 2]
        x[:, c] = flat.reshape(N, H, W)
    top, qidx, _ = orc.quant(x, wb)
    g0, g1 = rng.standard_normal(case.shape).astype(F), rng.standard_normal(case.shape).astype(F)
    out = dict(x=x, wb=wb, top=top, qidx=qidx, g0=g0, g1=g1)
    for v in out.values():
        v.setflags(write=False)
    return out


DYADIC = (0.25, 0.5, 0.125, 0.375, 0.75)


def _log_of_dyadic(d):
    """the float32 w with lic360_expf(w) == d exactly (searched within 16 ulps of log d)"""
    cands = [F(math.log(d))]
    for _ in range(16):
        cands = [np.nextafter(cands[0], F(-np.inf))] + cands + [np.nextafter(cands[-1], F(np.inf))]
    cands = np.array(cands, F)
    ok = np.flatnonzero(orc.expf(cands) == F(d))
    assert len(ok), d
    return cands[ok[0]]


def quant_bwd_branches(case):
    """how many elements take each branch of the beta rule (from the oracle's forward)"""
    d = quant_bwd_inputs(case)
    L = case.levels
    q, lt, gt, eq = d["qidx"].astype(int), d["top"] < d["x"], d["top"] > d["x"], d["top"] == d["x"]
    wq = quant_weights(d["wb"])
    beta = data_diff_beta(d["x"], d["top"], d["qidx"], wq, L, clamp=False)
    return {"eq_first": int((eq & (q == 0)).sum()), "eq_middle": int((eq & (q > 0) & (q < L - 1)).sum()),
            "eq_last": int((eq & (q == L - 1)).sum()), "sentinel_above": int((lt & (q == L - 1)).sum()),
            "sentinel_below": int((gt & (q == 0)).sum()), "beta_clamp": int((beta < F(BETA_MIN)).sum())}


def data_diff_beta(x, top, qidx, wq, levels, clamp=True, swapped=False):
    """the beta of k_quant_data_diff per element (float32); swapped: the `top < bottom` and `top > bottom` rules exchanged"""
    N, C, H, W = x.shape
    q = qidx.astype(int)
    w = np.broadcast_to(wq[None, :, None, None, :], (N, C, H, W, levels))
    at = lambda k: np.take_along_axis(w, np.clip(k, 0, levels - 1)[..., None], -1)[..., 0]
    up = np.where(q < levels - 1, at(q + 1), F(BETA_INF))
    down = np.where(q > 0, at(q), F(BETA_INF))
    mid = ((at(q).astype(np.float64) + at(q + 1).astype(np.float64)) / 2.0).astype(F)
    same = np.where(q == 0, at(q + 1), np.where(q < levels - 1, mid, at(q)))
    lt, gt = (top < x, top > x) if not swapped else (top > x, top < x)
    beta = np.where(lt, up, np.where(gt, down, same)).astype(F)
    return np.maximum(beta, F(BETA_MIN)) if clamp else beta


def data_diff_model(case, swapped=False):
    d = quant_bwd_inputs(case)
    if case.ntop == 1:
        return d["g0"].copy()
    beta = data_diff_beta(d["x"], d["top"], d["qidx"], quant_weights(d["wb"]), case.levels, swapped=swapped)
    return (d["g0"] + (QUANT_ALPHA * d["g1"]).astype(F) / beta).astype(F)


def weight_diff_f64(case, first_level_offset=0):
    """-> (weight_diff float64 [C, L], bound [C, L]): sum over the channel's elements with index >= j (+ offset: the broken suffix sum)
    of the float32 differences top - bottom, in float64, times the level increment for j > 0.  bound: the fp32 summation error of the
    kernels' fixed order -- a chain of N * ceil(inner / 256) additions per thread, then 8 tree steps -- (chain + 8) 2^-24 sum|d| wq"""
    d = quant_bwd_inputs(case)
    N, C, H, W = case.shape
    L = case.levels
    wq = quant_weights(d["wb"]).astype(np.float64)
    wq[:, 0] = 1.0
    diff = (d["top"] - d["x"]).astype(np.float64).transpose(1, 0, 2, 3).reshape(C, -1)
    q = d["qidx"].astype(int).transpose(1, 0, 2, 3).reshape(C, -1)
    out, bound = np.zeros((C, L)), np.zeros((C, L))
    chain = N * -(-(H * W) // WG)
    for j in range(L):
        sel = q >= j + first_level_offset
        out[:, j] = (diff * sel).sum(1) * wq[:, j]
        bound[:, j] = (chain + 8) * 2.0 ** -24 * (np.abs(diff) * sel).sum(1) * wq[:, j]
    return out, bound


# ==================================================================================================== update_weight
UpdateCase = collections.namedtuple("UpdateCase", "id levels channels pattern")
UPDATE_PATTERNS = ("all_empty", "level0_empty", "tail_empty", "none_empty")
UPDATE_CASES = tuple(UpdateCase("L%d_C1_%s" % (L, p), L, 1, p) for L in (3, 8) for p in UPDATE_PATTERNS) + \
    tuple(UpdateCase("L%d_C300_mixed" % L, L, 300, "mixed") for L in (3, 8))


def update_inputs(case):
    """-> weight [C, L], ncount [C, L]; 'mixed': channel c takes pattern c % 4"""
    rng = _rng("update", case.id)
    C, L = case.channels, case.levels
    w = rng.uniform(-2, 0.3, (C, L)).astype(F)
    cnt = rng.uniform(0.5, 40.0, (C, L)).astype(F)
    for c in range(C):
        p = case.pattern if case.pattern != "mixed" else UPDATE_PATTERNS[c % 4]
        if p == "all_empty":
            cnt[c] = 0.0
        elif p == "level0_empty":
            cnt[c, 0] = 0.0005
        elif p == "tail_empty":
            cnt[c, max(2, L // 2):] = 0.0
    return w, cnt


# ==================================================================================================== dtow / wtod
DtowCase = collections.namedtuple("DtowCase", "id shape stride d2w offset")
DTOW_CASES = (
    DtowCase("s3_d2w", (1, 18, 3, 5), 3, True, 0), DtowCase("s3_wtod", (1, 2, 9, 15), 3, False, 0),
    DtowCase("s4_d2w", (2, 16, 2, 3), 4, True, 0), DtowCase("s4_wtod", (2, 1, 8, 12), 4, False, 0),
    DtowCase("s2_d2w_w6", (1, 8, 3, 6), 2, True, 0),                  # Ws % 4 != 0, both directions
    DtowCase("s2_wtod_w12", (1, 2, 4, 12), 2, False, 0),              # w % 4 == 0 but (w / 2) % 4 != 0: the fallback of wtod alone
    DtowCase("s2_d2w_unaligned", (1, 8, 4, 8), 2, True, 1), DtowCase("s2_wtod_unaligned", (1, 2, 8, 16), 2, False, 1),
    DtowCase("s2_d2w_groups65540", (1, 262160, 1, 4), 2, True, 0), DtowCase("s2_wtod_groups65540", (1, 65540, 2, 8), 2, False, 0),
    DtowCase("s2_d2w_fast", (1, 8, 4, 8), 2, True, 0), DtowCase("s2_wtod_fast", (1, 2, 8, 16), 2, False, 0),   # k_dtow2, for contrast
)


def dtow_inputs(case):
    return _rng("dtow", case.id).standard_normal(case.shape).astype(F)


def dtow_ref(x, stride, d2w):
    """pixel shuffle as reshape / transpose: out(co, h s + i, w s + j) = in(co s^2 + i s + j, h, w), and its inverse"""
    N, C, H, W = x.shape
    s = stride
    if d2w:
        return x.reshape(N, C // (s * s), s, s, H, W).transpose(0, 1, 4, 2, 5, 3).reshape(N, C // (s * s), H * s, W * s)
    return x.reshape(N, C, H // s, s, W // s, s).transpose(0, 1, 3, 5, 2, 4).reshape(N, C * s * s, H // s, W // s)


# ==================================================================================================== sphere ops
SphereCase = collections.namedtuple("SphereCase", "id shape pad")       # shape: the UNPADDED tensor
SPHERE_FWD_CASES = (
    SphereCase("pad_eq_h", (2, 2, 3, 7), 3), SphereCase("pad_eq_w", (1, 3, 7, 3), 3), SphereCase("pad_eq_h_eq_w", (1, 2, 3, 3), 3),
    SphereCase("pad_eq_h_2", (1, 2, 2, 5), 2),
)
TrimCase = collections.namedtuple("TrimCase", "id shape pad")           # shape: the tensor that is trimmed
SPHERE_TRIM_CASES = (TrimCase("h_eq_2pad", (2, 3, 4, 9), 2), TrimCase("w_eq_2pad", (1, 2, 7, 6), 3), TrimCase("vec_rows", (1, 2, 6, 8), 1),
                     TrimCase("scalar_rows", (1, 2, 6, 7), 1))
SPHERE_BWD_CASES = (                                                     # the last legal sizes of the backward
    SphereCase("2pad_eq_h", (1, 2, 4, 9), 2), SphereCase("2pad_eq_w", (2, 1, 7, 6), 3), SphereCase("2pad_eq_h_eq_w", (1, 1, 4, 4), 2),
)
SPHERE_BWD_REFUSED = (                                                   # one step beyond: the entry points refuse
    SphereCase("h3_pad2", (1, 1, 3, 8), 2), SphereCase("h4_pad3", (1, 1, 4, 8), 3), SphereCase("w3_pad2", (1, 1, 6, 3), 2),
)


def sphere_inputs(case):
    rng = _rng("sphere", case.id)
    N, C, H, W = case.shape
    p = case.pad
    return rng.standard_normal(case.shape).astype(F), rng.standard_normal((N, C, H + 2 * p, W + 2 * p)).astype(F)


def sphere_pad_ref(x, pad):
    """the roll / flip formulation of the ERP border (no oracle): wrap in longitude, pole rows mirrored and seen from across the pole"""
    mid = np.concatenate([x[..., x.shape[-1] - pad:], x, x[..., :pad]], -1)
    top = mid[:, :, :pad][:, :, ::-1, ::-1]
    bot = mid[:, :, mid.shape[2] - pad:][:, :, ::-1, ::-1]
    return np.concatenate([top, mid, bot], 2)


def sphere_pad_adjoint_f64(g, shape, pad):
    """-> (F^T g in float64, sum of |terms| per cell): scatter-add of the padded gradient over the forward's own index map"""
    N, C, H, W = shape
    src = sphere_pad_ref(np.arange(H * W, dtype=np.int64).reshape(1, 1, H, W), pad).reshape(-1)
    out, mag = np.zeros((N * C, H * W)), np.zeros((N * C, H * W))
    gg = g.astype(np.float64).reshape(N * C, -1)
    for p in range(N * C):
        np.add.at(out[p], src, gg[p])
        np.add.at(mag[p], src, np.abs(gg[p]))
    return out.reshape(shape), mag.reshape(shape)


# ==================================================================================================== tables
TABLE_COUNTS = (1, 63, 65, 300)
GmmTableCase = collections.namedtuple("GmmTableCase", "id ng nstep count")
GMM_TABLE_CASES = tuple(GmmTableCase("ng%d_nstep%d_n%d" % (g, s, n), g, s, n) for g, s in ((1, 8), (3, 4), (5, 16), (16, 2), (3, 8))
                        for n in TABLE_COUNTS)
EntropyTableCase = collections.namedtuple("EntropyTableCase", "id nstep count")
ENTROPY_TABLE_CASES = tuple(EntropyTableCase("nstep%d_n%d" % (s, n), s, n) for s in (1, 2, 10, 48, 64, 49) for n in TABLE_COUNTS)
TABLE_TOTAL = 65536


def gmm_table_inputs(case):
    """-> logits, sigma, mu [count, ng] and the bias; row 0 is degenerate (tiny / negative sigmas: zero-width bins, the fix-up acts)"""
    rng = _rng("gmm_table", case.id)
    n, g = case.count, case.ng
    w = (rng.standard_normal((n, g)) * 2).astype(F)
    s = rng.uniform(-0.3, 2.5, (n, g)).astype(F)
    bias = (case.nstep - 1) / 2.0
    m = rng.uniform(-bias - 1.5, bias + 1.5, (n, g)).astype(F)
    s[0] = ([1e-6, -1.0, 0.0, 3e-4] * g)[:g]
    m[0] = -bias + 0.25                                                  # all the mass in the first bin
    return w, s, m, bias


def entropy_table_inputs(case):
    """-> logits [count, nstep]; row 0 is one-hot (many zero-width bins: the fix-up acts wherever nstep > 1)"""
    rng = _rng("entropy_table", case.id)
    lg = (rng.standard_normal((case.count, case.nstep)) * 3).astype(F)
    lg[0] = -40.0
    lg[0, min(5, case.nstep - 1)] = 10.0
    return lg


def table_row_without_fixup(kind, case):
    """row 0 of the case by tests/independent_tables.py with its fix-up taken out (the model of a generic path that skips it)"""
    import independent_tables as it
    keep = it.fixup
    it.fixup = lambda T, n, b: T
    try:
        exp, erf = (lambda v: orc.expf(v)[0]), (lambda v: orc.erff(v)[0])
        if kind == "gmm":
            w, s, m, bias = gmm_table_inputs(case)
            return np.array(it.gmm_table_row(w[0], s[0], m[0], exp, erf, case.nstep, bias, float(TABLE_TOTAL), 1e-6)[2], F)
        return np.array(it.entropy_table_row(entropy_table_inputs(case)[0], exp, float(TABLE_TOTAL)), F)
    finally:
        it.fixup = keep


# ==================================================================================================== GMM loss
GmmLossCase = collections.namedtuple("GmmLossCase", "id ng M degenerate")
GMM_LOSS_CASES = tuple(GmmLossCase("ng%d_M%d" % (g, M), g, M, False) for g in (1, 3, 5) for M in (1, 255, 257, 4000)) + \
    tuple(GmmLossCase("ng%d_degenerate" % g, g, 257, True) for g in (1, 3, 5))
GMM_MIN_P = 0.02             # rows the float64 comparison keeps: 1e-5 on the log needs p >~ 0.01 (fp32 Phi_b - Phi_a carries ~6e-8)
GMM_MIN_KEPT = 0.85
# MEASURED: max |oracle - float64 autograd| over the four gradients, rows with p > GMM_MIN_P (test_ops_edge_cases_cpu.py::
# test_gmm_loss_oracle_vs_float64 re-measures and prints them); the gradients reach ~15 at sigma = 0.3.  Filled in from that run.
GMM_F64_TOL = {                                                          # measured (3 digits) -> recorded (rounded up)
    "ng1_M1": 2.4e-8,       # 2.31e-08 at gradient scale 1.03, 100 % of rows kept
    "ng1_M255": 1.2e-6,     # 1.18e-06 at 4.93, 100 %
    "ng1_M257": 1.4e-5,     # 1.37e-05 at 16.8, 100 %
    "ng1_M4000": 2.8e-5,    # 2.70e-05 at 16.4, 99.6 %
    "ng3_M1": 6.1e-8,       # 6.05e-08 at 1.10, 100 %
    "ng3_M255": 5.4e-7,     # 5.38e-07 at 3.15, 100 %
    "ng3_M257": 1.1e-6,     # 1.01e-06 at 3.77, 100 %
    "ng3_M4000": 2.0e-6,    # 1.96e-06 at 6.57, 100 %
    "ng5_M1": 1.7e-7,       # 1.61e-07 at 2.03, 100 %
    "ng5_M255": 9.4e-7,     # 9.38e-07 at 4.52, 100 %
    "ng5_M257": 6.8e-7,     # 6.75e-07 at 3.92, 100 %
    "ng5_M4000": 1.3e-6,    # 1.28e-06 at 4.91, 100 %
}
GMM_UNDERFLOW_LOSS = F(-math.log(1e-7))                                  # the loss of a row whose p underflows, to fp32


@functools.lru_cache(maxsize=None)
def gmm_loss_inputs(case):
    """-> dict(w, d, m, lab [M,1], top [M]).  Labels are the re-centred symbols k - 3.5 of the 8-symbol alphabet; the first rows sit at
    both ends of it.  degenerate: sigma = 0.01 with the mean 3 away from the label, so p underflows to 0."""
    rng = _rng("gmm_loss", case.id)
    M, g = case.M, case.ng
    w = rng.random((M, g)).astype(F) + F(0.05)
    w /= w.sum(1, keepdims=True)
    lab = (rng.integers(0, 8, (M, 1)) - 3.5).astype(F)
    lab[0] = -3.5
    if M > 1:
        lab[1] = 3.5
    if case.degenerate:
        d = np.full((M, g), 0.01, F)
        m = (lab + np.where(lab > 0, -3.0, 3.0) + rng.uniform(-0.2, 0.2, (M, g))).astype(F)
    else:
        d = rng.uniform(0.3, 2.0, (M, g)).astype(F)
        m = (lab + rng.normal(0, 0.6, (M, g))).astype(F)
    top = rng.uniform(0.5, 1.5, M).astype(F)
    out = dict(w=w, d=d, m=m, lab=lab, top=top)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gmm_loss_f64(case):
    """-> (loss, wd, dd, md, ld, p) in float64: autograd of top * -log(sum w (Phi_b - Phi_a) + 1e-7)"""
    import torch
    d = gmm_loss_inputs(case)
    w, s, m, lab = (torch.tensor(d[k].astype(np.float64), requires_grad=True) for k in ("w", "d", "m", "lab"))
    phi = lambda z: 0.5 + 0.5 * torch.erf(z / math.sqrt(2.0))
    p = (w * (phi((lab + 0.5 - m) / s) - phi((lab - 0.5 - m) / s))).sum(1)
    loss = -torch.log(p + 1e-7)
    grads = torch.autograd.grad(loss, (w, s, m, lab), torch.tensor(d["top"].astype(np.float64)))
    return (loss.detach().numpy(),) + tuple(g.numpy() for g in grads) + (p.detach().numpy(),)


def gmm_oracle_with_top(case):
    """the oracle's forward, then what k_entropy_gmm_bwd does: every gradient times top, the label's once per row"""
    d = gmm_loss_inputs(case)
    loss, wd, dd, md, ld = orc.entropy_gmm(d["w"], d["d"], d["m"], d["lab"])
    t = d["top"][:, None]
    return loss, wd * t, dd * t, md * t, ld * t


# ==================================================================================================== viewport
ViewportCase = collections.namedtuple("ViewportCase", "id H W")
VIEWPORT_CASES = (ViewportCase("erp8x16", 8, 16), ViewportCase("erp32x64", 32, 64))
VIEWPORT_HO, VIEWPORT_WO, VIEWPORT_FOV, VIEWPORT_C = 10, 14, 80.0, 2
VIEWPORT_ANGLES = np.array([(3.1, 0.0), (-3.1, 0.3), (math.pi, 1.2), (0.5, 1.5), (2.0, -1.5707), (0.0, 0.0)], F)
# MEASURED: max |oracle view - float64 sampling at the coordinates rebuilt from the oracle's angles|, standard-normal images
# (test_ops_edge_cases_cpu.py::test_viewport_oracle_vs_float64).  Filled in from that run.
VIEWPORT_F64_TOL = {
    "erp8x16": 1.4e-6,      # measured 1.33e-06; 43 / 46 seam samples (tw == -1 / W - 1), 18 / 12 pole samples (th == -1 / th + 1 >= H)
    "erp32x64": 5.2e-6,     # measured 5.19e-06; 11 / 13 seam samples, no pole samples
}


def viewport_inputs(case):
    return _rng("viewport", case.id).standard_normal((len(VIEWPORT_ANGLES), VIEWPORT_C, case.H, case.W)).astype(F)


def viewport_coords(angles, H, W):
    """ERP pixel coordinates (float64) rebuilt from the returned (longitude, latitude) [n, ho, wo, 2]: the inverse of k_vp_angles"""
    a = angles.astype(np.float64)
    return (a[..., 0] / (2 * math.pi) + 0.5) * W - 0.5, (0.5 - a[..., 1] / math.pi) * H - 0.5


def viewport_edge_counts(angles, H, W):
    fx, fy = viewport_coords(angles, H, W)
    tw, th = np.floor(fx).astype(int), np.floor(fy).astype(int)
    return {"tw_m1": int((tw == -1).sum()), "tw_last": int((tw == W - 1).sum()), "th_m1": int((th == -1).sum()),
            "th_last": int((th + 1 >= H).sum())}


def viewport_sample_f64(x, angles, wrap_plus_ws=True, pole_clamp=True):
    """bilinear sampling in float64 with the longitude wrap and the pole clamp written out.  The two switches are the broken models:
    C's `tw % ws` without `+ ws` (-1 stays -1) and rows th, th + 1 unclamped -- both then index the flat tensor as the kernel would
    (wrapped into the allocation here, where the kernel would read a neighbouring plane or leave the tensor)"""
    N, C, H, W = x.shape
    fx, fy = viewport_coords(angles, H, W)
    tw, th = np.floor(fx).astype(int), np.floor(fy).astype(int)
    tx, ty = (fx - tw)[:, None], (fy - th)[:, None]
    aw = (tw + W) % W if wrap_plus_ws else np.where(tw < 0, tw, tw % W)
    bw = (tw + 1) % W
    ah, bh = (np.maximum(th, 0), np.minimum(th + 1, H - 1)) if pole_clamp else (th, th + 1)
    flat = x.astype(np.float64).reshape(-1)
    base = (np.arange(N)[:, None] * C + np.arange(C)[None, :])[:, :, None, None] * (H * W)
    at = lambda r, c: flat[(base + (r * W + c)[:, None]) % flat.size]
    return at(ah, aw) * (1 - tx) * (1 - ty) + at(ah, bw) * tx * (1 - ty) + at(bh, aw) * (1 - tx) * ty + at(bh, bw) * tx * ty


# ==================================================================================================== importance map
IMP_KERNELS_AS_RULE0 = (4, 7)
IMP_SHAPE, IMP_LEVELS = (2, 12, 5, 7), 6


def imp_inputs():
    rng = _rng("imp")
    N, C, H, W = IMP_SHAPE
    g = rng.standard_normal(IMP_SHAPE).astype(F)
    imp = (np.floor(rng.random((N, 1, H, W)) * (IMP_LEVELS + 1)) / IMP_LEVELS).astype(F)
    sc = rng.standard_normal((N, 1, H)).astype(F)
    return g, imp, sc


# ==================================================================================================== dispatch, restated
def _aligned(offset):
    return offset % 4 == 0            # views start `offset` floats into a 256-byte aligned allocation


def which_kernel(op, case):
    """-> tuple of names: the kernel the launcher picks for the case, then the in-kernel edges the case reaches"""
    if op == "quant":
        N, C, H, W = case.shape
        inner, L = H * W, case.levels
        al16 = inner % 4 == 0 and _aligned(case.offset)
        if L <= SLAB4_MAX_LEVELS and al16 and N * C < BIG30 and inner // 4 < BIG30:
            inner4 = inner // 4
            iters = -(-inner4 // WG)
            tags = ["k_quant_slab4"]
            if 4 * iters > FLUSH_AFTER:
                tags.append("slab4_flush_in_loop")
                if iters > FLUSH_AFTER // 4 + 1:
                    tags.append("slab4_elements_after_flush")
            if inner4 % WG:
                tags.append("slab4_ragged_last_iteration")
            return tuple(tags)
        if L <= SLAB_MAX_LEVELS and N * C < BIG30:
            return ("k_quant_slab", "slab_unaligned" if inner % 4 == 0 else "slab_inner_not_4")
        total = N * C * inner
        return ("k_quant",) + (("k_quant_tail_shorter_than_wave",) if 0 < total % WG % 64 else ())
    if op == "dquant":
        N, C, H, W = case.shape
        inner = H * W
        if inner % 4 == 0 and _aligned(case.offset) and N * C <= MAX_GRID_Y and inner // 4 < BIG30:
            return ("k_dquant_plane4",)
        return ("k_dquant", "dquant_inner_not_4" if inner % 4 else ("dquant_unaligned" if not _aligned(case.offset) else "dquant_planes_gt_65535"))
    if op == "quant_bwd":
        return ("k_quant_weight_diff8" if case.levels <= SLAB4_MAX_LEVELS else "k_quant_weight_diff",
                "weight_diff8_below_8" if case.levels < SLAB4_MAX_LEVELS else "weight_diff_levels_%s" % ("8" if case.levels == 8 else "gt_8"),
                "k_quant_data_diff_ntop%d" % case.ntop) + tuple("data_diff_" + k for k, v in quant_bwd_branches(case).items() if v and case.ntop == 2)
    if op == "update":
        tags = ["k_quant_update_weight", "update_levels_%d" % case.levels]
        if case.channels > WG:
            tags.append("update_second_workgroup")
        pats = UPDATE_PATTERNS if case.pattern == "mixed" else (case.pattern,)
        return tuple(tags + ["update_" + p for p in pats])
    if op == "dtow":
        N, C, H, W = case.shape
        gen = "k_dtow" if case.d2w else "k_wtod"
        if case.stride != 2:
            return (gen, "dtow_stride_%d" % case.stride)
        if not _aligned(case.offset):
            return (gen, "dtow_unaligned")
        Hs, Ws, groups = (H, W, N * (C // 4)) if case.d2w else (H // 2, W // 2, N * C)
        if Ws % 4:
            return (gen, "dtow_ws_not_4" + ("_wtod_alone" if not case.d2w and W % 4 == 0 else ""))
        if groups > MAX_GRID_Y:
            return (gen, "dtow_groups_gt_65535")
        assert Hs * Ws < BIG28
        return ("k_dtow2<%s>" % ("true" if case.d2w else "false"),)
    if op == "sphere_fwd":
        N, C, H, W = case.shape
        assert N * C <= MAX_GRID_Y and (H + 2 * case.pad) * (W + 2 * case.pad) < BIG30
        return ("k_sphere_pad_plane", "k_sphere_pad_inplace_plane", "k_sphere_cut_edge_plane", "k_sphere_trim_plane") + \
            (("sphere_pad_eq_h",) if case.pad == H else ()) + (("sphere_pad_eq_w",) if case.pad == W else ())
    if op == "sphere_trim":
        N, C, H, W = case.shape
        if H == 2 * case.pad or W == 2 * case.pad:
            return ("sphere_trim_memset",)
        return ("k_sphere_trim_plane", "trim_vec" if W % 4 == 0 else "trim_scalar")
    if op == "sphere_bwd":
        N, C, H, W = case.shape
        if 2 * case.pad > H or 2 * case.pad > W:
            return ("sphere_pad_backward_refused",)
        return ("k_sphere_pad_backward",) + (("sphere_bwd_2pad_eq_h",) if 2 * case.pad == H else ()) + (("sphere_bwd_2pad_eq_w",) if 2 * case.pad == W else ())
    if op == "gmm_table":
        return ("k_gmm_table<16, 3, 8>",) if (case.ng, case.nstep) == (3, 8) else ("k_gmm_table<16, 0, 0>",)
    if op == "entropy_table":
        return ("k_entropy_table_static<49>",) if case.nstep == 49 else ("k_entropy_table",) + (("entropy_table_second_workgroup",) if case.count > 64 else ())
    if op == "gmm_loss":
        return ("k_entropy_gmm", "k_entropy_gmm_bwd", "gmm_ng_%d" % case.ng) + (("gmm_second_workgroup",) if case.M > WG else ()) + \
            (("gmm_p_underflow",) if case.degenerate else ())
    if op == "viewport":
        ang = orc.viewport_forward(viewport_inputs(case), VIEWPORT_ANGLES, VIEWPORT_HO, VIEWPORT_WO, F(VIEWPORT_FOV))[4]
        return ("k_vp_sample",) + tuple("vp_" + k for k, v in viewport_edge_counts(ang, case.H, case.W).items() if v)
    raise KeyError(op)


FAMILIES = (("quant", QUANT_CASES), ("dquant", DQUANT_CASES), ("quant_bwd", QUANT_BWD_CASES), ("update", UPDATE_CASES),
            ("dtow", DTOW_CASES), ("sphere_fwd", SPHERE_FWD_CASES), ("sphere_trim", SPHERE_TRIM_CASES),
            ("sphere_bwd", SPHERE_BWD_CASES + SPHERE_BWD_REFUSED), ("gmm_table", GMM_TABLE_CASES),
            ("entropy_table", ENTROPY_TABLE_CASES), ("gmm_loss", GMM_LOSS_CASES), ("viewport", VIEWPORT_CASES))

# every kernel and in-kernel branch that some case must reach
REACH = (
    "k_quant", "k_quant_tail_shorter_than_wave", "k_quant_slab", "slab_unaligned", "slab_inner_not_4", "k_quant_slab4",
    "slab4_flush_in_loop", "slab4_elements_after_flush", "slab4_ragged_last_iteration",
    "k_dquant", "dquant_inner_not_4", "dquant_unaligned", "dquant_planes_gt_65535", "k_dquant_plane4",
    "k_quant_weight_diff", "k_quant_weight_diff8", "weight_diff8_below_8", "weight_diff_levels_8", "weight_diff_levels_gt_8",
    "k_quant_data_diff_ntop1", "k_quant_data_diff_ntop2", "data_diff_eq_first", "data_diff_eq_middle", "data_diff_eq_last",
    "data_diff_sentinel_above", "data_diff_sentinel_below", "data_diff_beta_clamp",
    "k_quant_update_weight", "update_levels_3", "update_levels_8", "update_second_workgroup", "update_all_empty", "update_level0_empty",
    "update_tail_empty", "update_none_empty",
    "k_dtow", "k_wtod", "dtow_stride_3", "dtow_stride_4", "dtow_ws_not_4", "dtow_ws_not_4_wtod_alone", "dtow_unaligned",
    "dtow_groups_gt_65535", "k_dtow2<true>", "k_dtow2<false>",
    "sphere_pad_eq_h", "sphere_pad_eq_w", "sphere_trim_memset", "trim_vec", "trim_scalar", "sphere_bwd_2pad_eq_h", "sphere_bwd_2pad_eq_w",
    "sphere_pad_backward_refused",
    "k_gmm_table<16, 0, 0>", "k_gmm_table<16, 3, 8>", "k_entropy_table", "entropy_table_second_workgroup", "k_entropy_table_static<49>",
    "k_entropy_gmm", "k_entropy_gmm_bwd", "gmm_ng_1", "gmm_ng_3", "gmm_ng_5", "gmm_second_workgroup", "gmm_p_underflow",
    "k_vp_sample", "vp_tw_m1", "vp_tw_last", "vp_th_m1", "vp_th_last",
)

BROKEN = ("flush_dropped", "flush_at_256", "wrap_without_ws", "pole_clamp_missing", "beta_branches_swapped", "suffix_sum_one_level_late",
          "stride_taken_as_2", "fixup_skipped_generic", "ld_scaled_per_component")
