"""Cases of the first decode layer's three-nets-per-task launch (k_cconv4v6<1, false, false, 3> / k_cconv4v6t<1, 3>, csrc/cconv4v6_dc.inc), with the
launch arithmetic the native code will pick, restated.  No GPU and no oracle in here: tests/test_dc_first_nets_cpu.py checks this file by itself
(the case tables reach every class of merged launch it names) and against the library's host-only lic360_dc4_tape_layout;
tests/test_gpu_dc_first_nets.py compares the kernels with the oracle on these cases, bit for bit.

What the cases are for.  The first layer of the three stacked latent nets reads ONE input (sample i of every net reads image i: x_mod * 3 == n).
In throughput mode on images of at most 64 rows the launch is scheduled over its n / 3 images and every task -- (group block, image) or (group
block, wave of a tape of images) -- runs the three nets on one staged band: net k with its own weights, accumulators and epilogue, stored
k * (n / 3) samples further.  What can go wrong there and nowhere else: a net with another net's weights / bias / slopes, a net stored at another
net's samples, the per-net exchange buffers rewritten under a slow reader (tasks of ONE double step, back to back in one workgroup), the
schedule over images (uneven XCD lists, tapes of 2..6 images, windows cut at 61 rows)."""
import collections

PS = 3                     # C4_PS: groups (staggered diagonals) of a task
GRID = 256                 # D6_GRID: persistent workgroups, 32 per XCD
TAPE_BLOCKS = 16           # D6_TAPE_BLOCKS
TAPE_WAVES = 6             # D6_TAPE_WAVES
LATENCY_TASKS = 128        # dc6_schedule: at most this many three-group tasks -> one group per task (latency mode, never merged)
SENTINEL = 7.0

Schedule = collections.namedtuple("Schedule", "nets samples gs blocks tape_c tape_n nw rows h")


def nseg(h):
    return 1 if h <= 64 else 1 + (h - 62 + 59) // 60                        # D6_NSEG


def block_rows(G, h, w, psum, g0, gs=PS):
    """union of the row ranges of the block's staggered diagonals (dc6_build_tape / decode)"""
    lo, hi = 1 << 30, -1
    for q in range(gs):
        s = psum - g0 - q
        if g0 + q >= G or s < 0 or s >= h + w - 1:
            continue
        lo, hi = min(lo, s - w + 1 if s >= w else 0), max(hi, s if s < h else h - 1)
    return lo, hi


def wave_pieces(lo, hi, h, c, k, slo):
    """dc6_wave_pieces: the (up to three) pieces (k, slo, shi, a0) of one wave of a tape, and where the next wave starts"""
    out, pos = [], 0
    while len(out) < 3 and k < c:
        a0 = pos
        if slo != 0 and a0 < 2:
            a0 = 2
        a0 += (slo - a0) & 3
        top = 63 if hi == h - 1 else 61
        shi = hi
        if a0 + (hi - slo) > top:
            shi = slo + (61 - a0)
        if a0 > 61 or (shi < hi and (a0 > 57 or shi - slo + 1 < 4)):
            break
        out.append((k, slo, shi, a0))
        pos = ((a0 + (shi - slo) + 4) // 4 + 1) * 4
        slo = shi + 1
        if slo > hi:
            slo, k = lo, k + 1
    return out, k, slo


def _plain_schedule(G, n, nb, h, w, psum, x_mod, gstep_mode):
    """dc6_schedule + dc6_build_tape over n samples of nb nets; None: nothing to launch on this plane"""
    S = h + w - 1
    n_gb3 = (G + PS - 1) // PS
    gs = 1 if gstep_mode == 0 and n * n_gb3 <= LATENCY_TASKS and nseg(h) == 1 else PS
    live = [gb for gb in range((G + gs - 1) // gs) if not (psum - gb * gs - (gs - 1) >= S or psum - gb * gs < 0)]
    if not live:
        return None
    blocks = [gb * gs for gb in range(live[-1], live[0] - 1, -1)]          # launch order: heaviest (last) group block first
    npb, c = n // nb, 0
    for t in range(TAPE_WAVES, 1, -1):
        if (npb // 8) % t == 0:
            c = t
            break
    ok = nseg(h) == 1 and gs == PS and n % 8 == 0 and npb % 8 == 0 and c >= 2 and x_mod % (8 * c) == 0 and len(blocks) <= TAPE_BLOCKS
    nw, rows = [], [block_rows(G, h, w, psum, g0, gs) for g0 in blocks]
    if ok:
        for (lo, hi) in rows:
            k, slo, cnt, fits = 0, lo, 0, hi >= 0
            while fits and k < c:
                if cnt >= TAPE_WAVES:
                    fits = False
                    break
                pcs, k, slo = wave_pieces(lo, hi, h, c, k, slo)
                fits = bool(pcs)
                cnt += 1
            nw.append(c if (not fits or cnt >= c) else cnt)
        if not sum(nw) < c * len(blocks):
            ok = False
    if not ok:
        return Schedule(1, n, gs, blocks, 0, 1, [0] * len(blocks), rows, h)
    return Schedule(1, n, gs, blocks, c, n // 8 // c, nw, rows, h)


def schedule(G, n, nb, h, w, psum, x_mod, cin=1, no_nets=False):
    """dc6_schedule_nets: what launch_cconv4v6_dc launches on plane psum -- nets = 3: the merged form, scheduled over the n / 3 images"""
    s = _plain_schedule(G, n, nb, h, w, psum, x_mod, 0)
    if s is None or no_nets or cin != 1 or nb != 3 or x_mod * nb != n or s.gs != PS or nseg(h) != 1:
        return s
    return _plain_schedule(G, n // nb, 1, h, w, psum, x_mod, 3)._replace(nets=3)


def double_steps(G, g0, cin=1, hidden=0):
    """steps_of: input groups a task of group block g0 walks, in double steps of 2 TCS (cin = 1: eight) input groups"""
    return (min(g0 + (PS - 1) + 4 + hidden, G) + (8 if cin == 1 else 2) - 1) // (8 if cin == 1 else 2)


def list_tasks(s, xcd):
    """the task list of XCD xcd, in launch order: (block index j, first group) per task -- decode() of the kernel's producer wave"""
    ns_x = (s.samples - xcd + 7) >> 3
    out = []
    for j, g0 in enumerate(s.blocks):
        out += [(j, g0)] * (s.tape_n * s.nw[j] if s.tape_c else ns_x)
    return out


def workgroup_tasks(s, wg):
    """the tasks workgroup wg (blockIdx.x) takes, in its order: the boustrophedon walk over its XCD's list (nth_task)"""
    xcd, wix = wg & 7, wg >> 3
    per = (GRID - xcd + 7) >> 3
    tasks, out, k = list_tasks(s, xcd), [], 0
    while True:
        u = k * per + (per - 1 - wix if k & 1 else wix)
        if u >= len(tasks):
            return out
        out.append(tasks[u])
        k += 1


def consecutive_single_step_tasks(G, s):
    """workgroups of the launch that run two tasks of ONE double step back to back (the round-6 race geometry)"""
    n = 0
    for wg in range(GRID):
        t = workgroup_tasks(s, wg)
        n += any(double_steps(G, a[1]) == 1 and double_steps(G, b[1]) == 1 for a, b in zip(t, t[1:]))
    return n


def tape_waves(s, j):
    """the waves (tasks) of one tape of block j, each a list of pieces (k, slo, shi, a0); []: the block keeps plain tasks"""
    if not s.tape_c or s.nw[j] >= s.tape_c:
        return []
    (lo, hi), k, slo, out = s.rows[j], 0, s.rows[j][0], []
    while k < s.tape_c:
        pcs, k, slo = wave_pieces(lo, hi, s.h, s.tape_c, k, slo)
        out.append(pcs)
    return out


def launch_class(s):
    """what distinguishes one merged launch from another as far as the kernel's paths go"""
    if s is None or s.nets != 3:
        return None
    if not s.tape_c:
        return ("plain", "uneven" if s.samples % 8 else "even", "full" if any(hi - lo == 63 for lo, hi in s.rows) else "short")
    cut = any(shi < s.rows[j][1] for j in range(len(s.blocks)) for wv in tape_waves(s, j) for (k, slo, shi, a0) in wv)
    return ("taped", s.tape_c, "mixed" if any(nw == s.tape_c for nw in s.nw) else "all", "cut" if cut else "whole")


# ---- the cases: (G, H, W, B, planes, residual); planes None: every plane of the layer.  cout = 4, PReLU, first-layer constraint, three nets.
TAPE_CASES = [
    (12, 16, 24, 16, None, True),      # tapes of 2 images
    (12, 64, 20, 24, None, False),     # tapes of 3; 64-row windows cut at 61 rows
    (12, 64, 20, 48, None, False),     # tapes of 6
]
PLAIN_CASES = [
    (48, 16, 24, 5, None, True),       # 5 images: XCD lists of one and of no image (15 samples x 16 group blocks: throughput mode)
]
FULL_CASES = [
    (48, 64, 128, 8, (0, 1, 2, 63, 64, 110, 190, 237), False),     # the bench's latent shape: full-length planes keep one image per task
]
# every task is ONE double step (six input groups); 324 images: plain tasks, 40 / 41 per XCD list per group block on 32 workgroups; 320: its taped twin
# (tapes of 5: at most 32 tasks per XCD list, one per workgroup -- see test_dc_first_nets_cpu.py); 640: the taped launch whose workgroups do take two
RACE_CASES = [
    (6, 8, 8, 324, None, False),
    (6, 8, 8, 320, None, False),
    (6, 8, 8, 640, None, False),
]
MERGED_CASES = TAPE_CASES + PLAIN_CASES + FULL_CASES + RACE_CASES
# launches that keep the one-net kernels: (G, H, W, N, nb, x_mod)
OLD_FORM_CASES = [
    (12, 16, 24, 48, 3, 48),           # three nets, each with its own input
    (12, 16, 24, 48, 1, 48),           # one net
]
# FusedCodec round trips: (G, H, W, B)
CODEC_CASES = [(12, 16, 24, 16), (12, 16, 24, 24)]


def planes_of(case):
    G, h, w, B, planes, res = case
    return tuple(planes) if planes is not None else tuple(range(h + w + G - 2))


def case_id(case):
    return "g%d_%dx%d_b%d" % case[:4]
