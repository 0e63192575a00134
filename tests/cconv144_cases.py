"""Cases of the importance-map net's own kernel (k_cconv144, csrc/cconv144_kernels.hip) at batches where its workgroups persist, with the launch
geometry the native code will pick, restated.  No GPU and no oracle in here: tests/test_cconv144_cases_cpu.py checks this file by itself (the
case tables reach every class of launch it names, the constants below are the kernel's own), tests/test_gpu_cconv144_batch.py compares the
kernel with the oracle on these cases, bit for bit.

What the cases are for.  k_cconv144 caps its grid at MAX_GRID workgroups and walks `for (task = blockIdx.x; task < ntasks; task += grid)`;
the decode-order launch also picks how many output-channel tiles (`og`) a task takes, so that a plane yields at least MIN_TASKS tasks.  A
workgroup that takes a second task re-stages its x tile behind the top-of-task barrier and carries the `parity` of its double-buffered
epilogue tile from one task to the next; a task with og > 1 decodes ot_lo = (rem - seg * n_og) * og and clips ot_hi to n_ot.  None of that
runs at the batches of tests/test_gpu_ops.py (N <= 3); all of it runs in production (64 maps of 32 x 64)."""
import collections

import numpy as np

# ---- the kernel's constants, restated (tests/test_cconv144_cases_cpu.py reads them out of cconv144_kernels.hip and compares)
NT_EC = 2                  # I144_NT_EC (cconv144_kernels.hip:297): rows of a task, encode order
NT_DC = 2                  # I144_NT_DC (:298): 16-row tiles of a task's window on the anti-diagonal, decode order
MIN_TASKS = 192            # the `< 192` of the og loop (:353)
MAX_GRID = 256             # the `< 256` grid caps (:322, :356)
R0, C0 = 4, 2              # I144_R0, I144_C0 (conv_plan.h:22-23): decode-order cell (th, tw) at row th + tw + R0, column th + C0
SENTINEL = 7.0

Geometry = collections.namedtuple("Geometry", "tasks grid n_seg og n_og groups n_ot tiles_r tiles_c th_lo th_hi th0")


def n_otiles(nout):
    return (nout + 15) // 16                                               # conv144_otiles (:64)


def ec_geometry(n, h, w, nout=144):
    """lic360_cconv144_ec, cconv144_kernels.hip:319-323: a task = NT_EC rows x 16 columns of one map and all n_ot output tiles"""
    n_ot = n_otiles(nout)
    tiles_r, tiles_c = (h + NT_EC - 1) // NT_EC, (w + 15) // 16            # :319
    tasks = n * tiles_r * tiles_c                                          # :321
    grid = min(tasks, MAX_GRID)                                            # :322
    return Geometry(tasks, grid, 1, n_ot, 1, (n_ot,), n_ot, tiles_r, tiles_c, 0, 0, 0)     # :320: og = n_ot, n_og = n_seg = 1


def dc_geometry(n, h, w, nout, s):
    """lic360_cconv144_dc_plane, cconv144_kernels.hip:349-357: a task = one 16 NT_DC-row segment of anti-diagonal s of one map and `og`
    consecutive output tiles (the last group of a map is short when og does not divide n_ot)"""
    assert 0 <= s < h + w - 1
    n_ot = n_otiles(nout)
    th_lo, th_hi = (s - w + 1 if s >= w else 0), (s if s < h else h - 1)   # :349
    th0 = th_lo & ~3
    n_seg = (th_hi - th0) // (16 * NT_DC) + 1                              # :351
    og = n_ot                                                              # :352
    while og > 1 and n * n_seg * ((n_ot + og - 1) // og) < MIN_TASKS:      # :353
        og -= 1
    n_og = (n_ot + og - 1) // og                                           # :354
    tasks = n * n_og * n_seg                                               # :355
    grid = min(tasks, MAX_GRID)                                            # :356
    groups = tuple(min(og, n_ot - g * og) for g in range(n_og))            # ot_lo .. ot_hi of the task loop (:180-181)
    return Geometry(tasks, grid, n_seg, og, n_og, groups, n_ot, 1, 1, th_lo, th_hi, th0)


def tasks_per_workgroup(g):
    """(fewest, most) tasks a workgroup of the launch takes: workgroup b takes tasks b, b + grid, b + 2 grid, ..."""
    return g.tasks // g.grid, (g.tasks + g.grid - 1) // g.grid


# ---- the cases
# encode order (lic360_cconv144_ec): (N, H, W, nout, act, ooff)
EC_CASES = [
    (129, 3, 17, 144, True, 2),        # 516 tasks on 256 workgroups (4 take three), odd H, W = 17, residual, haloed output
    (129, 3, 17, 49, False, 0),        # the last layer into plain NCHW
    (257, 2, 16, 49, False, 0),        # 257 tasks: only workgroup 0 takes a second one
]
# decode order (lic360_cconv144_dc_plane): (N, H, W, nout, act, planes); planes None: the first, the middle and the last one
DC_CASES = [
    (33, 3, 4, 144, True, None),       # og = 1, 297 tasks
    (40, 4, 6, 144, True, None),       # groups [2, 2, 2, 2, 1]
    (72, 3, 4, 144, True, None),       # groups [4, 4, 1]: the production split
    (100, 3, 4, 144, True, None),      # groups [8, 1]
    (260, 3, 4, 144, True, None),      # og = 9, 260 tasks
    (100, 3, 4, 49, False, None),      # last layer, groups [3, 1]
    (72, 3, 4, 49, False, None),       # last layer, og = 1, 288 tasks
    (30, 33, 33, 144, True, (31, 32, 33)),     # planes 32 and 33: n_seg = 2, og = 2, 300 tasks (plane 31: one segment, og = 1)
]
EC_REPEAT, DC_REPEAT = EC_CASES[0], DC_CASES[0]
# what bench.py's step runs: 64 maps of 32 x 64, hidden layers (144 outputs) and the last layer (49)
PRODUCTION = [(64, 32, 64, 144), (64, 32, 64, 49)]


def dc_planes(case):
    n, h, w, nout, act, planes = case
    return tuple(planes) if planes is not None else (0, (h + w - 2) // 2, h + w - 2)


def ec_id(case):
    return "n%d_%dx%d_to%d" % case[:4]


dc_id = ec_id


def ec_class(g):
    """what distinguishes one encode-order launch from another as far as the task loop goes"""
    return g.n_ot, g.tasks > g.grid


def dc_class(g):
    return g.n_ot, g.groups, g.n_seg


# ---- where a wrong output sits, in the kernel's own terms: map, output tile, task, workgroup (= task mod grid) and which of its turns
def describe_ec_mismatch(case, got, want):
    n_, h, w, nout, act, ooff = case
    g = ec_geometry(n_, h, w, nout)
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return "equal"
    n, o, r, c = (int(v) for v in bad[0])
    msg = "%s: %d of %d floats differ; first at out%s = %r, expected %r" % (ec_id(case), len(bad), got.size, (n, o, r, c), float(got[n, o, r, c]), float(want[n, o, r, c]))
    y, x = r - ooff, c - ooff
    if not (0 <= y < h and 0 <= x < w):
        return msg + ": a HALO cell was written"
    task = (n * g.tiles_r + y // NT_EC) * g.tiles_c + x // 16
    return msg + ": map %d, output tile %d, task %d = workgroup %d's turn %d (of %d tasks on %d workgroups)" % (n, o // 16, task, task % g.grid, task // g.grid, g.tasks, g.grid)


def describe_dc_mismatch(case, got, want):
    n_, h, w, nout, act, _ = case
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return "equal"
    n, o, row, col = (int(v) for v in bad[0])
    msg = "%s: %d of %d floats differ; first at out%s = %r, expected %r" % (dc_id(case), len(bad), got.size, (n, o, row, col), float(got[n, o, row, col]), float(want[n, o, row, col]))
    s, th = row - R0, col - C0
    if not (0 <= s < h + w - 1 and 0 <= th < h and 0 <= s - th < w):
        return msg + ": a PADDING cell was written"
    if s not in dc_planes(case):
        return msg + ": cell (%d, %d) of plane %d, which was not launched" % (th, s - th, s)
    g = dc_geometry(n_, h, w, nout, s)
    seg, grp = (th - g.th0) // (16 * NT_DC), (o // 16) // g.og
    task = (n * g.n_seg + seg) * g.n_og + grp
    return msg + ": plane %d, map %d, cell (%d, %d), output tile %d = tile %d of group %d %r, segment %d, task %d = workgroup %d's turn %d (of %d tasks on %d workgroups)" % (
        s, n, th, s - th, o // 16, (o // 16) % g.og, grp, list(g.groups), seg, task, task % g.grid, task // g.grid, g.tasks, g.grid)


# ---- one definition of the weights, the plan and the pack of a 144-channel layer (tests/test_gpu_ops.py uses it too)
def i144_setup(lic, rng, nout, act):
    import ctypes as C
    import torch
    from util import conv_params
    w, b, a = conv_params(rng, None, nout, 144, act=act)
    L = lic._lib
    plan = C.c_void_p(0)
    assert L.lic360_conv_plan_create(144, 1, nout, 5, 6, C.byref(plan)) == 0
    assert L.lic360_conv144_supported(plan) == 1
    packed = torch.empty(L.lic360_conv144_packed_floats(plan), dtype=torch.float32, device="cuda:0")
    wd = torch.from_numpy(np.ascontiguousarray(w)).to("cuda:0")
    assert L.lic360_conv144_pack(lic._stream(0), plan, lic._p(wd), lic._p(packed)) == 0, L.lic360_last_error()
    return w, b, a, plan, packed
