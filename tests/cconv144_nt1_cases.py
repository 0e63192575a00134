"""Cases of k_cconv144's one-tile decode-order instantiation (k_cconv144<1, true, 1>, csrc/cconv144_kernels.hip), on top of the launch
geometry restated in tests/cconv144_cases.py.  No GPU and no oracle in here: tests/test_cconv144_nt1_cases_cpu.py checks this file by itself
(the rule below is the launch code's own, the tables reach every class they name), tests/test_gpu_cconv144_nt1.py compares the kernel with the
oracle on these cases, bit for bit.

The rule.  lic360_cconv144_dc_plane computes th_lo / th_hi / th0, n_seg, og and the grid as before and then picks the kernel: a plane whose
window of rows th0 .. th_hi fits ONE 16-row position tile runs the one-tile instantiation (a 5 x 20 x-window per channel, half the MFMAs),
every other plane the two-tile one.  Tasks, groups, grid, buffers and pitch do not depend on the choice."""
import cconv144_cases as cc

ONE_TILE_ROWS = 16         # the `< 16` of the dispatch condition: rows of one position tile


def one_tile(g):
    """the launch code's condition on a Geometry of cconv144_cases.dc_geometry: `a.n_seg == 1 && a.th_hi - a.th0 < 16`"""
    return g.n_seg == 1 and g.th_hi - g.th0 < ONE_TILE_ROWS


def instantiation(n, h, w, nout, s):
    """the NT of the k_cconv144<1, true, NT> that plane s of n maps of h x w runs"""
    return 1 if one_tile(cc.dc_geometry(n, h, w, nout, s)) else cc.NT_DC


# ---- the map and its planes: every class of window on one 20 x 15 map
H, W = 20, 15
#          s : (th_lo, th_hi, th0, one tile?, what it covers)
PLANES = {
    0: (0, 0, 0, True, "a one-row window"),
    15: (1, 15, 0, True, "the largest window that fits; it starts before the diagonal's first cell"),
    16: (2, 16, 0, False, "the smallest window that does not fit: the boundary"),
    19: (5, 19, 4, True, "th0 > 0"),
    33: (19, 19, 16, True, "the last plane"),
}
# ---- the batches: (N, nout, act, tasks, grid, groups, what it covers); cases in the form of cconv144_cases.DC_CASES
BATCHES = [
    (33, 144, True, 297, 256, (1,) * 9, "a workgroup's second task re-stages the narrow tile and carries `parity`"),
    (130, 144, True, 260, 256, (8, 1), "og > 1 with the short last group, persistent"),
    (72, 49, False, 288, 256, (1,) * 4, "the last layer"),
]
DC_CASES = [(n, H, W, nout, act, tuple(sorted(PLANES))) for n, nout, act, tasks, grid, groups, what in BATCHES]
# two chained layers (x -> y -> z), planes launched in decode order on one stream: one-tile and two-tile launches mixed, each plane of the
# second layer reads what the planes so far left in y
CHAIN_N, CHAIN_PLANES = 33, (14, 15, 16, 17, 18, 19)


def nt1_id(case):
    return cc.dc_id(case)
