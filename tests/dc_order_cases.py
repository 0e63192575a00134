"""Cases of the decode lists' ORDER (csrc/need.h: dcl_group_pos, dcl_place_round; need_kernels.hip: k_dc_tasks, k_dc_place; LIC360_DC_ORDER), with the
grouped emission, the placement pass and the decode kernel's walk restated from DESIGN.md 4.6 ("List order").  No GPU and no call of the library in
here: tests/test_dc_order_cpu.py checks this file against the library's host-only lic360_dcl_order_layout, tests/test_gpu_dc_order.py runs codecs
under every order.

The walk.  Workgroup w of an XCD's W runs, as its k-th task, the record at k W + w (k even) or k W + W - 1 - w (k odd) of the XCD's list: a ROUND is W
consecutive records.  Emission decides which records share a round, placement which workgroup of the round gets which.

Emission.  The visible blocks of a plane, heaviest first, in groups of NB; inside a group net, then record index r, then block; a block with fewer
records runs out.  NB = 1 is block major: block, net, r.

Placement.  Round by round: the round's records sorted by cost descending (ties: list index) go to the workgroups that have a slot in the round (a
short last round fills its first slots) by load ascending (ties: workgroup index); load += cost.  Cost = steps of the block's longest chain,
min(g0 + 7, G), + 3 per task.  The rounds are taken in list order, except that a short last round is taken FIRST: its workgroups are fixed by its
slots, and charged first the full rounds even them out.  The rule is greedy: where it still leaves the most loaded workgroup heavier than the list
as emitted does, the list stays as emitted."""
import os

import numpy as np

GRID = 256                  # D6_GRID: workgroups of a decode launch
TASK_SWITCH = 3             # DCL_TASK_SWITCH
ORDERS = {"1": (1, False), "1p": (1, True), "2": (2, True), "4": (4, True), "8": (8, True)}      # LIC360_DC_ORDER -> (NB, placement)
DEFAULT_ORDER = "8"        # what a codec created without the switch builds
GOLDEN = "dc_order_counts.npz"
GOLDEN_SHAPE = (48, 64, 128)                                      # G, H, W of tools/dc_probe.py, the shape of the bench's main codec
GOLDEN_LAYERS = (2, 6, 10, 11)
GOLDEN_IMAGES = tuple(range(0, 64, 8))                            # the eight samples of XCD 0's list in a batch of 64
# FusedCodec shapes (G, H, W, B) of tests/test_gpu_dc_order.py
GPU_SHAPES = [
    (48, 16, 20, 16),       # two samples per XCD, 96 records on a middle plane: three rounds, one of them short
    (48, 16, 20, 64),       # eight samples per XCD, the bench's chunk
    (12, 16, 24, 16),       # lists shorter than a round
]


def shape_id(s):
    return "g%d_%dx%d_b%d" % tuple(s)


def wgs_of_xcd(xcd, grid=GRID):
    """workgroups blockIdx.x = xcd (mod 8) of a launch of `grid`"""
    return (grid - xcd + 7) >> 3


def cost(g0, G):
    return min(g0 + 7, G) + TASK_SWITCH


def ids_of(nrec):
    """[(block j, net, r)] in block-major order: the identity of a record is its index here"""
    return [(j, net, r) for j, n in enumerate(nrec) for net in range(3) for r in range(n)]


def emission(nrec, nb):
    """-> emit[id]: the position of every record after the grouped emission"""
    nrec = list(nrec)
    first = np.concatenate([[0], np.cumsum([3 * n for n in nrec])]).tolist()
    seq = []
    for j0 in range(0, len(nrec), nb):
        grp = range(j0, min(len(nrec), j0 + nb))
        for net in range(3):
            for r in range(max([nrec[j] for j in grp], default=0)):
                seq += [first[j] + net * nrec[j] + r for j in grp if nrec[j] > r]
    emit = np.zeros(len(seq), np.int64)
    emit[np.array(seq, np.int64)] = np.arange(len(seq))
    return emit


def placement(costs, W):
    """costs in list order -> to[e]: where the placement pass puts the record at list position e"""
    n = len(costs)
    to, load = np.zeros(n, np.int64), [0] * W
    rounds = list(enumerate(range(0, n, W)))
    if n % W:
        rounds = rounds[-1:] + rounds[:-1]                                  # a short last round is charged first
    for k, r0 in rounds:
        m = min(W, n - r0)
        recs = sorted(range(m), key=lambda i: (-costs[r0 + i], i))
        wgs = sorted(range(W - m, W) if k & 1 else range(m), key=lambda w: (load[w], w))
        for i, w in zip(recs, wgs):
            to[r0 + i] = r0 + (W - 1 - w if k & 1 else w)
            load[w] += costs[r0 + i]
    asis = walk_loads(np.arange(n), np.array(costs, np.int64), W)
    if n and max(load) > asis.max():                                        # the greedy rule lost (a short last round): the list stays as emitted
        return np.arange(n)
    return to


def layout(g0, nrec, G, nb, place, W):
    """-> (emit[id], slot[id]) as lic360_dcl_order_layout reports them"""
    emit = emission(nrec, nb)
    if not place:
        return emit, emit.copy()
    c = costs_by_id(g0, nrec, G)
    in_list = np.zeros(len(c), np.int64)
    in_list[emit] = c
    return emit, placement(in_list.tolist(), W)[emit]


def costs_by_id(g0, nrec, G):
    return np.array([cost(g0[j], G) for (j, _net, _r) in ids_of(nrec)], np.int64)


def walk_loads(slot, costs, W):
    """load of each of the W workgroups when record id sits at list position slot[id] (the kernel's boustrophedon walk)"""
    load = np.zeros(W, np.int64)
    k, pos = slot // W, slot % W
    np.add.at(load, np.where(k & 1, W - 1 - pos, pos), costs)
    return load


def max_over_mean(loads):
    """of a set of launches (one load vector each): every launch waits for its most loaded workgroup"""
    tot = sum(float(l.mean()) for l in loads)
    return sum(float(l.max()) for l in loads) / tot if tot else 1.0


def count_cases():
    """(g0 per block, records per net per block, G): the edges the issue names around W = 31 / 32, then seeded lists"""
    out = [([], [], 48), ([45], [0], 48), ([45], [1], 48), ([0], [5], 3), ([45, 42], [0, 0], 48)]
    for total in (10, 11, 30, 31, 32, 33, 63, 64, 65, 96):                  # 3 * nrec records: below, at and one past a round of 31 / 32, and one short
        if total % 3 == 0:
            out.append(([45], [total // 3], 48))
    out.append(([45, 42], [10, 1], 48))                                     # 33 = W + 1 records at W = 32
    out.append(([45, 42, 39], [5, 5, 1], 48))                               # 33 again over three blocks
    out.append(([45, 42], [10, 0], 48))                                     # 30
    out.append(([9, 6, 3, 0], [3, 3, 3, 2], 12))                            # 33 with a short last block
    out.append(([6, 3, 0], [4, 4, 3], 8))                                   # 33, G no multiple of 3
    rng = np.random.default_rng(20241)
    for _ in range(120):
        G = int(rng.choice([5, 12, 24, 48, 72]))
        n_gb = (G + 2) // 3
        vis = int(rng.integers(1, n_gb + 1))
        top = int(rng.integers(vis - 1, n_gb))                              # blocks top, top - 1, ..: heaviest first
        g0 = [3 * (top - j) for j in range(vis)]
        kind = int(rng.integers(0, 4))
        hi = (2, 9, 17, 49)[kind]
        nrec = rng.integers(0, hi, vis)
        if kind == 0:
            nrec[rng.random(vis) < 0.5] = 0
        out.append((g0, nrec.tolist(), G))
    return out


# ---- the recorded smooth-mask counts: blocks and records per net of XCD 0's lists at the bench's main shape (layers GOLDEN_LAYERS, every plane),
# ---- from tests/util.py masks through the list builder restated in tests/dc_tall_cases.py plus the plain-or-packed choice of latents of <= 64 rows
def smooth_mask_counts():
    import dc_tall_cases as tall
    from util import make_latent
    G, H, W = GOLDEN_SHAPE
    mask = np.concatenate([make_latent("smooth", np.random.default_rng(i), G, H, W)[1] for i in GOLDEN_IMAGES], 0)
    need = tall.need_maps(mask)
    rows = []                                                               # (layer, plane, g0, records per net)
    for p in range(H + W + G - 2):
        for g0 in tall.visible_blocks(G, H, W, p):
            lo, hi, _gm = tall.block_hulls(need, G, H, W, p, g0)            # [8, 12]
            for l in GOLDEN_LAYERS:
                clo, chi = lo[:, l].tolist(), hi[:, l].tolist()
                live = sum(b >= a for a, b in zip(clo, chi))
                k, slo, packed = 0, clo[0], 0
                while k < len(clo):
                    pcs, k, slo = tall.wave_pieces(clo, chi, H, len(clo), k, slo)
                    if not pcs:
                        break
                    packed += 1
                rows.append((l, p, g0, live if packed >= live else packed))
    return np.array(rows, np.int16)


def write_golden():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)
    np.savez_compressed(path, rows=smooth_mask_counts(), shape=np.array(GOLDEN_SHAPE), images=np.array(GOLDEN_IMAGES))
    return path


def golden_lists():
    """{layer: [(g0 per block, records per net per block)] per plane with a visible block} from the fixture"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN))
    assert tuple(g["shape"]) == GOLDEN_SHAPE and tuple(g["images"]) == GOLDEN_IMAGES
    out = {l: {} for l in GOLDEN_LAYERS}
    for l, p, g0, n in g["rows"].tolist():
        a = out[l].setdefault(p, ([], []))
        a[0].append(g0)
        a[1].append(n)
    return {l: [out[l][p] for p in sorted(out[l])] for l in out}


def batch(shape, second=False):
    """code, mask [B, G, H, W] of a GPU shape: SURVEY 8d's smooth masks, the last two images i.i.d. (second: other masks, half of them i.i.d.)"""
    import dc_tall_cases as tall
    G, H, W, B = shape
    return tall.batch(G, H, W, B, (7100 if second else 6100) + G + B, n_iid=B // 2 if second else 2)


def weight_seed(shape):
    return 410 + shape[0]


# The CPU oracle's bitstreams of these batches are a committed fixture (written by tools/gen_golden_dc_order.py: the oracle takes about a second per image)
GOLDEN_STREAMS = "dc_order_streams.npz"


def stream_key(shape, second):
    return shape_id(shape) + ("_second" if second else "")


def golden_streams(shape, second, code, mask):
    """the oracle's bitstreams of the shape's batch from the fixture; code / mask: the batch, whose digests must be the fixture's"""
    import hashlib
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN_STREAMS))
    k = stream_key(shape, second)
    assert [hashlib.sha256(code.tobytes()).hexdigest(), hashlib.sha256(mask.tobytes()).hexdigest()] == [str(v) for v in g[k + "_sha256"]], "the fixture is of another batch"
    ends = np.cumsum(g[k + "_lengths"])
    assert len(ends) == shape[3]
    data = g[k + "_bytes"].tobytes()
    return [data[e - n:e] for e, n in zip(ends.tolist(), g[k + "_lengths"].tolist())]


if __name__ == "__main__":
    print(write_golden())
