"""Cases of "how old is a skipped cell" ("Why skipping is safe"): a model of which activation cells the fused latent codec writes
in a call and which stale cells the written ones read with a possibly non-zero weight, over a SEQUENCE of calls in the same buffers.  No GPU, no
oracle and no call of the library in here: tests/test_skip_age_cpu.py asserts on the model, tests/test_gpu_skip_age.py runs the sequences on
codecs and reads the buffers back (lic360_codec_debug_absmax), tools/gen_golden_skip_age.py writes the oracle's bytes of the batches.

The model.  Every interior cell of an activation buffer carries a DEPTH: the number of conv layers between it and real symbols.  The initial
fill is 0, layer 0's outputs are 1 (they read the symbols and nothing else); a cell that a task computes gets 1 + the largest depth it reads with
a possibly non-zero weight -- the residual input of an even layer counts as such a read --, a cell that nobody writes keeps what it has.

  * Reads (csrc/need.h).  Layer l >= 1 at (g, p) reads q = p + d, d in [-2, 2]^2, input groups g' <= min(G - 1, g - d_y - d_x).  The kernels read
    zero-haloed planes (cconv16_kernels.hip: "rows / columns beyond the image are never written and stay zero"; the decode layout likewise): a q
    outside the image is a zero, depth 0; nothing wraps around in longitude.
  * Encode order (codec_fused.hip: net_walk; need_kernels.hip: k_ec_tasks).  Three ping-pong buffers: layers 0, 4, 8 write e_buf[0], layers 1, 3,
    5, 7, 9 e_buf[1], layers 2, 6, 10 e_buf[2]; layer l reads out(l - 1), an even l > 0 adds out(l - 2).  Layer 0 runs in full.  A (4 x 16 tile,
    block of 4 groups) task of layer 1..10 runs when the tile's largest need reaches the block's first group, and stores EVERY cell of the tile for
    the block's groups, dead ones included.  The fused last layer (blocks of 5) stores no activation.  Plane of (net n, sample i) = n B + i: it
    moves when B changes.  `clear`: e_buf[1] and e_buf[2] <- 0 over the call's 3 B samples before layer 0 (what lic360_codec_encode does).
  * Decode order.  One buffer per layer, d_act[0..10] and d_y.  Layer l on plane t reads cells of layer l - 1 on planes <= t, all of which this
    call's layer l - 1 has passed already, and a cell is stored at most once per call (on its own plane): the plane-by-plane walk leaves what a
    layer-by-layer walk leaves, and the model walks layer by layer.  Below the list regime (B < 16 or 8 does not divide B) every cell of the 3 B
    samples is stored; in it, layer 0 is stored in full and of layers 1..11 per (sample, plane, block of 3 groups) the hull of the rows that need
    one of the block's groups (dc_tall_cases.block_hulls), for the groups that are needed somewhere on the plane.  (A wave that packs several
    samples, and a plain whole-image record, store a little more: the depth bound l + 1 of d_act[l] does not depend on which cells are stored.)

The bound.  M_0 = 3.5 (|symbol - 3.5|), M_d = R M_{d-1} + b with R = the largest row sum of |W_l| over layers 0..10, + 1 (the residual), and b the
largest |bias|: PReLU slopes are at most 1 in magnitude, so |cell| <= M_d for every cell of depth <= d, in exact arithmetic; fp32 rounding of the
at most 25 * 4 G + 2 terms of a cell is covered by the factor (1 + 2^-20) per layer."""
import hashlib
import os

import numpy as np

import dc_tall_cases as tall

TILE_H, TILE_W = 4, 16
EC_GROUPS = 4               # groups per block of the encode order's hidden layers
LAYERS = 12
CODERS = ("device", "host")

# ---- the two codecs and their sequences.  batches: name -> (B, seed of the codes, patch column of the importance map (mask columns 2 c, 2 c + 1),
# ---- images that carry the patch: "most" = all but every fourth); calls: the batch of every call; background: the importance level outside the patch.
# ---- Chosen with the model (tests/test_skip_age_cpu.py holds the argument):
# ----   * the recurrence needs a tile that is skipped at EVERY layer next to one that is computed.  With 12 groups a background of level 2 keeps every
# ----     (tile, block) live up to layer 8 (need_l = 1 + 2 (11 - l) + rows above, >= 8 for l <= 8): nothing is ever stale.  Level 0 leaves only the patch's cone.
# ----   * a patch's cone grows two columns per layer to the LEFT (need rises by one per column) and fades to the right (falls by one per column), so
# ----     the tile left of a patch is live at the early layers and is refreshed in all three buffers.  X's patch (tile column 1, columns 22, 23) and
# ----     Y's (tile column 3, columns 52, 53) are 30 columns apart: under X tile 2's upper blocks are skipped at every layer, under Y tile 1's, and
# ----     the computed cells on either side of column 32 read each other's leftovers, call after call.
# ----   * the 48-group latent is two tiles wide: Y's patch cannot be 20 columns right of tile 0, so Y always refreshes what X will read.
CODECS = {
    "g12": dict(shape=(12, 8, 64), max_batch=24, weight_seed=612, background=0,
                batches={"X": (24, 5100, 11, "most"), "Y": (16, 5200, 26, "most"), "Z": (3, 5300, 3, "all")},
                calls=["X", "Y", "X", "Y", "X", "Y", "Z", "Y", "X", "Y", "X", "Y"]),
    "g48": dict(shape=(48, 8, 32), max_batch=16, weight_seed=648, background=2,
                batches={"X": (16, 5400, 3, "most"), "Y": (16, 5500, 11, "most")},
                calls=["X", "Y"] * 5),
}
PATCH_ROW = 1               # map row of the patch: mask rows 2, 3 -- the lower half of the upper tile row
GOLDEN = "skip_age_streams.npz"

# ---- the weights: make_main_params(weight_seed, G) with layers 1..10 times SCALE and layer 11 divided by GROWTH (scaled_params).  Chosen on the
# ---- CPU from the oracle's fp32 net_ec over batch X (tools/gen_golden_skip_age.py --scale prints the table): the largest |activation| after
# ---- layer 0 and after each residual block, which must at least double per block and stay below 1e12 at layer 10.
SCALE = {"g12": 16.0, "g48": 12.0}
GROWTH = {"g12": 1.25e9, "g48": 1.3e7}                                      # (4.863e9 / 3.847 and 5.855e7 / 4.404, rounded)
BLOCK_MAXIMA = {"g12": (2.455, 193.7, 1.75e4, 1.239e6, 7.877e7, 4.863e9),   # about 9 x per layer; the unscaled net: 2.455 .. 3.847
                "g48": (3.101, 164.3, 6412.0, 1.643e5, 3.259e6, 5.855e7)}   # about 5 x per layer; the unscaled net: 3.101 .. 4.404


def codec_id(name):
    return "%s_%dx%dx%d" % ((name,) + CODECS[name]["shape"])


def batch(name, which):
    """code, mask [B, G, H, W] of batch `which` of codec `name`: prefix masks of level BACKGROUND, a 2 x 2 patch of level G on the chosen images;
    codes from util.latent's generator"""
    from util import latent
    G, H, W = CODECS[name]["shape"]
    B, seed, col, who = CODECS[name]["batches"][which]
    cs, ms = [], []
    for i in range(B):
        c, _, _ = latent(np.random.default_rng(seed + i), G, H, W)
        L = np.full((H // 2, W // 2), CODECS[name]["background"], np.int64)
        if who == "all" or i % 4 != 3:
            L[PATCH_ROW, col] = G
        Lup = np.repeat(np.repeat(L, 2, 0), 2, 1)
        cs.append(c)
        ms.append((np.arange(G)[:, None, None] < Lup[None]).astype(np.float32)[None])
    return np.concatenate(cs, 0), np.concatenate(ms, 0)


# ---------------------------------------------------------------------------------------------------------------- the depth model
def _read_depth(src, G):
    """src [N, G, H, W] depths of a layer's input -> [N, G, H, W]: the largest depth that (g, p) reads with a possibly non-zero weight"""
    N, _, H, W = src.shape
    pad = np.zeros((N, G + 1, H + 4, W + 4), src.dtype)                     # group index 0: "reads nothing"; halo: zeros
    pad[:, 1:, 2:-2, 2:-2] = np.maximum.accumulate(src, 1)                  # [g + 1] = max over g' <= g
    out = np.zeros_like(src)
    for k in range(-4, 5):
        top = np.clip(np.arange(G) - k, -1, G - 1) + 1                      # highest input group of output group g at a tap with d_y + d_x = k
        sel = pad[:, top]
        for dy in range(max(-2, k - 2), min(2, k + 2) + 1):
            dx = k - dy
            np.maximum(out, sel[:, :, 2 + dy:2 + dy + H, 2 + dx:2 + dx + W], out=out)
    return out


def ec_written(need, G, H, W, l):
    """need [B, 12, H, W] -> [B, G, H, W] bool: the cells the encode order's layer l (1..10) stores"""
    B = need.shape[0]
    nty, ntx = (H + TILE_H - 1) // TILE_H, (W + TILE_W - 1) // TILE_W
    t = np.full((B, nty * TILE_H, ntx * TILE_W), -1, np.int64)
    t[:, :H, :W] = need[:, l]
    tmax = t.reshape(B, nty, TILE_H, ntx, TILE_W).max((2, 4))               # [B, nty, ntx]
    cell = np.repeat(np.repeat(tmax, TILE_H, 1), TILE_W, 2)[:, :H, :W]      # the tile maximum at every cell
    first = np.arange(G) // EC_GROUPS * EC_GROUPS                           # first group of g's block
    return cell[:, None] >= first[None, :, None, None]


def ec_buffer(l):
    return 1 if l % 2 else (2 if l % 4 else 0)


class EncodeModel:
    """depths of e_buf[0..2] [3 max_batch, G, H, W] over a sequence of encode calls"""

    def __init__(self, G, H, W, max_batch, clear):
        self.G, self.H, self.W, self.clear = G, H, W, clear
        self.buf = [np.zeros((3 * max_batch, G, H, W), np.int16) for _ in range(3)]

    def call(self, mask):
        G, H, W = self.G, self.H, self.W
        B = mask.shape[0]
        need = tall.need_maps(mask)
        if self.clear:
            self.buf[1][:3 * B] = 0
            self.buf[2][:3 * B] = 0
        self.buf[0][:3 * B] = 1                                             # layer 0, in full
        for l in range(1, 11):
            src, dst = self.buf[ec_buffer(l - 1)], self.buf[ec_buffer(l)]
            d = _read_depth(src[:3 * B], G)
            if l % 2 == 0:
                d = np.maximum(d, self.buf[ec_buffer(l - 2)][:3 * B])
            wr = np.concatenate([ec_written(need, G, H, W, l)] * 3, 0)      # plane n B + i: the three nets share the sample's lists
            dst[:3 * B] = np.where(wr, d + 1, dst[:3 * B])
        return [int(b.max()) for b in self.buf]


def dc_written(need, G, H, W, lists):
    """need [B, 12, H, W] -> [12, B, G, H, W] bool: the cells the decode order's layers store in one call"""
    B = need.shape[0]
    out = np.ones((LAYERS, B, G, H, W), bool)
    if not lists:
        return out
    out[1:] = False
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for p in range(H + W + G - 2):
        for g0 in tall.visible_blocks(G, H, W, p):
            lo, hi, gm = tall.block_hulls(need, G, H, W, p, g0)             # [B, 12]
            for q in range(tall.PS):
                g, s = g0 + q, p - g0 - q
                if g >= G or s < 0 or s >= H + W - 1:
                    continue
                on = (yy + xx == s)[None, None] & (yy[None, None] >= lo[:, :, None, None]) & (yy[None, None] <= hi[:, :, None, None])
                on &= (gm >> q & 1).astype(bool)[:, :, None, None]          # [B, 12, H, W]
                out[1:, :, g] |= on.transpose(1, 0, 2, 3)[1:]
    return out


class DecodeModel:
    """depths of d_act[0..10] and d_y (index 11) [3 max_batch, G, H, W] over a sequence of decode calls"""

    def __init__(self, G, H, W, max_batch):
        self.G, self.H, self.W = G, H, W
        self.lists_possible = max_batch % 8 == 0 and max_batch >= 16 and H <= 128
        self.buf = [np.zeros((3 * max_batch, G, H, W), np.int16) for _ in range(LAYERS)]

    def call(self, mask, cache=None):
        """cache: a dict that keeps the stored cells of this mask batch between calls"""
        G, H, W = self.G, self.H, self.W
        B = mask.shape[0]
        lists = self.lists_possible and B % 8 == 0 and B >= 16
        cache = {} if cache is None else cache
        if "wr" not in cache:
            cache["wr"] = dc_written(tall.need_maps(mask), G, H, W, lists)
        wr = cache["wr"]
        self.buf[0][:3 * B] = 1
        for l in range(1, LAYERS):
            d = _read_depth(self.buf[l - 1][:3 * B], G)
            if l % 2 == 0 and l < 11:
                d = np.maximum(d, self.buf[l - 2][:3 * B])
            w3 = np.concatenate([wr[l]] * 3, 0)
            self.buf[l][:3 * B] = np.where(w3, d + 1, self.buf[l][:3 * B])
        return [int(b.max()) for b in self.buf]


def encode_series(name, clear):
    """-> [calls][3]: the largest depth in e_buf[0..2] after every call of the codec's sequence"""
    cfg = CODECS[name]
    enc = EncodeModel(*cfg["shape"], cfg["max_batch"], clear)
    masks = {k: batch(name, k)[1] for k in cfg["batches"]}
    return [enc.call(masks[k]) for k in cfg["calls"]]


def decode_series(name):
    """-> [calls][12]: the largest depth in d_act[0..10] and d_y after every call of the codec's sequence"""
    cfg = CODECS[name]
    dec = DecodeModel(*cfg["shape"], cfg["max_batch"])
    masks = {k: batch(name, k)[1] for k in cfg["batches"]}
    written = {}
    return [dec.call(masks[k], written.setdefault(k, {})) for k in cfg["calls"]]


# ---------------------------------------------------------------------------------------------------------------- weights and the bound
def scaled_params(name, scale=None, growth=None):
    """make_main_params with layers 1..10 times `scale` and layer 11 divided by `growth` (defaults: the recorded SCALE / GROWTH)"""
    from util import make_main_params
    G = CODECS[name]["shape"][0]
    s = np.float32(SCALE[name] if scale is None else scale)
    gr = np.float32(GROWTH[name] if growth is None else growth)
    layers = make_main_params(CODECS[name]["weight_seed"], G)
    for l in range(1, 11):
        layers[l]["w"] = (layers[l]["w"] * s).astype(np.float32)
    layers[11]["w"] = (layers[11]["w"] / gr).astype(np.float32)
    return layers


def depth_bound(layers, depth=12):
    """M_depth in fp64, from the weights alone"""
    R, b = 0.0, 0.0
    for l in range(11):
        w = np.abs(layers[l]["w"].astype(np.float64))                       # [3, nout, C, 5, 5]
        R = max(R, float(w.sum((2, 3, 4)).max()))
        b = max(b, float(np.abs(layers[l]["b"].astype(np.float64)).max()))
        assert float(np.abs(layers[l]["a"]).max()) <= 1.0
    M = 3.5
    for _ in range(depth):
        M = ((R + 1.0) * M + b) * (1.0 + 2.0 ** -20)
    return M


# ---------------------------------------------------------------------------------------------------------------- the oracle's bytes
def stream_key(name, which):
    return "%s_%s" % (name, which)


def golden_streams(name, which, code, mask):
    """the oracle's bitstreams of a batch from the fixture; code / mask: the batch, whose digests must be the fixture's"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN))
    k = stream_key(name, which)
    assert [hashlib.sha256(code.tobytes()).hexdigest(), hashlib.sha256(mask.tobytes()).hexdigest()] == [str(v) for v in g[k + "_sha256"]], "the fixture is of another batch"
    assert [float(g[name + "_scale"]), float(g[name + "_growth"])] == [float(SCALE[name]), float(GROWTH[name])], "the fixture is of other weights"
    ends = np.cumsum(g[k + "_lengths"])
    assert len(ends) == code.shape[0]
    data = g[k + "_bytes"].tobytes()
    return [data[e - n:e] for e, n in zip(ends.tolist(), g[k + "_lengths"].tolist())]
