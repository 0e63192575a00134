"""Cases, references and broken-kernel models for the backward of the one-pass GDN (csrc/gdn_grad_kernels.hip, lic360.gdn_backward).  With
s_i = beta_i + sum_j gamma_ij x_j^2, n_i = sqrt(s_i) and the upstream gradient g:
               GDN (y = x / n)                    inverse (y = x * n)
    r_i        g_i / n_i                          g_i * n_i
    t_i        (g_i * (x_i / n_i)) / s_i          (g_i * x_i) / n_i
    u_k        sum_i gamma_ik t_i                 same
    dx_k       r_k - x_k * u_k                    r_k + x_k * u_k
    dgamma_ij  -1/2 sum_{n,p} t_i x_j^2           +1/2 sum_{n,p} t_i x_j^2
    dbeta_i    -1/2 sum_{n,p} t_i                 +1/2 sum_{n,p} t_i
every operation one rounding in the order written.  Two tiers of data:
  exact    channel j has a fixed magnitude a_j in {1, 2, 4} with random signs per cell, gamma is integer in 0 .. 3, beta_i = 4^m - sum_j gamma_ij a_j^2 >= 1,
           g integer in -15 .. 15.  Then s = 4^m everywhere, n = 2^m, t = g x 2^-3m (g x 2^-m for the inverse) and every sum is a sum of integers in one
           unit that stays below 2^24 (assert_exact_domain): exact in fp32 in ANY order -- dx, the t-map, dgamma and dbeta are compared bit for bit.
  integer  sconv_cases.gdn_make's data (x integer in -15 .. 15, gamma 0 .. 3, beta 1 .. 16: real norms) plus integer g.  s is an exact integer, so the
           t-map is bit for bit the numpy fp32 restatement (sqrt, / and * are correctly rounded); dx, dgamma and dbeta lie within an fp32 summation bound
           of the float64 result (integer_bounds derives it from the term magnitudes).
The geometry of the kernels is restated here (TILE, MAX_SPLITS, geometry()): the case list is checked against it on the CPU (tests/test_gdn_grad_cases_cpu.py),
and every broken-kernel model of MUTATIONS changes the reference on at least one listed case."""
import collections

import numpy as np

import sconv_cases as sc

CHANNELS = sc.GDN_CHANNELS
TILE = 32                        # positions per workgroup of k_gdn_backward_dx and per tile of k_gdn_backward_param; a tile never straddles two images
MAX_SPLITS = 256                 # workgroups of k_gdn_backward_param at most
EPS = 2.0 ** -24                 # unit roundoff of fp32
EXACT_BELOW = float(1 << 24)
UNWRITTEN = 7.7701e33            # gpu_support.SENTINEL[torch.float32]

GradCase = collections.namedtuple("GradCase", "name c n h w inverse misaligned")
CASES = [
    GradCase("b16_one_split", 16, 1, 4, 5, False, False),                  # P = 20: one tile, one split
    GradCase("b16_p35", 16, 1, 5, 7, True, False),                         # P = 35: odd, a short second tile
    GradCase("b16_more_tiles_than_splits", 16, 3, 3, 919, False, False),   # P = 2757: 87 tiles an image, 261 tiles, 131 splits of 2, the last one of 1
    GradCase("b32_p64", 32, 1, 8, 8, True, False),                         # P = 64: two full tiles
    GradCase("b32_p66_n3", 32, 3, 6, 11, False, False),                    # P % 4 == 2, three images
    GradCase("b48_p65", 48, 1, 5, 13, True, False),                        # P = 64 + 1
    GradCase("b48_p128", 48, 1, 8, 16, False, False),                      # P = 128
    GradCase("b64_misaligned", 64, 1, 8, 8, False, True),                  # P % 4 == 0 through views 4 bytes past a 16-byte boundary
    GradCase("b64_p80_n3", 64, 3, 4, 20, True, False),                     # an image ends inside a tile's width: the tile ends with it
    GradCase("b96_odd", 96, 1, 9, 15, True, False),
    GradCase("b96_vec", 96, 1, 16, 20, False, False),
    GradCase("b128_p130", 128, 1, 10, 13, False, False),
    GradCase("b128_p128", 128, 1, 8, 16, True, False),
    GradCase("b192_p777_n3", 192, 3, 21, 37, False, False),                # 25 tiles an image, the last one of 9 positions
    GradCase("b192_p777_inverse", 192, 1, 21, 37, True, False),
    GradCase("b192_vec", 192, 1, 12, 20, False, False),
    GradCase("b192_misaligned", 192, 1, 12, 20, True, True),
]
MODULE_CASE = GradCase("b192_68x132", 192, 1, 68, 132, False, False)       # the smallest production map: 281 tiles, 141 splits of 2, the last one of 1


Geometry = collections.namedtuple("Geometry", "tpi ntiles tps nsplit vec scratch_bytes")


def geometry(case):
    """the launch of lic360_gdn_backward restated: tiles an image, tiles, tiles a split, splits, the 16-byte form, scratch bytes"""
    p = case.h * case.w
    tpi = -(-p // TILE)
    ntiles = tpi * case.n
    tps = max(1, -(-ntiles // MAX_SPLITS))
    nsplit = -(-ntiles // tps)
    tmap = -(-(case.n * case.c * p * 4) // 16) * 16
    return Geometry(tpi, ntiles, tps, nsplit, p % 4 == 0 and not case.misaligned, tmap + min(ntiles, MAX_SPLITS) * (case.c * case.c + case.c) * 4)


def _rng(case, tier):
    return np.random.default_rng(sc._stable(("gdn_grad", tier, case.name)))


def make_exact(case):
    rng = _rng(case, "exact")
    c, shape = case.c, (case.n, case.c, case.h, case.w)
    a = rng.choice(np.array([1.0, 2.0, 4.0], np.float32), c)
    x = (a[None, :, None, None] * rng.choice(np.array([-1.0, 1.0], np.float32), shape)).astype(np.float32)
    gamma = rng.integers(0, 4, (c, c)).astype(np.float32)
    load = gamma.astype(np.float64) @ (a.astype(np.float64) ** 2)
    m = 1
    while 4 ** m < load.max() + 1:
        m += 1
    beta = (4.0 ** m - load).astype(np.float32)
    return dict(x=x, gy=sc._ints(rng, 15, shape), gamma=gamma, beta=beta, m=m)


def make_integer(case):
    data = sc.gdn_make(sc.GdnCase(case.name, case.c, case.n, case.h, case.w, case.inverse, case.misaligned, False))
    data["gy"] = sc._ints(_rng(case, "integer"), 15, data["x"].shape)
    return data


def assert_exact_domain(case, data):
    """s = 4^m in every cell, and every sum of the backward is a sum of integers times one power of two that stays below 2^24"""
    m, p = data["m"], case.h * case.w
    s = sums(data)
    assert float(data["beta"].min()) >= 1 and float(data["gamma"].min()) >= 0 and np.all(s == 4.0 ** m), case.name
    assert np.abs(data["x"]).max() <= 4 and np.abs(data["gy"]).max() <= 15
    # in units of 2^-3m (2^-m for the inverse): |t| <= 60, |t x_j^2| <= 960, |u| <= 3 * 60 * c, |x u| <= 4 * that, |r| <= 15 * 4^m
    assert 60 * 16 * case.n * p < EXACT_BELOW, (case.name, 960 * case.n * p)
    assert 15 * 4.0 ** m + 4 * 3 * 60 * case.c < EXACT_BELOW, (case.name, m)
    return m


def sums(data):
    """s in float64 (exact: integers far below 2^53)"""
    x = data["x"].astype(np.float64)
    n, c, h, w = x.shape
    return np.matmul(data["gamma"].astype(np.float64)[None], (x * x).reshape(n, c, h * w)) + data["beta"].astype(np.float64)[None, :, None]


def cells(case, data, dtype=np.float32, mut=None):
    """(x, r, t) [n, c, P] in `dtype`, every operation one rounding in the stated order; s is exact in either dtype"""
    n, c, p = case.n, case.c, case.h * case.w
    x, g = data["x"].reshape(n, c, p).astype(dtype), data["gy"].reshape(n, c, p).astype(dtype)
    s = sums(data).astype(dtype)
    assert np.array_equal(s.astype(np.float64), sums(data))
    nrm = np.sqrt(s)
    if case.inverse and mut != "direction_ignored":
        r, t = g * nrm, (g * x) / nrm
    else:
        r, t = g / nrm, (g * (x / nrm)) / (nrm if mut == "t_over_n" else s)
    return x, r, t


def _weights(case, mut):
    """how often each position counts in the two parameter sums, [n, P], under a broken-kernel model of the tiles and splits"""
    geo, p = geometry(case), case.h * case.w
    w = np.ones((case.n, p))
    tile_of = (np.arange(case.n)[:, None] * geo.tpi + np.arange(p)[None, :] // TILE)                  # [n, P] -> tile
    if mut == "last_tile_dropped":
        w[tile_of == geo.ntiles - 1] = 0
    if mut == "last_split_dropped":
        w[tile_of // geo.tps == geo.nsplit - 1] = 0
    if mut == "split_twice":
        w[tile_of // geo.tps == 0] = 2
    return w


def reference(case, data, dtype=np.float32, mut=None):
    """dict(t, gx, ggamma, gbeta) in float64 from cells evaluated in `dtype`: with dtype float32 on the exact tier every value is an fp32 number and every sum
    exact (the expected bits); with float64 it is the reference of the integer tier"""
    x, r, t = (v.astype(np.float64) for v in cells(case, data, dtype, mut))
    gamma = data["gamma"].astype(np.float64)
    sign = 1.0 if (case.inverse and mut != "direction_ignored") else -1.0
    u = np.matmul((gamma if mut == "gamma_not_transposed" else gamma.T)[None], t)
    gx = r + sign * (x * u)
    w = _weights(case, mut)[:, None, :]
    tw = t * w
    half = 1.0 if mut == "half_missing" else 0.5
    x2 = x if mut == "x_not_squared" else x * x
    tg = tw[:1] if mut == "first_image_only" else tw
    ggamma = sign * half * np.einsum("nip,njp->ij", tg, x2[:tg.shape[0]])
    gbeta = sign * half * tw.sum((0, 2))
    if mut == "beta_rotated":
        gbeta = np.roll(gbeta, -4)
    shape = (case.n, case.c, case.h, case.w)
    return dict(t=t.reshape(shape), gx=gx.reshape(shape), ggamma=ggamma, gbeta=gbeta)


def as_fp32(ref):
    """the exact tier's expected arrays: float64 values that are fp32 numbers"""
    out = {}
    for k, v in ref.items():
        out[k] = v.astype(np.float32)
        assert np.array_equal(out[k].astype(np.float64), v), k
    return out


def integer_bounds(case, data):
    """how far the fp32 evaluation may lie from reference(..., float64) on the integer tier, per element, from the term magnitudes (first order in EPS, doubled
    for the higher orders).  t carries four roundings (sqrt, x / n, the product with g, / s): |dt| <= 4 EPS |t|; r two.
      gx      x_k * u_k - r_k: a chain of c fp32 additions in u (at most c EPS of sum_i |gamma_ik t_i|), t's four, the product with x_k and the final
              subtraction one each: (c + 6) EPS |x_k| sum_i |gamma_ik t_i| + 3 EPS |r_k|
      ggamma  a split adds tps * TILE terms in fp32, the splits are added in double and rounded once: (tps * TILE + 4 + 1) EPS sum |t_i| x_j^2
      gbeta   the same with x_j^2 = 1"""
    x, r, t = (np.abs(v.astype(np.float64)) for v in cells(case, data, np.float64))
    gamma = data["gamma"].astype(np.float64)
    chain = geometry(case).tps * TILE
    shape = (case.n, case.c, case.h, case.w)
    return dict(gx=(2 * EPS * ((case.c + 6) * x * np.matmul(gamma.T[None], t) + 3 * r)).reshape(shape),
                ggamma=2 * EPS * (chain + 5) * np.einsum("nip,njp->ij", t, x * x), gbeta=2 * EPS * (chain + 5) * t.sum((0, 2)))


# broken-kernel models: name -> the cases on which the model must change the reference
MUTATIONS = {
    "gamma_not_transposed": lambda c: True,
    "direction_ignored": lambda c: c.inverse,
    "half_missing": lambda c: True,
    "t_over_n": lambda c: not c.inverse,
    "x_not_squared": lambda c: True,
    "last_tile_dropped": lambda c: True,
    "last_split_dropped": lambda c: geometry(c).nsplit > 1,
    "split_twice": lambda c: True,
    "first_image_only": lambda c: c.n > 1,
    "beta_rotated": lambda c: True,
}


def changed(case, data, mut):
    """which outputs a broken-kernel model changes on this case"""
    a, b = reference(case, data), reference(case, data, mut=mut)
    return [k for k in a if not np.array_equal(a[k], b[k])]


# ---- real data for the module test: float64 autograd of the composition
def composition(x, gamma, beta, inverse):
    """the reference's composition on torch tensors of any dtype: x [n, c, h, w], effective gamma [c, c] and beta [c]"""
    import torch
    c = x.shape[1]
    norm = torch.sqrt(torch.nn.functional.conv2d(x * x, gamma.view(c, c, 1, 1), beta))
    return x * norm if inverse else x / norm
