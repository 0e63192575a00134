"""Shared helpers for the parity tests: seeded synthetic weights / latents."""
import numpy as np


def _stable(key):
    """a process-independent integer of a (nested) tuple of ints / bools / None / strings: hash() of a tuple holding None depends
    on the object's address in CPython 3.10, so seeds drawn from it changed from run to run (VERDICT r2 #3b)"""
    import zlib
    return zlib.crc32(repr(key).encode())


def rng_for(*key):
    return np.random.default_rng(_stable(tuple(key)))


def case_rng(case):
    return np.random.default_rng(_stable(case))


def conv_params(rng, nb, nout, C, k=5, act=True):
    """Kaiming-normal weights, bias U(-.1,.1), PReLU slope 0.25 (+ jitter so that it matters)."""
    fan_in = C * k * k
    lead = () if nb is None else (nb,)
    w = (rng.standard_normal(lead + (nout, C, k, k)) * np.sqrt(2.0 / fan_in)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, lead + (nout,)).astype(np.float32)
    a = (0.25 + rng.uniform(-0.05, 0.05, lead + (nout,))).astype(np.float32) if act else None
    return w, b, a


def latent(rng, G, H, W, mean=0.5, spread=0.25):
    """code in {0..7} ~ round(N(3.5,1.2^2)); importance level L[h/2,w/2] in {0..G} ~ round(G (mean + spread N(0,1))); mask[g,y,x] = g < L.
    (mean / spread: the mask density; the defaults are the generator every committed digest was made with)"""
    code = np.clip(np.rint(rng.normal(3.5, 1.2, (1, G, H, W))), 0, 7).astype(np.float32)
    L = np.clip(np.rint(G * mean + G * spread * rng.standard_normal((H // 2, W // 2))), 0, G).astype(np.int64)
    Lup = np.repeat(np.repeat(L, 2, 0), 2, 1)
    mask = (np.arange(G)[:, None, None] < Lup[None]).astype(np.float32)[None]
    return code, mask, L.astype(np.float32)[None, None]


def smooth_field(rng, h, w, sigma=3.0):
    """unit-variance smooth noise on an [h, w] importance map ("n smooth noise"): white N(0,1) noise convolved with a separable
    Gaussian of `sigma` map cells (radius 3 sigma; longitude wraps around, latitude reflects at the poles), divided by the kernel's L2 norm.
    Plain numpy sums in a fixed order: the same values on every numpy / scipy version."""
    r = int(np.ceil(3 * sigma))
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= np.sqrt((k ** 2).sum())
    z = rng.standard_normal((h, w))
    zp = np.concatenate([z[r - 1::-1] if r <= h else np.resize(z[::-1], (r, w)), z, z[:-r - 1:-1] if r <= h else np.resize(z[::-1], (r, w))], 0)   # reflect
    y = sum(k[i] * zp[i:i + h] for i in range(2 * r + 1))
    cols = (np.arange(-r, w + r) % w)
    yp = np.ascontiguousarray(y[:, cols])                                                                                                       # wrap
    return np.ascontiguousarray(sum(k[i] * yp[:, i:i + w] for i in range(2 * r + 1)))


def latent_smooth(rng, G, H, W, sigma=3.0):
    """SURVEY.md 8d's latent-level workload: code in {0..7} ~ round(N(3.5, 1.2^2)); importance level of map cell (r, c)
    L = clip(round(G/2 + G/4 cos(lat_r) n[r, c]), 0, G) with n = smooth_field (sigma map cells) and lat_r the latitude of map row r
    (-pi/2 .. pi/2 over the H/2 rows): real importance maps are smooth and flatten towards the poles; mask[g, y, x] = g < L[y/2, x/2]."""
    code = np.clip(np.rint(rng.normal(3.5, 1.2, (1, G, H, W))), 0, 7).astype(np.float32)
    h, w = H // 2, W // 2
    lat = (np.arange(h) + 0.5) / h * np.pi - np.pi / 2
    L = np.clip(np.rint(G / 2 + G / 4 * np.cos(lat)[:, None] * smooth_field(rng, h, w, sigma)), 0, G).astype(np.int64)
    Lup = np.repeat(np.repeat(L, 2, 0), 2, 1)
    mask = (np.arange(G)[:, None, None] < Lup[None]).astype(np.float32)[None]
    return code, mask, L.astype(np.float32)[None, None]


def make_latent(kind, rng, G, H, W, mean=0.5, spread=0.25):
    """kind "smooth": SURVEY.md 8d's importance maps (latent_smooth); "iid": every map cell drawn independently (latent) -- no real map looks
    like that; it is kept as the adversarial case (nothing for the dead-cone skip to find) and for the digests committed before round 6"""
    return latent_smooth(rng, G, H, W) if kind == "smooth" else latent(rng, G, H, W, mean, spread)


# ---- synthetic, seeded parameters of the two entropy models (no oracle involved: bench.py uses these too)
def make_main_params(seed, G):
    """12 layers x 3 stacked nets [weight, sigma, mu] (lic360_demo.py:104-112,302)."""
    rng = np.random.default_rng(seed)
    shapes = [(G * 1, G * 4, 5, True)] + [(G * 4, G * 4, 6, True)] * 10 + [(G * 4, G * 3, 6, False)]
    layers = []
    for C, nout, constrain, act in shapes:
        w, b, a = conv_params(rng, 3, nout, C, act=act)
        layers.append(dict(w=w, b=b, a=a, constrain=constrain))
    layers[-1]["b"][1] += 2.0          # sigma net: last bias +2 (test/model_zoo.py:263)
    return layers


def make_imp_params(seed, cpg=144, nsym=49):
    rng = np.random.default_rng(seed)
    shapes = [(1, cpg, 5, True)] + [(cpg, cpg, 6, True)] * 10 + [(cpg, nsym, 6, False)]
    layers = []
    for C, nout, constrain, act in shapes:
        w, b, a = conv_params(rng, None, nout, C, act=act)
        layers.append(dict(w=w, b=b, a=a, constrain=constrain))
    return layers


# ---- torch-side helpers of the transforms' GPU tests (test_gpu_models.py, test_gpu_sconv_bf16x3.py)
def _pad_torch(x, pad):
    """the sphere apron of `pad` cells around a torch map [..., H, W]: longitude wraps, pole rows reflect and mirror"""
    import torch
    W = x.shape[-1]
    body = torch.cat([x[..., W - pad:], x, x[..., :pad]], -1)
    def across(r):
        r = torch.flip(r, (-1,))
        return torch.cat([r[..., W - pad:], r, r[..., :pad]], -1)
    return torch.cat([across(torch.flip(x[..., :pad, :], (-2,))), body, across(torch.flip(x[..., x.shape[-2] - pad:, :], (-2,)))], -2)


def _refresh(x, pad=2):
    """SpherePad in place: the apron of a padded map recomputed from its interior"""
    return _pad_torch(x[..., pad:-pad, pad:-pad], pad)


def _block_params(blk):
    """numpy parameters of a block under its state_dict keys + the constants of its GDN (the oracle's `blocks` take these)"""
    p = {k: v.detach().cpu().numpy() for k, v in blk.state_dict().items()}
    for name, m in blk.named_modules():
        if type(m).__name__ == "GDN":
            p[name + ".pedestal"], p[name + ".beta_bound"], p[name + ".gamma_bound"] = m.pedestal, m.beta_bound, m.gamma_bound
    return p
