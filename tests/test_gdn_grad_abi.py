"""The C entries of the one-pass GDN's backward (include/lic360_hip_gdn_grad.h, csrc/gdn_grad_kernels.hip) without a GPU: declared in the third header
only, present in the third binding table, bound and exported, the other two tables unchanged; the scratch query positive, monotone and 0 for refused or
empty arguments; every refusal before anything is launched; GDN and lic360_models.set_gdn_grad take the route."""
import ctypes
import importlib.util
import os
import re

import pytest

import gdn_grad_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKWARD = ("c_int", ["c_void_p"] * 9 + ["c_int", "c_int", "c_long", "c_int"])
SCRATCH = ("c_long", ["c_int", "c_int", "c_long"])
NAMES = ("lic360_gdn_backward", "lic360_gdn_backward_scratch_bytes")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_abi", os.path.join(ROOT, "tools", "gen_abi.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_entries_are_declared_bound_and_exported():
    import lic360
    from lic360._abi_table import ABI
    from lic360._abi_table_grad import ABI_GRAD
    from lic360._abi_table_gdn_grad import ABI_GDN_GRAD
    read = lambda name: open(os.path.join(ROOT, "include", name)).read()
    header = read("lic360_hip_gdn_grad.h")
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        for other in ("lic360_hip.h", "lic360_hip_grad.h"):
            assert not re.search(r"\b%s\b" % name, read(other)), (name, other)
    assert ABI_GDN_GRAD == {"lic360_gdn_backward": BACKWARD, "lic360_gdn_backward_scratch_bytes": SCRATCH}
    assert len(ABI) == 167 and len(ABI_GRAD) == 2 and not set(ABI_GDN_GRAD) & (set(ABI) | set(ABI_GRAD))
    g = _gen()
    assert len(g.TABLES) == 3 and [t[2] for t in g.TABLES] == ["ABI", "ABI_GRAD", "ABI_GDN_GRAD"]
    for (hdr, out, name), table in zip(g.TABLES, (ABI, ABI_GRAD, ABI_GDN_GRAD)):
        assert g.parse(open(hdr).read()) == table, "run tools/gen_abi.py after editing %s" % hdr
        assert open(out).read() == g.render(table, os.path.basename(hdr), name), out
    assert g.TABLES[2][1].endswith("_abi_table_gdn_grad.py")
    raw = ctypes.CDLL(lic360.LIBRARY_PATH)                          # the built library itself, not the bound handle
    for name in NAMES:
        assert getattr(raw, name) is not None
        assert len(getattr(lic360._lib, name).argtypes) == len(ABI_GDN_GRAD[name][1])
    with pytest.raises(ctypes.ArgumentError):                       # bound with the range check: not truncated
        lic360._lib.lic360_gdn_backward_scratch_bytes(2 ** 40, 16, 4)
    for fn in ("gdn_backward", "gdn_backward_scratch_bytes", "gdn_forward"):
        assert callable(getattr(lic360, fn)), fn
    makefile = open(os.path.join(ROOT, "360-image-compression_amd", "csrc", "Makefile")).read()
    assert "gdn_grad_kernels.hip" in makefile and "lic360_hip_gdn_grad.h" in makefile


def test_scratch_bytes_is_positive_and_monotone():
    import lic360
    q = lic360._lib.lic360_gdn_backward_scratch_bytes
    assert q(1, 16, 1) == 64 + (16 * 16 + 16) * 4 and q(1, 48, 3) == 576 + (48 * 48 + 48) * 4      # the t-map, one split's partial and row sums
    assert q(1, 16, 33) == 16 * 33 * 4 + 2 * (16 * 16 + 16) * 4
    for case in gc.CASES + [gc.MODULE_CASE]:                                   # the restated geometry is the library's
        assert q(case.n, case.c, case.h * case.w) == gc.geometry(case).scratch_bytes == lic360.gdn_backward_scratch_bytes(case.n, case.c, case.h * case.w)
    sizes = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 8160, 8192, 8193, 16384, 16385, 100000, 134160)
    for c in gc.CHANNELS:
        for fixed, vary in ((lambda v: (v, c, 777)), "n"), ((lambda v: (3, c, v)), "p"):
            prev = 0
            for v in sizes:
                cur = q(*fixed(v))
                assert cur > prev, (vary, c, v, cur, prev)
                prev = cur
    for a in ((0, 192, 64), (2, 192, 0), (-1, 192, 64), (2, 192, -64), (2, 0, 64), (2, -16, 64), (2, 24, 64), (2, 80, 64), (2, 208, 64), (2, 256, 64),
              (2 ** 31 - 1, 192, 2 ** 40), (2, 192, 2 ** 62), (65536, 16, 2 ** 21), (1, 16, 2 ** 36)):
        assert q(*a) == 0, a                                                   # refused or empty
    assert q(1, 16, 2 ** 31) > 0                                               # 2^26 tiles: an offset past 2^31 elements is legal


def _host_buffers():
    """host addresses that are never read: every call below is refused, or is a no-op"""
    block = (ctypes.c_double * (1 << 16))()
    base = (ctypes.addressof(block) + 15) // 16 * 16
    return block, lambda i: ctypes.c_void_p(base + i * 65536)


def test_entry_refuses_before_any_launch():
    import lic360
    L = lic360._lib
    block, slot = _host_buffers()
    names = ("x", "gy", "gamma", "beta", "gx", "ggamma", "gbeta", "scratch")
    good = dict({k: slot(i) for i, k in enumerate(names)}, n=2, c=32, p=35, inverse=0)

    def call(**kw):
        a = dict(good, **kw)
        rc = L.lic360_gdn_backward(None, *[a[k] for k in names], a["n"], a["c"], a["p"], a["inverse"])
        return rc, L.lic360_last_error().decode()

    off = lambda k: ctypes.c_void_p(slot(7).value + k)
    for kw in (dict(x=None), dict(gy=None), dict(gamma=None), dict(beta=None), dict(scratch=None),                       # null required pointers
               dict(x=None, ggamma=None, gbeta=None), dict(gamma=None, gx=None),
               dict(ggamma=None), dict(gbeta=None), dict(gx=None, ggamma=None), dict(gx=None, gbeta=None),               # exactly one of the parameters' outputs
               dict(c=0), dict(c=-32), dict(c=24), dict(c=80), dict(c=112), dict(c=160), dict(c=208), dict(c=256),       # unsupported channel counts
               dict(n=0), dict(p=0), dict(n=-1), dict(p=-35), dict(n=0, gx=None), dict(p=0, ggamma=None, gbeta=None),    # nothing to sum while outputs are asked for
               dict(n=-1, gx=None, ggamma=None, gbeta=None), dict(p=-1, gx=None, ggamma=None, gbeta=None),
               dict(scratch=off(8)), dict(scratch=off(4)), dict(scratch=off(1)), dict(scratch=off(8), ggamma=None, gbeta=None),   # scratch off 16 bytes
               dict(n=2 ** 31 - 1, p=2 ** 40), dict(p=2 ** 62), dict(n=65536, c=16, p=2 ** 21), dict(n=1, c=16, p=2 ** 36)):     # counts that leave int or long
        rc, msg = call(**kw)
        assert rc == 2 and msg.startswith("bad argument"), (kw, rc, msg)
    for kw in (dict(n=0, gx=None, ggamma=None, gbeta=None), dict(gx=None, ggamma=None, gbeta=None),
               dict(n=0, x=None, gy=None, gamma=None, beta=None, gx=None, ggamma=None, gbeta=None, scratch=None)):
        rc, msg = call(**kw)                                                    # nothing asked for: no error, nothing launched
        assert rc == 0, (kw, rc, msg)
    del block


def test_gdn_takes_its_route():
    """constructing needs no device; an unknown route names both; both routes hold the same state"""
    import torch
    from lic360_operator import GDN
    import lic360_models as lm
    assert GDN.GRADS == ("library", "fused")
    assert GDN(32).grad == "library" and GDN(32, 0, True, grad="fused").grad == "fused" and GDN(32, 0, True, 1e-6, .1, 2 ** -18, "fused").inverse
    with pytest.raises(ValueError, match="'library'.*'fused'"):
        GDN(32, grad="native")
    a, b = GDN(48), GDN(48, grad="fused")
    assert list(a.state_dict()) == list(b.state_dict()) == ["beta", "gamma"]
    assert all(torch.equal(a.state_dict()[k].cpu(), b.state_dict()[k].cpu()) and a.state_dict()[k].shape == b.state_dict()[k].shape for k in a.state_dict())
    b.load_state_dict(a.state_dict())
    net = torch.nn.Sequential(GDN(16), torch.nn.Sequential(GDN(32, inverse=True), torch.nn.PReLU()), GDN(24))
    assert lm.set_gdn_grad(net, "fused") == 3 and [m.grad for m in net.modules() if isinstance(m, GDN)] == ["fused"] * 3
    assert lm.set_gdn_grad(net[1], "library") == 1 and [m.grad for m in net.modules() if isinstance(m, GDN)] == ["fused", "library", "fused"]
    assert lm.set_gdn_grad(torch.nn.PReLU(), "fused") == 0
    with pytest.raises(ValueError, match="'library'.*'fused'"):
        lm.set_gdn_grad(net, "native")
    assert [m.grad for m in net.modules() if isinstance(m, GDN)] == ["fused", "library", "fused"]      # a refused route changes nothing


def test_fused_route_leaves_cpu_tensors_on_the_composition():
    """under "fused" a CPU tensor, another dtype and an unsupported channel count take the composition, with the library route's values and gradients"""
    import torch
    from lic360_operator import GDN
    for ch, dtype in ((16, torch.float32), (16, torch.float64), (24, torch.float32)):
        torch.manual_seed(ch)
        mods = {g: GDN(ch, grad=g).cpu().to(dtype) for g in GDN.GRADS}
        mods["fused"].load_state_dict(mods["library"].state_dict())
        x0 = torch.randn(2, ch, 5, 7, dtype=dtype)
        res = {}
        for g, m in mods.items():
            x = x0.clone().requires_grad_(True)
            y = m(x)
            y.square().sum().backward()
            res[g] = (y.detach(), x.grad, m.gamma.grad, m.beta.grad)
        for a, b in zip(res["library"], res["fused"]):
            assert torch.equal(a, b)
