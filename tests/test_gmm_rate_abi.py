"""The C entries of the fused GMM rate loss (include/lic360_hip.h, csrc/gmm_rate_kernels.hip) without a GPU: they are declared, bound with the
argument contract of the table and exported by the built library; the scratch query is positive and monotone; every refusal comes before
anything is launched; the modules take their keywords."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORWARD = ("c_int", ["c_void_p"] * 6 + ["c_int"] * 5 + ["c_void_p"] * 4)
BACKWARD = ("c_int", ["c_void_p"] * 7 + ["c_int"] * 5 + ["c_void_p"] * 4)
SCRATCH = ("c_long", ["c_int"] * 4)
NAMES = ("lic360_gmm_rate_scratch_bytes", "lic360_gmm_rate", "lic360_gmm_rate_backward")


def test_entries_are_declared_bound_and_exported():
    import lic360
    from lic360._abi_table import ABI
    header = open(os.path.join(ROOT, "include", "lic360_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert ABI["lic360_gmm_rate"] == FORWARD and ABI["lic360_gmm_rate_backward"] == BACKWARD and ABI["lic360_gmm_rate_scratch_bytes"] == SCRATCH
    raw = ctypes.CDLL(lic360.LIBRARY_PATH)                          # the built library itself, not the bound handle
    for name in NAMES:
        assert getattr(raw, name) is not None
        assert len(getattr(lic360._lib, name).argtypes) == len(ABI[name][1])
    assert callable(lic360.gmm_rate) and callable(lic360.gmm_rate_backward) and callable(lic360.gmm_rate_scratch_bytes)


def test_scratch_bytes_is_positive_and_monotone():
    import lic360
    q = lic360.gmm_rate_scratch_bytes
    assert q(1, 1, 1, 1) > 0 and q(8, 48, 64, 128) == 8 * 48 * 8 * 16           # a double and an int64 per workgroup of 1024 cells
    base = (2, 3, 40, 50)
    for k in range(4):
        prev = 0
        for v in (1, 2, 3, 7, 40, 50, 51, 52, 600, 5000):
            dims = list(base)
            dims[k] = v
            cur = q(*dims)
            assert cur > 0 and cur >= prev, (dims, cur, prev)
            prev = cur
        assert prev > q(*base)                                                   # and it does grow
    for dims in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (-1, 1, 1, 1), (1, 1, 1, -4), (65536, 65536, 65536, 65536),
                 (1, 1, 65536, 65536)):
        assert q(*dims) == 0, dims


def _host_buffers():
    """host addresses that are never read: every call below is refused, or has no symbol.  Slots of 64 KB, each larger than any buffer of the
    geometry used (n 2, g 3, 4 x 8, ng 3: at most 2 * 9 * 32 * 4 = 2304 bytes)"""
    block = (ctypes.c_double * (1 << 17))()
    base = (ctypes.addressof(block) + 15) // 16 * 16
    return block, lambda i: ctypes.c_void_p(base + i * 65536)


def test_forward_entry_refuses_before_any_launch():
    import lic360
    L = lic360._lib
    block, slot = _host_buffers()
    good = dict(logit=slot(0), sigma=slot(1), mean=slot(2), label=slot(3), mask=slot(4), n=2, g=3, h=4, w=8, ng=3, nats=slot(5), symbols=slot(6),
                map=slot(7), scratch=slot(8))

    def call(**kw):
        a = dict(good, **kw)
        rc = L.lic360_gmm_rate(None, a["logit"], a["sigma"], a["mean"], a["label"], a["mask"], a["n"], a["g"], a["h"], a["w"], a["ng"], a["nats"],
                               a["symbols"], a["map"], a["scratch"])
        return rc, L.lic360_last_error().decode()

    for kw in (dict(logit=None), dict(sigma=None), dict(mean=None), dict(label=None), dict(nats=None), dict(symbols=None), dict(scratch=None),   # null pointers
               dict(n=-1), dict(g=-3), dict(h=-4), dict(w=-8),                                                                                # negative dimensions
               dict(ng=0), dict(ng=17), dict(ng=-3),                                                                                          # ng outside 1 .. 16
               dict(n=0, ng=0), dict(n=0, ng=17),                                                                                             # ... also without a symbol
               dict(n=65536, g=65536, h=65536, w=65536), dict(h=65536, w=65536), dict(n=65536, g=65536, h=1024, w=1024),                      # products that overflow
               dict(n=2 ** 31 - 1, g=2 ** 31 - 1, h=2 ** 31 - 1, w=2 ** 31 - 1), dict(n=2 ** 20, g=2 ** 12, h=1, w=1),
               dict(scratch=ctypes.c_void_p(slot(8).value + 4))):                                                                             # scratch off 8 bytes
        rc, msg = call(**kw)
        assert rc == 2 and msg.startswith("bad argument"), (kw, rc, msg)
    for kw in (dict(n=0), dict(n=0, logit=None, nats=None, scratch=None)):                                                                    # no symbol: no error, nothing launched
        rc, msg = call(**kw)
        assert rc == 0, (kw, rc, msg)
    del block


def test_backward_entry_refuses_before_any_launch():
    import lic360
    L = lic360._lib
    block, slot = _host_buffers()
    good = dict(logit=slot(0), sigma=slot(1), mean=slot(2), label=slot(3), mask=slot(4), grad=slot(5), n=2, g=3, h=4, w=8, ng=3, d_logit=slot(6),
                d_sigma=slot(7), d_mean=slot(8), d_label=slot(9))

    def call(**kw):
        a = dict(good, **kw)
        rc = L.lic360_gmm_rate_backward(None, a["logit"], a["sigma"], a["mean"], a["label"], a["mask"], a["grad"], a["n"], a["g"], a["h"], a["w"], a["ng"],
                                        a["d_logit"], a["d_sigma"], a["d_mean"], a["d_label"])
        return rc, L.lic360_last_error().decode()

    for kw in (dict(logit=None), dict(sigma=None), dict(mean=None), dict(label=None), dict(grad=None), dict(d_logit=None), dict(d_sigma=None), dict(d_mean=None),
               dict(n=-1), dict(g=-3), dict(h=-4), dict(w=-8), dict(ng=0), dict(ng=17), dict(ng=-3), dict(n=0, ng=0),
               dict(n=65536, g=65536, h=65536, w=65536), dict(h=65536, w=65536), dict(n=65536, g=65536, h=1024, w=1024), dict(n=2 ** 20, g=2 ** 12, h=1, w=1)):
        rc, msg = call(**kw)
        assert rc == 2 and msg.startswith("bad argument"), (kw, rc, msg)
    for kw in (dict(n=0), dict(g=0), dict(h=0, logit=None, d_mean=None)):
        rc, msg = call(**kw)
        assert rc == 0, (kw, rc, msg)
    del block


def test_modules_take_their_keywords():
    """constructing needs no device; an unknown route names the routes"""
    from lic360_operator import GmmRateLoss
    import lic360_models
    assert GmmRateLoss.ROUTES == ("library", "fused")
    assert GmmRateLoss(4, route="library").route == "library" and GmmRateLoss(4, 5, "fused").route == "fused" and GmmRateLoss(4, 5, "fused").num_gaussian == 5
    with pytest.raises(ValueError, match="'library'.*'fused'"):
        GmmRateLoss(4, route="native")
    assert not list(GmmRateLoss(4).parameters()) and not GmmRateLoss(4).state_dict()          # the head adds nothing to a checkpoint
    net = lic360_models.EntropyNet2(4)
    assert net.head.route == "library" and lic360_models.EntropyNet2(4, head="fused").head.route == "fused"
    assert float(net.delta_net[7].bias.detach().min()) == 2.0 == float(net.delta_net[7].bias.detach().max()) and not float(net.weight_net[7].bias.detach().abs().max())
