"""The C entries of the fused cross-entropy rate loss (include/lic360_hip.h, csrc/ce_rate_kernels.hip) without a GPU: they are declared, bound
with the argument contract of the table and exported by the built library; the scratch query is positive and monotone and 0 for refused or
empty arguments; every refusal comes before anything is launched; the modules take their keywords."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORWARD = ("c_int", ["c_void_p"] * 3 + ["c_int"] * 5 + ["c_void_p"] * 5)
BACKWARD = ("c_int", ["c_void_p"] * 4 + ["c_int"] * 5 + ["c_void_p"])
SCRATCH = ("c_long", ["c_int"] * 4)
NAMES = ("lic360_ce_rate_scratch_bytes", "lic360_ce_rate", "lic360_ce_rate_backward")


def test_entries_are_declared_bound_and_exported():
    import lic360
    from lic360._abi_table import ABI
    header = open(os.path.join(ROOT, "include", "lic360_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert ABI["lic360_ce_rate"] == FORWARD and ABI["lic360_ce_rate_backward"] == BACKWARD and ABI["lic360_ce_rate_scratch_bytes"] == SCRATCH
    assert len(ABI) == 167
    raw = ctypes.CDLL(lic360.LIBRARY_PATH)                          # the built library itself, not the bound handle
    for name in NAMES:
        assert getattr(raw, name) is not None
        assert len(getattr(lic360._lib, name).argtypes) == len(ABI[name][1])
    assert callable(lic360.ce_rate) and callable(lic360.ce_rate_backward) and callable(lic360.ce_rate_scratch_bytes)


def test_scratch_bytes_is_positive_and_monotone():
    import lic360
    q = lic360.ce_rate_scratch_bytes
    assert q(1, 1, 1, 1) == 24 and q(8, 1, 64, 128) == 8 * 32 * 24               # a double and two int64 per workgroup of 256 cells
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
        assert q(*dims) == 0, dims                                               # refused or empty


def _host_buffers():
    """host addresses that are never read: every call below is refused, or has no symbol.  Slots of 64 KB, each larger than any buffer of the
    geometry used (n 2, g 3, 4 x 8, k 49: at most 2 * 147 * 32 * 4 = 37632 bytes)"""
    block = (ctypes.c_double * (1 << 17))()
    base = (ctypes.addressof(block) + 15) // 16 * 16
    return block, lambda i: ctypes.c_void_p(base + i * 65536)


OVERFLOWS = (dict(n=65536, g=65536, h=65536, w=65536), dict(h=65536, w=65536), dict(n=65536, g=65536, h=1024, w=1024),
             dict(n=2 ** 31 - 1, g=2 ** 31 - 1, h=2 ** 31 - 1, w=2 ** 31 - 1), dict(n=2 ** 20, g=2 ** 12, h=1, w=1), dict(n=2 ** 27, g=2 ** 27, h=1, w=64))


def test_forward_entry_refuses_before_any_launch():
    import lic360
    L = lic360._lib
    block, slot = _host_buffers()
    good = dict(logit=slot(0), label=slot(1), n=2, g=3, h=4, w=8, k=49, nats=slot(2), symbols=slot(3), invalid=slot(4), map=slot(5), scratch=slot(6))

    def call(**kw):
        a = dict(good, **kw)
        rc = L.lic360_ce_rate(None, a["logit"], a["label"], a["n"], a["g"], a["h"], a["w"], a["k"], a["nats"], a["symbols"], a["invalid"], a["map"],
                              a["scratch"])
        return rc, L.lic360_last_error().decode()

    for kw in (dict(logit=None), dict(label=None), dict(nats=None), dict(symbols=None), dict(invalid=None), dict(scratch=None),              # null pointers
               dict(n=-1), dict(g=-3), dict(h=-4), dict(w=-8),                                                                           # negative dimensions
               dict(k=0), dict(k=65), dict(k=-49),                                                                                       # k outside 1 .. 64
               dict(n=0, k=0), dict(n=0, k=65),                                                                                          # ... also without a symbol
               dict(h=0, nats=None), dict(w=0, symbols=None), dict(g=0, invalid=None),                                                   # no symbol, but images to zero
               dict(scratch=ctypes.c_void_p(slot(6).value + 4))) + OVERFLOWS:                                                           # scratch off 8 bytes; overflow
        rc, msg = call(**kw)
        assert rc == 2 and msg.startswith("bad argument"), (kw, rc, msg)
    for kw in (dict(n=0), dict(n=0, logit=None, label=None, nats=None, symbols=None, invalid=None, map=None, scratch=None)):             # no image: no error, nothing launched
        rc, msg = call(**kw)
        assert rc == 0, (kw, rc, msg)
    del block


def test_backward_entry_refuses_before_any_launch():
    import lic360
    L = lic360._lib
    block, slot = _host_buffers()
    good = dict(logit=slot(0), label=slot(1), grad=slot(2), n=2, g=3, h=4, w=8, k=49, d_logit=slot(3))

    def call(**kw):
        a = dict(good, **kw)
        rc = L.lic360_ce_rate_backward(None, a["logit"], a["label"], a["grad"], a["n"], a["g"], a["h"], a["w"], a["k"], a["d_logit"])
        return rc, L.lic360_last_error().decode()

    for kw in (dict(logit=None), dict(label=None), dict(grad=None), dict(d_logit=None), dict(n=-1), dict(g=-3), dict(h=-4), dict(w=-8), dict(k=0), dict(k=65),
               dict(k=-49), dict(n=0, k=0)) + OVERFLOWS:
        rc, msg = call(**kw)
        assert rc == 2 and msg.startswith("bad argument"), (kw, rc, msg)
    for kw in (dict(n=0), dict(g=0), dict(h=0, logit=None, d_logit=None), dict(w=0, label=None, grad=None)):
        rc, msg = call(**kw)
        assert rc == 0, (kw, rc, msg)
    del block


def test_modules_take_their_keywords():
    """constructing needs no device; an unknown route names the routes"""
    from lic360_operator import CeRateLoss
    import lic360_models
    assert CeRateLoss.ROUTES == ("library", "fused") and CeRateLoss(1, 49).route == "library"      # the default the probe's rule gives
    assert CeRateLoss(1, 49, route="library").route == "library" and CeRateLoss(2, 7, "fused").route == "fused" and CeRateLoss(2, 7).nclass == 7
    assert CeRateLoss(1, 49).check_labels is True and CeRateLoss(1, 49, check_labels=False).check_labels is False
    with pytest.raises(ValueError, match="'library'.*'fused'"):
        CeRateLoss(1, 49, route="native")
    assert not list(CeRateLoss(1, 49).parameters()) and not CeRateLoss(1, 49).state_dict()    # the head adds nothing to a checkpoint
    net = lic360_models.EntropyNet3(1, 12, 6)
    assert net.head.route == "library" and lic360_models.EntropyNet3(1, 12, 6, head="fused").head.route == "fused"
    assert net.head.nclass == 7 and net.scale == 2.5 and net.drop.drop == 0
    assert net.net[7].weight.shape[0] == 7 and all(k.startswith("net.") for k in net.state_dict())
