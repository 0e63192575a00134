"""k_cconv144 (csrc/cconv144_kernels.hip) against the oracle, bit for bit, at batches where its workgroups persist: more tasks than the 256
workgroups of a launch, so that a workgroup re-stages its x tile and carries the parity of its epilogue buffer into a next task, and decode-order
tasks of more than one output tile (og > 1), with the short last group and with two segments per anti-diagonal.  The cases and the launch
geometry they produce are in tests/cconv144_cases.py; tests/test_cconv144_cases_cpu.py asserts that they reach what is claimed here.
Calling convention and layouts as in tests/test_gpu_ops.py::test_cconv144_ec_bit_exact / test_cconv144_dc_planes_bit_exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import cconv144_cases as cc
import oracle as orc
from util import case_rng
from gpu_support import dev, host, lic  # noqa: F401

pytestmark = pytest.mark.gpu


class _Call(object):
    """one case, ready to launch: device operands, `launch(out, residual)` and `want(fill, residual)`, the expected whole output buffer.  The two
    cases that the repeat test runs as well are set up (and their oracle reference computed) once and shared; nothing writes to them."""
    _shared = {}

    @classmethod
    def of(cls, lic, kind, case):
        if (kind, case) in cls._shared:
            return cls._shared[(kind, case)]
        call = (_ec_call if kind == "ec" else _dc_call)(lic, case)
        if case in (cc.EC_REPEAT, cc.DC_REPEAT):
            cls._shared[(kind, case)] = call
        return call

    def done(self):
        """the plan of a case that is not shared goes with its test"""
        if self not in self._shared.values():
            self.destroy()


def _ec_call(lic, case):
    N, H, W, nout, act, ooff = case
    rng = case_rng(case)
    w, b, a, plan, packed = cc.i144_setup(lic, rng, nout, act)
    x = rng.standard_normal((N, 144, H, W)).astype(np.float32)
    x[rng.random(x.shape) < 0.1] = 0.0
    res = rng.standard_normal((N, nout, H, W)).astype(np.float32)
    ref = orc.cconv_ec(x, w, b, a, 1, 6)
    L = lic._lib
    hp, wp = C.c_int(), C.c_int()
    assert L.lic360_ec144_layout(H, W, C.byref(hp), C.byref(wp)) == 0
    hp, wp = hp.value, wp.value

    def pad(t, fill=0.0):
        return np.pad(t, ((0, 0), (0, 0), (2, hp - H - 2), (2, wp - W - 2)), constant_values=fill)
    call = _Call()
    xd, bd, ad = dev(pad(x)), dev(b), (dev(a) if act else None)
    if ooff:
        rd, call.shape, oplane, opitch = dev(pad(res)), (N, nout, hp, wp), hp * wp, wp
        call.want = lambda fill, residual=True: pad(ref + res if residual else ref, fill)
    else:
        rd, call.shape, oplane, opitch = dev(res), (N, nout, H, W), H * W, W
        call.want = lambda fill, residual=True: ref + res if residual else ref
    P = lic._p
    call.keep, call.destroy = (xd, bd, ad, rd, packed), lambda: L.lic360_conv_plan_destroy(plan)

    def launch(out, residual=True):
        assert L.lic360_cconv144_ec(lic._stream(0), plan, P(xd), P(packed), P(bd), P(ad), P(rd if residual else None), P(out), N, H, W, oplane, opitch, ooff) == 0, L.lic360_last_error()
    call.launch = launch
    call.describe = lambda got, want: cc.describe_ec_mismatch(case, got, want)
    return call


def _dc_call(lic, case):
    N, H, W, nout, act, _ = case
    planes = cc.dc_planes(case)
    rng = case_rng(case)
    w, b, a, plan, packed = cc.i144_setup(lic, rng, nout, act)
    x = rng.standard_normal((N, 144, H, W)).astype(np.float32)
    res = rng.standard_normal((N, nout, H, W)).astype(np.float32)
    L = lic._lib
    rows, pitch = C.c_int(), C.c_int()
    assert L.lic360_dc144_layout(H, W, C.byref(rows), C.byref(pitch)) == 0
    rows, pitch = rows.value, pitch.value
    th, tw = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")

    def skew(t, fill=0.0):
        o = np.full(t.shape[:2] + (rows, pitch), fill, np.float32)
        o[:, :, th + tw + cc.R0, th + cc.C0] = t
        return o
    # a decode-order plane depends on x alone: only the planes that are launched, on the kernel and on the oracle
    idx, pidx = orc.code_contex(H, W)
    ref = np.zeros((N, nout, H, W), np.float32)
    for s in planes:
        orc.cconv_dc_plane(x, w, b, a, ref, 1, 6, idx, pidx, s)
    on = np.isin(th + tw, planes)
    assert not ref[:, :, ~on].any() and on.sum() == sum(min(s, H - 1) - max(0, s - W + 1) + 1 for s in planes)
    call = _Call()
    xd, rd, bd, ad = dev(skew(x)), dev(skew(res)), dev(b), (dev(a) if act else None)
    call.shape = (N, nout, rows, pitch)

    def want(fill, residual=True):
        o = np.full(call.shape, fill, np.float32)
        o[:, :, (th + tw + cc.R0)[on], (th + cc.C0)[on]] = (ref + res if residual else ref)[:, :, on]
        return o
    call.want = want
    P = lic._p
    call.keep, call.destroy = (xd, rd, bd, ad, packed), lambda: L.lic360_conv_plan_destroy(plan)

    def launch(out, residual=True):
        for s in planes:
            assert L.lic360_cconv144_dc_plane(lic._stream(0), plan, P(xd), P(packed), P(bd), P(ad), P(rd if residual else None), P(out), N, H, W, s) == 0, L.lic360_last_error()
    call.launch = launch
    call.describe = lambda got, want: cc.describe_dc_mismatch(case, got, want)
    return call


@pytest.mark.parametrize("case", cc.EC_CASES, ids=cc.ec_id)
def test_cconv144_ec_persistent_bit_exact(lic, case):
    """encode order with more tasks than workgroups == oracle over the whole buffer; the halo of the haloed layout is still zero afterwards.
    The last layer also as the codec calls it: without a residual."""
    call = _Call.of(lic, "ec", case)
    for residual in (True,) if case[4] else (True, False):
        out = torch.zeros(call.shape, dtype=torch.float32, device="cuda:0")
        call.launch(out, residual)
        got, want = host(out), call.want(0.0, residual)
        assert np.array_equal(got, want), "residual %s: %s" % (residual, call.describe(got, want))
    call.done()


@pytest.mark.parametrize("case", cc.DC_CASES, ids=cc.dc_id)
def test_cconv144_dc_persistent_bit_exact(lic, case):
    """decode order, the case's planes only, into a buffer that starts as a finite sentinel: the launched anti-diagonals equal oracle + residual
    and every other float -- the other diagonals, the zero padding's cells, the pitch padding -- is still the sentinel"""
    call = _Call.of(lic, "dc", case)
    for residual in (True,) if case[4] else (True, False):
        out = torch.full(call.shape, cc.SENTINEL, dtype=torch.float32, device="cuda:0")
        call.launch(out, residual)
        got, want = host(out), call.want(cc.SENTINEL, residual)
        assert (want != cc.SENTINEL).sum() > 0 and (want == cc.SENTINEL).mean() > 0.5
        assert np.array_equal(got, want), "residual %s: %s" % (residual, call.describe(got, want))
    call.done()


@pytest.mark.parametrize("kind,case", [("ec", cc.EC_REPEAT), ("dc", cc.DC_REPEAT)], ids=lambda v: v if isinstance(v, str) else cc.ec_id(v))
def test_persistent_launches_repeat_bit_for_bit(lic, kind, case):
    """10 launches, alternately on two streams into two outputs refilled with the sentinel before each launch: every output equals the
    reference.  Determinism under ordinary use (as tests/test_gpu_sconv_exact.py::test_production_cases_repeat_bit_for_bit); stops at the
    first difference."""
    call = _Call.of(lic, kind, case)
    want = call.want(cc.SENTINEL)
    want_d = dev(want)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.empty(call.shape, dtype=torch.float32, device="cuda:0") for _ in streams]
    torch.cuda.synchronize()
    try:
        for rep in range(0, 10, 2):
            for k, s in enumerate(streams):
                with torch.cuda.stream(s):
                    outs[k].fill_(cc.SENTINEL)
                    call.launch(outs[k])
            for k, s in enumerate(streams):
                s.synchronize()
                if not torch.equal(outs[k], want_d):
                    pytest.fail("launch %d (stream %d): %s" % (rep + k, k, call.describe(host(outs[k]), want)))
    finally:
        torch.cuda.synchronize()
