"""The split-bf16 one-pass GDN (csrc/gdn_bf16x3.inc, lic360.gdn_bf16x3_forward) bit for bit on all ten k_gdn_b3<C, VEC> kernels: on the integer tiers of
tests/gdn_bf16x3_cases.py the three kept bf16 products add to one fp32 number, and the library's correctly rounded fp32 square root and division leave one
right output -- numpy's float32 x / sqrt(s) (x * sqrt(s) for the inverse).  Cells whose sum is a perfect square are compared first (an approximate square
root would still get those right), so that a failure says which of the two it is.  Plus: the pack's bytes, nothing outside `out` is written, the operand
checks, and the production shapes repeated on two streams."""
import numpy as np
import pytest
import torch

import gdn_bf16x3_cases as gc
from gpu_support import dev, lic  # noqa: F401

pytestmark = pytest.mark.gpu


def _off16(t, off):
    """the same values in a contiguous view that starts `off` floats past a 16-byte boundary (inside a larger sentinel buffer)"""
    buf = torch.full((t.numel() + 64,), gc.SENTINEL, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    v = buf[16 + off:16 + off + t.numel()].view(t.shape)
    v.copy_(t)
    return buf, v


def _dev(data):
    return tuple(dev(data[k]) for k in ("x", "gamma", "beta"))


@pytest.mark.parametrize("tier", gc.TIERS)
@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_gdn_bf16x3_is_exact(lic, case, tier):
    data = gc.make(case, tier)
    gc.assert_exact_domain(case, data)
    want = gc.reference(case, data)
    x, gamma, beta = _dev(data)
    if case.misaligned:
        keep, x = _off16(x, 1)
        assert x.is_contiguous() and x.data_ptr() % 16 == 4                 # taken as it is: no copy, the scalar-access kernels
    assert (x.numel() // (case.n * case.c) % 4 == 0 and x.data_ptr() % 16 == 0) == gc.branch_of(case)[1]
    got = lic.gdn_bf16x3_forward(x, lic.gdn_bf16x3_pack(gamma), beta, case.inverse).cpu().numpy()
    sq = gc.perfect_squares(data)
    assert np.array_equal(got[sq], want[sq]), "%s / %s: cells with an integer norm differ" % (case.name, tier)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s / %s: %d of %d cells differ, first (n, c, row, col) = %s: %r, expected %r" % (
        case.name, tier, len(bad), got.size, tuple(bad[0]), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))


@pytest.mark.parametrize("c", gc.CHANNELS)
def test_pack_bytes(lic, c):
    """the pack against the numpy restatement of its layout and rounding, on values with lo parts, ties and both signs"""
    rng = np.random.default_rng(c)
    gamma = (rng.standard_normal((c, c)) * 3).astype(np.float32)
    gamma[::3, ::5] = rng.integers(257, 512, gamma[::3, ::5].shape)         # integers of 256 .. 512: ties and exact values
    packed = lic.gdn_bf16x3_pack(dev(gamma))
    assert packed.dtype == torch.bfloat16 and packed.numel() == 2 * c * c and packed.data_ptr() % 16 == 0
    want = torch.from_numpy(gc.packed_layout(gamma)).bfloat16()             # (exact: the values are bf16 numbers)
    assert np.array_equal(want.float().numpy(), gc.packed_layout(gamma))
    assert np.array_equal(packed.cpu().view(torch.int16).numpy(), want.view(torch.int16).numpy())


@pytest.mark.parametrize("name", ["b32_odd_small", "b64_p65", "b96_vec", "b192_odd_n3", "b192_vec"])
@pytest.mark.parametrize("off", [0, 1])
def test_writes_nothing_outside_out(lic, name, off):
    """`out` a slice of a larger sentinel buffer, on a 16-byte boundary and 4 bytes past one: the slice is exact, the rest untouched"""
    case = next(c for c in gc.SMALL if c.name == name)
    data = gc.make(case, "both")
    x, gamma, beta = _dev(data)
    buf, out = _off16(torch.zeros_like(x), off)
    ret = lic.gdn_bf16x3_forward(x, lic.gdn_bf16x3_pack(gamma), beta, case.inverse, out=out)
    torch.cuda.synchronize()
    assert ret.data_ptr() == out.data_ptr()
    assert np.array_equal(out.cpu().numpy(), gc.reference(case, data))
    assert bool((buf[:16 + off] == gc.SENTINEL).all()) and bool((buf[16 + off + x.numel():] == gc.SENTINEL).all())


def test_operand_checks(lic):
    """a wrong `out`, pack or beta is an error before anything is launched, not a stray device access; `out` keeps its sentinel"""
    c = 32
    case = gc.GdnCase("checks", c, 2, 6, 10, False, False, False)
    data = gc.make(case, "both")
    x, gamma, beta = _dev(data)
    packed = lic.gdn_bf16x3_pack(gamma)
    good = lambda: torch.full(x.shape, 777.0, device="cuda:0")
    bad_outs = {"too small": torch.full((2, c, 6, 9), 777.0, device="cuda:0"), "too large": torch.full((2, c, 6, 11), 777.0, device="cuda:0"),
                "same size, other shape": torch.full((2, c, 10, 6), 777.0, device="cuda:0"), "float64": torch.full(x.shape, 777.0, device="cuda:0", dtype=torch.float64),
                "on the host": torch.full(x.shape, 777.0), "not contiguous": torch.full((2, c, 6, 20), 777.0, device="cuda:0")[..., ::2]}
    for what, out in bad_outs.items():
        with pytest.raises(lic.Lic360Error):
            lic.gdn_bf16x3_forward(x, packed, beta, False, out=out)
        torch.cuda.synchronize()
        assert bool((out == 777.0).all()), "out (%s) was written" % what
    bad_params = {"gamma itself": (gamma, beta), "a pack of another channel count": (lic.gdn_bf16x3_pack(torch.zeros((64, 64), device="cuda:0")), beta),
                  "a pack one value short": (packed[:-1], beta), "a float32 pack": (packed.float(), beta), "a pack on the host": (packed.cpu(), beta),
                  "a strided pack": (torch.zeros(4 * c * c, dtype=torch.bfloat16, device="cuda:0")[::2], beta),
                  "beta [c - 1]": (packed, beta[:-1]), "beta float64": (packed, beta.double()), "beta on the host": (packed, beta.cpu())}
    for what, (pk, bt) in bad_params.items():
        out = good()
        with pytest.raises(lic.Lic360Error):
            lic.gdn_bf16x3_forward(x, pk, bt, False, out=out)
        torch.cuda.synchronize()
        assert bool((out == 777.0).all()), "%s: out was written" % what
    with pytest.raises(lic.Lic360Error):
        lic.gdn_bf16x3_forward(x[..., ::2], packed, beta)
    x48 = torch.ones((1, 48, 4, 4), device="cuda:0")
    with pytest.raises(lic.Lic360Error):                                    # a channel count the form does not take: an error, not the fp32 kernel
        lic.gdn_bf16x3_forward(x48, packed, torch.ones(48, device="cuda:0"))
    for bad_gamma in (torch.zeros((48, 48), device="cuda:0"), torch.zeros((c, c + 1), device="cuda:0"), gamma.double(), gamma.cpu(), gamma.reshape(-1)):
        with pytest.raises(lic.Lic360Error):
            lic.gdn_bf16x3_pack(bad_gamma)
    # a strided gamma is copied by the pack; a view 4 bytes past a 16-byte boundary is legal for x and out; and the good call still runs
    want = gc.reference(case, data)
    gt = gamma.t().contiguous().t()
    assert not gt.is_contiguous()
    assert np.array_equal(lic.gdn_bf16x3_forward(x, lic.gdn_bf16x3_pack(gt), beta).cpu().numpy(), want)
    _, xo = _off16(x, 1)
    buf, out = _off16(torch.zeros_like(x), 1)
    assert np.array_equal(lic.gdn_bf16x3_forward(xo, packed, beta, out=out).cpu().numpy(), want)
    out = good()
    lic.gdn_bf16x3_forward(x, packed, beta, out=out)
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("case", gc.PRODUCTION, ids=lambda c: c.name)
def test_production_shapes_repeat_on_two_streams(lic, case):
    """each production case 20 times, alternating between two streams that run side by side: every output equals the reference"""
    data = gc.make(case, "both")
    want = dev(gc.reference(case, data))
    x, gamma, beta = _dev(data)
    packed = lic.gdn_bf16x3_pack(gamma)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.empty_like(x), torch.empty_like(x)]
    torch.cuda.synchronize()
    parts = [torch.zeros((), dtype=torch.int64, device="cuda:0") for _ in streams]
    for it in range(20):
        k = it % 2
        with torch.cuda.stream(streams[k]):
            outs[k].fill_(gc.SENTINEL)
            lic.gdn_bf16x3_forward(x, packed, beta, case.inverse, out=outs[k])
            parts[k] += (outs[k] != want).sum()
    torch.cuda.synchronize()
    wrong = int(parts[0]) + int(parts[1])
    assert wrong == 0, "%s: %d wrong cells over 20 runs" % (case.name, wrong)
