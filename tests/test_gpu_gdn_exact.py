"""The one-pass GDN (csrc/gdn_kernels.hip, lic360.gdn_forward) bit for bit on all fourteen k_gdn<CT, VEC> kernels: integer x, gamma and beta make
beta + sum_j gamma[i][j] x[j]^2 exact on the fp32 MFMA (tests/sconv_cases.py), and the library is built with -fno-fast-math, i.e. with hipcc's
correctly rounded fp32 square root and division, so the output must EQUAL numpy's float32 x / sqrt(s) (x * sqrt(s) for the inverse).  On the
cells whose sum is a perfect square the norm is an integer and equality would hold under an approximate square root as well; they are compared
first, so that a failure says which of the two it is.  Plus: nothing outside `out` is written; the operand checks of gdn_forward."""
import numpy as np
import pytest
import torch

import sconv_cases as sc
from gpu_support import dev, lic  # noqa: F401

pytestmark = pytest.mark.gpu


def _off16(t, off):
    """the same values in a contiguous view that starts `off` floats past a 16-byte boundary (inside a larger sentinel buffer)"""
    buf = torch.full((t.numel() + 64,), sc.SENTINEL, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    v = buf[16 + off:16 + off + t.numel()].view(t.shape)
    v.copy_(t)
    return buf, v


@pytest.mark.parametrize("case", sc.GDN_CASES, ids=lambda c: c.name)
def test_gdn_is_exact(lic, case):
    data = sc.gdn_make(case)
    sc.gdn_assert_exact_domain(case, data)
    want = sc.gdn_reference(case, data)
    x = dev(data["x"])
    if case.misaligned:
        keep, x = _off16(x, 1)
        assert x.is_contiguous() and x.data_ptr() % 16 == 4                 # gdn_forward takes such a view as it is: no copy, the scalar-access kernels
    assert (x.numel() // (case.n * case.c) % 4 == 0 and x.data_ptr() % 16 == 0) == sc.gdn_branch_of(case)[1]
    got = lic.gdn_forward(x, dev(data["gamma"]), dev(data["beta"]), case.inverse).cpu().numpy()
    sq = sc.gdn_perfect_squares(data)
    assert sq.any() and np.array_equal(got[sq], want[sq]), "%s: cells with an integer norm differ" % case.name
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d of %d cells differ, first (n, c, row, col) = %s: %r, expected %r" % (
        case.name, len(bad), got.size, tuple(bad[0]), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))


@pytest.mark.parametrize("name", ["g16_odd_small", "g48_p65", "g96_vec", "g192_odd_n3", "g192_vec"])
@pytest.mark.parametrize("off", [0, 1])
def test_gdn_writes_nothing_outside_out(lic, name, off):
    """`out` a slice of a larger sentinel buffer, on a 16-byte boundary and 4 bytes past one: the slice is exact, the rest untouched"""
    case = next(c for c in sc.GDN_SMALL if c.name == name)
    data = sc.gdn_make(case)
    x = dev(data["x"])
    buf, out = _off16(torch.zeros_like(x), off)
    ret = lic.gdn_forward(x, dev(data["gamma"]), dev(data["beta"]), case.inverse, out=out)
    torch.cuda.synchronize()
    assert ret.data_ptr() == out.data_ptr()
    assert np.array_equal(out.cpu().numpy(), sc.gdn_reference(case, data))
    assert bool((buf[:16 + off] == sc.SENTINEL).all()) and bool((buf[16 + off + x.numel():] == sc.SENTINEL).all())


def test_gdn_operand_checks(lic):
    """a wrong `out`, gamma or beta is an error before anything is launched, not a stray device access; `out` keeps its sentinel"""
    c = 32
    case = sc.GdnCase("checks", c, 2, 6, 10, False, False, False)
    data = sc.gdn_make(case)
    x, gamma, beta = (dev(data[k]) for k in ("x", "gamma", "beta"))
    good = lambda: torch.full(x.shape, 777.0, device="cuda:0")
    bad_outs = {"too small": torch.full((2, c, 6, 9), 777.0, device="cuda:0"), "too large": torch.full((2, c, 6, 11), 777.0, device="cuda:0"),
                "same size, other shape": torch.full((2, c, 10, 6), 777.0, device="cuda:0"), "float64": torch.full(x.shape, 777.0, device="cuda:0", dtype=torch.float64),
                "on the host": torch.full(x.shape, 777.0), "not contiguous": torch.full((2, c, 6, 20), 777.0, device="cuda:0")[..., ::2]}
    for what, out in bad_outs.items():
        with pytest.raises(lic.Lic360Error):
            lic.gdn_forward(x, gamma, beta, False, out=out)
        torch.cuda.synchronize()
        assert bool((out == 777.0).all()), "out (%s) was written" % what
    bad_params = {"gamma [c, c + 1]": (torch.zeros((c, c + 1), device="cuda:0"), beta), "gamma [c - 1, c - 1]": (torch.zeros((c - 1, c - 1), device="cuda:0"), beta),
                  "gamma [c * c]": (gamma.reshape(-1), beta), "gamma float64": (gamma.double(), beta), "gamma on the host": (gamma.cpu(), beta),
                  "beta [c - 1]": (gamma, beta[:-1]), "beta float64": (gamma, beta.double()), "beta on the host": (gamma, beta.cpu())}
    for what, (gm, bt) in bad_params.items():
        out = good()
        with pytest.raises(lic.Lic360Error):
            lic.gdn_forward(x, gm, bt, False, out=out)
        torch.cuda.synchronize()
        assert bool((out == 777.0).all()), "%s: out was written" % what
    with pytest.raises(lic.Lic360Error):
        lic.gdn_forward(x[..., ::2], gamma, beta)
    # strided parameters are copied, as before; a view 4 bytes past a 16-byte boundary is legal for x and out; and the good call still runs
    want = sc.gdn_reference(case, data)
    gt = gamma.t().contiguous().t()
    assert not gt.is_contiguous()
    assert np.array_equal(lic.gdn_forward(x, gt, beta).cpu().numpy(), want)
    _, xo = _off16(x, 1)
    buf, out = _off16(torch.zeros_like(x), 1)
    assert np.array_equal(lic.gdn_forward(xo, gamma, beta, out=out).cpu().numpy(), want)
    out = good()
    lic.gdn_forward(x, gamma, beta, out=out)
    assert np.array_equal(out.cpu().numpy(), want)


def test_the_module_reaches_the_kernel_at_a_production_shape(lic, monkeypatch):
    """lic360_operator.GDN without a recorded gradient calls gdn_forward with the whole padded map: the shape the production rows stand for"""
    import lic360_operator as lo
    seen = []
    real = lic.gdn_forward
    monkeypatch.setattr(lic, "gdn_forward", lambda x, *a, **k: (seen.append(tuple(x.shape)), real(x, *a, **k))[1])
    m = lo.GDN(192, 0, True).to("cuda:0")
    with torch.no_grad():
        y = m(torch.ones((1, 192, 68, 132), device="cuda:0"))
    assert seen == [(1, 192, 68, 132)] and tuple(y.shape) == (1, 192, 68, 132)
