"""The backward of the one-pass GDN on the device (csrc/gdn_grad_kernels.hip, lic360.gdn_backward, autograd.GdnFn, GDN(grad="fused")), against
tests/gdn_grad_cases.py.
  * exact tier, every case: gx, the t-map (read back from the scratch), ggamma and gbeta bit for bit -- every sum of that tier is exact in fp32 in any order.
  * integer tier, every case: the t-map bit for bit the numpy fp32 restatement (so s is the forward's exact integer and the cell arithmetic has the stated
    order); gx, ggamma and gbeta within gdn_grad_cases.integer_bounds of the float64 result, the library composition's own distance printed beside it.
  * every operand and output carved from canaried allocations (gpu_support.Arena), the scratch of exactly the stated size: nothing is written outside them.
  * need_x / need_params skip their outputs, leave their buffers untouched and return the other's bits; two calls return identical bits.
  * the module: GDN(grad="fused") under recording returns lic360.gdn_forward's bits and gradients within twice the library route's distance from a float64
    reference on real data (the project's criterion for its fused routes); "library" never reaches gdn_backward; a down-sampling stage trains a step."""
import numpy as np
import pytest
import torch

import gdn_grad_cases as gc
from gpu_support import lic, dev, host, Arena, SENTINEL, same_bits, jitter      # noqa: F401

pytestmark = pytest.mark.gpu
IDS = [c.name for c in gc.CASES]
U8 = torch.uint8


def run(lic, case, data, need_x=True, need_params=True):
    """one call on canaried operands; dict of host arrays (None where not asked for), the buffers themselves under "_bufs" """
    c, p, off = case.c, case.h * case.w, (1 if case.misaligned else 0)
    shape = (case.n, c, case.h, case.w)
    ar = Arena()
    x, gy = ar.put(data["x"], off), ar.put(data["gy"], off)
    gamma, beta = ar.put(data["gamma"]), ar.put(data["beta"])
    gx, gg, gb = ar.new(shape, off), ar.new((c, c)), ar.new((c,))
    nbytes = lic.gdn_backward_scratch_bytes(case.n, c, p)
    assert nbytes == gc.geometry(case).scratch_bytes
    scratch = ar.new((nbytes,), 0, U8)
    assert (x.data_ptr() % 16 == 4) == case.misaligned and scratch.data_ptr() % 16 == 0
    got = lic.gdn_backward(x, gy, gamma, beta, case.inverse, need_x=need_x, need_params=need_params, out=(gx, gg, gb), scratch=scratch)
    ar.check()
    assert (got[0] is gx) == need_x and (got[1] is gg) == need_params and (got[2] is gb) == need_params and all(t is None or t is b for t, b in zip(got, (gx, gg, gb)))
    for t, a in ((x, data["x"]), (gy, data["gy"]), (gamma, data["gamma"]), (beta, data["beta"])):
        assert same_bits(host(t), a), "%s: an operand was written" % case.name
    tmap = host(scratch[:case.n * c * p * 4].view(torch.float32).view(shape)) if need_params else None
    return dict(gx=host(gx), ggamma=host(gg), gbeta=host(gb), t=tmap, scratch=host(scratch))


def describe(case, name, got, want):
    bad = np.argwhere(got != want)
    return "%s %s: %d of %d elements differ, first at %s: got %r, want %r" % (case.name, name, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("case", gc.CASES, ids=IDS)
def test_exact_tier_bit_for_bit(lic, case):
    data = gc.make_exact(case)
    gc.assert_exact_domain(case, data)
    want = gc.as_fp32(gc.reference(case, data, np.float32))
    got = run(lic, case, data)
    for k in ("t", "gx", "ggamma", "gbeta"):
        assert np.array_equal(got[k], want[k]), describe(case, k, got[k], want[k])
    again = run(lic, case, data)
    for k in ("t", "gx", "ggamma", "gbeta"):
        assert same_bits(again[k], got[k]), "%s %s: two calls differ" % (case.name, k)


@pytest.mark.parametrize("case", gc.CASES, ids=IDS)
def test_integer_tier_restatement_and_bounds(lic, case):
    data = gc.make_integer(case)
    t32 = gc.reference(case, data, np.float32)["t"].astype(np.float32)
    ref, bound = gc.reference(case, data, np.float64), gc.integer_bounds(case, data)
    got = run(lic, case, data)
    assert np.array_equal(got["t"], t32), describe(case, "t", got["t"], t32)
    # the library route on the same data, for the record
    x, gamma, beta = (dev(data[k]).requires_grad_(True) for k in ("x", "gamma", "beta"))
    gc.composition(x, gamma, beta, case.inverse).backward(dev(data["gy"]))
    lib = dict(gx=host(x.grad), ggamma=host(gamma.grad), gbeta=host(beta.grad))
    worst = {}
    for k in ("gx", "ggamma", "gbeta"):
        err, err_lib = np.abs(got[k].astype(np.float64) - ref[k]), np.abs(lib[k].astype(np.float64) - ref[k])
        worst[k] = float((err / np.maximum(bound[k], 1e-300)).max())
        print("%s %s: max |fused - f64| = %.3g (%.3g of its bound), max |library - f64| = %.3g, max |f64| = %.3g" % (
            case.name, k, err.max(), worst[k], err_lib.max(), np.abs(ref[k]).max()))
    for k, v in worst.items():
        assert v <= 1.0, "%s %s: %.3g times the fp32 summation bound" % (case.name, k, v)


@pytest.mark.parametrize("case", [c for c in gc.CASES if c.name in ("b16_p35", "b64_misaligned", "b192_p777_n3", "b16_more_tiles_than_splits")], ids=lambda c: c.name)
def test_need_flags_skip_their_outputs(lic, case):
    data = gc.make_integer(case)
    full = run(lic, case, data)
    only_x = run(lic, case, data, need_params=False)
    only_p = run(lic, case, data, need_x=False)
    sent = np.float32(SENTINEL[torch.float32])
    assert same_bits(only_x["gx"], full["gx"]) and np.all(only_x["ggamma"] == sent) and np.all(only_x["gbeta"] == sent)
    assert np.all(only_x["scratch"] == SENTINEL[U8]), "%s: the scratch was written without need_params" % case.name
    assert same_bits(only_p["ggamma"], full["ggamma"]) and same_bits(only_p["gbeta"], full["gbeta"]) and same_bits(only_p["t"], full["t"])
    assert np.all(only_p["gx"] == sent)
    none = run(lic, case, data, need_x=False, need_params=False)
    assert np.all(none["gx"] == sent) and np.all(none["ggamma"] == sent) and np.all(none["scratch"] == SENTINEL[U8])


def test_own_buffers_and_operand_checks(lic):
    case = gc.CASES[4]                                                      # 32 channels, three images, P = 66
    data = gc.make_exact(case)
    want = gc.as_fp32(gc.reference(case, data, np.float32))
    x, gy, gamma, beta = (dev(data[k]) for k in ("x", "gy", "gamma", "beta"))
    got = lic.gdn_backward(x, gy, gamma, beta, case.inverse)                # its own outputs and scratch
    for k, t in zip(("gx", "ggamma", "gbeta"), got):
        assert np.array_equal(host(t), want[k]), describe(case, k, host(t), want[k])
    gamma_t = gamma.t().contiguous().t()                                    # strided parameters are copied, as in gdn_forward
    assert not gamma_t.is_contiguous() and all(torch.equal(a, b) for a, b in zip(lic.gdn_backward(x, gy, gamma_t, beta, case.inverse), got))
    assert lic.gdn_backward(x, gy, gamma, beta, need_params=False)[1:] == (None, None) and lic.gdn_backward(x, gy, gamma, beta, need_x=False)[0] is None
    nbytes = lic.gdn_backward_scratch_bytes(case.n, case.c, case.h * case.w)
    scratch = torch.empty(nbytes + 16, dtype=U8, device="cuda:0")
    bad = [dict(x=x.cpu()), dict(x=x.double()), dict(x=x[:, :, :, ::2]), dict(x=x[:, :24]), dict(x=x[:0]), dict(x=x[0, 0]),
           dict(gy=gy.cpu()), dict(gy=gy.double()), dict(gy=gy[:, :, :, :-1]), dict(gy=gy.transpose(2, 3)), dict(gy=None),
           dict(gamma=gamma[:, :-1]), dict(gamma=gamma.cpu()), dict(gamma=gamma.double()), dict(beta=beta[:-1]), dict(beta=beta.cpu()), dict(beta=None),
           dict(out=(torch.empty_like(x)[:, :, :-1], None, None)), dict(out=(None, torch.empty(case.c, case.c + 1, device="cuda:0"), None)),
           dict(out=(None, None, torch.empty(case.c, device="cuda:0", dtype=torch.float64))), dict(out=(torch.empty_like(x).cpu(), None, None)),
           dict(scratch=scratch[:nbytes - 16]), dict(scratch=scratch[4:]), dict(scratch=scratch.cpu()), dict(scratch=scratch[::2])]
    good = dict(x=x, gy=gy, gamma=gamma, beta=beta)
    for kw in bad:
        with pytest.raises(lic.Lic360Error):
            lic.gdn_backward(**dict(good, **kw))
    assert np.array_equal(host(lic.gdn_backward(x, gy, gamma, beta, case.inverse, scratch=scratch)[1]), want["ggamma"])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- the module
def _real(case, seed=5):
    g = torch.Generator().manual_seed(seed)
    shape = (case.n, case.c, case.h, case.w)
    return torch.randn(shape, generator=g) * 2.0, torch.randn(shape, generator=g) * 0.05


def _modules(case, inverse):
    from lic360_operator import GDN
    torch.manual_seed(11)
    mods = {k: jitter(GDN(case.c, 0, inverse, grad=k)) for k in GDN.GRADS}
    mods["fused"].load_state_dict(mods["library"].state_dict())
    return mods


def _step(mod, x0, gy):
    x = x0.clone().requires_grad_(True)
    mod.zero_grad(set_to_none=True)
    y = mod(x)
    y.backward(gy)
    return dict(y=y.detach(), x=x.grad, gamma=mod.gamma.grad, beta=mod.beta.grad)


@pytest.mark.parametrize("inverse", [False, True], ids=["gdn", "igdn"])
def test_module_fused_route_on_real_data(lic, inverse):
    case = gc.MODULE_CASE
    x0, gy = _real(case)
    mods = _modules(case, inverse)
    ref_mod = _modules(case, inverse)["library"].cpu().double()
    ref_mod.load_state_dict({k: v.cpu().double() for k, v in mods["library"].state_dict().items()})
    ref = _step(ref_mod, x0.double(), gy.double())
    res = {k: _step(m, x0.cuda(), gy.cuda()) for k, m in mods.items()}
    with torch.no_grad():
        m = mods["fused"]
        beta = m.beta.clamp_min(m.beta_bound) ** 2 - m.pedestal
        gamma = m.gamma.clamp_min(m.gamma_bound) ** 2 - m.pedestal
        assert torch.equal(res["fused"]["y"], lic.gdn_forward(x0.cuda(), gamma, beta, inverse)), "the recording forward is not gdn_forward's"
        assert torch.equal(m(x0.cuda()), res["fused"]["y"]), "the recording forward and the inference forward differ"
    dist = {}
    for k in ("x", "gamma", "beta"):
        dist[k] = {r: float((res[r][k].double().cpu() - ref[k]).abs().max()) for r in res}
        print("%s d%s: max |fused - f64| = %.3g, max |library - f64| = %.3g, max |f64| = %.3g" % (
            "igdn" if inverse else "gdn", k, dist[k]["fused"], dist[k]["library"], float(ref[k].abs().max())))
    for k, d in dist.items():
        assert d["fused"] <= 2 * d["library"], "d%s: fused %.3g from float64, library %.3g" % (k, d["fused"], d["library"])


def test_library_route_never_reaches_gdn_backward(lic, monkeypatch):
    calls = []
    real = lic.gdn_backward
    monkeypatch.setattr(lic, "gdn_backward", lambda *a, **k: (calls.append(a[0].shape), real(*a, **k))[1])
    case = gc.CASES[3]
    x0, gy = (t.cuda() for t in _real(case))
    mods = _modules(case, case.inverse)
    lib = _step(mods["library"], x0, gy)
    assert calls == []
    fused = _step(mods["fused"], x0, gy)
    assert calls == [x0.shape]
    for k in ("y", "x", "gamma", "beta"):
        assert float((fused[k] - lib[k]).abs().max()) <= 1e-4 * float(lib[k].abs().max()), k
    x = x0.clone().requires_grad_(True)                                     # a frozen module: only x needs a gradient, the parameters get none
    for prm in mods["fused"].parameters():
        prm.requires_grad_(False)
    mods["fused"](x).backward(gy)
    assert len(calls) == 2 and torch.equal(x.grad, fused["x"]) and mods["fused"].gamma.grad is not None


def test_down_stage_trains_a_step_on_both_routes(lic):
    import lic360_models as lm
    torch.manual_seed(3)
    x = torch.randn(1, 192, 36, 68, device="cuda:0")
    blocks = {}
    for k in ("library", "fused"):
        torch.manual_seed(4)
        blocks[k] = lm.ResidualBlockDown(192, 192, 0).to("cuda:0")
        assert lm.set_gdn_grad(blocks[k], k) == 1
    blocks["fused"].load_state_dict(blocks["library"].state_dict())
    after = {}
    for k, b in blocks.items():
        opt = torch.optim.SGD(b.parameters(), lr=1e-3)
        opt.zero_grad()
        b(x.clone()).square().mean().backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in b.parameters()), k
        opt.step()
        after[k] = {n: p.detach().clone() for n, p in b.named_parameters()}
    for n in after["library"]:
        assert torch.allclose(after["fused"][n], after["library"][n], rtol=1e-3, atol=1e-6), n
