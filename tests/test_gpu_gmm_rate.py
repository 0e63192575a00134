"""The fused GMM rate loss on the GPU (csrc/gmm_rate_kernels.hip; cases, reference and tolerances in tests/gmm_rate_cases.py, their CPU side in
tests/test_gmm_rate_cases_cpu.py).  Kernels: map and the gradients bit for bit the reference's, symbols equal, nats within the bound of a double
sum in any fixed order and the same bits on every call; every output carved from a canary-guarded, sentinel-filled allocation
(gpu_support.Arena), the scratch poisoned.  Modules: GmmRateLoss's two routes against the float64 statement of the head, the
fallbacks, and lic360_models.EntropyNet2 under both heads."""
import numpy as np
import pytest
import torch

import gmm_rate_cases as gc
from gpu_support import SENTINEL, Arena, differing, host, lic, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

F = np.float32
assert SENTINEL[torch.float32] == float(gc.UNWRITTEN)


def operands(ar, case):
    d = gc.inputs(case)
    t = {k: ar.put(d[k], case.offset) for k in ("logit", "sigma", "mean", "label")}
    t["mask"] = None if d["mask"] is None else ar.put(d["mask"], case.offset)
    t["grad"] = ar.put(d["grad"])
    return t


# ---------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: "%s-%s_%s" % (c.id, gc.form(c), gc.instantiation(c)))
def test_forward(lic, case):
    ref = gc.reference(case)
    ar = Arena()
    t = operands(ar, case)
    shape = (case.N, case.G, case.H, case.W)
    runs = []
    for with_map in (True, False):
        nats, symbols = ar.new((case.N,), dtype=torch.float64), ar.new((case.N,), dtype=torch.int64)
        mp = ar.new(shape, case.offset) if with_map else None
        scratch = ar.new((lic.gmm_rate_scratch_bytes(*shape),), dtype=torch.uint8)                 # poisoned: the sentinel byte
        out = lic.gmm_rate(t["logit"], t["sigma"], t["mean"], t["label"], t["mask"], ngroup=case.G, nats=nats, symbols=symbols, map=mp, scratch=scratch)
        assert len(out) == (3 if with_map else 2)
        ar.check()
        runs.append((host(nats), host(symbols), None if mp is None else host(mp)))
    nats, symbols, mp = runs[0]
    assert same_bits(mp, ref["map"]), "%d of %d map cells differ" % (differing(mp, ref["map"]), mp.size)
    assert np.array_equal(symbols, ref["symbols"]) and np.array_equal(runs[1][1], ref["symbols"])
    err, bound = np.abs(nats - ref["nats"]), gc.nats_bound(ref)
    print("%s: |nats - fsum| %s, bound %s" % (case.id, err.tolist(), bound.tolist()))
    assert (err <= bound).all()
    assert same_bits(nats, runs[1][0]), "nats differ between two calls"
    for k in ("logit", "sigma", "mean", "label"):                                                   # the inputs are read only
        assert same_bits(host(t[k]), gc.inputs(case)[k])


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: "%s-%s_%s" % (c.id, gc.form(c), gc.instantiation(c)))
def test_backward(lic, case):
    ref = gc.reference(case)
    ar = Arena()
    t = operands(ar, case)
    wide, narrow = (case.N, case.G * case.ng, case.H, case.W), (case.N, case.G, case.H, case.W)
    for need_label in (True, False):
        out = tuple(ar.new(wide, case.offset) for _ in range(3)) + (ar.new(narrow, case.offset) if need_label else None,)
        spare = ar.new(narrow, case.offset)                                                         # a fourth buffer the call is not given
        got = lic.gmm_rate_backward(t["logit"], t["sigma"], t["mean"], t["label"], t["mask"], t["grad"], need_label=need_label, ngroup=case.G, out=out)
        ar.check()
        for k, g in zip(("d_logit", "d_sigma", "d_mean", "d_label"), got):
            if g is None:
                assert k == "d_label" and not need_label
                continue
            g = host(g)
            assert same_bits(g, ref[k]), "%s (d_label %s): %d of %d elements differ, %d left unwritten" % (
                k, need_label, differing(g, ref[k]), g.size, int((g == gc.UNWRITTEN).sum()))
        assert (host(spare) == gc.UNWRITTEN).all()


def test_wrappers_allocate_what_they_are_not_given(lic):
    case = gc.BY_ID["r_2x4x6x8_ng3_ones"]
    ref, d = gc.reference(case), gc.inputs(case)
    t = {k: torch.from_numpy(np.array(d[k])).cuda() for k in ("logit", "sigma", "mean", "label", "mask", "grad")}
    nats, symbols, mp = lic.gmm_rate(t["logit"], t["sigma"], t["mean"], t["label"], t["mask"], return_map=True)
    assert nats.dtype == torch.float64 and symbols.dtype == torch.int64 and same_bits(host(mp), ref["map"]) and np.array_equal(host(symbols), ref["symbols"])
    got = lic.gmm_rate_backward(t["logit"], t["sigma"], t["mean"], t["label"], t["mask"], t["grad"])
    assert got[3] is None and all(same_bits(host(g), ref[k]) for g, k in zip(got, ("d_logit", "d_sigma", "d_mean")))
    for bad in (dict(logit=t["logit"][:, :-1]), dict(sigma=t["sigma"].double()), dict(mask=t["mask"][:1]), dict(label=t["label"].cpu())):
        with pytest.raises(lic.Lic360Error):
            lic.gmm_rate(**dict(dict(logit=t["logit"], sigma=t["sigma"], mean=t["mean"], label=t["label"], mask=t["mask"]), **bad))


# ---------------------------------------------------------------------------------------------------- GmmRateLoss
def module_pass(route, case, t, label_grad=True, **kw):
    """one recording pass of GmmRateLoss on leaf copies of the operands -> dict of numpy results (gradients of sum_n grad[n] nats[n])"""
    from lic360_operator import GmmRateLoss
    mod = GmmRateLoss(case.G, case.ng, route)
    leaf = {k: t[k].detach().clone().requires_grad_(k != "label" or label_grad) for k in ("logit", "sigma", "mean", "label")}
    out = mod(leaf["logit"], leaf["sigma"], leaf["mean"], leaf["label"], t["mask"], **kw)
    (out[0] * t["grad"].to(out[0].dtype)).sum().backward()
    got = dict(nats=host(out[0]), symbols=host(out[1]), map=host(out[2]) if len(out) > 2 else None)
    for k in leaf:
        got["d_" + k] = None if leaf[k].grad is None else host(leaf[k].grad)
    return got


@pytest.mark.parametrize("case", gc.REGULAR, ids=lambda c: c.id)
def test_module_routes_against_float64(lic, case):
    """both routes within twice the recorded distance of the reference from the float64 statement (the margin test_gpu_ops_edges.py gives the GPU
    over the CPU measurement, for the same reason: a different expf -- here torch.softmax's in the library route); the fused route's worst gradient
    error no larger than twice the library route's on the same inputs"""
    ar = Arena()
    t = operands(ar, case)
    fused, library = module_pass("fused", case, t), module_pass("library", case, t)
    ar.check()
    tol, tol_n = gc.F64_TOL[case.id]
    ref = gc.reference(case)
    assert np.array_equal(fused["symbols"], ref["symbols"]) and np.array_equal(library["symbols"], ref["symbols"])
    assert fused["nats"].dtype == np.float64 == library["nats"].dtype and fused["symbols"].dtype == np.int64 == library["symbols"].dtype
    (wf, nf, _, scale), (wl, nl, _, _) = gc.f64_distance(case, fused), gc.f64_distance(case, library)
    print("%s: against float64, gradients fused %.3g library %.3g (recorded %.3g, scale %.3g); nats fused %.3g library %.3g (recorded %.3g)" % (
        case.id, wf, wl, tol, scale, nf, nl, tol_n))
    for k in ("d_logit", "d_sigma", "d_mean", "d_label"):                                           # the fused route is the kernels' bits
        assert same_bits(fused[k], ref[k]), k
    assert wf <= 2 * tol and wl <= 2 * tol
    assert nf <= 2 * tol_n and nl <= 2 * tol_n
    assert wf <= 2 * wl


def test_module_without_label_gradient(lic):
    case = gc.BY_ID["r_2x4x6x8_ng5_stair"]
    t = operands(Arena(), case)
    a, b = module_pass("fused", case, t, label_grad=False), module_pass("fused", case, t)
    assert a["d_label"] is None and b["d_label"] is not None
    assert all(same_bits(a[k], b[k]) for k in ("nats", "symbols", "d_logit", "d_sigma", "d_mean"))


def test_module_no_grad_call_is_the_plain_entry(lic):
    from lic360_operator import GmmRateLoss
    case = gc.BY_ID["r_2x2x25x45_ng3_runs64"]
    t, ref = operands(Arena(), case), gc.reference(case)
    mod = GmmRateLoss(case.G, case.ng)
    nats, symbols, mp = mod(t["logit"], t["sigma"], t["mean"], t["label"], t["mask"], return_map=True)
    assert not nats.requires_grad and same_bits(host(mp), ref["map"]) and np.array_equal(host(symbols), ref["symbols"])
    with torch.no_grad():
        leaf = t["logit"].clone().requires_grad_(True)
        again = mod(leaf, t["sigma"], t["mean"], t["label"], t["mask"])
    assert same_bits(host(again[0]), host(nats))
    lib = GmmRateLoss(case.G, case.ng, "library")(t["logit"], t["sigma"], t["mean"], t["label"], t["mask"], return_map=True)
    assert np.array_equal(host(lib[1]), ref["symbols"]) and lib[2].shape == mp.shape and not host(lib[2])[~ref["coded"]].any()


@pytest.mark.parametrize("kind", ("non_contiguous", "float64", "map_while_recording", "cpu"))
def test_module_fallbacks_take_the_library_route(lic, kind):
    """what the fused route does not take goes through the library composition and agrees with route="library" exactly"""
    case = gc.BY_ID["r_2x4x6x8_ng3_ones"]
    d = gc.inputs(case)
    t = {k: torch.from_numpy(np.array(d[k])).cuda() for k in ("logit", "sigma", "mean", "label", "mask", "grad")}
    kw = {}
    if kind == "non_contiguous":
        t["logit"] = t["logit"].permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
        assert not t["logit"].is_contiguous()
    elif kind == "float64":
        t = {k: v.double() for k, v in t.items()}
    elif kind == "cpu":
        t = {k: v.cpu() for k, v in t.items()}
    else:
        kw = dict(return_map=True)
    a, b = module_pass("fused", case, t, **kw), module_pass("library", case, t, **kw)
    for k in a:
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or same_bits(a[k], b[k])), k
    assert a["d_logit"] is not None and (a["map"] is not None) == (kind == "map_while_recording")
    if kind == "float64":
        assert a["d_logit"].dtype == np.float64
    # and it is the library's arithmetic, not the kernel's: torch.softmax rounds differently from lic360_softmax_inplace somewhere in 384 rows
    worst = gc.f64_distance(case, {k: v for k, v in a.items() if k.startswith("d_")})[0]
    assert worst <= 2 * gc.F64_TOL[case.id][0]


def test_double_backward_raises(lic):
    from lic360_operator import GmmRateLoss
    case = gc.BY_ID["r_2x4x6x8_ng3_ones"]
    d = gc.inputs(case)
    t = {k: torch.from_numpy(np.array(d[k])).cuda() for k in ("logit", "sigma", "mean", "label", "mask")}
    t["logit"].requires_grad_(True)
    nats, _ = GmmRateLoss(case.G, case.ng, "fused")(t["logit"], t["sigma"], t["mean"], t["label"], t["mask"])
    (g,) = torch.autograd.grad(nats.sum(), t["logit"], create_graph=True)
    with pytest.raises(RuntimeError):                                     # once_differentiable: the gradient carries no graph
        g.sum().backward()


# ---------------------------------------------------------------------------------------------------- EntropyNet2
NET_G, NET_CPN, NET_SHAPE = 4, 4, (2, 4, 6, 10)
# MEASURED on this graph (MI355X), filled in from a run of test_entropy_net_rate_under_both_heads, which prints every figure again.
# nats: the library head against the float64 statement on the same nets' outputs, 2.69e-4 (the fused head: 2.69e-4) at nats of 375 and 392 -- the
# untrained nets leave most symbols at p of a few percent, where fp32's Phi_b - Phi_a shows; recorded rounded up, both heads get twice that.
NET_NATS_TOL = 2.7e-4
# parameter gradients, max |a - b| / max |b| per parameter: the library head run to run 0 (bit-identical), the fused head against the library head
# 7.31e-7.  The heads' gradients of the nets' outputs differ by a few fp32 roundings (F64_TOL: 2e-7 .. 4e-6 at scales 1 .. 16), and twelve
# layers of library convolutions, whose algorithm -- and with it the order of their sums -- may differ from box to box, carry that to the
# parameters: 64 fp32 roundings, 64 * 2^-24 = 3.8e-6, five times the measured figure.
NET_GRAD_RTOL = 3.8e-6


@pytest.fixture(scope="module")
def net(lic):
    import lic360_models
    torch.manual_seed(20)
    return lic360_models.EntropyNet2(NET_G, NET_CPN).to("cuda:0")


def net_inputs():
    rng = np.random.default_rng(77)
    n, g, h, w = NET_SHAPE
    x = (rng.integers(0, 8, NET_SHAPE) - 3.5).astype(F)
    L = rng.integers(0, g + 1, (n, 1, h, w))
    L[:, :, 0, 0] = g
    mask = (np.arange(g)[None, :, None, None] < L).astype(F)
    return torch.from_numpy(x).cuda(), torch.from_numpy(mask).cuda()


def test_entropy_net_state_dict_is_what_the_codec_drivers_consume(net):
    import lic360_codec
    expected = set()
    for prefix in ("ent.weight_net", "ent.delta_net", "ent.mean_net"):
        expected |= {key[len("ent."):] for key in lic360_codec._key_map(prefix).values()}
    assert set(net.state_dict().keys()) == expected
    assert float(net.delta_net[7].bias.detach().min()) == 2.0 == float(net.delta_net[7].bias.detach().max())


def net_pass(net, head, x, mask):
    net.head.route = head
    net.zero_grad(set_to_none=True)
    leaf = x.clone().requires_grad_(True)
    nats, symbols = net.rate(leaf, mask)
    assert ("GmmRateFn" in type(nats.grad_fn).__name__) == (head == "fused")                      # the head the route names did run
    nats.sum().backward()
    grads = {k: host(p.grad).astype(np.float64) for k, p in net.named_parameters()}
    grads["x"] = host(leaf.grad).astype(np.float64)
    return host(nats), host(symbols), grads


def rel_spread(a, b):
    """max over the parameters of max|a - b| / max|b|"""
    return max(float(np.abs(a[k] - b[k]).max()) / max(float(np.abs(b[k]).max()), 1e-30) for k in b)


def test_entropy_net_rate_under_both_heads(net):
    x, mask = net_inputs()
    lib1, lib2, fused = net_pass(net, "library", x, mask), net_pass(net, "library", x, mask), net_pass(net, "fused", x, mask)
    with torch.no_grad():
        logit, sigma, mean, tx = net._nets(x)
        f64 = gc.head_f64_torch(logit.double().cpu(), sigma.double().cpu(), mean.double().cpu(), tx.double().cpu(), mask.double().cpu(), None, NET_G, 3)[0].numpy()
    dn_l, dn_f = float(np.abs(lib1[0] - f64).max()), float(np.abs(fused[0] - f64).max())
    run, route = rel_spread(lib2[2], lib1[2]), rel_spread(fused[2], lib1[2])
    print("EntropyNet2 %s: nats %s; against float64 library %.3g fused %.3g; parameter gradients, relative: library run to run %.3g, fused to library %.3g" % (
        NET_SHAPE, lib1[0].tolist(), dn_l, dn_f, run, route))
    assert np.array_equal(lib1[1], fused[1]) and np.array_equal(lib1[1], host((mask >= 0.5).reshape(NET_SHAPE[0], -1).sum(1)))
    assert set(fused[2]) == set(lib1[2]) and all(np.isfinite(v).all() and v.any() for v in fused[2].values())
    assert dn_l <= 2 * NET_NATS_TOL and dn_f <= 2 * NET_NATS_TOL
    assert run <= NET_GRAD_RTOL and route <= NET_GRAD_RTOL


def test_entropy_net_forward_is_the_library_loss_vec(net):
    from lic360_operator import GmmRateLoss
    x, _ = net_inputs()
    for head in ("library", "fused"):
        net.head.route = head
        with torch.no_grad():
            vec = net(x)
            logit, sigma, mean, tx = net._nets(x)
            want = GmmRateLoss(NET_G, 3, "library")(logit, sigma, mean, tx, None, return_map=True)[2]
        assert vec.shape == (x.numel(),) and torch.equal(vec.view_as(want), want)
    net.head.route = "library"
