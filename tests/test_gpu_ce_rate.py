"""The fused cross-entropy rate loss on the GPU (csrc/ce_rate_kernels.hip; cases, reference and tolerances in tests/ce_rate_cases.py, their CPU side
in tests/test_ce_rate_cases_cpu.py).  Kernels: map and d_logit bit for bit the reference's, symbols and invalid equal, nats within the bound of a
double sum in any fixed order and the same bits on every call; every output carved from a canary-guarded, sentinel-filled allocation
(gpu_support.Arena), the scratch poisoned.  Modules: CeRateLoss's two routes against the float64 statement of the head, the label
check, the fallbacks, and lic360_models.EntropyNet3 under both heads and beside the coder's own estimate."""
import math

import numpy as np
import pytest
import torch

import ce_rate_cases as cc
from gpu_support import SENTINEL, Arena, differing, host, lic, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

F = np.float32
assert SENTINEL[torch.float32] == float(cc.UNWRITTEN)


def operands(ar, case):
    d = cc.inputs(case)
    return dict(logit=ar.put(d["logit"], case.offset), label=ar.put(d["label"], case.offset), grad=ar.put(d["grad"]))


CASE_ID = lambda c: "%s-%s_%s" % (c.id, cc.form(c), cc.instantiation(c))


# ---------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("case", cc.CASES, ids=CASE_ID)
def test_forward(lic, case):
    ref, d = cc.reference(case), cc.inputs(case)
    ar = Arena()
    t = operands(ar, case)
    shape = (case.N, case.G, case.H, case.W)
    runs = []
    for with_map in (True, False):
        nats = ar.new((case.N,), dtype=torch.float64)
        symbols, invalid = ar.new((case.N,), dtype=torch.int64), ar.new((case.N,), dtype=torch.int64)
        mp = ar.new(shape, case.offset) if with_map else None
        scratch = ar.new((lic.ce_rate_scratch_bytes(*shape),), dtype=torch.uint8)                 # poisoned: the sentinel byte
        out = lic.ce_rate(t["logit"], t["label"], nclass=case.K, ngroup=case.G, nats=nats, symbols=symbols, invalid=invalid, map=mp, scratch=scratch)
        assert len(out) == (4 if with_map else 3) and out[0] is nats and out[1] is symbols and out[2] is invalid
        ar.check()
        runs.append((host(nats), host(symbols), host(invalid), None if mp is None else host(mp)))
    nats, symbols, invalid, mp = runs[0]
    assert not (mp == cc.UNWRITTEN).any(), "%d map cells left at the sentinel" % int((mp == cc.UNWRITTEN).sum())
    assert same_bits(mp, ref["map"]), "%d of %d map cells differ" % (differing(mp, ref["map"]), mp.size)
    for run in runs:
        assert np.array_equal(run[1], ref["symbols"]) and np.array_equal(run[2], ref["invalid"])
    err, bound = np.abs(nats - ref["nats"]), cc.nats_bound(ref)
    print("%s: |nats - fsum| %s, bound %s" % (case.id, err.tolist(), bound.tolist()))
    assert (err <= bound).all()
    assert same_bits(nats, runs[1][0]), "nats differ between two calls"
    assert same_bits(host(t["logit"]), d["logit"]) and same_bits(host(t["label"]), d["label"])    # the inputs are read only


@pytest.mark.parametrize("case", cc.CASES, ids=CASE_ID)
def test_backward(lic, case):
    ref, d = cc.reference(case), cc.inputs(case)
    ar = Arena()
    t = operands(ar, case)
    wide = (case.N, case.G * case.K, case.H, case.W)
    for _ in range(2):
        out, spare = ar.new(wide, case.offset), ar.new(wide, case.offset)                          # spare: a buffer the call is not given
        got = lic.ce_rate_backward(t["logit"], t["label"], t["grad"], nclass=case.K, ngroup=case.G, out=out)
        assert got is out
        ar.check()
        g = host(got)
        assert same_bits(g, ref["d_logit"]), "%d of %d elements differ, %d left unwritten" % (differing(g, ref["d_logit"]), g.size, int((g == cc.UNWRITTEN).sum()))
        assert (host(spare) == cc.UNWRITTEN).all()
    assert same_bits(host(t["logit"]), d["logit"]) and same_bits(host(t["label"]), d["label"]) and same_bits(host(t["grad"]), d["grad"])


def test_empty_batches_launch_nothing_and_zero_the_totals(lic):
    logit, label = torch.empty((2, 49, 0, 5), device="cuda:0"), torch.empty((2, 1, 0, 5), device="cuda:0")
    nats = torch.full((2,), 3.0, dtype=torch.float64, device="cuda:0")
    symbols, invalid = torch.full((2,), 7, dtype=torch.int64, device="cuda:0"), torch.full((2,), 7, dtype=torch.int64, device="cuda:0")
    lic.ce_rate(logit, label, nats=nats, symbols=symbols, invalid=invalid)
    assert not host(nats).any() and not host(symbols).any() and not host(invalid).any()
    assert lic.ce_rate_backward(logit, label, torch.ones(2, device="cuda:0")).shape == logit.shape


def test_wrappers_allocate_what_they_are_not_given(lic):
    case = cc.BY_ID["r_2x2x6x8_k49_mixed"]
    ref, d = cc.reference(case), cc.inputs(case)
    t = {k: torch.from_numpy(np.array(d[k])).cuda() for k in ("logit", "label", "grad")}
    nats, symbols, invalid, mp = lic.ce_rate(t["logit"], t["label"], return_map=True)
    assert nats.dtype == torch.float64 and symbols.dtype == torch.int64 == invalid.dtype and same_bits(host(mp), ref["map"])
    assert np.array_equal(host(symbols), ref["symbols"]) and np.array_equal(host(invalid), ref["invalid"])
    assert len(lic.ce_rate(t["logit"], t["label"])) == 3
    assert same_bits(host(lic.ce_rate_backward(t["logit"], t["label"], t["grad"])), ref["d_logit"])
    good = dict(logit=t["logit"], label=t["label"])
    for bad in (dict(logit=t["logit"][:, :-1]), dict(logit=t["logit"].double()), dict(label=t["label"][:1]), dict(label=t["label"].cpu()), dict(logit=t["logit"].cpu()),
                dict(label=t["label"].long()), dict(nclass=48), dict(ngroup=1), dict(nats=torch.empty(2, device="cuda:0")), dict(invalid=torch.empty(3, dtype=torch.int64, device="cuda:0")),
                dict(map=torch.empty((2, 2, 6, 9), device="cuda:0")), dict(scratch=torch.empty(8, dtype=torch.uint8, device="cuda:0")),
                dict(logit=t["logit"].transpose(2, 3).contiguous().transpose(2, 3))):
        with pytest.raises(lic.Lic360Error):
            lic.ce_rate(**dict(good, **bad))
    for bad in (dict(grad_nats=t["grad"].double()), dict(grad_nats=t["grad"][:1]), dict(grad_nats=t["grad"].cpu()), dict(out=torch.empty((2, 98, 6, 9), device="cuda:0")),
                dict(label=t["label"].cpu()), dict(nclass=7)):
        with pytest.raises(lic.Lic360Error):
            lic.ce_rate_backward(**dict(dict(good, grad_nats=t["grad"]), **bad))


# ---------------------------------------------------------------------------------------------------- CeRateLoss
def module_pass(route, case, t, check_labels=False, **kw):
    """one recording pass of CeRateLoss on a leaf copy of the logits -> dict of numpy results (gradient of sum_n grad[n] nats[n])"""
    from lic360_operator import CeRateLoss
    mod = CeRateLoss(case.G, case.K, route, check_labels=check_labels)
    leaf = t["logit"].detach().clone().requires_grad_(True)
    out = mod(leaf, t["label"], **kw)
    (out[0] * t["grad"].to(out[0].dtype)).sum().backward()
    return dict(nats=host(out[0]), symbols=host(out[1]), map=host(out[2]) if len(out) > 2 else None, d_logit=host(leaf.grad), fn=type(out[0].grad_fn).__name__)


def valid_only(case, t):
    """the operands of the case's valid-only variant (cc.valid_variant: every invalid label replaced by class 0, all the library route takes)"""
    var = cc.valid_variant(case)
    return dict(t, label=torch.from_numpy(np.array(cc.inputs(var)["label"])).cuda()), var


@pytest.mark.parametrize("case", cc.REGULAR, ids=lambda c: c.id)
def test_module_routes_against_float64(lic, case):
    """CeRateLoss against the float64 statement of the head (cc.head_f64), every figure printed before it is held.
    The fused route, on the case's own labels and on its valid-only variant (whose inputs the recorded figures of that variant were measured on):
    the gradient is the reference's bits, and elements and nats lie within twice the reference's recorded distances F64_TOL -- the margin
    test_gpu_gmm_rate.py gives the GPU over the CPU measurement.
    The library route, on the variant (torch raises on an invalid label): per element within twice F64_TOL as well; nats within twice its OWN recorded
    figure, cc.LIBRARY_NATS_TOL -- it does not meet twice the reference's (see there).  The fused route's worst element error is no larger than twice
    the library route's on the same inputs."""
    from lic360_operator import CeRateLoss
    ar = Arena()
    t = operands(ar, case)
    ref = cc.reference(case)
    own = module_pass("fused", case, t)
    assert own["fn"].startswith("CeRateFn") and same_bits(own["d_logit"], ref["d_logit"]) and np.array_equal(own["symbols"], ref["symbols"])
    assert own["nats"].dtype == np.float64 and own["symbols"].dtype == np.int64
    w_own, n_own = cc.f64_distance(case, own)
    tv, var = valid_only(case, t)
    got = {}
    for route in ("fused", "library"):
        got[route] = module_pass(route, var, tv)
        with torch.no_grad():
            got[route]["map"] = host(CeRateLoss(case.G, case.K, route)(tv["logit"], tv["label"], return_map=True)[2])
    ar.check()
    assert not got["library"]["fn"].startswith("CeRateFn") and got["fused"]["fn"].startswith("CeRateFn")
    assert same_bits(got["fused"]["d_logit"], cc.reference(var)["d_logit"]) and same_bits(got["fused"]["map"], cc.reference(var)["map"])
    per = case.G * case.H * case.W
    dist = {}
    for route, g in got.items():
        assert (g["symbols"] == per).all() and g["nats"].dtype == np.float64 and g["symbols"].dtype == np.int64
        dist[route] = cc.f64_distance(var, g)
    (tol, tol_n), (vtol, vtol_n), ltol_n = cc.F64_TOL[case.id], cc.F64_TOL[var.id], cc.LIBRARY_NATS_TOL[var.id]
    print("%s: against float64, own labels, fused: gradient %.3g (recorded %.3g) nats %.3g (recorded %.3g); valid-only: elements fused %.3g library %.3g "
          "(recorded %.3g), nats fused %.3g (recorded %.3g) library %.3g (recorded %.3g)" % (
              case.id, w_own, tol, n_own, tol_n, dist["fused"][0], dist["library"][0], vtol, dist["fused"][1], vtol_n, dist["library"][1], ltol_n))
    assert w_own <= 2 * tol and n_own <= 2 * tol_n
    assert dist["fused"][0] <= 2 * vtol and dist["fused"][1] <= 2 * vtol_n
    assert dist["library"][0] <= 2 * vtol and dist["library"][1] <= 2 * ltol_n
    assert dist["fused"][0] <= 2 * dist["library"][0]


def test_check_labels_raises_on_a_planted_class(lic):
    from lic360_operator import CeRateLoss
    case = cc.BY_ID["r_2x2x6x8_k49_mixed"]
    tv, _ = valid_only(case, {k: torch.from_numpy(np.array(v)).cuda() for k, v in cc.inputs(case).items() if k != "edges"})
    clean = CeRateLoss(case.G, case.K, "fused")(tv["logit"], tv["label"])
    assert len(clean) == 2 and (host(clean[1]) == case.G * case.H * case.W).all()
    planted = tv["label"].clone()
    planted[1, 0, 2, 3] = case.K
    with pytest.raises(IndexError):
        CeRateLoss(case.G, case.K, "fused")(tv["logit"], planted)
    with pytest.raises(IndexError):                                                              # ... in a recording pass as well
        CeRateLoss(case.G, case.K, "fused")(tv["logit"].clone().requires_grad_(True), planted)
    nats, symbols = CeRateLoss(case.G, case.K, "fused", check_labels=False)(tv["logit"], planted)
    assert host(symbols).tolist() == [case.G * case.H * case.W, case.G * case.H * case.W - 1]
    _, _, mp = CeRateLoss(case.G, case.K, "fused")(tv["logit"], tv["label"], return_map=True)
    assert host(nats)[0] == host(clean[0])[0] and abs(host(nats)[1] - (host(clean[0])[1] - float(host(mp)[1, 0, 2, 3]))) <= 1e-9 * host(clean[0])[1]


def test_module_no_grad_call_is_the_plain_entry(lic):
    from lic360_operator import CeRateLoss
    case = cc.BY_ID["r_2x1x15x19_k49_mixed"]
    t, ref = operands(Arena(), case), cc.reference(case)
    mod = CeRateLoss(case.G, case.K, "fused", check_labels=False)
    nats, symbols, mp = mod(t["logit"], t["label"], return_map=True)
    assert not nats.requires_grad and same_bits(host(mp), ref["map"]) and np.array_equal(host(symbols), ref["symbols"])
    with torch.no_grad():
        again = mod(t["logit"].clone().requires_grad_(True), t["label"])
    assert len(again) == 2 and same_bits(host(again[0]), host(nats))
    mod.route = "native"
    with pytest.raises(ValueError):
        mod(t["logit"], t["label"])
    with pytest.raises(ValueError):
        CeRateLoss(case.G, case.K + 1, "fused")(t["logit"], t["label"])


@pytest.mark.parametrize("kind", ("non_contiguous", "float64", "map_while_recording", "cpu"))
def test_module_fallbacks_take_the_library_route(lic, kind):
    """what the fused route does not take goes through the library composition and agrees with route="library" exactly"""
    case = cc.BY_ID["r_2x2x6x8_k49_mixed"]
    t, _ = valid_only(case, {k: torch.from_numpy(np.array(v)).cuda() for k, v in cc.inputs(case).items() if k != "edges"})
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
    assert not a["fn"].startswith("CeRateFn")
    for k in a:
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or k == "fn" or same_bits(a[k], b[k])), k
    assert a["d_logit"] is not None and (a["map"] is not None) == (kind == "map_while_recording")
    if kind == "float64":
        assert a["d_logit"].dtype == np.float64


def test_double_backward_raises(lic):
    from lic360_operator import CeRateLoss
    case = cc.BY_ID["r_2x2x6x8_k49_mixed"]
    d = cc.inputs(case)
    logit, label = torch.from_numpy(np.array(d["logit"])).cuda().requires_grad_(True), torch.from_numpy(np.array(d["label"])).cuda()
    nats, _ = CeRateLoss(case.G, case.K, "fused", check_labels=False)(logit, label)
    (g,) = torch.autograd.grad(nats.sum(), logit, create_graph=True)
    with pytest.raises(RuntimeError):                                     # once_differentiable: the gradient carries no graph
        g.sum().backward()
    assert label.grad is None


# ---------------------------------------------------------------------------------------------------- EntropyNet3
NET_CPN, NET_NVALUE, NET_SHAPE = 12, 6, (2, 1, 8, 12)
# MEASURED on this graph (MI355X), filled in from a run of test_entropy_net_rate_under_both_heads, which prints every figure again.
# nats: the library head against the float64 statement on the same net's output, 2.98e-6 (the fused head: 1.29e-6) at nats of 314 and 311; recorded
# rounded up, both heads get twice that -- against float64 and against each other.
NET_NATS_TOL = 3.0e-6
# parameter gradients, max |a - b| / max |b| per parameter, the fused head against the library head: the bound test_gpu_gmm_rate.py derives for the same
# twelve layers of library convolutions behind a head whose output gradients differ by a few fp32 roundings: 64 fp32 roundings
NET_GRAD_RTOL = 64 * 2.0 ** -24


@pytest.fixture(scope="module")
def net(lic):
    import lic360_models
    torch.manual_seed(21)
    return lic360_models.EntropyNet3(1, NET_CPN, NET_NVALUE).to("cuda:0")


def net_input():
    rng = np.random.default_rng(78)
    return torch.from_numpy(rng.integers(0, NET_NVALUE + 1, NET_SHAPE).astype(F)).cuda()


def net_pass(net, head, x):
    net.head.route = head
    net.zero_grad(set_to_none=True)
    leaf = x.clone().requires_grad_(True)
    nats, symbols = net.rate(leaf)
    assert ("CeRateFn" in type(nats.grad_fn).__name__) == (head == "fused")                       # the head the route names did run
    nats.sum().backward()
    assert leaf.grad is None or not host(leaf.grad).any()                                          # DropGrad(True): nothing reaches the input
    return host(nats), host(symbols), {k: host(p.grad).astype(np.float64) for k, p in net.named_parameters()}


def test_entropy_net_state_dict_is_what_the_codec_drivers_consume(net):
    import lic360_codec
    expected = {key[len("imp_ent."):] for key in lic360_codec._key_map("imp_ent.net").values()}
    assert set(net.state_dict().keys()) == expected
    driver_keys = list(lic360_codec._key_map("imp_ent.net").keys())          # an importance-map driver's state_dict keys (ImpEntEncoderFast / ImpEntDecoder)
    ckpt = {"imp_ent." + k: v for k, v in net.state_dict().items()}
    cast = lic360_codec.cast_imp_entropy_parameter(ckpt, {k: None for k in driver_keys})
    assert len(cast) == len(ckpt) == 35 and all(v is not None for v in cast.values())
    assert cast["net.6.weight"] is ckpt["imp_ent.net.7.weight"] and cast["net.3.conv2.relu"] is ckpt["imp_ent.net.4.net.3.weight"]
    assert cast["net.6.bias"].shape == (NET_NVALUE + 1,) and cast["net.0.weight"].shape == (NET_CPN, 1, 5, 5) and cast["net.6.weight"].shape == (NET_NVALUE + 1, NET_CPN, 5, 5)


def test_entropy_net_rate_under_both_heads(net):
    x = net_input()
    lib, fused = net_pass(net, "library", x), net_pass(net, "fused", x)
    with torch.no_grad():
        logit, label = net._net(x)
        f64 = cc.head_f64_torch(logit.double().cpu(), label.double().cpu(), 1, NET_NVALUE + 1)[0].numpy()
    dn_l, dn_f = float(np.abs(lib[0] - f64).max()), float(np.abs(fused[0] - f64).max())
    route = max(float(np.abs(fused[2][k] - lib[2][k]).max()) / max(float(np.abs(lib[2][k]).max()), 1e-30) for k in lib[2])
    print("EntropyNet3 %s: nats %s; against float64 library %.3g fused %.3g (tolerance %.3g); parameter gradients, relative, fused to library %.3g" % (
        NET_SHAPE, lib[0].tolist(), dn_l, dn_f, NET_NATS_TOL, route))
    per = NET_SHAPE[1] * NET_SHAPE[2] * NET_SHAPE[3]
    assert lib[1].tolist() == fused[1].tolist() == [per] * NET_SHAPE[0]
    assert set(fused[2]) == set(lib[2]) and all(np.isfinite(v).all() and v.any() for v in fused[2].values())
    assert dn_l <= 2 * NET_NATS_TOL and dn_f <= 2 * NET_NATS_TOL
    assert float(np.abs(fused[0] - lib[0]).max()) <= 2 * NET_NATS_TOL                             # rate under both heads agrees
    assert route <= NET_GRAD_RTOL
    net.head.route = "library"


def test_entropy_net_forward_is_the_library_loss_vec(net):
    from lic360_operator import CeRateLoss
    x = net_input()
    for head in ("library", "fused"):
        net.head.route = head
        with torch.no_grad():
            vec = net(x)
            logit, label = net._net(x)
            want = CeRateLoss(1, NET_NVALUE + 1, "library").loss_vec(logit, label)
        assert vec.shape == (x.numel(),) and torch.equal(vec, want)
    net.head.route = "library"


def test_entropy_net_rate_beside_the_coder_s_estimate(net):
    """prints, per image, how far both heads' bits lie from FusedImpCodec.estimate on the cast parameters -- the coder prices the symbols with
    tables quantised to 16 bits, the heads with the softmax itself; that distance is reported, not asserted.  Asserted: the two heads
    agree."""
    import lic360_codec
    from lic360_fused import FusedImpCodec
    x = net_input()
    heads = {}
    with torch.no_grad():
        for head in ("library", "fused"):
            net.head.route = head
            heads[head] = host(net.rate(x)[0]) / math.log(2.0)
    net.head.route = "library"
    ckpt = {"imp_ent." + k: v for k, v in net.state_dict().items()}           # (after a forward: MaskConv2 has masked its weights in place)
    keys = ["net.0"] + ["net.%d.conv%d" % (b, c) for b in range(1, 6) for c in (1, 2)] + ["net.6"]
    cast = lic360_codec.cast_imp_entropy_parameter(ckpt, {k + s: None for k in keys for s in (".weight", ".bias", ".relu") if k + s != "net.6.relu"})
    layers = [dict(w=cast[k + ".weight"], b=cast[k + ".bias"], a=cast.get(k + ".relu")) for k in keys]
    ic = FusedImpCodec(NET_SHAPE[2], NET_SHAPE[3], max_batch=NET_SHAPE[0], hidden_channels=NET_CPN, nsym=NET_NVALUE + 1)
    ic.load_layers(layers)
    est = np.asarray(ic.estimate(x).bits, np.float64)
    for i in range(NET_SHAPE[0]):
        print("EntropyNet3 image %d: coder's estimate %.4f bits; library head %.4f (%+.4f), fused head %.4f (%+.4f)" % (
            i, est[i], heads["library"][i], heads["library"][i] - est[i], heads["fused"][i], heads["fused"][i] - est[i]))
    assert np.abs(heads["fused"] - heads["library"]).max() <= 2 * NET_NATS_TOL / math.log(2.0)
