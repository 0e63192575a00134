"""The native backward of the group-causal convolution on the device (csrc/cconv_wgrad_kernels.hip, lic360.cconv_wgrad / cconv_dgrad / cconv_forward,
MaskConv2(route="fused"), the `conv` keyword of the entropy nets), against tests/maskconv_grad_cases.py.
  * wgrad on integer operands: bit for bit the float64 sums (exact in fp32, so any order gives them), from a sentinel-filled buffer with a guard row on
    either side; masked taps +0.0; two calls and twenty launches on two streams give the same bits.
  * wgrad on trained-scale real operands: within gamma_K * sum |gy x| of the float64 sum of the same products, K = n h w: the fp32 bound of a sum of K
    terms in any order (an accumulator chain of a split rounds once per product, the finish adds the splits in double and rounds once: fewer than K
    roundings on any path).
  * dgrad: bit for bit R F oracle.cconv_ec(R F gy, w', 0) -- the identity runs on the kernel the codec evaluates.
  * MaskConv2 and the entropy nets on both routes against float64 statements on the CPU: the fused route lies within twice the library route's
    distance from float64 (the rule of GmmRateLoss's tests), every figure printed before it is held."""
import numpy as np
import pytest
import torch

import ce_rate_cases
import gmm_rate_cases
import maskconv_grad_cases as mc
import oracle as orc
from ops_edge_cases import GMM_MIN_P
from gpu_support import lic, dev, host, check_whole_output, frame_is_untouched, sentinel_call, repeat_on_two_streams      # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = float(F(7.7701e33))
ids = lambda c: c.id


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def describe(got, want):
    bad = np.argwhere(got != want)
    return "%d of %d elements differ, first at %s: got %r, want %r" % (len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


# ---------------------------------------------------------------------------------------------------- the weight gradient
def wgrad_into_frame(lic, case, x, gy):
    """call(out) for out [1, 1, nout + 2, channel * 25]: the gradient goes to rows 1 .. nout, a guard row stays on either side"""
    channel, nout = mc.channels(case)

    def call(out):
        lic.cconv_wgrad(x, gy, case.G, case.constrain, out=out[0, 0, 1:1 + nout].view(nout, channel, 5, 5))
        return out
    return call, (1, 1, nout + 2, channel * 25)


@pytest.mark.parametrize("case", mc.CASES, ids=ids)
def test_wgrad_integer_cases_bit_for_bit(lic, case):
    t, want = mc.inputs(case), mc.wgrad_reference(case)
    channel, nout = mc.channels(case)
    call, shape = wgrad_into_frame(lic, case, dev(t["x"]), dev(t["gy"]))
    got = sentinel_call(call, shape, SENTINEL)
    assert frame_is_untouched(got, 1, 1 + nout, 0, channel * 25, SENTINEL), "%s: a guard row was written" % case.id
    gw = got[0, 0, 1:1 + nout].reshape(nout, channel, 5, 5)
    check_whole_output(gw, want, describe)
    keep = mc.keep_mask(case.G, case.cin, case.cout, case.constrain)
    assert not bits(gw[~keep]).any(), "%s: a masked tap is not +0.0" % case.id
    again = sentinel_call(call, shape, SENTINEL)
    assert np.array_equal(bits(again), bits(got)), "%s: two calls differ" % case.id


def test_wgrad_from_its_own_buffers_and_empty_batches(lic):
    case = mc.BY_ID["g6_4x3_straddle"]
    t, want = mc.inputs(case), mc.wgrad_reference(case)
    channel, nout = mc.channels(case)
    x, gy = dev(t["x"]), dev(t["gy"])
    assert np.array_equal(host(lic.cconv_wgrad(x, gy, case.G, case.constrain)), want)
    nbytes = lic.cconv_wgrad_scratch_bytes(case.n, channel, nout, case.h, case.w, case.G, case.constrain)
    scratch = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda:0")                # poisoned: nothing is read before it is written
    assert np.array_equal(host(lic.cconv_wgrad(x, gy, case.G, case.constrain, scratch=scratch)), want)
    with pytest.raises(lic.Lic360Error):
        lic.cconv_wgrad(x, gy, case.G, case.constrain, scratch=scratch[:nbytes - 16])
    with pytest.raises(lic.Lic360Error):
        lic.cconv_wgrad(x, gy[:, :-1], case.G, case.constrain)
    with pytest.raises(lic.Lic360Error):
        lic.cconv_wgrad(x.cpu(), gy, case.G, case.constrain)
    empty = lic.cconv_wgrad(x[:0], gy[:0], case.G, case.constrain, out=torch.full((nout, channel, 5, 5), SENTINEL, device="cuda:0"))
    assert not bits(host(empty)).any()


def test_wgrad_repeats_on_two_streams(lic):
    case = mc.BY_ID["g6_4x3_straddle"]
    t, want = mc.inputs(case), mc.wgrad_reference(case)
    channel, nout = mc.channels(case)
    x, gy = dev(t["x"]), dev(t["gy"])
    repeat_on_two_streams(lambda out: lic.cconv_wgrad(x, gy, case.G, case.constrain, out=out), (nout, channel, 5, 5), want, SENTINEL, describe)


@pytest.mark.parametrize("case", mc.CASES, ids=ids)
def test_wgrad_real_valued_within_the_fp32_bound(lic, case):
    t = mc.real_inputs(case)
    got = host(lic.cconv_wgrad(dev(t["x"]), dev(t["gy"]), case.G, case.constrain)).astype(np.float64)
    exact, mag = mc.wgrad_f64(case, t["x"], t["gy"]), mc.wgrad_f64(case, t["x"], t["gy"], absolute=True)
    k = case.n * case.h * case.w
    err, bound = np.abs(got - exact), mc.gamma(k) * mag
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: K = %d, gamma_K = %.3g; max |got - exact| = %.3g, largest share of its bound %.3g" % (case.id, k, mc.gamma(k), float(err.max()), worst))
    assert (err <= bound).all(), "%s: %d elements past gamma_K * sum |gy x|" % (case.id, int((err > bound).sum()))
    keep = mc.keep_mask(case.G, case.cin, case.cout, case.constrain)
    assert not bits(got.astype(F)[~keep]).any() and got[keep].any()


# ---------------------------------------------------------------------------------------------------- data gradient and forward
@pytest.mark.parametrize("case", mc.CASES, ids=ids)
def test_dgrad_is_the_oracle_on_transformed_operands(lic, case):
    t = mc.inputs(case)
    got = lic.cconv_dgrad(dev(t["gy"]), dev(t["weight"]), case.G, case.constrain)
    assert got.is_contiguous() and tuple(got.shape) == (case.n, case.G * case.cin, case.h, case.w)
    check_whole_output(host(got), mc.dgrad_oracle(case, t["gy"], t["weight"]), describe)
    again = lic.cconv_dgrad(dev(t["gy"]), dev(t["weight"]), case.G, case.constrain)
    assert again.data_ptr() != got.data_ptr() and torch.equal(again, got)                     # caller-owned: the next call leaves it alone


def layer(case, route):
    import lic360_operator as lo
    t = mc.inputs(case)
    m = lo.MaskConv2(case.G, case.cin, case.cout, 5, case.constrain == 6, 0, False, route).to("cuda:0")
    with torch.no_grad():
        m.weight.copy_(dev(t["weight"]))
        m.bias.copy_(dev(t["bias"]))
    return m


@pytest.mark.parametrize("case", mc.CASES, ids=ids)
def test_forward_under_fused_is_the_oracle(lic, case):
    t, x = mc.inputs(case), mc.real_inputs(case)["x"]
    m = layer(case, "fused")
    with torch.no_grad():
        y = m(dev(x))
    check_whole_output(host(y), orc.cconv_ec(x, t["weight"], t["bias"], None, case.G, case.constrain), describe)
    rec = m(dev(x).requires_grad_(True))
    assert "MaskConvFn" in type(rec.grad_fn).__name__ and torch.equal(rec, y)
    lib = layer(case, "library")(dev(x).requires_grad_(True))
    assert "MaskConvFn" not in type(lib.grad_fn).__name__                                     # the default route is the library's convolution


# ---------------------------------------------------------------------------------------------------- MaskConv2 on both routes
def layer_f64(case):
    """the layer as mathematics on the CPU -> (y, dx, dw, db) in float64 for the real-valued x and gy"""
    t, r = mc.inputs(case), mc.real_inputs(case)
    x = torch.from_numpy(r["x"].astype(np.float64)).requires_grad_()
    w = torch.from_numpy(t["weight"].astype(np.float64)).requires_grad_()
    b = torch.from_numpy(t["bias"].astype(np.float64)).requires_grad_()
    y = mc.conv_f64(x, w, b, case.G, case.cin, case.cout, case.constrain)
    (y * torch.from_numpy(r["gy"].astype(np.float64))).sum().backward()
    return [v.detach().numpy() for v in (y, x.grad, w.grad, b.grad)]


def layer_pass(case, route, need_x=True):
    r = mc.real_inputs(case)
    m = layer(case, route)
    x = dev(r["x"]).requires_grad_(need_x)
    y = m(x)
    (y * dev(r["gy"])).sum().backward()
    return [None if v is None else host(v).astype(np.float64) for v in (y, x.grad, m.weight.grad, m.bias.grad)]


@pytest.mark.parametrize("case", mc.MODULE_CASES, ids=ids)
def test_maskconv2_routes_against_float64(lic, case, monkeypatch):
    keep = mc.keep_mask(case.G, case.cin, case.cout, case.constrain)
    want, lib, fused = layer_f64(case), layer_pass(case, "library"), layer_pass(case, "fused")
    assert not want[2][~keep].any()
    pick = lambda i, v: v[keep] if i == 2 else v
    dist = lambda got: [float(np.abs(pick(i, got[i]) - pick(i, want[i])).max()) for i in range(4)]
    d_lib, d_fused = dist(lib), dist(fused)
    for name, a, b, ref in zip(("output", "x.grad", "weight.grad at kept taps", "bias.grad"), d_fused, d_lib, want):
        print("%s %s: against float64 fused %.3g library %.3g (scale %.3g)" % (case.id, name, a, b, float(np.abs(ref).max())))
    for name, a, b in zip(("output", "x.grad", "weight.grad", "bias.grad"), d_fused, d_lib):
        assert a <= 2 * b, "%s %s: fused %g from float64, library %g" % (case.id, name, a, b)
    assert not bits(fused[2].astype(F)[~keep]).any()                                          # exact zeros at masked taps
    assert lib[2][~keep].any()                                                                # (the library route's dense gradient there: the documented difference)
    # the input's gradient is not computed when the input does not need one

    def refuse(*a, **k):
        raise AssertionError("cconv_dgrad ran for an input that needs no gradient")
    monkeypatch.setattr(lic, "cconv_dgrad", refuse)
    no_x = layer_pass(case, "fused", need_x=False)
    assert no_x[1] is None and np.array_equal(no_x[2], fused[2]) and np.array_equal(no_x[3], fused[3]) and np.array_equal(no_x[0], fused[0])


# ---------------------------------------------------------------------------------------------------- whole models
NET_SHAPE = (2, 9, 35)


def well_posed(net):
    """biases off zero and PReLU slopes at exactly 1.  A PReLU with another slope has a jump in its derivative at 0, and the two routes' forward bits differ
    by roundings: one pre-activation within 1e-6 of zero (among half a million; under the strict mask the first layer's output at (0, 0) is its bias, exactly 0
    as initialised) takes one branch on one route and the other in float64, which moves a bias gradient by 1 % and says nothing about either convolution.
    With slope 1 the derivative has no jump; every convolution, PReLU weight gradient, residual and head still runs."""
    from gpu_support import jitter
    jitter(net)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.PReLU):
                m.weight.fill_(1.0)
    return net


def net_grads(net, run):
    net.zero_grad(set_to_none=True)
    nats = run(net)
    nats.sum().backward()
    return host(nats).astype(np.float64), {k: host(p.grad).astype(np.float64) for k, p in net.named_parameters()}


def two_times_rule(what, net_fused, net_lib, run, f64):
    """net_lib: the same net and head with conv="library"; both hold the same parameters; f64(params) -> nats in float64 from float64 CPU copies of them"""
    from lic360_operator import MaskConv2
    net_lib.load_state_dict(net_fused.state_dict())
    nats_f, g_f = net_grads(net_fused, run)
    nats_l, g_l = net_grads(net_lib, run)
    params = {k: v.detach().double().cpu().requires_grad_() for k, v in net_fused.state_dict().items()}      # after a forward: masked weights
    nats64 = f64(params)
    nats64.sum().backward()
    keeps = {name + ".weight": mc.keep_mask(m.ngroup, m.weight.shape[1] // m.ngroup, m.weight.shape[0] // m.ngroup, m.constrain)
             for name, m in net_fused.named_modules() if isinstance(m, MaskConv2)}
    assert len(keeps) == sum(isinstance(m, MaskConv2) for m in net_lib.modules()) and set(g_f) == set(g_l) == set(params)
    worst = []
    for k in sorted(params):
        want = params[k].grad.numpy()
        sel = keeps.get(k, np.ones(want.shape, bool))
        a, b = float(np.abs(g_f[k][sel] - want[sel]).max()), float(np.abs(g_l[k][sel] - want[sel]).max())
        print("%s %s: gradient against float64 fused %.3g library %.3g (scale %.3g)" % (what, k, a, b, float(np.abs(want).max())))
        if k in keeps:
            assert not g_f[k][~sel].any(), (what, k)
        if a > 2 * b:
            worst.append((k, a, b))
    dn_f, dn_l = float(np.abs(nats_f - nats64.detach().numpy()).max()), float(np.abs(nats_l - nats64.detach().numpy()).max())
    print("%s: nats %s; against float64 fused %.3g library %.3g" % (what, nats_f.tolist(), dn_f, dn_l))
    assert not worst, "%s: fused further than twice the library's distance from float64: %s" % (what, worst)
    assert dn_f <= 2 * dn_l, (what, dn_f, dn_l)


def parent_forward(self, x):
    """MaskConv2.forward as it was before routes existed"""
    from lic360_operator.extras import _MaskConstrainFn
    self.weight.data = _MaskConstrainFn.apply(self.weight.data, self.op)
    return torch.nn.functional.conv2d(x, self.weight, self.bias, padding=self.pad)


def graph_of(t):
    """the autograd nodes behind t, by type name, in visiting order"""
    seen, order, todo = set(), [], [t.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        order.append(type(fn).__name__)
        todo.extend(nxt for nxt, _ in fn.next_functions)
    return order


def default_route_is_unchanged(what, default, state, run, lic, monkeypatch):
    """an object built without `conv` runs the code it ran before the keyword existed: no native cconv entry, the same autograd graph and the same bits
    forward as with MaskConv2.forward replaced by its earlier text.  (Gradients are not compared bit for bit: the library's convolution backward may
    choose another algorithm from one call to the next.)"""
    from lic360_operator import MaskConv2
    default.load_state_dict(state)
    assert all(m.route == "library" for m in default.modules() if isinstance(m, MaskConv2))

    def refuse(*a, **k):
        raise AssertionError("%s: a native cconv entry ran under the default route" % what)
    for name in ("cconv_forward", "cconv_dgrad", "cconv_wgrad"):
        monkeypatch.setattr(lic, name, refuse)
    now = run(default)
    now.sum().backward()
    monkeypatch.setattr(MaskConv2, "forward", parent_forward)
    before = run(default)
    monkeypatch.undo()
    assert torch.equal(now, before) and graph_of(now) == graph_of(before) and "MaskConvFnBackward" not in graph_of(now), what
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in default.parameters())


def test_entropy_net2_under_both_routes(lic, monkeypatch):
    import lic360_models as lm
    G, cpn, ng = 6, 4, 3
    torch.manual_seed(31)
    fused, lib = well_posed(lm.EntropyNet2(G, cpn, ng, conv="fused", head="fused").to("cuda:0")), lm.EntropyNet2(G, cpn, ng, head="fused").to("cuda:0")
    rng = np.random.default_rng(79)
    x = (rng.integers(0, 8, (NET_SHAPE[0], G) + NET_SHAPE[1:]) - 3.5).astype(F)
    x64 = torch.from_numpy(x.astype(np.float64))

    def head64(p, mask):
        outs = [mc.entropy_net_f64(p, x64, G, cpn, ng, pre) for pre in ("weight_net.", "delta_net.", "mean_net.")]
        return gmm_rate_cases.head_f64_torch(outs[0], outs[1], outs[2], x64, mask, None, G, ng)
    # coded: the symbols whose probability the fp32 heads resolve (Phi_b - Phi_a carries ~6e-8 in fp32: tests/ops_edge_cases.py GMM_MIN_P); the others are
    # masked out for both routes and for the float64 statement, so the three evaluate the same function
    with torch.no_grad():
        fused.rate(dev(x))                                                                     # masks the weights in place
        prob = head64({k: v.detach().double().cpu() for k, v in fused.state_dict().items()}, None)[2]
    mask64 = (prob >= 2 * GMM_MIN_P).to(torch.float64)
    print("EntropyNet2: %.1f %% of the symbols coded (p >= %g in float64)" % (100 * float(mask64.mean()), 2 * GMM_MIN_P))
    assert float(mask64.mean()) >= 0.25                                                     # enough symbols left to carry a gradient to every parameter
    mask = mask64.float().to("cuda:0")
    run = lambda net: net.rate(dev(x), mask)[0]
    f64 = lambda p: head64(p, mask64)[0]
    two_times_rule("EntropyNet2", fused, lib, run, f64)
    assert "MaskConvFnBackward" in graph_of(run(fused)) and "GmmRateFnBackward" in graph_of(run(fused))
    default_route_is_unchanged("EntropyNet2", lm.EntropyNet2(G, cpn, ng).to("cuda:0"), fused.state_dict(), run, lic, monkeypatch)


def test_entropy_net3_under_both_routes(lic, monkeypatch):
    import lic360_models as lm
    cpn, nvalue = 20, 6
    torch.manual_seed(32)
    fused, lib = well_posed(lm.EntropyNet3(1, cpn, nvalue, conv="fused").to("cuda:0")), lm.EntropyNet3(1, cpn, nvalue).to("cuda:0")
    rng = np.random.default_rng(80)
    x = rng.integers(0, nvalue + 1, (NET_SHAPE[0], 1) + NET_SHAPE[1:]).astype(F)
    run = lambda net: net.rate(dev(x))[0]
    calls = []
    real = lic.cconv_dgrad
    monkeypatch.setattr(lic, "cconv_dgrad", lambda gy, w, *a: calls.append(tuple(w.shape)) or real(gy, w, *a))

    def f64(p):
        x64 = torch.from_numpy(x.astype(np.float64))
        logit = mc.entropy_net_f64(p, x64 / ((nvalue - 1.0) / 2.0) - 1.0, 1, cpn, nvalue + 1, "net.")
        return ce_rate_cases.head_f64_torch(logit, x64, 1, nvalue + 1)[0]
    two_times_rule("EntropyNet3", fused, lib, run, f64)
    assert len(calls) == 11 and (cpn, 1, 5, 5) not in calls                                   # the first layer's input needs no gradient
    monkeypatch.undo()
    default_route_is_unchanged("EntropyNet3", lm.EntropyNet3(1, cpn, nvalue).to("cuda:0"), fused.state_dict(), run, lic, monkeypatch)
