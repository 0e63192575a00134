"""The backward of the fused viewport metrics (csrc/viewport_quality_kernels.hip; lic360.viewport_quality_coef / viewport_quality_backward;
lic360_operator.ViewportQuality(grad="fused")) against the fp32 restatement of tests/viewport_quality_grad_cases.py.  Both images are projected with
ProjectsOp.forward and the restatement runs on those views on the CPU.  Bit for bit: mse / ssim against the plain entry, the four coefficient maps
and the view gradients gva / gvb against the restatement.  The ERP gradients are float atomic sums in an order that is not fixed: per ERP cell they
lie within n_terms * 2^-24 * sum |products| of the float64 sum of the kernel's own fp32 products, the first-order bound of fp32 summation in any
order (derived, not measured), and a cell no view touches is exactly 0.  Plus: one side only, nearest sampling (a case), sentinel-filled buffers,
two streams, the module against a float64 reference, the refusal of a table that leaves the ERP."""
import ctypes

import numpy as np
import pytest
import torch

import viewport_quality_cases as vq
import viewport_quality_grad_cases as vg
from gpu_support import lic  # noqa: F401

pytestmark = pytest.mark.gpu
IDS = [c.name for c in vg.CASES]


def _op(lic, case):
    from lic360_operator import MultiProject
    return lic.ProjectsOp(case.view[0], case.view[1], list(MultiProject.THETAS), list(MultiProject.PHIS), case.fov, case.near, 0)


def _cpu(ts):
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


@pytest.fixture(scope="module")
def results(lic):
    """per case, computed once and left unchanged: device inputs, the projected views, the table, the restatement, the fused outputs (CPU)"""
    out = {}
    for case in vg.CASES:
        a, b = (torch.from_numpy(x).cuda() for x in vq.make_erp_pair(case))
        op, taps = _op(lic, case), vg.taps_of(case)
        assert op._table_inside(*case.erp)
        tf = op._coords(a, *case.erp).cpu().numpy()
        va, vb = op.forward(a)[0].cpu().numpy(), op.forward(b)[0].cpu().numpy()
        g_mse, g_ssim = (torch.from_numpy(g).cuda() for g in vg.upstream(case))
        plain = lic.viewport_quality(op, a, b, taps)
        mse, ssim, coefs = lic.viewport_quality_coef(op, a, b, taps)
        back = lic.viewport_quality_backward(op, a, b, taps, coefs, g_mse, g_ssim, return_views=True)
        ref_coefs = vg.ref_coefs(va, vb, taps)
        ref_views = vg.ref_view_grads(va, vb, taps, ref_coefs, *vg.upstream(case))
        sums = [vg.scatter_sums(tf, g, case.n, case.c, case.erp[0], case.erp[1], case.near) for g in ref_views]
        out[case.name] = dict(a=a, b=b, op=op, taps=taps, tf=tf, va=va, vb=vb, g_mse=g_mse, g_ssim=g_ssim, plain=_cpu(plain), mse=mse.cpu().numpy(),
                              ssim=ssim.cpu().numpy(), coefs_dev=coefs, coefs=_cpu(coefs), back=_cpu(back), ref_coefs=ref_coefs, ref_views=ref_views, sums=sums)
    torch.cuda.synchronize()
    return out


def _assert_within_summation_bound(grad, sums, what):
    """per ERP cell: |grad - float64 sum of the fp32 products| <= n_terms * 2^-24 * sum |products|; untouched cells exactly 0"""
    total, mag, count = sums
    err, bound = np.abs(grad.astype(np.float64) - total), count * 2.0 ** -24 * mag
    print("%s: %d of %d cells touched, up to %d terms; largest error / bound %.3g" % (
        what, int((count > 0).sum()), count.size, int(count.max()), float((err[bound > 0] / bound[bound > 0]).max())))
    assert (count > 0).any() and np.isfinite(grad).all()
    assert (err <= bound).all(), (what, np.argwhere(err > bound)[0], float(err.max()))
    assert (grad[count == 0] == 0).all()


@pytest.mark.parametrize("case", vg.CASES, ids=IDS)
def test_coef_entry_gives_the_plain_entrys_values_and_the_restated_maps(results, case):
    r = results[case.name]
    assert np.array_equal(r["mse"].view(np.uint32), r["plain"][0].view(np.uint32)) and np.array_equal(r["ssim"].view(np.uint32), r["plain"][1].view(np.uint32))
    for name, got, ref in zip(("Pa", "Pb", "Q", "R"), r["coefs"], r["ref_coefs"]):
        assert got.shape == ref.shape == (vq.NVIEW * case.n, case.c) + case.view and np.isfinite(ref).all() and np.ptp(ref) > 0
        diff = got != ref
        print("%s %s: cells that differ %d of %d" % (case.name, name, int(diff.sum()), diff.size))
        assert np.array_equal(got, ref), "%s: first differing cell %s: %r vs %r" % (name, np.argwhere(diff)[0], got[diff][0], ref[diff][0])


@pytest.mark.parametrize("case", vg.CASES, ids=IDS)
def test_view_gradients_match_the_restatement_bit_for_bit(results, case):
    r = results[case.name]
    for name, got, ref in zip(("gva", "gvb"), r["back"][2:], r["ref_views"]):
        assert np.isfinite(ref).all() and np.ptp(ref) > 0
        diff = got != ref
        print("%s %s: cells that differ %d of %d" % (case.name, name, int(diff.sum()), diff.size))
        assert np.array_equal(got, ref), "%s: first differing cell %s: %r vs %r" % (name, np.argwhere(diff)[0], got[diff][0], ref[diff][0])


@pytest.mark.parametrize("case", vg.CASES, ids=IDS)
def test_erp_gradients_lie_within_the_summation_bound(results, case):
    r = results[case.name]
    for name, got, sums in zip(("grad_a", "grad_b"), r["back"][:2], r["sums"]):
        assert got.shape == (case.n, case.c) + case.erp
        _assert_within_summation_bound(got, sums, "%s %s" % (case.name, name))


def test_outputs_do_not_depend_on_what_the_buffers_held(lic, results):
    """the C entries on caller-owned buffers filled with zeros and with the all-ones pattern (a NaN in every float): maps and view gradients bit for
    bit what the fixture got, the ERP gradients (zeroed by the entry, then summed with atomics) within the bound"""
    case = vg.CASES[1]
    r = results[case.name]
    n, c, (h, w), (ho, wo) = case.n, case.c, case.erp, case.view
    taps = (ctypes.c_float * len(r["taps"]))(*[float(t) for t in r["taps"]])
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    tf = r["op"]._coords(r["a"], h, w)
    for fill in (0x00, 0xFF):
        buf = lambda *shape: torch.full(shape + (4,), fill, dtype=torch.uint8, device="cuda:0").view(torch.float32).squeeze(-1)
        mse, ssim, scratch = buf(n, 14), buf(n, 14), torch.full((lic.viewport_quality_scratch_bytes(n, ho, wo),), fill, dtype=torch.uint8, device="cuda:0")
        coefs = [buf(14 * n, c, ho, wo) for _ in range(4)]
        rc = lic._lib.lic360_viewport_quality_coef(stream, p(r["a"]), p(r["b"]), p(tf), n, c, h, w, ho, wo, int(case.near), taps, len(taps), p(scratch), p(mse), p(ssim),
                                                   *[p(t) for t in coefs])
        assert rc == 0, lic._lib.lic360_last_error()
        ga, gb, gva, gvb = buf(n, c, h, w), buf(n, c, h, w), buf(14 * n, c, ho, wo), buf(14 * n, c, ho, wo)
        rc = lic._lib.lic360_viewport_quality_backward(stream, p(r["a"]), p(r["b"]), p(tf), n, c, h, w, ho, wo, int(case.near), taps, len(taps), *[p(t) for t in coefs],
                                                       p(r["g_mse"]), p(r["g_ssim"]), p(ga), p(gb), p(gva), p(gvb))
        assert rc == 0, lic._lib.lic360_last_error()
        for got, ref in zip([mse, ssim] + coefs + [gva, gvb], (r["mse"], r["ssim"]) + r["coefs"] + r["back"][2:]):
            assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32))
        for name, got, sums in zip(("grad_a", "grad_b"), (ga, gb), r["sums"]):
            _assert_within_summation_bound(got.cpu().numpy(), sums, "fill %#x %s" % (fill, name))


@pytest.mark.parametrize("case", [vg.CASES[1], vg.CASES[2]], ids=[vg.CASES[1].name, vg.CASES[2].name])
def test_one_side_only_gives_the_same_gradient_and_keeps_no_map_of_the_other(lic, results, case):
    r = results[case.name]
    for side in (0, 1):
        need = dict(need_a=side == 0, need_b=side == 1)
        mse, ssim, coefs = lic.viewport_quality_coef(r["op"], r["a"], r["b"], r["taps"], **need)
        assert coefs[1 - side] is None and coefs[side] is not None                   # no map of the other side was allocated
        assert np.array_equal(mse.cpu().numpy().view(np.uint32), r["mse"].view(np.uint32)) and np.array_equal(ssim.cpu().numpy().view(np.uint32), r["ssim"].view(np.uint32))
        for got, ref in zip(coefs, r["coefs"]):
            assert got is None or np.array_equal(got.cpu().numpy(), ref)
        back = lic.viewport_quality_backward(r["op"], r["a"], r["b"], r["taps"], coefs, r["g_mse"], r["g_ssim"], return_views=True, **need)
        assert back[1 - side] is None and back[3 - side] is None
        assert np.array_equal(back[2 + side].cpu().numpy(), r["ref_views"][side])
        _assert_within_summation_bound(back[side].cpu().numpy(), r["sums"][side], "%s side %d alone" % (case.name, side))
        with pytest.raises(lic.Lic360Error, match="kept no"):                          # the other side cannot be asked of these maps
            lic.viewport_quality_backward(r["op"], r["a"], r["b"], r["taps"], coefs, r["g_mse"], r["g_ssim"])


def test_two_streams_keep_their_own_results(lic, results):
    r1, r2 = results["partial_tiles"], results["production"]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    got = []
    for _ in range(3):
        for s, r in zip(streams, (r1, r2)):
            with torch.cuda.stream(s):
                mse, ssim, coefs = lic.viewport_quality_coef(r["op"], r["a"], r["b"], r["taps"])
                got.append((r, mse, ssim, coefs, lic.viewport_quality_backward(r["op"], r["a"], r["b"], r["taps"], coefs, r["g_mse"], r["g_ssim"], return_views=True)))
    torch.cuda.synchronize()
    for i, (r, mse, ssim, coefs, back) in enumerate(got):
        for x, ref in zip((mse, ssim) + tuple(coefs) + tuple(back[2:]), (r["mse"], r["ssim"]) + r["coefs"] + r["back"][2:]):
            assert np.array_equal(x.cpu().numpy().view(np.uint32), ref.view(np.uint32))
        for name, x, sums in zip(("grad_a", "grad_b"), back[:2], r["sums"]):
            _assert_within_summation_bound(x.cpu().numpy(), sums, "launch %d %s" % (i, name))


def _f64_module_grads(r, case, g_mse, g_ssim):
    """d loss / d (a, b) in float64 on the CPU: the views are index-only gathers of the ERP with the downloaded table's cells and (float64) weights,
    the metrics f64_quality's formula, the loss sum of upstream * value"""
    erp = [torch.tensor(x.cpu().numpy(), dtype=torch.float64, requires_grad=True) for x in (r["a"], r["b"])]
    terms = vg.sample_terms(r["tf"], case.erp[0], case.erp[1], case.near)
    views = []
    for x in erp:
        flat = x.reshape(case.n * case.c, -1)
        v = sum(flat[:, torch.from_numpy(idx)] * (1.0 if wgt is None else torch.from_numpy(wgt.astype(np.float64))) for idx, wgt in terms)       # [n c, 14, inner]
        views.append(v.permute(1, 0, 2).reshape((vq.NVIEW * case.n, case.c) + case.view))
    vg.torch_loss(*vg.torch_quality(views[0], views[1], r["taps"]), g_mse, g_ssim).backward()
    return [x.grad.numpy() for x in erp]


@pytest.mark.parametrize("case", vq.CASES, ids=[c.name for c in vq.CASES])
def test_module_with_fused_grad_is_as_close_to_float64_as_the_library_pass(lic, results, case, monkeypatch):
    """ViewportQuality(grad="fused") and (grad="library") in a recording pass, both against the float64 reference; the fused gradients may deviate
    4 times as far as the library pass does on the same case (largest absolute difference over the largest float64 gradient).  The fused pass
    launches no projection."""
    from lic360_operator import ViewportQuality
    r = results[case.name]
    calls = []
    forward = lic.ProjectsOp.forward
    monkeypatch.setattr(lic.ProjectsOp, "forward", lambda self, x: (calls.append(1), forward(self, x))[1])
    g_mse, g_ssim = vg.upstream(case)
    ref = _f64_module_grads(r, case, g_mse, g_ssim)
    scale = max(float(np.abs(x).max()) for x in ref)
    dev, values = {}, {}
    for mode in ("library", "fused"):
        q = ViewportQuality(case.view[0], case.view[1], case.fov, case.near, 0, window_size=case.window, grad=mode)
        a, b = r["a"].clone().requires_grad_(), r["b"].clone().requires_grad_()
        del calls[:]
        mse, ssim = q(a, b)
        ((r["g_mse"] * mse).sum() + (r["g_ssim"] * ssim).sum()).backward()
        assert (len(calls) == 0) == (mode == "fused") and (type(mse.grad_fn).__name__ == "ViewportQualityFnBackward") == (mode == "fused")
        dev[mode] = max(float(np.abs(t.grad.cpu().numpy().astype(np.float64) - x).max()) for t, x in zip((a, b), ref)) / scale
        values[mode] = (mse.detach().cpu().numpy(), ssim.detach().cpu().numpy())
    print("%s: deviation from float64 over the largest gradient (%.3e): library %.3e, fused %.3e" % (case.name, scale, dev["library"], dev["fused"]))
    assert np.array_equal(values["fused"][0].view(np.uint32), r["mse"].view(np.uint32)) and np.array_equal(values["fused"][1].view(np.uint32), r["ssim"].view(np.uint32))
    assert scale > 0 and dev["library"] > 0 and dev["fused"] <= 4 * dev["library"], dev


def test_module_routes_and_refusals(lic, results, monkeypatch):
    """"library" -> "fused" -> "library" on one module, and a module whose mode was never set, take the library path: two projection launches, no
    ViewportQualityFn node, and its values bit for bit (its gradients are the atomic sums of ProjectsOp.backward, which no two runs need share).
    One side recording differentiates one side.  return_map under recording stays on the library path.  A pole-touching table is refused in
    every fused form."""
    from lic360_operator import MultiProject, ViewportQuality
    case = vg.CASES[1]
    r = results[case.name]
    calls = []
    forward = lic.ProjectsOp.forward
    monkeypatch.setattr(lic.ProjectsOp, "forward", lambda self, x: (calls.append(1), forward(self, x))[1])

    def run(q, **kw):
        a = r["a"].clone().requires_grad_()
        del calls[:]
        out = q(a, r["b"], **kw)
        ((r["g_mse"] * out[0]).sum() + (r["g_ssim"] * out[1]).sum()).backward()
        return [t.detach().cpu().numpy() for t in out[:2]], a.grad.cpu().numpy(), len(calls), type(out[0].grad_fn).__name__

    q = ViewportQuality(case.view[0], case.view[1], case.fov, case.near, 0, window_size=case.window)
    never_set = ViewportQuality(case.view[0], case.view[1], case.fov, case.near, 0, window_size=case.window)
    del never_set.grad
    first = run(q)
    q.grad = "fused"
    fused = run(q)
    with_map = run(q, return_map=True)
    q.grad = "library"
    again, unset = run(q), run(never_set)
    assert fused[2] == 0 and fused[3] == "ViewportQualityFnBackward"
    _assert_within_summation_bound(fused[1], r["sums"][0], "module, side a alone")      # b does not record: only a is differentiated
    for other in (first, again, unset, with_map):
        assert other[2] == 2 and other[3] != "ViewportQualityFnBackward"
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(other[0], first[0]))
    q.grad = "neither"
    with pytest.raises(ValueError, match="'library'.*'fused'"):
        q(r["a"].clone().requires_grad_(), r["b"])
    one = results["one_tile"]
    op = lic.ProjectsOp(16, 16, list(MultiProject.THETAS), list(MultiProject.PHIS), 0.5, False, 0)
    assert not op._table_inside(32, 64)
    with pytest.raises(lic.Lic360Error, match="sample outside"):
        lic.viewport_quality_coef(op, one["a"], one["b"], one["taps"])
    with pytest.raises(lic.Lic360Error, match="sample outside"):
        lic.viewport_quality_backward(op, one["a"], one["b"], one["taps"], one["coefs_dev"], one["g_mse"], one["g_ssim"])
    with pytest.raises(lic.Lic360Error, match="sample outside"):
        ViewportQuality(16, 16, 0.5, False, 0, grad="fused")(one["a"].clone().requires_grad_(), one["b"])
    assert op._tf is None                                                             # nothing was uploaded for it
