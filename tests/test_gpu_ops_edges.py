"""The pointwise, table and projection ops on every dispatch path of their launchers (tests/ops_edge_cases.py; the CPU side of the
cases is tests/test_ops_edge_cases_cpu.py).  Each case runs through the drop-in ops of `lic360`.  Every buffer an op writes is carved
from a larger allocation with canary floats on both sides and pre-filled with a sentinel (gpu_support.Arena): the canaries must be intact after the launch,
and whatever an op leaves unwritten shows as the sentinel.  Equality with the CPU oracle wherever tests/test_gpu_ops.py demands it;
the float64 statements at the bounds derived or measured in ops_edge_cases.py."""
import numpy as np
import pytest
import torch

import oracle as orc
import ops_edge_cases as oe
from gpu_support import SENTINEL as _SENTINEL, Arena, host, lic  # noqa: F401

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = _SENTINEL[torch.float32]


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to("cuda:0")          # a copy: the cached case arrays are read-only


def written(a):
    return not np.any(a == F(SENTINEL))


# ---------------------------------------------------------------------------------------------------- quantiser
@pytest.mark.parametrize("case", oe.QUANT_CASES, ids=lambda c: "-".join((c.id,) + oe.which_kernel("quant", c)))
def test_quant_forward(lic, case):
    x, wb = oe.quant_inputs(case)
    rt, rq, rc = orc.quant(x, wb)
    N, C, H, W = case.shape
    a = Arena()
    op = lic.QuantOp(C, case.levels, 0.9, 100, 2, 0.1, 0, False)
    op._top = [a.new(case.shape, case.offset), a.new(case.shape, case.offset)]
    op.weight_, op.count_data_ = a.new((C, case.levels)), a.new((C, case.levels))
    top, qidx = op.forward(a.put(x, case.offset), dev(wb), dev(np.zeros((C, case.levels), F)), False)
    assert top is op._top[0] and qidx is op._top[1]
    a.check()
    assert np.array_equal(host(top), rt) and np.array_equal(host(qidx), rq)
    got = host(op.count_data_)
    print(case.id, "count", got[0].tolist())
    assert np.array_equal(got, rc) and np.array_equal(got, oe.count_histogram(rq, case.levels))
    assert np.array_equal(host(op.weight_), oe.quant_weights(wb))


@pytest.mark.parametrize("case", oe.DQUANT_CASES, ids=lambda c: "-".join((c.id,) + oe.which_kernel("dquant", c)))
def test_dquant(lic, case):
    q, mask, wb = oe.dquant_inputs(case)
    N, C, H, W = case.shape
    a = Arena()
    op = lic.DquantOp(C, case.levels, 0, False)
    op._top = [a.new(case.shape, case.offset)]
    op.weight_ = a.new((C, case.levels))
    out = op.forward(a.put(q, case.offset), a.put(mask, case.offset), dev(wb))[0]
    assert out is op._top[0]
    a.check()
    assert np.array_equal(host(out), orc.dquant(q, mask, wb))


@pytest.mark.parametrize("case", oe.QUANT_BWD_CASES, ids=lambda c: "-".join((c.id,) + oe.which_kernel("quant_bwd", c)))
def test_quant_backward(lic, case):
    d = oe.quant_bwd_inputs(case)
    N, C, H, W = case.shape
    L = case.levels
    a = Arena()
    op = lic.QuantOp(C, L, 0.9, 100, case.ntop, float(oe.QUANT_ALPHA), 0, False)
    xd = dev(d["x"])
    out = op.forward(xd, dev(d["wb"]), dev(np.zeros((C, L), F)), True)
    assert np.array_equal(host(out[0]), d["top"]) and np.array_equal(host(op.quant_), d["qidx"])
    op._bottom = [a.new(case.shape), a.new((C, L))]
    tops = [dev(d["g0"]), dev(d["g1"])] if case.ntop == 2 else [dev(d["g0"])]
    dd, wdif, cd = op.backward(tops, xd, out[0])
    assert dd is op._bottom[0] and wdif is op._bottom[1] and cd is op.count_data_
    a.check()
    rd, rw = orc.quant_backward(d["g0"], d["g1"] if case.ntop == 2 else None, d["x"], d["top"], d["qidx"], d["wb"], oe.QUANT_ALPHA)
    assert np.array_equal(host(dd), rd)
    got = host(wdif)
    assert np.allclose(got, rw, rtol=1e-5, atol=1e-4 * float(np.abs(rw).max()))               # the rule of test_quant_training_path
    w64, bound = oe.weight_diff_f64(case)
    err = np.abs(got - w64)
    print(case.id, "weight gradient: max |kernel - float64| / bound = %.3g" % float((err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound)


@pytest.mark.parametrize("case", oe.UPDATE_CASES, ids=lambda c: "-".join((c.id,) + oe.which_kernel("update", c)))
def test_quant_update_weight(lic, case):
    w, cnt = oe.update_inputs(case)
    C, L = case.channels, case.levels
    rw, rc = orc.quant_update_weight(w, cnt, F(0.9))
    a = Arena()
    op = lic.QuantOp(C, L, 0.9, 2, 1, 0.1, 0, False)
    op.iter_ = 2                                                                              # the update runs before this forward
    wd, cd = a.put(w), a.put(cnt)
    x = oe._rng("update_x", case.id).uniform(-1, 3, (1, C, 2, 2)).astype(F)
    top = op.forward(dev(x), wd, cd, True)[0]
    a.check()
    assert np.array_equal(host(wd), rw) and np.array_equal(host(cd), rc)
    assert np.array_equal(host(top), orc.quant(x, rw)[0])                                     # and the forward quantises with the updated weights


# ---------------------------------------------------------------------------------------------------- pixel shuffle
@pytest.mark.parametrize("case", oe.DTOW_CASES, ids=lambda c: "-".join((c.id,) + oe.which_kernel("dtow", c)))
def test_dtow(lic, case):
    x = oe.dtow_inputs(case)
    ref = oe.dtow_ref(x, case.stride, case.d2w)
    a = Arena()
    op = lic.DtowOp(case.stride, case.d2w, 0, False)
    op._top = [a.new(ref.shape, case.offset)]
    xd = a.put(x, case.offset)
    out = op.forward(xd)[0]
    assert out is op._top[0]
    a.check()
    assert np.array_equal(host(out), ref) and np.array_equal(ref, orc.dtow(x, case.stride, case.d2w))
    assert np.array_equal(host(op.backward(out)[0]), x)                                       # the inverse permutation, same dispatch rules


# ---------------------------------------------------------------------------------------------------- sphere ops
@pytest.mark.parametrize("case", oe.SPHERE_FWD_CASES, ids=lambda c: "-".join((c.id,) + oe.which_kernel("sphere_fwd", c)[4:]))
def test_sphere_forward_pad_equal_to_size(lic, case):
    x, _ = oe.sphere_inputs(case)
    p = case.pad
    ref = orc.sphere_pad(x, p)
    assert np.array_equal(ref, oe.sphere_pad_ref(x, p))
    a = Arena()
    op = lic.SpherePadOp(p, False, 0, False)
    op._top = [a.new(ref.shape)]
    assert np.array_equal(host(op.forward(dev(x))[0]), ref)
    y = ref.copy()
    y[:, :, :p] = 7; y[:, :, -p:] = 7; y[..., :p] = 7; y[..., -p:] = 7
    yd = a.put(y)
    assert lic.SpherePadOp(p, True, 0, False).forward(yd)[0] is yd and np.array_equal(host(yd), ref)
    ce = lic.SphereCutEdgeOp(p, 0, False)
    ce._top = [a.new(x.shape)]
    assert np.array_equal(host(ce.forward(dev(ref))[0]), x)
    td = a.put(ref)
    lic.SphereTrimOp(p, 0, False).forward(td)
    assert np.array_equal(host(td), orc.sphere_trim(ref.copy(), p))
    a.check()


@pytest.mark.parametrize("case", oe.SPHERE_TRIM_CASES, ids=lambda c: "-".join((c.id,) + oe.which_kernel("sphere_trim", c)))
def test_sphere_trim(lic, case):
    x = oe._rng("trim", case.id).standard_normal(case.shape).astype(F)
    a = Arena()
    td = a.put(x)
    lic.SphereTrimOp(case.pad, 0, False).forward(td)
    a.check()
    assert np.array_equal(host(td), orc.sphere_trim(x.copy(), case.pad))


@pytest.mark.parametrize("case", oe.SPHERE_BWD_CASES, ids=lambda c: "-".join((c.id,) + oe.which_kernel("sphere_bwd", c)))
def test_sphere_pad_backward_last_legal_size(lic, case):
    x, g = oe.sphere_inputs(case)
    p = case.pad
    a = Arena()
    op = lic.SpherePadOp(p, False, 0, False)
    op._bottom = [a.new(case.shape)]
    got = host(op.backward(dev(g))[0])
    gi = a.put(g)
    assert lic.SpherePadOp(p, True, 0, False).backward(gi)[0] is gi
    a.check()
    assert np.array_equal(got, orc.sphere_pad_backward(g, p))
    assert np.array_equal(host(gi), orc.sphere_pad_backward_inplace(g.copy(), p)) and np.array_equal(host(gi)[..., p:-p, p:-p], got)
    f64, mag = oe.sphere_pad_adjoint_f64(g, case.shape, p)
    assert np.all(np.abs(got - f64) <= 3 * 2.0 ** -24 * mag)                                  # the adjoint: at most four terms, three fp32 additions
    y = host(op.forward(dev(x))[0])
    lhs, rhs = float((y.astype(np.float64) * g).sum()), float((x.astype(np.float64) * got).sum())
    assert abs(lhs - rhs) <= 1e-5 * (abs(lhs) + 1)


@pytest.mark.parametrize("case", oe.SPHERE_BWD_REFUSED, ids=lambda c: "-".join((c.id,) + oe.which_kernel("sphere_bwd", c)))
def test_sphere_pad_backward_refuses_beyond(lic, case):
    x, g = oe.sphere_inputs(case)
    p = case.pad
    op = lic.SpherePadOp(p, False, 0, False)
    assert np.array_equal(host(op.forward(dev(x))[0]), oe.sphere_pad_ref(x, p))               # the forward keeps pad <= min(h, w)
    with pytest.raises(lic.Lic360Error):
        op.backward(dev(g))
    gi = dev(g)
    with pytest.raises(lic.Lic360Error):
        lic.SpherePadOp(p, True, 0, False).backward(gi)
    assert np.array_equal(host(gi), g)                                                        # refused before anything is written


# ---------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("case", oe.GMM_TABLE_CASES, ids=lambda c: "-".join((c.id,) + oe.which_kernel("gmm_table", c)))
def test_gmm_table(lic, case):
    w, s, m, bias = oe.gmm_table_inputs(case)
    rw, rs = w.copy(), s.copy()
    ref = orc.gmm_table(rw, rs, m, case.count, case.nstep, bias, float(oe.TABLE_TOTAL))
    n, g = case.count, case.ng
    a = Arena()
    op = lic.EntropyGmmTableOp(case.nstep, bias, g, oe.TABLE_TOTAL, 1e-6, 0, False)
    op._top = [a.new((n * g, case.nstep + 1))]
    wd, sd, md = (a.put(t.reshape(1, 1, n, g)) for t in (w, s, m))
    got = host(op.forward(wd, sd, md, torch.tensor([n], dtype=torch.int32))[0])
    a.check()
    assert np.array_equal(got[:n], ref)
    assert np.all(got[n:] == F(SENTINEL))                                                     # rows past tnum are not touched
    assert np.array_equal(host(wd).reshape(n, g), rw) and np.array_equal(host(sd).reshape(n, g), rs)      # softmax / sigma floor in place
    assert np.all(np.diff(got[:n], axis=1) > 0) and np.all(got[:n, 0] == 0) and np.all(got[:n, -1] == oe.TABLE_TOTAL)


@pytest.mark.parametrize("case", oe.ENTROPY_TABLE_CASES, ids=lambda c: "-".join((c.id,) + oe.which_kernel("entropy_table", c)))
def test_entropy_table(lic, case):
    lg = oe.entropy_table_inputs(case)
    n = case.count
    ref = orc.entropy_table(lg.reshape(-1), n, case.nstep, float(oe.TABLE_TOTAL))
    a = Arena()
    op = lic.EntropyTableOp(case.nstep, oe.TABLE_TOTAL, 0, False)
    op._top = [a.new((n + 3, case.nstep + 1))]
    data = np.zeros((1, case.nstep, n + 3, 1), F)
    data.reshape(-1)[:lg.size] = lg.reshape(-1)
    got = host(op.forward(a.put(data), torch.tensor([n], dtype=torch.int32))[0])
    a.check()
    assert np.array_equal(got[:n], ref) and np.all(got[n:] == F(SENTINEL))
    assert np.all(np.diff(ref, axis=1) > 0) and np.all(ref[:, -1] == oe.TABLE_TOTAL)


# ---------------------------------------------------------------------------------------------------- GMM loss
@pytest.mark.parametrize("case", oe.GMM_LOSS_CASES, ids=lambda c: "-".join((c.id,) + oe.which_kernel("gmm_loss", c)[2:]))
def test_entropy_gmm_loss_and_gradients(lic, case):
    d = oe.gmm_loss_inputs(case)
    M, g = case.M, case.ng
    a = Arena()
    op = lic.EntropyGmmOp(g, -1, 0, False)
    op._top = [a.new((M,))]
    op._diff = [a.new((M, g)), a.new((M, g)), a.new((M, g)), a.new((M, 1))]
    loss = host(op.forward(dev(d["w"]), dev(d["d"]), dev(d["m"]), dev(d["lab"]))[0])
    grads = [host(t) for t in op.backward(dev(d["top"]))]
    a.check()
    ref = oe.gmm_oracle_with_top(case)
    assert np.array_equal(loss, ref[0])                                                       # same routines -> identical
    assert all(np.isfinite(t).all() and written(t) for t in grads)
    if case.degenerate:
        assert np.all(loss == oe.GMM_UNDERFLOW_LOSS)
        return
    for got, r in zip(grads, ref[1:]):
        assert np.allclose(got, r, rtol=1e-5, atol=1e-6)
    f64 = oe.gmm_loss_f64(case)
    keep = f64[5] > oe.GMM_MIN_P
    err = max(float(np.abs(got - f.reshape(got.shape))[keep].max()) for got, f in zip(grads, f64[1:5]))
    tol = 2 * oe.GMM_F64_TOL[case.id]
    print("%s: max |kernel - float64| = %.3g over the four gradients, allowed %.3g (twice the oracle's measured error)" % (case.id, err, tol))
    assert np.abs(loss - f64[0])[keep].max() < 1e-5
    assert err <= tol


# ---------------------------------------------------------------------------------------------------- viewport
@pytest.mark.parametrize("case", oe.VIEWPORT_CASES, ids=lambda c: "-".join((c.id,) + oe.which_kernel("viewport", c)))
def test_viewport_seam_and_poles(lic, case):
    x = oe.viewport_inputs(case)
    tp = oe.VIEWPORT_ANGLES
    N, ho, wo = len(tp), oe.VIEWPORT_HO, oe.VIEWPORT_WO
    a = Arena()
    op = lic.ViewportOp(oe.VIEWPORT_FOV, ho, wo, 0, False)
    op._top = [a.new((N, oe.VIEWPORT_C, ho, wo)), a.new((N, ho, wo, 3)), a.new((N, ho, wo, 3)), a.new((N, ho, wo, 2))]
    op._rota = a.new((N, 9))
    view, rays0, rota, rays, ang = [host(t) for t in op.forward(dev(x), dev(tp))]
    a.check()
    assert all(written(t) and np.isfinite(t).all() for t in (view, rays0, rota, rays, ang))
    rv, r0, rr, ry, ra = orc.viewport_forward(x, tp, ho, wo, F(oe.VIEWPORT_FOV))
    assert np.allclose(rays0, r0, atol=1e-6) and np.allclose(rota, rr, atol=1e-6) and np.allclose(rays, ry, atol=1e-5)
    counts = oe.viewport_edge_counts(ang, case.H, case.W)
    f64 = oe.viewport_sample_f64(x, ang)                                                      # at the op's OWN coordinates: no libm in between
    err, tol = float(np.abs(view - f64).max()), 2 * oe.VIEWPORT_F64_TOL[case.id]
    print("%s: max |kernel - float64| = %.3g, allowed %.3g; edge samples %s" % (case.id, err, tol, counts))
    assert counts["tw_m1"] > 0 and counts["tw_last"] > 0 and (case.H > 8 or counts["th_m1"] > 0 and counts["th_last"] > 0)
    assert err <= tol
    c = host(op.forward(dev(np.full(x.shape, -1.25, F)), dev(tp))[0])
    assert np.allclose(c, -1.25, atol=1e-6)                                                   # the four weights sum to one across the seam and at the poles


# ---------------------------------------------------------------------------------------------------- importance map
@pytest.mark.parametrize("imp_kernel", oe.IMP_KERNELS_AS_RULE0)
def test_imp_map_backward_kernels_above_3_are_rule_0(lic, imp_kernel):
    g, imp, sc = oe.imp_inputs()
    N, C, H, W = oe.IMP_SHAPE
    a = Arena()
    op = lic.ImpMapOp(oe.IMP_LEVELS, 0.13, 0.7, 0.5, 0.61, 0.61, imp_kernel, 1, 0, False)
    op._bottom = [a.new(oe.IMP_SHAPE), a.new((N, 1, H, W))]
    dd, di = op.backward(dev(g), dev(imp), dev(sc))
    a.check()
    rd, ri = orc.imp_map_backward(g, imp, sc, host(op._alpha), oe.IMP_LEVELS, 0, F(0.7))
    assert np.array_equal(host(dd), rd) and np.array_equal(host(di), ri)
    op0 = lic.ImpMapOp(oe.IMP_LEVELS, 0.13, 0.7, 0.5, 0.61, 0.61, 0, 1, 0, False)
    assert np.array_equal(host(op0.backward(dev(g), dev(imp), dev(sc))[1]), host(di))
