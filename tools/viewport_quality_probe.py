"""The viewport metrics of the evaluation mode on 512x1024 ERP pairs with the 14 viewports of 171x256 (fov 0.5), at batch 8 and batch 1:
  library  two MultiProject calls (k_projects_forward), lic360_operator.SSIM(11, 3) (five grouped 11x11 library convolutions and the
           elementwise launches around them) and the MSE of the views: two scalars;
  fused    lic360_operator.ViewportQuality (lic360.viewport_quality, k_viewport_quality): mse and ssim per image and viewport.
The two alternate in one process: --repeats (20) repeats of 5 calls each, each after 2 warm-up calls, timed with device events; median
(min - max) ms per call.  The fused form is "faster" only if its median lies below the library's by more than the two min-max ranges added.
Also: the achieved bytes/s against the least the metric has to read, the two ERP batches once (2 * n * 3 * 512 * 1024 * 4 bytes), and how far
the two forms' scalars lie apart.  --json FILE keeps the table (default profiles/viewport_quality_probe.json).
--grad: the training loss instead, forward + backward of sum(g_mse * mse + g_ssim * ssim) through ViewportQuality(grad="library") (MultiProject +
SSIM + torch.mean and their autograd) and ViewportQuality(grad="fused") (lic360.viewport_quality_coef / viewport_quality_backward), at batch 8 and 1,
with one image and with both recording gradients; same alternation, timing and rule, plus each form's peak device memory above what the inputs
hold (torch.cuda.max_memory_allocated), how far the two forms' gradients lie apart, and the fused form's two launches timed on their own with the
backward's rate of added bytes (cells * 4 adds * 4 B per differentiated image).  Default table: profiles/viewport_quality_grad_probe.json."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "360-image-compression_amd"))
import torch  # noqa: E402

H, W, VH, VW, FOV = 512, 1024, 171, 256, 0.5


def timed(fn, calls=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def grad_probe(args):
    import lic360_operator as lo
    dev = "cuda:0"
    torch.manual_seed(0)
    mods = {k: lo.ViewportQuality(VH, VW, FOV, False, 0, grad=k) for k in ("library", "fused")}
    rows = []
    for n in (8, 1):
        for sides in (1, 2):
            a = torch.rand((n, 3, H, W), device=dev).requires_grad_()
            b = (a.detach() + 0.02 * torch.randn_like(a)).clamp(0, 1).requires_grad_(sides == 2)
            g_mse, g_ssim = torch.randn((n, 14), device=dev), torch.randn((n, 14), device=dev)

            def step(q):
                a.grad, b.grad = None, None
                mse, ssim = q(a, b)
                ((g_mse * mse).sum() + (g_ssim * ssim).sum()).backward()
                return a.grad, b.grad

            t, peak, grads = {k: [] for k in mods}, {}, {}
            for _ in range(args.repeats):
                for k, q in mods.items():
                    t[k].append(timed(lambda: step(q)))
            for k, q in mods.items():
                a.grad, b.grad = None, None
                torch.cuda.synchronize()
                held = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                grads[k] = [None if g is None else g.clone() for g in step(q)]
                torch.cuda.synchronize()
                peak[k] = torch.cuda.max_memory_allocated() - held
            # the fused form's two launches on their own (medians of the same repeats): where the atomic adds of the backward put it
            import lic360
            op, taps, need = mods["fused"].project.op[0], mods["fused"].taps, dict(need_a=True, need_b=sides == 2)
            with torch.no_grad():
                ad, bd = a.detach(), b.detach()
                coefs = lic360.viewport_quality_coef(op, ad, bd, taps, **need)[2]
                parts = {"forward_coef": [], "backward": []}
                for _ in range(args.repeats):
                    parts["forward_coef"].append(timed(lambda: lic360.viewport_quality_coef(op, ad, bd, taps, **need)))
                    parts["backward"].append(timed(lambda: lic360.viewport_quality_backward(op, ad, bd, taps, coefs, g_mse, g_ssim, **need)))
                del coefs
            med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
            spread = {k: max(v) - min(v) for k, v in t.items()}
            apart = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(grads["fused"], grads["library"]) if x is not None)
            row = {"batch": n, "sides": sides, "erp": [H, W], "viewport": [VH, VW], "speedup": med["library"] / med["fused"],
                   "fused_is_faster": bool(med["library"] - med["fused"] > spread["library"] + spread["fused"]), "gradients_apart_rel_max": apart}
            for k, v in t.items():
                row[k] = {"median_ms": med[k], "min_ms": min(v), "max_ms": max(v), "peak_bytes": peak[k]}
            atomic_bytes = sides * 14.0 * n * 3 * VH * VW * 4 * 4
            row["fused_parts"] = {k: {"median_ms": sorted(v)[len(v) // 2], "min_ms": min(v), "max_ms": max(v)} for k, v in parts.items()}
            row["fused_parts"]["backward"]["atomic_bytes"] = atomic_bytes
            row["fused_parts"]["backward"]["atomic_GBps"] = atomic_bytes / row["fused_parts"]["backward"]["median_ms"] / 1e6
            rows.append(row)
            print("    fused alone: forward with maps %.3f (%.3f - %.3f) ms   backward %.3f (%.3f - %.3f) ms = %.0f GB/s of added bytes" % (
                row["fused_parts"]["forward_coef"]["median_ms"], min(parts["forward_coef"]), max(parts["forward_coef"]), row["fused_parts"]["backward"]["median_ms"],
                min(parts["backward"]), max(parts["backward"]), row["fused_parts"]["backward"]["atomic_GBps"]), flush=True)
            print("batch %d, %d side(s)   library %.3f (%.3f - %.3f) ms, peak %.0f MB   fused %.3f (%.3f - %.3f) ms, peak %.0f MB   %.2fx   %s   gradients apart %.2e" % (
                n, sides, med["library"], min(t["library"]), max(t["library"]), peak["library"] / 1e6, med["fused"], min(t["fused"]), max(t["fused"]), peak["fused"] / 1e6,
                row["speedup"], "fused is faster" if row["fused_is_faster"] else "NOT faster by the rule", apart), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), forms=["library", "fused"], workload="forward + backward of sum(g_mse * mse + g_ssim * ssim), 1 or 2 images recording",
                           repeats="median of %d alternating repeats of 5 steps, each after 2 warm-up steps; device events; ms per step" % args.repeats,
                           rule="fused_is_faster: the fused median lies below the library median by more than the two min-max ranges added",
                           memory="peak_bytes: torch.cuda.max_memory_allocated over one step, minus what was allocated before it",
                           apart="gradients_apart_rel_max: largest |fused - library| over the largest |library| gradient, per ERP batch", rows=rows), f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--grad", action="store_true", help="time forward + backward of the training loss instead (library against grad=\"fused\")")
    args = ap.parse_args()
    if args.json is None:
        args.json = os.path.join(ROOT, "profiles", "viewport_quality_grad_probe.json" if args.grad else "viewport_quality_probe.json")
    if args.grad:
        return grad_probe(args)
    import lic360_operator as lo
    dev = "cuda:0"
    torch.manual_seed(0)
    pr, ssim, vq = lo.MultiProject(VH, VW, FOV, False, 0), lo.SSIM(11, 3), lo.ViewportQuality(VH, VW, FOV, False, 0)
    rows = []
    for n in (8, 1):
        a = torch.rand((n, 3, H, W), device=dev)
        b = (a + 0.02 * torch.randn_like(a)).clamp(0, 1)

        def library():
            with torch.no_grad():
                va, vb = pr(a).clone(), pr(b)
                return torch.mean((va - vb) ** 2), ssim(va, vb)

        def fused():
            return vq(a, b)

        forms = {"library": library, "fused": fused}
        t = {k: [] for k in forms}
        for _ in range(args.repeats):
            for k, fn in forms.items():
                t[k].append(timed(fn))
        (l_mse, l_ssim), (f_mse, f_ssim) = library(), fused()
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        spread = {k: max(v) - min(v) for k, v in t.items()}
        floor_bytes = 2.0 * n * 3 * H * W * 4
        row = {"batch": n, "erp": [H, W], "viewport": [VH, VW], "erp_read_floor_bytes": floor_bytes,
               "fused_is_faster": bool(med["library"] - med["fused"] > spread["library"] + spread["fused"]), "speedup": med["library"] / med["fused"],
               "mse": {"library": float(l_mse), "fused": float(f_mse.mean())}, "ssim": {"library": float(l_ssim), "fused": float(f_ssim.mean())}}
        for k, v in t.items():
            row[k] = {"median_ms": med[k], "min_ms": min(v), "max_ms": max(v), "floor_GBps": floor_bytes / med[k] / 1e6}
        rows.append(row)
        print("batch %d   library %.4f (%.4f - %.4f) ms   fused %.4f (%.4f - %.4f) ms   %.2fx   fused reads the ERP floor at %.0f GB/s   %s" % (
            n, med["library"], min(t["library"]), max(t["library"]), med["fused"], min(t["fused"]), max(t["fused"]), row["speedup"], row["fused"]["floor_GBps"],
            "fused is faster" if row["fused_is_faster"] else "NOT faster by the rule"), flush=True)
        print("          mse library %.9g fused %.9g   ssim library %.9g fused %.9g" % (row["mse"]["library"], row["mse"]["fused"], row["ssim"]["library"], row["ssim"]["fused"]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), forms=["library", "fused"],
                           repeats="median of %d alternating repeats of 5 calls, each after 2 warm-up calls; device events; ms per call" % args.repeats,
                           rule="fused_is_faster: the fused median lies below the library median by more than the two min-max ranges added",
                           bytes="floor_GBps: the two ERP batches read once (2 * n * 3 * 512 * 1024 * 4 bytes) over the median time", rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
