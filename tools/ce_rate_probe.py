"""The cross-entropy rate loss of the importance map's entropy model on the raw output of its net: G = 1 group of 64 x 128 symbols (the map of a
512 x 1024 ERP image), K = 49 classes, at batch 8 and batch 1, on one stream:
  library  lic360_operator.CeRateLoss(route="library"): ContextReshape, torch.nn.functional.cross_entropy(reduction="none"), a per-image float64
           sum, and their autograd;
  fused    CeRateLoss(route="fused"): lic360.ce_rate (k_ce_rate, k_plane_sum_finish) and, recording, autograd.CeRateFn with lic360.ce_rate_backward
           (k_ce_rate_backward).  The module's label check is on, as by default (one synchronisation per call).
The two alternate in one process: --repeats (20) timed windows of --calls (50) calls each, each after 5 warm-up calls, timed with device events
around the window -- a window of a few milliseconds, so that the events' resolution and one scheduling hiccup do not make the figure; median
(min - max) over the windows of the mean ms per call (the spread of window means, which is narrower than the spread of single calls), for the
forward alone (no gradient recorded) and for forward + backward of sum(g * nats) with the logits recording.  The fused form is "faster" only if its
median lies below the library's by more than the two min-max ranges added.
Also: GB/s against the bytes the algorithm must move -- (K + 1) * 4 bytes per symbol forward, (2 K + 1) * 4 backward.  For the module's step that is
a whole-program rate (host work, allocations, the label check's synchronisation and launch gaps included), not a kernel's.  "fused_entries" times
lic360.ce_rate / ce_rate_backward with every buffer given, by the same device events around the Python calls: launch gaps and host pacing are in it,
so it is an upper bound on the kernels' time, not the kernels' time.  And how far the two forms' results lie apart.  --json FILE keeps the table
(default profiles/ce_rate_probe.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "360-image-compression_amd"))
import torch  # noqa: E402

G, H, W, K = 1, 64, 128, 49


def timed(fn, calls, warm=5):
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


def summary(v, nbytes):
    med = sorted(v)[len(v) // 2]
    return {"median_ms": med, "min_ms": min(v), "max_ms": max(v), "GBps": nbytes / med / 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "ce_rate_probe.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    import lic360
    import lic360_operator as lo
    dev = "cuda:0"
    mods = {k: lo.CeRateLoss(G, K, k) for k in ("library", "fused")}
    rows = []
    for n in (8, 1):
        torch.manual_seed(n)
        logit = (2.0 * torch.randn((n, G * K, H, W), device=dev)).requires_grad_()
        label = torch.randint(0, K, (n, G, H, W), device=dev).float()
        g = torch.rand((n,), device=dev, dtype=torch.float64) + 0.5

        def forward(q):
            with torch.no_grad():
                return q(logit, label)

        def step(q):
            logit.grad = None
            nats, _ = q(logit, label)
            (g * nats).sum().backward()
            return nats.detach(), logit.grad

        t_f, t_s, res = {k: [] for k in mods}, {k: [] for k in mods}, {}
        for _ in range(args.repeats):
            for k, q in mods.items():
                t_f[k].append(timed(lambda: forward(q), args.calls))
            for k, q in mods.items():
                t_s[k].append(timed(lambda: step(q), args.calls))
        for k, q in mods.items():
            nats, grad = step(q)
            res[k] = (nats.clone(), grad.clone())
        with torch.no_grad():                                             # the fused entries with every buffer given: an upper bound on the kernels' time
            gf, ld = g.float(), logit.detach()
            out = lic360.ce_rate_backward(ld, label, gf)
            bufs = lic360.ce_rate(ld, label)
            scratch = torch.empty(lic360.ce_rate_scratch_bytes(n, G, H, W), dtype=torch.uint8, device=dev)
            parts = {"forward": [], "backward": []}
            for _ in range(args.repeats):
                parts["forward"].append(timed(lambda: lic360.ce_rate(ld, label, nats=bufs[0], symbols=bufs[1], invalid=bufs[2], scratch=scratch), args.calls))
                parts["backward"].append(timed(lambda: lic360.ce_rate_backward(ld, label, gf, out=out), args.calls))
        symbols = n * G * H * W
        bytes_f, bytes_b = (K + 1) * 4.0 * symbols, (2 * K + 1) * 4.0 * symbols
        row = {"batch": n, "shape": [G, H, W], "classes": K, "symbols": symbols, "bytes_forward": bytes_f, "bytes_backward": bytes_b,
               "workgroups": symbols // 256, "forward": {}, "forward_backward": {}}
        for name, t, nbytes in (("forward", t_f, bytes_f), ("forward_backward", t_s, bytes_f + bytes_b)):
            med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
            spread = {k: max(v) - min(v) for k, v in t.items()}
            for k, v in t.items():
                row[name][k] = summary(v, nbytes)
            row[name]["speedup"] = med["library"] / med["fused"]
            row[name]["fused_is_faster"] = bool(med["library"] - med["fused"] > spread["library"] + spread["fused"])
        row["fused_entries"] = {"forward": summary(parts["forward"], bytes_f), "backward": summary(parts["backward"], bytes_b)}
        row["nats_apart_rel_max"] = float(((res["fused"][0] - res["library"][0]).abs() / res["library"][0].abs()).max())
        row["gradients_apart_rel_max"] = float((res["fused"][1] - res["library"][1]).abs().max() / res["library"][1].abs().max())
        rows.append(row)
        for name in ("forward", "forward_backward"):
            r = row[name]
            print("batch %d, %-16s library %.4f (%.4f - %.4f) ms   fused %.4f (%.4f - %.4f) ms = %.0f GB/s   %.2fx   %s" % (
                n, name, r["library"]["median_ms"], r["library"]["min_ms"], r["library"]["max_ms"], r["fused"]["median_ms"], r["fused"]["min_ms"],
                r["fused"]["max_ms"], r["fused"]["GBps"], r["speedup"], "fused is faster" if r["fused_is_faster"] else "NOT faster by the rule"), flush=True)
        fp = row["fused_entries"]
        print("    fused entries alone (upper bound on the kernels): forward %.4f (%.4f - %.4f) ms = %.0f GB/s   backward %.4f (%.4f - %.4f) ms = %.0f GB/s   apart: nats %.2e, gradients %.2e" % (
            fp["forward"]["median_ms"], fp["forward"]["min_ms"], fp["forward"]["max_ms"], fp["forward"]["GBps"], fp["backward"]["median_ms"],
            fp["backward"]["min_ms"], fp["backward"]["max_ms"], fp["backward"]["GBps"], row["nats_apart_rel_max"], row["gradients_apart_rel_max"]), flush=True)
    verdict = all(r[name]["fused_is_faster"] for r in rows for name in ("forward", "forward_backward"))
    print("default route by the rule: %s" % ("fused" if verdict else "library"))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), forms=["library", "fused"],
                           workload="forward (no gradient recorded) and forward + backward of sum(g * nats), the logits recording; one stream",
                           repeats="median (min - max) over %d alternating windows of %d calls, each after 5 warm-up calls; device events around the window; "
                                   "mean ms per call of a window" % (args.repeats, args.calls),
                           rule="fused_is_faster: the fused median lies below the library median by more than the two min-max ranges added; "
                                "fused is CeRateLoss's default only if that holds for both workloads at both batches",
                           bytes="GBps: (K + 1) * 4 bytes per symbol forward, (2 K + 1) * 4 backward, their sum for forward + backward; over the median time: "
                                 "a whole-program rate for the module's steps; for fused_entries a lower bound on the kernels' rate (launch gaps included)",
                           apart="largest |fused - library| over the largest |library|, per tensor", fused_is_default=verdict, rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
