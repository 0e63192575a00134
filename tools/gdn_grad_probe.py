"""lic360_operator.GDN in training, forward + backward, on the six production shapes (192 channels; the three down-sampling stages' GDN and the three
up-sampling stages' inverse GDN on 68 x 132, 132 x 260 and 260 x 516 maps) at batch 1 and batch 8:
  library  GDN(grad="library"): x * x, a 1x1 conv2d, sqrt and a division or product, and autograd's chain through them (the only route before this probe);
  fused    GDN(grad="fused"): autograd.GdnFn -- lic360.gdn_forward, then lic360.gdn_backward (k_gdn_backward_dx, k_gdn_backward_param and its finish).
The two routes alternate in one process: --repeats (7) windows of a few steps each after warm-up steps, timed with device events; median (min - max) ms per
step (the reparametrisation of beta and gamma and its backward included on both routes).  The fused route is "faster" only if its median lies below the
library's by more than the two min-max ranges added; "slower" by the same rule the other way.  Also: the fused backward's entry on its own, each route's peak
device memory over one forward + backward above what was held before (torch.cuda.max_memory_allocated), and how far the routes' gradients lie apart.
--json FILE keeps the table (default profiles/gdn_grad_probe.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "360-image-compression_amd"))
import torch  # noqa: E402

C = 192
MAPS = ((68, 132), (132, 260), (260, 516))
SHAPES = [("down_%dx%d" % m, m, False) for m in MAPS] + [("up_%dx%d" % m, m, True) for m in MAPS]
ROUTES = ("library", "fused")


def timed(fn, calls=3, warm=1):
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


def summary(v):
    return {"median_ms": sorted(v)[len(v) // 2], "min_ms": min(v), "max_ms": max(v)}


def verdict(t):
    """library / fused medians by the project's rule: a difference counts only if it exceeds the two spreads added"""
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    spread = {k: max(v) - min(v) for k, v in t.items()}
    gap, noise = med["library"] - med["fused"], spread["library"] + spread["fused"]
    return dict({k: summary(v) for k, v in t.items()}, speedup=med["library"] / med["fused"],
                verdict="fused is faster" if gap > noise else "fused is slower" if -gap > noise else "no difference by the rule")


def peak_of(step):
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - held, out


def probe(name, hw, inverse, n, repeats):
    import lic360
    import lic360_operator as lo
    dev = "cuda:0"
    torch.manual_seed(n * 1000 + hw[0])
    mods = {k: lo.GDN(C, 0, inverse, grad=k).to(dev) for k in ROUTES}
    with torch.no_grad():
        mods["library"].gamma.add_(0.05 * torch.rand_like(mods["library"].gamma))
        mods["library"].beta.add_(0.05 * torch.rand_like(mods["library"].beta))
    mods["fused"].load_state_dict(mods["library"].state_dict())
    x = (torch.randn((n, C) + hw, device=dev) * 2.0).requires_grad_(True)
    gy = torch.randn((n, C) + hw, device=dev) * 0.05

    def step(m):
        x.grad = None
        m.zero_grad(set_to_none=True)
        m(x).backward(gy)
        return x.grad, m.gamma.grad, m.beta.grad

    t = {k: [] for k in ROUTES}
    for _ in range(repeats):
        for k in ROUTES:
            t[k].append(timed(lambda: step(mods[k])))
    peak, res = {}, {}
    for k in ROUTES:
        peak[k], res[k] = peak_of(lambda: [g.clone() for g in step(mods[k])])
    m = mods["fused"]
    with torch.no_grad():
        beta = m.beta.clamp_min(m.beta_bound) ** 2 - m.pedestal
        gamma = m.gamma.clamp_min(m.gamma_bound) ** 2 - m.pedestal
        xd = x.detach()
        scratch = torch.empty(lic360.gdn_backward_scratch_bytes(n, C, hw[0] * hw[1]), dtype=torch.uint8, device=dev)
        entry, fwd = [], []
        for _ in range(repeats):
            entry.append(timed(lambda: lic360.gdn_backward(xd, gy, gamma, beta, inverse, scratch=scratch)))
            fwd.append(timed(lambda: lic360.gdn_forward(xd, gamma, beta, inverse)))
        del scratch
    apart = lambda a, b: float((a - b).abs().max() / b.abs().max())
    row = {"shape": name, "batch": n, "chw": [C, hw[0], hw[1]], "inverse": inverse, "forward_backward": verdict(t), "fused_backward_entry": summary(entry),
           "fused_forward_entry": summary(fwd), "peak_bytes": peak, "scratch_bytes": lic360.gdn_backward_scratch_bytes(n, C, hw[0] * hw[1]),
           "apart_rel_max": {"x_grad": apart(res["fused"][0], res["library"][0]), "gamma_grad": apart(res["fused"][1], res["library"][1]),
                             "beta_grad": apart(res["fused"][2], res["library"][2])}}
    r = row["forward_backward"]
    print("batch %d %-13s library %.3f (%.3f - %.3f) ms   fused %.3f (%.3f - %.3f) ms   %.2fx   %s;  backward entry alone %.3f ms, forward entry %.3f ms;  peak library "
          "%.0f MB, fused %.0f MB (scratch %.0f MB);  apart %s" % (
              n, name, r["library"]["median_ms"], r["library"]["min_ms"], r["library"]["max_ms"], r["fused"]["median_ms"], r["fused"]["min_ms"], r["fused"]["max_ms"],
              r["speedup"], r["verdict"], row["fused_backward_entry"]["median_ms"], row["fused_forward_entry"]["median_ms"], peak["library"] / 1e6, peak["fused"] / 1e6,
              row["scratch_bytes"] / 1e6, row["apart_rel_max"]), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "gdn_grad_probe.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batches", default="1,8")
    args = ap.parse_args()
    rows = []
    for n in (int(v) for v in args.batches.split(",")):
        for name, hw, inverse in SHAPES:
            rows.append(probe(name, hw, inverse, n, args.repeats))
            torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), routes=list(ROUTES),
                           workload="lic360_operator.GDN(192) forward + backward of a given output gradient, x and both parameters requiring gradients",
                           repeats="median of %d alternating windows of 3 steps after 1 warm-up step; device events; ms per step" % args.repeats,
                           rule="a difference counts only if the medians lie apart by more than the two min-max ranges added",
                           entries="fused_backward_entry: lic360.gdn_backward alone (three kernels, its scratch allocated once); fused_forward_entry: lic360.gdn_forward alone",
                           memory="peak_bytes: torch.cuda.max_memory_allocated over one forward + backward (the gradients cloned), minus what was allocated before it",
                           apart="largest |fused - library| over the largest |library|, per gradient", rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
