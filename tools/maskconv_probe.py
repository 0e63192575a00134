"""The group-causal 5x5 convolution of the entropy nets in training, 48 groups on a 64 x 128 latent, at batch 1 and batch 8:
  library  lic360_operator.MaskConv2(route="library"): a dense conv2d over the masked weight and its autograd (the only route before this probe existed);
  fused    MaskConv2(route="fused"): autograd.MaskConvFn -- lic360_cconv_ec forward, the same kernel on transformed operands for the data gradient
           (lic360.cconv_dgrad), k_cconv_wgrad + its finish for the weight gradient (lic360.cconv_wgrad), a library sum for the bias.
Layers: first (1 -> 4 channels a group, constrain 5), hidden (4 -> 4, constrain 6), last (4 -> 3, constrain 6); whole model: EntropyNet2(48, 4, 3),
rate(x, mask).sum().backward() with the fused head on both sides.  The two routes alternate in one process: --repeats (10) repeats of a few calls each after
warm-up calls, timed with device events; median (min - max) ms per call for the forward alone (no gradient recorded) and for forward + backward.  The
fused route is "faster" only if its median lies below the library's by more than the two min-max ranges added; "slower" by the same rule the other way.
Also: the three parts of the fused backward on their own (dgrad; wgrad with its finish; the flips and the weight transpose of dgrad), each route's peak
device memory over one forward + backward above what was held before, and how far the routes' results lie apart.  --json FILE keeps the table (default
profiles/maskconv_probe.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "360-image-compression_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

G, H, W = 48, 64, 128
LAYERS = (("first", 1, 4, False), ("hidden", 4, 4, True), ("last", 4, 3, True))
ROUTES = ("library", "fused")


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


def show(name, n, row):
    for part in ("forward", "forward_backward"):
        r = row[part]
        print("batch %d %-7s %-16s library %.4f (%.4f - %.4f) ms   fused %.4f (%.4f - %.4f) ms   %.2fx   %s" % (
            n, name, part, r["library"]["median_ms"], r["library"]["min_ms"], r["library"]["max_ms"], r["fused"]["median_ms"], r["fused"]["min_ms"],
            r["fused"]["max_ms"], r["speedup"], r["verdict"]), flush=True)


def probe_layer(name, cin, cout, hidden, n, repeats):
    import lic360
    import lic360_operator as lo
    dev = "cuda:0"
    torch.manual_seed(n * 10 + cin + cout)
    mods = {k: lo.MaskConv2(G, cin, cout, 5, hidden, 0, False, k).to(dev) for k in ROUTES}
    mods["fused"].load_state_dict(mods["library"].state_dict())
    x = torch.randn((n, G * cin, H, W), device=dev).requires_grad_(name != "first")              # the first layer's input needs no gradient
    gy = torch.randn((n, G * cout, H, W), device=dev) * 0.05

    def forward(m):
        with torch.no_grad():
            return m(x)

    def step(m):
        x.grad = None
        m.zero_grad(set_to_none=True)
        y = m(x)
        y.backward(gy)
        return y.detach(), x.grad, m.weight.grad, m.bias.grad

    t_f, t_s = {k: [] for k in ROUTES}, {k: [] for k in ROUTES}
    for _ in range(repeats):
        for k in ROUTES:
            t_f[k].append(timed(lambda: forward(mods[k])))
        for k in ROUTES:
            t_s[k].append(timed(lambda: step(mods[k])))
    peak, res = {}, {}
    for k in ROUTES:
        peak[k], res[k] = peak_of(lambda: [None if t is None else t.clone() for t in step(mods[k])])
    constrain = 6 if hidden else 5
    w = mods["fused"].weight.detach()
    xd = x.detach()
    parts = {"dgrad": [], "wgrad_and_finish": [], "flips_and_transpose": []}
    with torch.no_grad():
        for _ in range(repeats):
            parts["dgrad"].append(timed(lambda: lic360.cconv_dgrad(gy, w, G, constrain)))
            parts["wgrad_and_finish"].append(timed(lambda: lic360.cconv_wgrad(xd, gy, G, constrain)))
            parts["flips_and_transpose"].append(timed(lambda: (lic360.cconv_group_flip(gy, G).contiguous(), lic360.cconv_transpose_weight(w, G).contiguous(),
                                                               lic360.cconv_group_flip(xd, G).contiguous())))
    keep = w != 0
    apart = lambda a, b: float((a - b).abs().max() / b.abs().max())
    row = {"layer": name, "batch": n, "shape": [G, cin, cout, H, W], "constrain": constrain, "forward": verdict(t_f), "forward_backward": verdict(t_s),
           "fused_backward_parts": {k: summary(v) for k, v in parts.items()}, "peak_bytes": peak,
           "scratch_bytes": lic360.cconv_wgrad_scratch_bytes(n, G * cin, G * cout, H, W, G, constrain),
           "apart_rel_max": {"output": apart(res["fused"][0], res["library"][0]),
                             "x_grad": None if res["library"][1] is None else apart(res["fused"][1], res["library"][1]),
                             "weight_grad_kept_taps": apart(res["fused"][2] * keep, res["library"][2] * keep), "bias_grad": apart(res["fused"][3], res["library"][3])}}
    show(name, n, row)
    p = row["fused_backward_parts"]
    print("    fused backward alone: dgrad %.4f (%.4f - %.4f) ms, of which flips and transpose %.4f (%.4f - %.4f) ms; wgrad + finish %.4f (%.4f - %.4f) ms; peak "
          "library %.0f MB, fused %.0f MB (wgrad scratch %.0f MB); apart %s" % (
              p["dgrad"]["median_ms"], p["dgrad"]["min_ms"], p["dgrad"]["max_ms"], p["flips_and_transpose"]["median_ms"], p["flips_and_transpose"]["min_ms"],
              p["flips_and_transpose"]["max_ms"], p["wgrad_and_finish"]["median_ms"], p["wgrad_and_finish"]["min_ms"], p["wgrad_and_finish"]["max_ms"],
              peak["library"] / 1e6, peak["fused"] / 1e6, row["scratch_bytes"] / 1e6, row["apart_rel_max"]), flush=True)
    return row


def probe_model(n, repeats):
    import lic360_models as lm
    import util
    dev = "cuda:0"
    torch.manual_seed(n)
    nets = {k: lm.EntropyNet2(G, 4, 3, head="fused", conv=k).to(dev) for k in ROUTES}
    nets["fused"].load_state_dict(nets["library"].state_dict())
    rng = np.random.default_rng(n)
    lat = [util.latent_smooth(rng, G, H, W) for _ in range(n)]
    x = torch.from_numpy(np.concatenate([c for c, _, _ in lat]) - np.float32(3.5)).to(dev)
    mask = torch.from_numpy(np.concatenate([m for _, m, _ in lat])).to(dev)

    def forward(net):
        with torch.no_grad():
            return net.rate(x, mask)[0]

    def step(net):
        net.zero_grad(set_to_none=True)
        nats = net.rate(x, mask)[0]
        nats.sum().backward()
        return nats.detach()

    t_f, t_s = {k: [] for k in ROUTES}, {k: [] for k in ROUTES}
    for _ in range(repeats):
        for k in ROUTES:
            t_f[k].append(timed(lambda: forward(nets[k]), calls=3, warm=1))
        for k in ROUTES:
            t_s[k].append(timed(lambda: step(nets[k]), calls=3, warm=1))
    peak, res = {}, {}
    for k in ROUTES:
        peak[k], nats = peak_of(lambda: step(nets[k]).clone())
        res[k] = (nats, {name: p.grad.clone() for name, p in nets[k].named_parameters()})
    grads = max(float(((res["fused"][1][name] - g) * (nets["fused"].state_dict()[name] != 0 if name.endswith("weight") and g.dim() == 4 else 1)).abs().max() /
                      g.abs().max()) for name, g in res["library"][1].items())
    row = {"model": "EntropyNet2(48, 4, 3, head='fused')", "batch": n, "shape": [G, H, W], "forward": verdict(t_f), "forward_backward": verdict(t_s),
           "peak_bytes": peak, "apart_rel_max": {"nats": float(((res["fused"][0] - res["library"][0]).abs() / res["library"][0].abs()).max()),
                                                 "parameter_grads_kept_taps": grads}}
    show("model", n, row)
    print("    peak library %.0f MB, fused %.0f MB; apart %s" % (peak["library"] / 1e6, peak["fused"] / 1e6, row["apart_rel_max"]), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "maskconv_probe.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--batches", default="1,8")
    args = ap.parse_args()
    layers, models = [], []
    for n in (int(v) for v in args.batches.split(",")):
        for name, cin, cout, hidden in LAYERS:
            layers.append(probe_layer(name, cin, cout, hidden, n, args.repeats))
        models.append(probe_model(n, args.repeats))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), routes=list(ROUTES),
                           workload="MaskConv2 layers of 48 groups on 64 x 128: forward (no gradient recorded) and forward + backward of a given output gradient; "
                                    "EntropyNet2(48, 4, 3).rate(x, mask).sum().backward() with the fused head on both routes",
                           repeats="median of %d alternating repeats of 5 calls after 2 warm-up calls (the model: 3 after 1); device events; ms per call" % args.repeats,
                           rule="a difference counts only if the medians lie apart by more than the two min-max ranges added",
                           parts="fused_backward_parts: lic360.cconv_dgrad (flips and transpose included), lic360.cconv_wgrad (plan, main and finish kernels), and the "
                                 "torch flips and weight transpose alone (two activation flips and one weight transpose, as dgrad makes them)",
                           memory="peak_bytes: torch.cuda.max_memory_allocated over one forward + backward, minus what was allocated before it",
                           apart="largest |fused - library| over the largest |library|, per tensor; weight gradients at kept taps only",
                           layers=layers, models=models), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
