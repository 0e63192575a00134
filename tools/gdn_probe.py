"""The one-pass GDN in fp32 (lic360.gdn_forward, k_gdn) against its split-bf16 form (lic360.gdn_bf16x3_forward, k_gdn_b3) on the six GDN calls of an image
pair -- ResidualBlockDown's on 260x516, 132x260 and 68x132 maps (forward), ResidualBlockUp's on 68x132, 132x260 and 260x516 (inverse), 192 channels --
at batch 8 (tools/transform_bench.py's chunk) and batch 1.  The two forms alternate in one process: 5 repeats of 10 launches each, each after 3 warm-up
launches; median (min - max) ms per launch, and the achieved bytes/s against the 8 bytes per element the pass moves (x read once, out written once).
The acceptance rule of DESIGN 7c'' / 7c''': on a shape the new form passes if its median lies below the fp32 median by more than the two min-max spreads
added.  --json FILE keeps the table (default profiles/gdn_bf16x3_probe.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "360-image-compression_amd"))
import torch  # noqa: E402

C = 192
MAPS = ((260, 516), (132, 260), (68, 132))
HBM_GBPS = 8000.0


def timed(fn, launches=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "gdn_bf16x3_probe.json"))
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import lic360
    dev = "cuda:0"
    torch.manual_seed(0)
    gamma = torch.rand((C, C), device=dev) * 0.02 + 0.1 * torch.eye(C, device=dev)
    beta = torch.rand((C,), device=dev) + 0.5
    packed = lic360.gdn_bf16x3_pack(gamma)
    rows = []
    for batch in (8, 1):
        for inverse, maps in ((False, MAPS), (True, MAPS[::-1])):
            for h, w in maps:
                x = torch.randn((batch, C, h, w), device=dev)
                out = torch.empty_like(x)
                forms = {"fp32": lambda: lic360.gdn_forward(x, gamma, beta, inverse, out),
                         "bf16x3": lambda: lic360.gdn_bf16x3_forward(x, packed, beta, inverse, out)}
                t = {k: [] for k in forms}
                for _ in range(args.repeats):
                    for k, fn in forms.items():
                        t[k].append(timed(fn))
                med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
                spread = {k: max(v) - min(v) for k, v in t.items()}
                nbytes = 8.0 * x.numel()
                row = {"shape": "%s %dx%d" % ("up (inverse)" if inverse else "down", h, w), "batch": batch, "channels": C, "bytes_per_launch": nbytes,
                       "passes": bool(med["fp32"] - med["bf16x3"] > spread["fp32"] + spread["bf16x3"])}
                for k, v in t.items():
                    row[k] = {"median_ms": med[k], "min_ms": min(v), "max_ms": max(v), "GBps": nbytes / med[k] / 1e6, "frac_of_hbm": nbytes / med[k] / 1e6 / HBM_GBPS}
                row["speedup"] = med["fp32"] / med["bf16x3"]
                rows.append(row)
                print("%-22s batch %d   fp32 %.4f (%.4f - %.4f) ms   bf16x3 %.4f (%.4f - %.4f) ms   %.2fx   %.0f GB/s   %s" % (
                    row["shape"], batch, med["fp32"], min(t["fp32"]), max(t["fp32"]), med["bf16x3"], min(t["bf16x3"]), max(t["bf16x3"]), row["speedup"],
                    row["bf16x3"]["GBps"], "passes" if row["passes"] else "FAILS the rule"), flush=True)
                del x, out
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), forms=["fp32", "bf16x3"],
                           repeats="median of %d alternating repeats of 10 launches, each after 3 warm-up launches; ms per launch" % args.repeats,
                           rule="passes: the bf16x3 median lies below the fp32 median by more than the two min-max spreads added",
                           bytes="8 bytes per element: x read once, out written once; frac_of_hbm against %.0f GB/s" % HBM_GBPS, rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
