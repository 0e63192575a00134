"""The tail of AttentionBlock -- x + trunk * sigmoid(conv1x1(a) + bias) -- on the library (nn.Conv2d 192 -> 192 through MIOpen / rocBLAS, then sigmoid, mul and
add as three torch elementwise kernels, followed by nothing: the library path's trim sits inside the trunk) against the fused tail (one launch of
lic360.sconv1x1_gate / _bf16x3 / _bf16x1 + lic360.sphere_apron_from, as lic360_models makes it with gate="fused"), on the production operands: 192 channels on
the 132 x 260 map, batch 8 (tools/transform_bench.py's chunk) and batch 2.  The two tails alternate in one process, per precision: 5 repeats of 10 launches
each, each after 3 warm-up launches; median (min - max) ms per call.  The routing rule of DESIGN 7c'': the fused tail keeps a shape and precision only if its
median lies below the library tail's median by more than the two min-max spreads added.  --json FILE keeps the table (default profiles/sconv_gate_probe.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "360-image-compression_amd"))
import torch  # noqa: E402

C, HP, WP = 192, 132, 260


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
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "sconv_gate_probe.json"))
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import lic360
    dev = "cuda:0"
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(C, C, 1).to(dev).eval()
    rows = []
    with torch.no_grad():
        for batch in (8, 2):
            a, t, x = (torch.randn((batch, C, HP, WP), device=dev) for _ in range(3))
            out = torch.empty_like(x)
            for precision in ("fp32", "bf16x3", "bf16x1"):
                sfx = "" if precision == "fp32" else "_" + precision
                gate, packed = getattr(lic360, "sconv1x1_gate" + sfx), getattr(lic360, "sconv1x1%s_pack" % sfx)(conv.weight)

                def fused():
                    gate(a, packed, conv.bias, t, x, out, ring=2)
                    return lic360.sphere_apron_from(x, out, 2)

                forms = {"library": lambda: x + t * torch.sigmoid(conv(a)), "fused": fused}
                tm = {k: [] for k in forms}
                for _ in range(args.repeats):
                    for k, fn in forms.items():
                        tm[k].append(timed(fn))
                med = {k: sorted(v)[len(v) // 2] for k, v in tm.items()}
                spread = {k: max(v) - min(v) for k, v in tm.items()}
                row = {"shape": "%d -> %d on %dx%d" % (C, C, HP, WP), "batch": batch, "precision": precision, "tensor_bytes": 4.0 * x.numel(),
                       "passes": bool(med["library"] - med["fused"] > spread["library"] + spread["fused"]), "speedup": med["library"] / med["fused"]}
                for k, v in tm.items():
                    row[k] = {"median_ms": med[k], "min_ms": min(v), "max_ms": max(v), "ms_per_image": med[k] / batch}
                rows.append(row)
                print("batch %d  %-6s  library %.4f (%.4f - %.4f) ms   fused %.4f (%.4f - %.4f) ms   %.2fx   %s" % (
                    batch, precision, med["library"], min(tm["library"]), max(tm["library"]), med["fused"], min(tm["fused"]), max(tm["fused"]), row["speedup"],
                    "passes" if row["passes"] else "FAILS the rule"), flush=True)
            del a, t, x, out
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), tails=["library", "fused"],
                           repeats="median of %d alternating repeats of 10 launches, each after 3 warm-up launches; ms per call" % args.repeats,
                           rule="passes: the fused median lies below the library median by more than the two min-max spreads added",
                           library="nn.Conv2d(192, 192, 1) + torch.sigmoid + mul + add (the library tail is fp32 in every precision)",
                           fused="lic360.sconv1x1_gate[_bf16x3|_bf16x1] + lic360.sphere_apron_from", rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
