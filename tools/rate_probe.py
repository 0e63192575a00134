"""Rate estimation (FusedCodec.estimate / FusedImpCodec.estimate, csrc/rate_kernels.hip) against the encode it stands in for, at the headline latent
48 x 64 x 128 with 64 and 192 images and on the importance codec's 32 x 64 maps:
  encode    the whole encode, the serial coder included (the only way to a rate before);
  estimate  the same launches up to the per-symbol records, then k_rate_sum with both breakdowns instead of the coder;
  kernel    lic360_*_rate_last alone: the reduction over the records the last call left (its output memsets included), with and without breakdowns.
The forms alternate in one process: --repeats (9) repeats of --calls (2) calls each after one warm-up call, timed with device events; median
(min - max) ms per call.  GB/s of the kernel: the records (8 bytes each) and, with a breakdown, the bucket indices (4 bytes per record) read once, over
the median time.  The calibration line is bench.py's: the fp32 MFMA rate and a 1 GiB device copy on this box, in this process.  --json FILE keeps the
table (default profiles/rate_probe.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("360-image-compression_amd", "tests", ""):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, calls, warm=1):
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


def stats(v):
    return {"median_ms": sorted(v)[len(v) // 2], "min_ms": min(v), "max_ms": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "rate_probe.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--batches", type=int, nargs="*", default=[64, 192])
    ap.add_argument("--parent", help="the commit this build's parent is (kept in the JSON: the figures belong to a build on top of it)")
    args = ap.parse_args()
    import bench
    import lic360
    from lic360 import _lib, _p, _stream
    from lic360_fused import FusedCodec, FusedImpCodec
    from util import make_latent, make_main_params, make_imp_params
    dev = "cuda:0"
    calib = bench.calibrate(0)
    print("calibration %s" % calib, flush=True)
    G, H, W, MH, MW = 48, 64, 128, 32, 64
    rows = []
    for B in args.batches:
        rng = np.random.default_rng(7)
        items = [make_latent("smooth", rng, G, H, W) for _ in range(8)]                 # SURVEY 8d's latents, eight of them tiled over the batch
        code = torch.from_numpy(np.concatenate([items[i % 8][0] for i in range(B)], 0)).to(dev)
        mask = torch.from_numpy(np.concatenate([items[i % 8][1] for i in range(B)], 0)).to(dev)
        levels = torch.from_numpy(np.concatenate([items[i % 8][2] for i in range(B)], 0)).to(dev).contiguous()
        fc, ic = FusedCodec(G, H, W, max_batch=B), FusedImpCodec(MH, MW, max_batch=B)
        fc.load_layers(make_main_params(1003, G))
        ic.load_layers(make_imp_params(1003))
        for name, codec, inputs, n, nb in (("latent %dx%dx%d" % (G, H, W), fc, (code, mask), G * H * W, (G, H)), ("importance %dx%d" % (MH, MW), ic, (levels,), MH * MW, (H // 2,))):
            outs = [torch.empty((B,), dtype=torch.int64, device=dev) for _ in range(2)] + [torch.empty((B, k), dtype=torch.int64, device=dev) for k in nb]
            last = _lib.lic360_codec_rate_last if codec is fc else _lib.lic360_impcodec_rate_last
            none = [None] * len(nb)
            forms = {"encode": lambda: codec.encode_async(*inputs),
                     "estimate": lambda: codec.estimate_async(*inputs, **({"groups": True, "rows": True} if codec is fc else {"rows": True})),
                     "kernel_breakdown": lambda: lic360._chk(last(_stream(0), codec._h, B, *[_p(t) for t in outs])),
                     "kernel_total": lambda: lic360._chk(last(_stream(0), codec._h, B, _p(outs[0]), _p(outs[1]), *[_p(t) for t in none]))}
            t = {k: [] for k in forms}
            for _ in range(args.repeats):
                for k, fn in forms.items():
                    t[k].append(timed(fn, args.calls))
            assert int(codec.err[:B].abs().sum().item()) == 0
            est = codec.estimate(*inputs)
            row = {"codec": name, "batch": B, "records_per_image": n, "mean_bits_per_image": float(est.bits.mean()), "mean_symbols_per_image": float(est.symbols.double().mean())}
            for k, v in t.items():
                row[k] = stats(v)
            row["kernel_breakdown"]["GBps"] = B * n * 12.0 / row["kernel_breakdown"]["median_ms"] / 1e6
            row["kernel_total"]["GBps"] = B * n * 8.0 / row["kernel_total"]["median_ms"] / 1e6
            row["estimate_over_encode"] = row["estimate"]["median_ms"] / row["encode"]["median_ms"]
            rows.append(row)
            print("%-22s batch %3d   encode %.3f (%.3f - %.3f) ms   estimate %.3f (%.3f - %.3f) ms   kernel with breakdowns %.4f (%.4f - %.4f) ms %.0f GB/s   "
                  "totals only %.4f (%.4f - %.4f) ms %.0f GB/s" % (
                      name, B, *[row["encode"][k] for k in ("median_ms", "min_ms", "max_ms")], *[row["estimate"][k] for k in ("median_ms", "min_ms", "max_ms")],
                      *[row["kernel_breakdown"][k] for k in ("median_ms", "min_ms", "max_ms", "GBps")],
                      *[row["kernel_total"][k] for k in ("median_ms", "min_ms", "max_ms", "GBps")]), flush=True)
        del fc, ic
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), calibration=calib, parent_commit=args.parent,
                           repeats="median (min - max) of %d alternating repeats of %d calls each after one warm-up call; device events; ms per call" % (args.repeats, args.calls),
                           bytes="GBps: 8 bytes per record and, with breakdowns, 4 bytes of bucket indices per record, read once, over the median time",
                           coder="encode: the codec's default coder mode (the device coder at these batch sizes)", rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
