"""A/B of the decode-order dead-cone lists on 128-row latents ("Tall latents"): bench.py's configuration 5 -- 1024 x 2048 ERPs,
48 x 128 x 256 latents, 16 images on each of three streams, both bitstreams, the latent decode gated behind the importance map's -- run in ONE
process on two sets of codecs, one created under LIC360_DC_NOTALL=1 (row-segment kernels, as before the tall lists) and one without, alternating.

  python tools/dc_tall_probe.py [--repeats 5] [--out profiles/dc_tall_lists_probe.json]

Per repeat and variant: the time of two steps (encode + decode of all 48 images), as bench.py times config 5.  Once per variant: the per-launch
times of the decode-order layer classes of one sub-batch alone on the GPU (the codec's own event profile), and what the lists execute of the hidden
and last layers' MACs (skip_stats, priced with bench.py's chain_macs).  Round trips are checked after the last repeat."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("", "tests", "360-image-compression_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np                                                          # noqa: E402
import torch                                                                # noqa: E402

import bench                                                                # noqa: E402
from lic360_fused import FusedCodec, FusedImpCodec                          # noqa: E402
from util import make_imp_params, make_main_params                          # noqa: E402

G, H5, W5, B5, NS = bench.G, 2 * bench.H, 2 * bench.W, 16, 3


class Variant(object):
    def __init__(self, notall, dev, data):
        old = os.environ.pop("LIC360_DC_NOTALL", None)
        if notall:
            os.environ["LIC360_DC_NOTALL"] = "1"
        try:
            self.c = [FusedCodec(G, H5, W5, max_batch=B5) for _ in range(NS)]
        finally:
            os.environ.pop("LIC360_DC_NOTALL", None)
            if old is not None:
                os.environ["LIC360_DC_NOTALL"] = old
        self.i = [FusedImpCodec(H5 // 2, W5 // 2, max_batch=B5) for _ in range(NS)]
        l5, il5 = make_main_params(1000 * bench.SSIM + 7, G), make_imp_params(1000 * bench.SSIM + 7)
        for c in self.c:
            c.load_layers(l5)
        for c in self.i:
            c.load_layers(il5)
        self.cd, self.mk, self.lv = data
        self.mb = [torch.zeros_like(m) for m in self.mk]
        self.ev = [torch.cuda.Event() for _ in self.mk]
        self.st = [torch.cuda.Stream(dev) for _ in range(NS)]
        self.ist = [torch.cuda.Stream(dev) for _ in range(NS)]
        self.active = self.c[0].skip_active()

    def step(self):                                                         # (bench.py: run5)
        for c, ic, a, b_, l_, st, ist in zip(self.c, self.i, self.cd, self.mk, self.lv, self.st, self.ist):
            with torch.cuda.stream(ist):
                ic.encode_async(l_)
            with torch.cuda.stream(st):
                c.encode_async(a, b_)
        for c, ic, st, ist, mb, ev in zip(self.c, self.i, self.st, self.ist, self.mb, self.ev):
            ist.wait_event(ev)
            with torch.cuda.stream(ist):
                gate = ic.decode_masked_async(B5, mb)
            with torch.cuda.stream(st):
                c.decode_async(mb, B5, gate=gate)
                ev.record(st)

    def timed(self, steps, dev):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / steps

    def exact(self):
        ok = all(bool(torch.equal(c.code_out[:B5], a * b_)) and int(c.err[:B5].abs().sum().item()) == 0 for c, a, b_ in zip(self.c, self.cd, self.mk))
        return ok and all(bool(torch.equal(mb, m)) for mb, m in zip(self.mb, self.mk))

    def alone(self, dev):
        """sub-batch 0 alone on the GPU: per-launch times of the decode-order classes, and the executed fraction of their MACs"""
        c = self.c[0]
        with torch.cuda.stream(self.st[0]):
            c.encode_async(self.cd[0], self.mk[0])
        torch.cuda.synchronize(dev)
        c.skip_stats(True)
        with torch.cuda.stream(self.st[0]):
            c.decode_async(self.mk[0], B5)
        torch.cuda.synchronize(dev)
        dec = c.skip_stats(False, read=True)[1]
        frac = {}
        for cls, layers in (("dc_hidden", range(1, 11)), ("dc_last", (11,))):
            num = den = 0.0
            for l in layers:
                cm = bench.chain_macs(l)
                den += 3.0 * B5 * H5 * W5 * cm.sum()
                num += float((dec[l, :G].astype(np.float64) * cm).sum()) if self.active == 2 else 3.0 * B5 * H5 * W5 * cm.sum()
            frac[cls] = num / den
        c.profile(True)
        with torch.cuda.stream(self.st[0]):
            c.decode_async(self.mk[0], B5)
        torch.cuda.synchronize(dev)
        prof = c.profile_read()
        c.profile(False)
        return {k: {"avg_launch_us": ms / n * 1e3, "launches": n} for k, (ms, n) in prof.items() if n and k.startswith("dc_")}, frac


def med(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "all": [float(x) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dc_tall_lists_probe.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    cd, mk, lv = bench.synth_latents(B5 * NS, seed0=5000000, h=H5, w=W5)
    data = tuple([torch.from_numpy(a[i * B5:(i + 1) * B5]).to(dev) for i in range(NS)] for a in (cd, mk, lv))
    variants = {"row_segments": Variant(True, dev, data), "tall_lists": Variant(False, dev, data)}
    assert variants["row_segments"].active == 1 and variants["tall_lists"].active == 2
    times = {k: [] for k in variants}
    for v in variants.values():
        v.timed(1, dev)                                                     # warm-up
    for _ in range(args.repeats):
        for k, v in variants.items():
            times[k].append(v.timed(2, dev))
    res = {"config": "48 x %d x %d latents, %d images on %d streams, both bitstreams (bench.py config 5)" % (H5, W5, B5 * NS, NS),
           "device": torch.cuda.get_device_name(0), "repeats": args.repeats}
    for k, v in variants.items():
        launches, frac = v.alone(dev)
        res[k] = {"skip_active": v.active, "roundtrip_exact": v.exact(), "step_ms": med([t * 1e3 for t in times[k]]),
                  "mpixel_s": med([B5 * NS * 4 * bench.PIXELS / t / 1e6 for t in times[k]]),
                  "alone_per_launch": launches, "executed_mac_fraction": frac}
    a, b = res["row_segments"]["step_ms"], res["tall_lists"]["step_ms"]
    res["gain"] = {"median_step_ms": a["median"] - b["median"], "relative": 1.0 - b["median"] / a["median"],
                   "outside_the_spread": bool(b["max"] < a["min"])}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
