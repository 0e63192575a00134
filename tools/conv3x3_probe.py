"""lic360_sconv3x3 (csrc/conv3x3_kernels.hip) next to torch.nn.functional.conv2d (MIOpen) on the transforms' 3x3 stride-1 shapes, batch 8:
correctness (max |diff| against conv2d over the sphere-padded map, fp32) and time per launch -- the library form timed WITH the launches the
fused kernel absorbs (in-place apron refresh, PReLU, trim) and without.  VERDICT r4 next #2.
--precision bf16x3: "ours" is the split-bf16 form (lic360_sconv3x3_bf16x3 / sconv1x1_bf16x3), timed in the same run next to the fp32 kernel.
--precision bf16x1: "ours" is the single-pass bf16 form (lic360_sconv3x3_bf16x1 / sconv1x1_bf16x1); fp32, bf16x3 and bf16x1 launches alternate in the same
run (median, min, max of 5 repeats of 10 launches), and --json FILE keeps that table.
--s2: the stride-2 forms instead (lic360_sconv3x3s2 / sconv1x1s2) on the analysis transform's three down-sampling shapes and two shortcuts, batches
1, 2, 4, 8, 32, each next to the library form of the same work (in-place SpherePad + conv2d(stride 2) + PReLU; shortcut conv2d + add + trim): median
of alternating repeats with the spread, and the smallest tile count from which the native form is not slower on any shape; --json FILE keeps the table.
--s2 --precision bf16x1: the single-pass bf16 stride-2 forms (lic360_sconv3x3s2_bf16x1 / sconv1x1s2_bf16x1) next to the fp32 stride-2 kernel on the five
production shapes at batch 8, launches alternating in one process (median, min, max of 5 repeats of 10 launches), and the rule for a form per shape: the
bf16x1 median lies below the fp32 median by more than the two min-max spreads added; --json FILE keeps the table.
--narrow: the narrow-workgroup forms (lic360.sconv3x3_narrow / sconv1x1_narrow / sconv1x1_gate_narrow, cpw 96 and 48, in fp32, bf16x3 and bf16x1) on the layers
whose wide launch has too few workgroups -- the 132 x 260 and 68 x 132 layers at batch 1, the 36 x 68 layers at batch 8 -- each next to the LIBRARY form of the
same layer (fp32 torch: what the models run there without small="narrow") and to the wide kernel, launches alternating in one process (median, min, max of 5
repeats of 10 launches); the rule per (layer, form, cpw): the narrow median lies below the library median by more than the two min-max spreads added;
--json FILE (default profiles/sconv_narrow_probe.json) keeps the table."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "360-image-compression_amd"))
import torch
import torch.nn.functional as F
import lic360

dev = "cuda:0"
ap = argparse.ArgumentParser()
ap.add_argument("--precision", choices=("fp32", "bf16x3", "bf16x1"), default="fp32")
ap.add_argument("--s2", action="store_true")
ap.add_argument("--narrow", action="store_true")
ap.add_argument("--json", default=None)
ARGS = ap.parse_args()
B3 = ARGS.precision != "fp32"                                             # a bf16 form is "ours", timed alternating with the forms before it in FORMS
FORMS = ("fp32", "bf16x3", "bf16x1")[:("fp32", "bf16x3", "bf16x1").index(ARGS.precision) + 1]
AB_ROWS = []


def alternating(kernel, what, fns):
    """5 repeats of 10 launches of every form in turn: median, min, max ms per launch; one line (--precision bf16x3: the line that mode always printed) and, for
    --precision bf16x1, one row of the --json table"""
    t = {f: [] for f in FORMS}
    for _ in range(5):
        for f in FORMS:
            t[f].append(timed(fns[f]))
    row = dict(layer=what)
    for f in FORMS:
        row.update({f + "_ms": sorted(t[f])[2], f + "_min": min(t[f]), f + "_max": max(t[f])})
    if ARGS.precision == "bf16x3":
        print("    bf16x3 vs fp32 %s, 5 alternating repeats: fp32 %.3f ms (min %.3f max %.3f), bf16x3 %.3f ms (min %.3f max %.3f), speedup %.2f" % (
            kernel, row["fp32_ms"], row["fp32_min"], row["fp32_max"], row["bf16x3_ms"], row["bf16x3_min"], row["bf16x3_max"], row["fp32_ms"] / row["bf16x3_ms"]), flush=True)
        return
    AB_ROWS.append(row)
    print("    %s, 5 alternating repeats: %s, speedup over fp32 %s" % (
        what, ", ".join("%s %.3f ms (min %.3f max %.3f)" % (f, row[f + "_ms"], row[f + "_min"], row[f + "_max"]) for f in FORMS),
        " / ".join("%.2f" % (row["fp32_ms"] / row[f + "_ms"]) for f in FORMS[1:])), flush=True)


def timed(fn, reps=10):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def s2_probe():
    rows = []
    batches = [int(v) for v in os.environ.get("S3_BATCHES", "1,2,4,8,32").split(",")]
    pad_op, trim_op = lic360.SpherePadOp(2, True, 0, False), lic360.SphereTrimOp(2, 0, False)
    for ks, hp, wp, what in ((3, 260, 516, "stage-2 conv1"), (3, 132, 260, "stage-3 conv1"), (3, 68, 132, "SphereConv2"),
                             (1, 260, 516, "stage-2 shortcut"), (1, 132, 260, "stage-3 shortcut")):
        for n in batches:
            c = 192
            oh, ow = (hp - 4) // 2, (wp - 4) // 2
            x = torch.randn(n, c, hp, wp, device=dev)
            w = torch.randn(c, c, ks, ks, device=dev) * 0.05
            b, sl = torch.randn(c, device=dev), torch.rand(c, device=dev) * 0.5
            res = torch.randn(n, c, oh + 4, ow + 4, device=dev)
            out = torch.zeros(n, c, oh + 4, ow + 4, device=dev)
            if ks == 3:
                pk = lic360.sconv3x3_pack(w)
                slope = None if what == "SphereConv2" else sl
                def lib():                                                  # SpherePad in place + conv + PReLU (SphereConv2: + trim, no PReLU)
                    y = F.conv2d(pad_op.forward(x)[0], w, b, 2, 3)
                    return trim_op.forward(y)[0] if slope is None else F.prelu(y, slope)
                ours = lambda: lic360.sconv3x3s2(x, pk, b, slope, None, out, pad=2, sphere=True, oring=2)
            else:
                pk = lic360.sconv1x1_pack(w)
                lib = lambda: trim_op.forward(F.conv2d(x, w, b, 2, 2) + res)[0]      # shortcut + the block's add + its final trim
                ours = lambda: lic360.sconv1x1s2(x, pk, b, None, res, out, pad=2, oring=2)
            win = (slice(None), slice(None), slice(2, 2 + oh), slice(2, 2 + ow))
            err = (ours()[win] - lib()[win]).abs().max().item()
            tl, to = [], []
            for _ in range(5):                                              # alternating repeats
                tl.append(timed(lib, 40))
                to.append(timed(ours, 40))
            tiles = n * ((oh + 15) // 16) * ((ow + 15) // 16)
            row = dict(layer=what, ks=ks, n=n, hp=hp, wp=wp, tiles=tiles, max_abs_diff=err, library_ms=sorted(tl)[2], library_min=min(tl), library_max=max(tl),
                       native_ms=sorted(to)[2], native_min=min(to), native_max=max(to), native_over_library=sorted(to)[2] / sorted(tl)[2])
            rows.append(row)
            print("s2 %dx%d %-16s @%dx%d x%-2d (%4d tiles): max|diff| %.2e | library %.3f ms (%.3f .. %.3f) | native %.3f ms (%.3f .. %.3f) | native / library = %.2f" % (
                ks, ks, what, hp, wp, n, tiles, err, row["library_ms"], row["library_min"], row["library_max"], row["native_ms"], row["native_min"], row["native_max"],
                row["native_over_library"]), flush=True)
            del x, res, out
    # the smallest tile count from which the native form is not slower (medians) on every measured (shape, batch) with at least that many tiles
    counts = sorted({r["tiles"] for r in rows})
    thr = None
    for t in reversed(counts):
        if all(r["native_over_library"] <= 1.0 for r in rows if r["tiles"] >= t):
            thr = t
        else:
            break
    print("smallest tile count from which the native form is not slower on any measured shape: %s" % thr, flush=True)
    if ARGS.json:
        with open(ARGS.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), repeats="median of 5 alternating repeats of 40 launches, each after 3 warm-up launches; ms per launch",
                           threshold_tiles=thr, rows=rows), f, indent=1)


def s2_bf16x1_probe():
    rows, n, c = [], int(os.environ.get("S3_N", "8")), 192
    for ks, hp, wp, what in ((3, 260, 516, "stage-2 conv1"), (3, 132, 260, "stage-3 conv1"), (3, 68, 132, "SphereConv2"),
                             (1, 260, 516, "stage-2 shortcut"), (1, 132, 260, "stage-3 shortcut")):
        oh, ow = (hp - 4) // 2, (wp - 4) // 2
        x = torch.randn(n, c, hp, wp, device=dev)
        w = torch.randn(c, c, ks, ks, device=dev) * 0.05
        b, sl = torch.randn(c, device=dev), torch.rand(c, device=dev) * 0.5
        res = torch.randn(n, c, oh + 4, ow + 4, device=dev)
        outs = {f: torch.zeros(n, c, oh + 4, ow + 4, device=dev) for f in ("fp32", "bf16x1")}
        if ks == 3:
            slope = None if what == "SphereConv2" else sl
            pk, pb = lic360.sconv3x3_pack(w), lic360.sconv3x3_bf16x1_pack(w)
            fns = {"fp32": lambda: lic360.sconv3x3s2(x, pk, b, slope, None, outs["fp32"], pad=2, sphere=True, oring=2),
                   "bf16x1": lambda: lic360.sconv3x3s2_bf16x1(x, pb, b, slope, None, outs["bf16x1"], pad=2, sphere=True, oring=2)}
        else:
            pk, pb = lic360.sconv1x1_pack(w), lic360.sconv1x1_bf16x1_pack(w)
            fns = {"fp32": lambda: lic360.sconv1x1s2(x, pk, b, None, res, outs["fp32"], pad=2, oring=2),
                   "bf16x1": lambda: lic360.sconv1x1s2_bf16x1(x, pb, b, None, res, outs["bf16x1"], pad=2, oring=2)}
        err = (fns["bf16x1"]() - fns["fp32"]()).abs().max().item()
        t = {f: [] for f in fns}
        for _ in range(5):                                                  # alternating repeats
            for f in fns:
                t[f].append(timed(fns[f]))
        row = dict(layer=what, ks=ks, n=n, hp=hp, wp=wp, tiles=n * ((oh + 15) // 16) * ((ow + 15) // 16), max_abs_diff_to_fp32=err)
        for f in fns:
            row.update({f + "_ms": sorted(t[f])[2], f + "_min": min(t[f]), f + "_max": max(t[f])})
        spreads = (row["fp32_max"] - row["fp32_min"]) + (row["bf16x1_max"] - row["bf16x1_min"])
        row.update(speedup=row["fp32_ms"] / row["bf16x1_ms"], spreads_added=spreads, passes=bool(row["fp32_ms"] - row["bf16x1_ms"] > spreads))
        rows.append(row)
        print("s2 %dx%d %-16s @%dx%d x%d (%4d tiles): max|bf16x1 - fp32| %.2e | fp32 %.3f ms (%.3f .. %.3f) | bf16x1 %.3f ms (%.3f .. %.3f) | fp32 / bf16x1 = %.2f | "
              "median gap %.3f ms vs spreads %.3f ms: %s" % (ks, ks, what, hp, wp, n, row["tiles"], err, row["fp32_ms"], row["fp32_min"], row["fp32_max"], row["bf16x1_ms"],
                                                           row["bf16x1_min"], row["bf16x1_max"], row["speedup"], row["fp32_ms"] - row["bf16x1_ms"], spreads,
                                                           "passes" if row["passes"] else "DOES NOT PASS"), flush=True)
        del x, res, outs
    if ARGS.json:
        with open(ARGS.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), forms=["fp32", "bf16x1"],
                           repeats="median of 5 repeats of 10 launches, each after 3 warm-up launches, the two forms alternating within a repeat; ms per launch",
                           rule="a shape passes when fp32_ms - bf16x1_ms > (fp32_max - fp32_min) + (bf16x1_max - bf16x1_min)", rows=rows), f, indent=1)


def narrow_probe():
    c, rows = 192, []
    pad_op, trims = lic360.SpherePadOp(2, True, 0, False), {r: lic360.SphereTrimOp(r, 0, False) for r in (1, 2)}
    # (name, ks, cin, cout, ring, ring_w, sphere, prelu, residual, crop / shuffle, gate)
    layers = [("V2 conv1", 3, c, c, 1, 2, 1, True, False, False, False), ("V2 conv2", 3, c, c, 2, 2, 2, True, True, False, False),
              ("GDN conv2", 3, c, c, 2, 2, 1, False, False, False, False), ("bottleneck 1x1 in", 1, c, c // 2, 2, 2, 0, True, False, False, False),
              ("bottleneck 3x3", 3, c // 2, c // 2, 2, 2, 1, True, False, False, False), ("bottleneck 1x1 out", 1, c // 2, c, 2, 2, 0, False, True, False, False),
              ("gate", 1, c, c, 2, 2, 0, False, True, False, True), ("Up conv1", 3, c, 4 * c, 2, 2, 1, True, False, True, False),
              ("Up shortcut", 1, c, 4 * c, 2, 2, 0, False, True, True, False)]
    maps = [(1, 132, 260, layers[:7]), (1, 68, 132, layers[:3] + layers[7:]), (8, 36, 68, layers)]
    for n, hp, wp, ls in maps:
        for name, ks, cin, cout, ring, ring_w, sphere, prelu, has_res, up, gate in ls:
            x = torch.randn(n, cin, hp, wp, device=dev)
            w = torch.randn(cout, cin, ks, ks, device=dev) * 0.05
            b, sl = torch.randn(cout, device=dev), (torch.rand(cout, device=dev) * 0.5 if prelu else None)
            crop = 1 if up else 0
            oshape = (n, cout // 4, 2 * (hp - 2), 2 * (wp - 2)) if up else (n, cout, hp, wp)
            res = torch.randn(oshape, device=dev) if has_res else None
            trunk = torch.randn(oshape, device=dev) if gate else None
            kw = dict(ring=ring, ring_w=ring_w, crop=crop, shuffle=up)
            if ks == 3:
                kw.update(pad=2, sphere=sphere)
            if gate:
                kw = dict(ring=ring)
            sfx = lambda f: "" if f == "fp32" else "_" + f
            packs = {f: getattr(lic360, "sconv%dx%d%s_pack" % (ks, ks, sfx(f)))(w) for f in ("fp32", "bf16x3", "bf16x1")}
            outs = {}
            def out_of(key):
                if key not in outs:
                    outs[key] = torch.zeros(oshape, device=dev)
                return outs[key]
            dt = lic360.DtowOp(2, True, 0, False) if up else None
            def lib():                                                      # the library form of the layer with the launches the kernel absorbs
                if gate:
                    return res + trunk * torch.sigmoid(F.conv2d(x, w, b))
                y = F.conv2d(pad_op.forward(x)[0], w, b, 1, 1) if ks == 3 and not up else (F.conv2d(pad_op.forward(x)[0], w, b) if up and ks == 3 else F.conv2d(x[:, :, 1:-1, 1:-1] if up else x, w, b))
                if sl is not None:
                    y = F.prelu(y, sl)
                if up:
                    y = dt.forward(y)[0]
                    return trims[2].forward(y + res if res is not None else y)[0]
                y = trims[ring].forward(y)[0]
                return y + res if res is not None else y
            def wide(f):
                if gate:
                    return lambda: getattr(lic360, "sconv1x1_gate" + sfx(f))(x, packs[f], b, trunk, res, out_of(("wide", f)), **kw)
                return lambda: getattr(lic360, "sconv%dx%d%s" % (ks, ks, sfx(f)))(x, packs[f], b, sl, res, out_of(("wide", f)), **kw)
            def narrow(f, cpw):
                if gate:
                    return lambda: lic360.sconv1x1_gate_narrow(x, packs[f], b, trunk, res, out_of((cpw, f)), form=f, cpw=cpw, **kw)
                return lambda: getattr(lic360, "sconv%dx%d_narrow" % (ks, ks))(x, packs[f], b, sl, res, out_of((cpw, f)), form=f, cpw=cpw, **kw)
            fns = {"library": lib}
            for f in ("fp32", "bf16x3", "bf16x1"):
                fns["wide " + f] = wide(f)
                for cpw in (96, 48):
                    if lic360.sconv_narrow_supported(f, ks, cin, cout, cpw):
                        fns["cpw%d %s" % (cpw, f)] = narrow(f, cpw)
            same = all(torch.equal(fns["cpw%d %s" % (cpw, f)](), fns["wide " + f]()) for f in ("fp32", "bf16x3", "bf16x1") for cpw in (96, 48) if "cpw%d %s" % (cpw, f) in fns)
            t = {k: [] for k in fns}
            for _ in range(5):
                for k in fns:
                    t[k].append(timed(fns[k]))
            nr, nc = hp - 2 * ring, wp - 2 * ring_w
            row = dict(layer=name, ks=ks, cin=cin, cout=cout, n=n, hp=hp, wp=wp, tiles=n * ((nr + 15) // 16 if nr % 16 > 8 or nr % 16 == 0 else nr // 16) * ((nc + 15) // 16),
                       narrow_equals_wide=bool(same))
            for k in fns:
                key = k.replace(" ", "_")
                row.update({key + "_ms": sorted(t[k])[2], key + "_min": min(t[k]), key + "_max": max(t[k])})
                if k.startswith("cpw"):
                    spreads = (max(t[k]) - min(t[k])) + (max(t["library"]) - min(t["library"]))
                    row[key + "_passes"] = bool(sorted(t["library"])[2] - sorted(t[k])[2] > spreads)
            rows.append(row)
            print("narrow x%d %dx%d %-18s (%d -> %d, %dx%d): narrow == wide: %s | %s" % (n, hp, wp, name, cin, cout, ks, ks, same, " | ".join(
                "%s %.3f (%.3f .. %.3f)%s" % (k, sorted(t[k])[2], min(t[k]), max(t[k]), "" if not k.startswith("cpw") else (" pass" if row[k.replace(" ", "_") + "_passes"] else " NO"))
                for k in fns)), flush=True)
            del x, res, trunk, outs
    path = ARGS.json or os.path.join(ROOT, "profiles", "sconv_narrow_probe.json")
    with open(path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0),
                       repeats="median of 5 repeats of 10 launches, each after 3 warm-up launches, all forms of a layer alternating within a repeat; ms per launch",
                       rule="(layer, form, cpw) passes when library_ms - narrow_ms > (library_max - library_min) + (narrow_max - narrow_min)", rows=rows), f, indent=1)


if ARGS.narrow:
    torch.manual_seed(0)
    narrow_probe()
    sys.exit(0)

if ARGS.s2:
    torch.manual_seed(0)
    if ARGS.precision == "bf16x1":
        s2_bf16x1_probe()
    else:
        s2_probe()
    sys.exit(0)

torch.manual_seed(0)
# ring 1 = the first convolution of ResidualBlockV2: rows of the 1-ring window, columns of the interior (its 1-ring columns repeat interior columns: ring_w = 2)
shapes = [(8, 192, 192, 260, 516, 1, 0), (8, 192, 192, 260, 516, 2, 0), (8, 192, 192, 132, 260, 1, 0), (8, 192, 192, 132, 260, 2, 0),
          (8, 96, 96, 132, 260, 2, 0), (8, 192, 768, 68, 132, 2, 1), (8, 192, 768, 132, 260, 2, 1), (8, 192, 768, 36, 68, 2, 1), (8, 192, 192, 36, 68, 2, 0)]
if os.environ.get("S3_QUICK"): shapes = shapes[2:3] + shapes[6:7]
if os.environ.get("S3_N"): shapes = [(int(os.environ["S3_N"]),) + sh[1:] for sh in shapes]      # another batch size (default 8)
for (n, cin, cout, hp, wp, ring, crop) in shapes:
    x = torch.randn(n, cin, hp, wp, device=dev)
    w = torch.randn(cout, cin, 3, 3, device=dev) * 0.05
    b, sl = torch.randn(cout, device=dev), torch.rand(cout, device=dev) * 0.5
    res = torch.randn(n, cout, hp, wp, device=dev) if crop == 0 else None
    pk = lic360.sconv3x3_pack(w)
    packs = {f: getattr(lic360, "sconv3x3_%s_pack" % f)(w) for f in FORMS[1:]}
    out = torch.zeros(n, cout, hp - 2 * crop, wp - 2 * crop, device=dev)
    pad_op, trim_op = lic360.SpherePadOp(2, True, 0, False), lic360.SphereTrimOp(ring, 0, False)

    def lib(full):
        xp = pad_op.forward(x)[0] if full else x                       # in-place apron refresh
        y = F.conv2d(xp, w, b, padding=1 - crop)
        if full:
            y = F.prelu(y, sl)
            if crop == 0:
                y = trim_op.forward(y)[0]
                y = y + res
        return y

    def fp32():
        return lic360.sconv3x3(x, pk, b, sl, res, out, pad=2, sphere=True, ring=ring, crop=crop, ring_w=max(ring, 2 - 2 * crop))

    def form(f):
        if f == "fp32":
            return fp32
        return lambda: getattr(lic360, "sconv3x3_" + f)(x, packs[f], b, sl, res, out, pad=2, sphere=True, ring=ring, crop=crop, ring_w=max(ring, 2 - 2 * crop))

    ours = form(ARGS.precision)

    want = lib(True)                                                    # (refreshes x's apron in place: the fused kernel ignores it anyway)
    got = ours()
    if crop == 0:
        win = (slice(None), slice(None), slice(ring, hp - ring), slice(2, wp - 2))
        err = (got[win] - want[win]).abs().max().item()
    else:                                                               # unpadded conv: out cell (i, j) = input cell (i + 1, j + 1); window in out coords
        win = (slice(None), slice(None), slice(ring - crop, hp - crop - ring), slice(ring - crop, wp - crop - ring))
        err = (got[win] - want[win]).abs().max().item()
    t_conv, t_full, t_ours = timed(lambda: lib(False)), timed(lambda: lib(True)), timed(ours)
    fl_lib = 2.0 * n * cout * cin * 9 * (hp - 2 * crop) * (wp - 2 * crop)
    rw_ = max(ring, 2 - 2 * crop)
    fl_win = 2.0 * n * cout * cin * 9 * (hp - 2 * ring) * (wp - 2 * rw_)
    print("3x3 %d->%d @%dx%d x%d ring %d crop %d: max|diff| %.2e | MIOpen conv alone %.3f ms (%.1f TF), with pad+prelu+trim+add %.3f ms | sconv3x3 %.3f ms "
          "(%.1f TF on its %dx%d window, %.1f TF nominal) | ours / library-with-epilogue = %.2f" % (
              cin, cout, hp, wp, n, ring, crop, err, t_conv, fl_lib / t_conv / 1e9, t_full, t_ours, fl_win / t_ours / 1e9, hp - 2 * ring, wp - 2 * rw_,
              fl_lib / t_ours / 1e9, t_ours / t_full), flush=True)
    if B3:
        alternating("sconv3x3", "3x3 %d->%d @%dx%d x%d ring %d crop %d" % (cin, cout, hp, wp, n, ring, crop), {f: form(f) for f in FORMS})

# ---- the 1x1 layers of ResidualBlock on the same kernel body, against the library GEMM (+ the elementwise launch each one absorbs)
for (n, cin, cout, hp, wp, what) in [(8, 192, 96, 132, 260, "prelu"), (8, 96, 192, 132, 260, "add"), (8, 192, 192, 132, 260, "prelu")]:
    if os.environ.get("S3_N"): n = int(os.environ["S3_N"])
    x = torch.randn(n, cin, hp, wp, device=dev)
    w = torch.randn(cout, cin, 1, 1, device=dev) * 0.05
    b, sl = torch.randn(cout, device=dev), torch.rand(cout, device=dev) * 0.5
    res = torch.randn(n, cout, hp, wp, device=dev)
    pk = lic360.sconv1x1_pack(w)
    packs = dict({f: getattr(lic360, "sconv1x1_%s_pack" % f)(w) for f in FORMS[1:]}, fp32=pk)
    out = torch.zeros(n, cout, hp, wp, device=dev)
    lib = (lambda: F.prelu(F.conv2d(x, w, b), sl)) if what == "prelu" else (lambda: F.conv2d(x, w, b) + res)

    def form(f):
        conv1 = getattr(lic360, "sconv1x1" + ("" if f == "fp32" else "_" + f))
        return (lambda: conv1(x, packs[f], b, sl, None, out, ring=2)) if what == "prelu" else (lambda: conv1(x, packs[f], b, None, res, out, ring=2))

    ours = form(ARGS.precision)
    win = (slice(None), slice(None), slice(2, hp - 2), slice(2, wp - 2))
    err = (ours()[win] - lib()[win]).abs().max().item()
    t_conv, t_lib, t_ours = timed(lambda: F.conv2d(x, w, b)), timed(lib), timed(ours)
    fl = 2.0 * n * cout * cin * (hp - 4) * (wp - 4)
    print("1x1 %d->%d @%dx%d x%d + %s: max|diff| %.2e | library conv alone %.3f ms, with the %s %.3f ms | sconv1x1 %.3f ms (%.1f TF on its window) | ours / library = %.2f" % (
        cin, cout, hp, wp, n, what, err, t_conv, what, t_lib, t_ours, fl / t_ours / 1e9, t_ours / t_lib), flush=True)
    if B3:
        alternating("sconv1x1", "1x1 %d->%d @%dx%d x%d + %s" % (cin, cout, hp, wp, n, what), {f: form(f) for f in FORMS})

if ARGS.precision == "bf16x1" and ARGS.json:
    with open(ARGS.json, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), forms=list(FORMS),
                       repeats="median of 5 repeats of 10 launches, each after 3 warm-up launches, the forms alternating within a repeat; ms per launch", rows=AB_ROWS), f, indent=1)
