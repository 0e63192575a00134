"""The argument contract of the sphere convolutions' C entry points (csrc/conv3x3_kernels.hip: sconv_ok, sconv_narrow_ok, sconv_plan, s3_pack / b3_pack), as a
list of calls and what each returned when the list was recorded: tests/golden/sconv_contract.json.  tests/test_sconv_contract_cpu.py replays every row against the
built library.  The GPU tests prove that a valid call computes what it did; this pins WHICH calls are valid.

Pure entry points (every *_supported, *_packed_floats, *_packed_bytes) are recorded by value over a grid of channel counts.  Launch and pack entry points are
recorded as "refused" (return code 2, the ARG_CHECK code) or not, from one or two valid base calls per entry point: every field mutated alone over a value list,
every pointer null and off a 16-byte boundary by 4 and by 8 bytes, and the fields the contract couples mutated together.  Pointers point into a 16-byte aligned
host buffer that nobody dereferences: a refusal precedes any launch, and WITHOUT a device a call that passes the contract ends in "kernel launch failed: no
ROCm-capable device is detected" (return code 1).  With a device visible such a call would launch on host pointers, so nothing here runs then.

    python tests/sconv_contract_cases.py <library>      writes the golden from that library (the sources beside it: <library's directory>/csrc), and checks
                                                         that every ARG_CHECK statement of the host half of conv3x3_kernels.hip refused at least one row"""
import ctypes
import itertools
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sconv_contract.json")

# ---- the pure entry points
CINS = (0, 3, 8, 16, 32, 48, 96, 192, 200, 384)
COUTS = (0, 48, 96, 100, 192, 288, 384, 768)
NARROW_FORMS, NARROW_KS, NARROW_CPWS = (-1, 0, 1, 2, 3, 4), (1, 3, 5), (0, 24, 48, 96, 144, 192)
PURE = tuple("lic360_sconv%s%s_%s" % (ks, form, what) for form, size in (("", "packed_floats"), ("_bf16x3", "packed_bytes"), ("_bf16x1", "packed_bytes"))
             for ks in ("3x3", "1x1") for what in ("supported", size)) + tuple("lic360_sconv%ss2%s_supported" % (ks, form) for form in ("", "_bf16x1") for ks in ("3x3", "1x1"))

# ---- the launch and pack entry points: parameter lists behind `stream`, by kind
_OPERANDS = ("x", "packed", "bias", "slope", "residual", "out")
_GATE_OPERANDS = ("x", "packed", "bias", "trunk", "residual", "out")
_MAP = ("n", "cin", "cout", "hp", "wp")
SIGNATURES = {
    "conv3": _OPERANDS + _MAP + ("pad", "sphere", "ring", "ring_w", "out_crop", "shuffle"),
    "conv1": _OPERANDS + _MAP + ("ring", "ring_w", "out_crop", "shuffle"),
    "gate": _GATE_OPERANDS + _MAP + ("ring", "ring_w"),
    "s2_3": _OPERANDS + _MAP + ("pad", "sphere", "oring"),
    "s2_1": _OPERANDS + _MAP + ("pad", "oring"),
    "narrow": ("form", "ks", "cpw") + _OPERANDS + _MAP + ("pad", "sphere", "ring", "ring_w", "out_crop", "shuffle"),
    "gate_narrow": ("form", "cpw") + _GATE_OPERANDS + _MAP + ("ring", "ring_w"),
    "pack": ("weight", "packed", "cin", "cout"),
}
POINTERS = ("x", "packed", "bias", "slope", "residual", "trunk", "out", "weight")
FORMS = ("", "_bf16x3", "_bf16x1")
ENTRIES = tuple(("lic360_sconv3x3" + f, "conv3") for f in FORMS) + tuple(("lic360_sconv1x1" + f, "conv1") for f in FORMS) + \
    tuple(("lic360_sconv1x1_gate" + f, "gate") for f in FORMS) + \
    tuple(("lic360_sconv3x3s2" + f, "s2_3") for f in ("", "_bf16x1")) + tuple(("lic360_sconv1x1s2" + f, "s2_1") for f in ("", "_bf16x1")) + \
    (("lic360_sconv_narrow", "narrow"), ("lic360_sconv1x1_gate_narrow", "gate_narrow")) + \
    tuple(("lic360_sconv%s%s_pack" % (ks, f), "pack") for f in FORMS for ks in ("3x3", "1x1"))

# a pointer is None or a byte offset into the aligned buffer; the base calls are valid: 192 -> 192 and 96 -> 96 channels on a 20 x 36 map, 36 x 36 at stride 2
_BASE = dict(x=0, packed=0, bias=0, slope=0, residual=None, trunk=0, out=0, weight=0, n=1, cin=192, cout=192, hp=20, wp=36, pad=2, sphere=1, ring=2, ring_w=2,
             out_crop=0, shuffle=0, oring=2, form=0, ks=3, cpw=96)
_C96 = dict(cin=96, cout=96)


def bases(kind):
    """name -> the valid calls of a kind of entry point"""
    if kind in ("s2_3", "s2_1"):
        return {"192": dict(_BASE, hp=36), "96": dict(_BASE, hp=36, **_C96)}
    if kind == "gate":
        return {"192": dict(_BASE, residual=0), "96": dict(_BASE, residual=0, **_C96)}
    if kind == "narrow":
        return {"192": _BASE, "96": dict(_BASE, form=1, ks=1, cpw=48, pad=0, sphere=0, **_C96)}
    if kind == "gate_narrow":
        return {"192": dict(_BASE, residual=0), "384": dict(_BASE, residual=0, form=3, cpw=48, cout=384)}
    return {"192": _BASE, "96": dict(_BASE, **_C96)}


_RINGS = (-1, 0, 1, 2, 3, 9, 10, 17, 18, 1 << 29)
_EXTENTS = (-20, 0, 1, 3, 4, 5, 7, 8, 19, 21, 35, 37, 1 << 14)
VALUES = {                                                                  # a field mutated alone
    "n": (-1, 0, 2, 1 << 30, (1 << 31) - 1), "cin": CINS, "cout": COUTS, "hp": _EXTENTS, "wp": _EXTENTS, "pad": (-1, 0, 1, 2, 3, 5, 9, 10),
    "sphere": (-1, 0, 1, 2, 3), "ring": _RINGS, "ring_w": _RINGS, "oring": _RINGS, "out_crop": (-1, 0, 1, 2, 3), "shuffle": (-1, 1, 2),
    "form": NARROW_FORMS, "ks": (0,) + NARROW_KS, "cpw": NARROW_CPWS,
}
VALUES.update((p, (None, 4, 8)) for p in POINTERS)
COUPLED = (                                                                 # fields the contract couples, mutated together
    (("ring", "ring_w"), tuple(itertools.product((0, 1, 2, 3, 9), (0, 1, 2, 3, 17)))),
    (("out_crop", "residual", "shuffle"), tuple(itertools.product((0, 1, 2), (None, 0, 4, 8), (0, 1)))),
    (("out", "shuffle"), ((4, 1), (8, 1))),
    (("pad", "sphere"), tuple(itertools.product((0, 1, 2, 5, 6, 9), (0, 1, 2)))),
    # a chunk's cells at 32-bit byte offsets: 16 channels x 2^26 cells x 4 bytes = 2^32 = 32 channels x 2^25 cells x 4 bytes
    (("hp", "wp"), ((8192, 8192), (8192, 8191), (8192, 8190), (4096, 8192), (4096, 8191), (4096, 8190), (1 << 14, 1 << 14))),
    (("n", "hp"), (((1 << 30) - 1, 68), (1 << 30, 68), ((1 << 31) - 1, 68), (1 << 30, 36))),      # 2^31 tiles (stride 2: two tile rows at 68)
    (("ks", "pad", "sphere"), ((1, 0, 0), (1, 2, 0), (1, 0, 1), (1, 2, 1), (1, 1, 2))),                # the narrow entry's 1x1 takes no apron
    (("cpw", "cin", "cout"), ((96, 96, 96), (48, 96, 96), (96, 192, 192), (48, 192, 192), (96, 192, 384), (192, 192, 384), (48, 192, 288), (96, 192, 768))),
)


def groups():
    """every group of rows: (entry point, kind, base name, fields mutated together, their value tuples)"""
    for name, kind in ENTRIES:
        sig = SIGNATURES[kind]
        for bname in sorted(bases(kind)):
            for f in sig:
                yield name, kind, bname, (f,), tuple((v,) for v in VALUES[f])
            for fields, values in COUPLED:
                if all(f in sig for f in fields):
                    yield name, kind, bname, fields, values


def key(name, bname, fields):
    return "%s %s %s" % (name, bname, ",".join(fields))


# ---- running them
def load(path):
    """the library at `path`, typed by lic360/_abi_table.py (read as a file: importing the package would load the tree's own library)"""
    scope = {}
    exec(open(os.path.join(ROOT, "360-image-compression_amd", "lic360", "_abi_table.py")).read(), scope)
    lib = ctypes.CDLL(path)
    for name, (res, args) in scope["ABI"].items():
        if "sconv" in name or name == "lic360_last_error":
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = getattr(ctypes, res), [getattr(ctypes, a) for a in args]
    return lib


def device_visible():
    import torch
    return torch.cuda.device_count() > 0


def record(lib, reported=None):
    """{"pure": {entry point: values over the grid}, "calls": {group: one character per row, "1" = refused}}; reported: a set that receives the file:line of
    every refusal's message"""
    if device_visible():
        raise RuntimeError("a GPU is visible: a call that passes the contract would launch on host pointers")
    pure = {name: [getattr(lib, name)(cin, cout) for cin in CINS for cout in COUTS] for name in PURE}
    for form, ks, cpw in itertools.product(NARROW_FORMS, NARROW_KS, NARROW_CPWS):
        pure["lic360_sconv_narrow_supported %d %d %d" % (form, ks, cpw)] = "".join(
            str(lib.lic360_sconv_narrow_supported(form, ks, cin, cout, cpw)) for cin in CINS for cout in COUTS)
    buf = (ctypes.c_char * 256)()
    origin = ctypes.addressof(buf)
    origin += (-origin) % 16 + 64
    calls = {}
    for name, kind, bname, fields, values in groups():
        fn, base, out = getattr(lib, name), bases(kind)[bname], ""
        for vs in values:
            v = dict(base, **dict(zip(fields, vs)))
            rc = fn(None, *(((None if v[f] is None else origin + v[f]) if f in POINTERS else v[f]) for f in SIGNATURES[kind]))
            out += "1" if rc == 2 else "0"
            if rc == 2 and reported is not None:
                reported.add(re.search(rb"\(([^()]*:\d+)\)$", lib.lic360_last_error()).group(1).decode())
        assert key(name, bname, fields) not in calls
        calls[key(name, bname, fields)] = out
    return {"pure": pure, "calls": calls}


def arg_checks(source):
    """(first line, last line) of every ARG_CHECK statement of the host half of conv3x3_kernels.hip (from sconv_ck to the end of the file)"""
    lines = open(source).read().split("\n")
    start = next(i for i, l in enumerate(lines) if "sconv_ck(" in l)
    spans, i = [], start
    while i < len(lines):
        if re.match(r"\s*ARG_CHECK\(", lines[i]):
            j = i
            while not lines[j].split("//")[0].rstrip().endswith(");"):
                j += 1
            spans.append((i + 1, j + 1))
            i = j
        i += 1
    return spans


def main(path):
    lib, reported = load(path), set()
    rec = record(lib, reported)
    lines = set(int(r.rsplit(":", 1)[1]) for r in reported if r.rsplit(":", 1)[0].endswith("conv3x3_kernels.hip"))
    silent = [s for s in arg_checks(os.path.join(os.path.dirname(os.path.abspath(path)), "csrc", "conv3x3_kernels.hip")) if not lines & set(range(s[0], s[1] + 1))]
    assert not silent, "ARG_CHECK statements that no row trips (lines): %s" % silent
    with open(GOLDEN, "w") as f:                                            # one group per line
        f.write("{\n" + ",\n".join('"%s": {\n%s\n}' % (part, ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in sorted(rec[part].items())))
                                   for part in ("pure", "calls")) + "\n}\n")
    rows = sum(len(v) for v in rec["calls"].values()) + sum(len(v) for v in rec["pure"].values())
    print("%d rows in %d groups, %d refused, %d ARG_CHECK lines reported -> %s" % (rows, len(rec["calls"]) + len(rec["pure"]), sum(v.count("1") for v in rec["calls"].values()),
                                                                                  len(lines), GOLDEN))


if __name__ == "__main__":
    main(sys.argv[1])
