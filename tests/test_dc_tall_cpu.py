"""The decode-order dead-cone lists on latents of 65..128 rows, on the CPU: the packing of row windows of up to 128 rows into waves
(csrc/need.h:dcl_wave_pieces through the host-only lic360_dcl_pack_layout) against the restatement of tests/dc_tall_cases.py and against the decode
kernel's lane rules; mutations of the restatement that the cases must see; the register / scratch / argument budgets of the built kernels.
No GPU work."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "360-image-compression_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dc_tall_cases as cases                                               # noqa: E402

LIB = os.path.join(ROOT, "360-image-compression_amd", "liblic360_hip.so")
READELF = shutil.which("llvm-readelf") or "/opt/rocm/lib/llvm/bin/llvm-readelf"


@pytest.fixture(scope="module")
def L():
    import lic360 as lic
    return lic._lib


def pack(L, h, lo, hi):
    c = len(lo)
    lo_a, hi_a = (C.c_int * c)(*lo), (C.c_int * c)(*hi)
    pieces = (C.c_uint * (9 * c))()
    nw = C.c_int(0)
    assert L.lic360_dcl_pack_layout(h, c, lo_a, hi_a, pieces, C.byref(nw)) == 0, L.lic360_last_error()
    return [[int(pieces[3 * w + i]) for i in range(3)] for w in range(nw.value)]


def check_rules(h, lo, hi, waves, fields=cases.piece_fields):
    """every live row of every sample stored by exactly one piece; the kernel's lane rules"""
    rows = [np.zeros(h, np.int32) for _ in lo]
    last_k = (-1, -1)
    for wv in waves:
        assert wv[0] >> 21, "a wave holds at least one piece"
        assert len(wv) == 3, "at most three pieces per wave"
        lanes, quads, prev_last = np.zeros(64, np.int32), set(), None
        for w in wv:
            if not w >> 21:
                continue
            k, slo, shi, a0 = fields(w)
            assert lo[k] <= slo <= shi <= hi[k] < h
            assert (a0 - slo) % 4 == 0
            assert a0 + shi - slo <= 63, "a piece fits the 64 lanes"
            lanes[a0:a0 + shi - slo + 1] += 1
            assert a0 >= 2 or slo == 0, "source lanes -2, -1 exist unless they are rows above the image"
            assert a0 + shi - slo <= 61 or shi == h - 1, "source lanes 64, 65 exist unless they are rows below the image"
            if shi < hi[k]:
                assert shi - slo + 1 >= 4 and a0 <= 57, "a cut piece is worth its halo"
            q = {col // 4 for col in range(a0, a0 + shi - slo + 5)}      # band columns lane .. lane + 4
            assert max(q) < 17 and not (q & quads), "neighbouring pieces lie in different band quads"
            quads |= q
            if prev_last is not None:
                assert a0 >= ((prev_last + 4) // 4 + 1) * 4
            prev_last = a0 + shi - slo
            assert (k, slo) > last_k, "samples, and rows inside a sample, in order"
            last_k = (k, slo)
            rows[k][slo:shi + 1] += 1
        assert lanes.max() <= 1, "pieces of a wave do not overlap"
    for k in range(len(lo)):
        want = np.zeros(h, np.int32)
        if hi[k] >= lo[k]:
            want[lo[k]:hi[k] + 1] = 1
        assert np.array_equal(rows[k], want), (k, lo, hi)


@pytest.mark.parametrize("h", cases.PACK_HEIGHTS)
def test_tall_windows_are_covered_once_by_legal_pieces_and_match_the_restatement(L, h):
    cut = three = 0
    for lo, hi in cases.pack_cases(h):
        waves = pack(L, h, lo, hi)
        assert waves == cases.pack_chunk(h, lo, hi), (h, lo, hi)
        check_rules(h, lo, hi, waves)
        live = sum(1 for k in range(len(lo)) if hi[k] >= lo[k])
        assert len(waves) <= cases.waves_per_window(h) * live, "the room the codec gives a list"
        assert (live == 0) == (not waves)
        for k in range(len(lo)):
            n = sum(1 for wv in waves for w in wv if w >> 21 and cases.piece_fields(w)[0] == k)
            cut += n > 1
            three += n > 2
    assert cut > 0 and (three > 0 or h < 123), "windows cut over two, and at full height over three, waves"


def test_a_full_height_window_takes_rows_0_61_then_62_121_then_122_127(L):
    waves = pack(L, 128, [0, 10], [127, 20])
    got = [[cases.piece_fields(w) for w in wv if w >> 21] for wv in waves]
    assert got == [[(0, 0, 61, 0)], [(0, 62, 121, 2)], [(0, 122, 127, 2), (1, 10, 20, 14)]]


@pytest.mark.parametrize("h", [64, 50, 20, 7])
def test_short_latents_keep_their_words(L, h):
    """at most 64 rows: the words are what tests/test_dcl_pack.py decodes with six-bit fields (bits 25, 26 stay zero), under that file's rules"""
    rng = np.random.default_rng(h)
    for _ in range(400):
        c = int(rng.integers(1, 9))
        lo, hi = [], []
        for _k in range(c):
            kind = int(rng.integers(0, 6))
            if kind == 0:
                a, b = 1, 0
            elif kind == 1:
                a, b = 0, h - 1
            elif kind == 2:
                a = b = int(rng.integers(h))
            else:
                a = int(rng.integers(h))
                b = int(rng.integers(a, h))
            lo.append(a)
            hi.append(b)
        waves = pack(L, h, lo, hi)
        assert all(w >> 22 == 0 for wv in waves for w in wv)
        assert waves == cases.pack_chunk(h, lo, hi) == cases.pack_chunk(h, lo, hi, row_bits=6)
        check_rules(h, lo, hi, waves, fields=lambda w: (w & 7, (w >> 3) & 63, (w >> 9) & 63, (w >> 15) & 63))
        live = sum(1 for k in range(c) if hi[k] >= lo[k])
        assert len(waves) <= max(live, 1) * 2


def test_heights_past_128_rows_are_refused(L):
    lo, hi = (C.c_int * 1)(0), (C.c_int * 1)(128)
    pieces, nw = (C.c_uint * 9)(), C.c_int(0)
    assert L.lic360_dcl_pack_layout(129, 1, lo, hi, pieces, C.byref(nw)) != 0


MUTATIONS = {
    "six-bit row fields": dict(row_bits=6),
    "no halo lanes at a cut": dict(halo=0),
    "the last row off by one": None,                                        # (last_row = h - 2, set per height below)
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_the_cases_see_each_mutation_of_the_restatement(L, name):
    """a restatement with the bug must disagree with the library on at least one case -- otherwise the cases could not see that bug in the library"""
    seen = 0
    for h in cases.PACK_HEIGHTS:
        kw = MUTATIONS[name] or dict(last_row=h - 2)
        for lo, hi in cases.pack_cases(h):
            seen += cases.pack_chunk(h, lo, hi, **kw) != pack(L, h, lo, hi)
    assert seen > 0, name


def test_list_room():
    """records per XCD list and the allocation DESIGN.md 4.6 quotes for the 48 x 128 x 256 latents of 1024 x 2048 ERPs"""
    assert [cases.waves_per_window(h) for h in (64, 65, 114, 115, 128)] == [1, 2, 2, 3, 3]
    P = 128 + 256 + 48 - 2
    for B, cap, mib in ((16, 288, 181.4), (64, 1152, 725.6)):
        assert cases.list_cap(48, B, 128) == cap
        assert abs(cases.LAYERS * P * 8 * cap * 16 / 2 ** 20 - mib) < 0.05
    assert cases.list_cap(48, 16, 64) == 96


def test_the_gpu_shapes_reach_cut_windows_and_three_wave_windows():
    """what the restated builder makes of the GPU shapes' seeded batches: rows past 63 everywhere, windows cut between waves on CUT_SHAPES (and
    only there: a diagonal of the narrow shapes is at most 24 rows), full-height windows over three waves at (3, 128, 132, 16)"""
    for shape in cases.GPU_SHAPES:
        if shape == (48, 128, 24, 16):
            continue                                                        # (seconds of Python, and nothing the other narrow shapes do not show)
        G, H, W, B = shape
        _, mask = cases.batch(G, H, W, B, cases.batch_seed(shape))
        need = cases.need_maps(mask)
        past63 = cut = most = 0
        for p in range(H + W + G - 2):
            for l, recs in cases.build_records(need, G, H, W, B, p, nets=(0,)).items():
                per = {}
                for (_x, g0, _n, _gm, pieces) in recs:
                    for (smp, slo, shi, _a0) in pieces:
                        past63 += shi > 63
                        per[(g0, smp)] = per.get((g0, smp), 0) + 1
                cut += sum(1 for v in per.values() if v > 1)
                most = max([most] + list(per.values()))
        assert past63 > 0, shape
        assert (cut > 0) == (shape in cases.CUT_SHAPES), shape
        assert most == {(3, 72, 68, 16): 2, (3, 128, 132, 16): 3}.get(shape, 1), shape


def test_the_fixture_holds_the_oracles_bytes():
    """tests/golden/dc_tall_lists.npz: every shape's batch has the stored digests, and the oracle reproduces the stored bytes of one image"""
    import ref_codec as rc
    from util import make_main_params
    for shape in cases.GPU_SHAPES:
        G, H, W, B = shape
        code, mask = cases.batch(G, H, W, B, cases.batch_seed(shape))
        want = cases.golden_streams(shape, code, mask)
        assert len(want) == cases.GOLDEN_IMAGES[shape] and all(want)
        if shape == cases.GPU_SHAPES[0]:
            i = B - 1                                                       # (an i.i.d. image)
            assert rc.encode_main(code[i:i + 1], mask[i:i + 1], make_main_params(cases.weight_seed(shape), G), G) == want[i]


# ---- resources of the built kernels (the method of tests/test_kernarg_bytes.py: the gfx950 code objects' notes, read with llvm-readelf)
NEW_KERNEL = "k_cconv4v6ltILi4EE"
# mangled name -> (VGPRs, AGPRs, scratch bytes, kernel argument bytes) of the decode-order kernels as built at the parent commit d1686b9
# ("Run the first decode layer's three nets in one task per image")
PARENT = {
    "_Z11k_cconv4v6tILi1ELi3EEv9Dc3Packed7Dc3Tape": (162, 0, 0, 160),
    "_Z10k_cconv4v6ILi1ELb0ELb0ELi3EEv9Dc3Packed": (165, 0, 0, 96),
    "_Z10k_cconv4v6ILi4ELb1ELb0ELi1EEv9Dc3Packed": (163, 0, 0, 96),
    "_Z10k_cconv4v6ILi1ELb1ELb0ELi1EEv9Dc3Packed": (93, 0, 0, 96),
    "_Z11k_cconv4v6tILi4ELi1EEv9Dc3Packed7Dc3Tape": (165, 0, 0, 160),
    "_Z11k_cconv4v6tILi1ELi1EEv9Dc3Packed7Dc3Tape": (97, 0, 0, 160),
    "_Z10k_cconv4v6ILi4ELb0ELb1ELi1EEv9Dc3Packed": (168, 0, 0, 96),
    "_Z10k_cconv4v6ILi4ELb0ELb0ELi1EEv9Dc3Packed": (168, 0, 0, 96),
    "_Z10k_cconv4v6ILi1ELb0ELb0ELi1EEv9Dc3Packed": (98, 0, 0, 96),
    "_Z11k_cconv4v6lILi4EEv9Dc3PackedPK15HIP_vector_typeIjLj4EEPKi": (168, 0, 0, 112),
}


def _kernel_notes():
    blob = open(LIB, "rb").read()
    out = {}
    for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", blob):
        p = m.start()
        (nent,) = struct.unpack_from("<Q", blob, p + 24)
        off = p + 32
        for _ in range(nent):
            eo, es, ts = struct.unpack_from("<QQQ", blob, off)
            off += 24
            triple = blob[off:off + ts].decode()
            off += ts
            if "gfx950" not in triple or not es:
                continue
            path = "/tmp/lic360_tall_co_%d.elf" % os.getpid()
            with open(path, "wb") as f:
                f.write(blob[p + eo:p + eo + es])
            notes = subprocess.run([READELF, "--notes", path], capture_output=True, text=True, check=True).stdout
            os.unlink(path)
            for block in notes.split("  - .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", block)
                if name:
                    out[name.group(1)] = "  - .agpr_count:" + block
    return out


def _figures(block):
    field = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
    return field("vgpr_count"), field("agpr_count"), field("private_segment_fixed_size"), field("kernarg_segment_size")


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(READELF)), reason="built library or llvm-readelf missing")
def test_kernel_budgets():
    notes = _kernel_notes()
    hits = [n for n in notes if NEW_KERNEL in n]
    assert len(hits) == 1, hits
    vgpr, agpr, scratch, kernarg = _figures(notes[hits[0]])
    assert vgpr + agpr <= 168, "three waves per SIMD (twelve-wave workgroups) have 168 registers each"
    assert scratch == 0
    assert kernarg == 112 and "hidden_" not in notes[hits[0]], "Dc3Packed + the list's two pointers, no implicit arguments"
    dc = {n: _figures(b) for n, b in notes.items() if "k_cconv4v6" in n and n != hits[0]}
    assert dc == PARENT, "the decode-order kernels that were there before keep their registers, scratch and argument bytes"
    assert not any("hidden_" in notes[n] for n in dc)
