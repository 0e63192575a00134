"""The first decode layer's three-nets-per-task launch, on the CPU: the case tables of tests/dc_first_nets_cases.py reach every class of merged
launch, the restated launch arithmetic agrees with the library's host-only lic360_dc4_tape_layout, the merged tapes obey the kernel's piece rules
and cover every row of every image exactly once, and the built kernels stay inside their register / scratch / argument budgets.  No GPU work.

The race geometry.  A task of G = 6 groups is ONE double step, so a workgroup that takes two of them back to back reaches the second task's
exchange with no step barrier in between (the round-6 race of the one-net kernel; the three-net kernel's per-net buffers, cconv4v6_dc.inc).
324 images: plain tasks, 40 / 41 per XCD list and group block on 32 workgroups.  Its taped twin of 320 images does NOT repeat that in the merged
schedule: tapes of 5 images are two tasks each, 8 tapes per XCD list and at most two group blocks = 32 tasks on 32 workgroups, one each (the one-net
schedule over 960 samples had 96).  The case stays; 640 images (64 tasks per XCD list) is the taped launch whose workgroups take two in a row."""
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

import dc_first_nets_cases as cases                                         # noqa: E402

NB_MAX, NW_MAX = 24, 6
LIB = os.path.join(ROOT, "360-image-compression_amd", "liblic360_hip.so")
READELF = shutil.which("llvm-readelf") or "/opt/rocm/lib/llvm/bin/llvm-readelf"


@pytest.fixture(scope="module")
def L():
    import lic360 as lic
    return lic._lib


def layout(L, G, cin, n, nb, h, w, psum, x_mod):
    tape_c, n_blocks = C.c_int(), C.c_int()
    blocks, nwaves = (C.c_int * NB_MAX)(), (C.c_int * NB_MAX)()
    windows = (C.c_uint * (NB_MAX * NW_MAX * 3))()
    assert L.lic360_dc4_tape_layout(G, cin, n, nb, h, w, psum, x_mod, C.byref(tape_c), C.byref(n_blocks), blocks, nwaves, windows) == 0
    return tape_c.value, n_blocks.value, list(blocks), list(nwaves), np.array(windows, dtype=np.uint32).reshape(NB_MAX, NW_MAX, 3)


def classes_of(case):
    G, h, w, B, planes, res = case
    return {cases.launch_class(cases.schedule(G, 3 * B, 3, h, w, p, B)) for p in cases.planes_of(case)} - {None}


def test_cases_reach_every_class_of_merged_launch():
    for case in cases.MERGED_CASES:                                        # every launched plane of every case is a merged launch
        G, h, w, B, planes, res = case
        for p in cases.planes_of(case):
            s = cases.schedule(G, 3 * B, 3, h, w, p, B)
            assert s is not None and s.nets == 3 and s.samples == B, (case, p)
    tape_c = {}
    for case in cases.TAPE_CASES:
        for cl in classes_of(case):
            assert cl[0] == "taped"
            tape_c.setdefault(cl[1], set()).add(cl[3])
    assert set(tape_c) == {2, 3, 6} and "cut" in tape_c[3] and "cut" in tape_c[6], "tapes of 2, 3 and 6 images, 64-row windows cut at 61 rows"
    assert classes_of(cases.PLAIN_CASES[0]) == {("plain", "uneven", "short")}
    assert classes_of(cases.FULL_CASES[0]) == {("plain", "even", "short"), ("plain", "even", "full")}
    G, h, w, B = cases.PLAIN_CASES[0][:4]
    s = cases.schedule(G, 3 * B, 3, h, w, 20, B)
    assert sorted({len(cases.list_tasks(s, x)) // len(s.blocks) for x in range(8)}) == [0, 1], "XCD lists of one image and of none"
    for (G, h, w, n, nb, x_mod) in cases.OLD_FORM_CASES:                   # ... and these never are
        assert all(s is None or s.nets == 1 for s in (cases.schedule(G, n, nb, h, w, p, x_mod) for p in range(h + w + G - 2)))
    assert cases.schedule(12, 9, 3, 16, 24, 10, 3).nets == 1, "few samples: latency mode keeps one net per task"
    assert cases.schedule(12, 144, 3, 128, 40, 30, 48).nets == 1, "taller than a wave: row segments keep one net per task"
    assert cases.schedule(12, 144, 3, 64, 20, 30, 48, no_nets=True).nets == 1
    assert cases.schedule(12, 144, 3, 64, 20, 30, 48, cin=4).nets == 1


def test_race_cases_put_one_double_step_tasks_back_to_back():
    seen = {}
    for case in cases.RACE_CASES:
        G, h, w, B, planes, res = case
        assert all(cases.double_steps(G, g0) == 1 for g0 in range(0, G, cases.PS)), "every task of the layer is one double step"
        per_plane = []
        for p in cases.planes_of(case):
            s = cases.schedule(G, 3 * B, 3, h, w, p, B)
            per_plane.append(cases.consecutive_single_step_tasks(G, s))
            seen.setdefault(B, set()).add(cases.launch_class(s)[0])
        seen[(B, "wgs")] = max(per_plane)
    assert seen[324] == {"plain"} and seen[320] == {"taped"} and seen[640] == {"taped"}
    assert seen[(324, "wgs")] > 0 and seen[(640, "wgs")] > 0, "workgroups that run two one-double-step tasks in a row"
    assert seen[(320, "wgs")] == 0, "32 tasks per XCD list on 32 workgroups (module docstring)"
    s = cases.schedule(6, 3 * 324, 3, 8, 8, 0, 324)
    assert [len(cases.list_tasks(s, x)) for x in range(8)] == [41] * 4 + [40] * 4 and max(len(cases.workgroup_tasks(s, wg)) for wg in range(256)) == 2


@pytest.mark.parametrize("case", cases.TAPE_CASES + cases.RACE_CASES[1:], ids=cases.case_id)
def test_merged_tapes_obey_the_piece_rules_and_match_the_restated_schedule(L, case):
    G, h, w, B, planes, res = case
    taped = 0
    for psum in cases.planes_of(case):
        c, nblk, blocks, nwaves, win = layout(L, G, 1, 3 * B, 3, h, w, psum, B)
        s = cases.schedule(G, 3 * B, 3, h, w, psum, B)
        assert (c, nblk, blocks[:nblk]) == (s.tape_c, len(s.blocks), s.blocks), psum
        assert c >= 2 and (B // 8) % c == 0, "the tape is laid over the images of an XCD's list, not over the samples of three nets"
        assert nwaves[:nblk] == s.nw
        taped += 1
        for j in range(nblk):
            lo, hi = s.rows[j]
            waves = cases.tape_waves(s, j)
            assert len(waves) == (nwaves[j] if nwaves[j] < c else 0)
            cover = np.zeros((c, h), np.int32)
            for t in range(NW_MAX):
                pieces = [int(v) for v in win[j, t] if v]
                assert (t < len(waves)) == bool(pieces), (psum, j, t)
                if pieces:
                    assert pieces == [k | slo << 3 | shi << 9 | a0 << 15 | 1 << 21 for (k, slo, shi, a0) in waves[t]]
                quads_taken, last_a0 = set(), -1
                for wd in pieces:
                    k, slo, shi, a0 = wd & 7, (wd >> 3) & 63, (wd >> 9) & 63, (wd >> 15) & 63
                    rows = shi - slo + 1
                    assert k < c and lo <= slo <= shi <= hi and (a0 - slo) % 4 == 0 and a0 > last_a0
                    last_a0 = a0
                    assert a0 + rows - 1 <= (63 if shi == h - 1 else 61) and a0 >= (0 if slo == 0 else 2)
                    q = {col // 4 for col in range(a0, a0 + rows + 4)}
                    assert max(q) < 17 and not (q & quads_taken), "pieces of a wave share no band quad"
                    quads_taken |= q
                    cover[k, slo:shi + 1] += 1
            if waves:
                assert (cover[:, lo:hi + 1] == 1).all() and cover.sum() == c * (hi - lo + 1), (psum, j)
    assert taped == len(cases.planes_of(case))


def test_layout_reports_the_one_net_schedule_for_every_other_launch(L):
    assert layout(L, 12, 1, 144, 3, 64, 20, 30, 48)[0] == 6 and layout(L, 12, 1, 144, 3, 64, 20, 30, 144)[0] == 6
    assert layout(L, 12, 1, 72, 3, 64, 20, 30, 24)[0] == 3              # 24 images: tapes of 3 (the one-net schedule of 72 samples tapes 3 as well)
    assert layout(L, 12, 1, 48, 3, 64, 20, 30, 16)[0] == 2 and layout(L, 12, 4, 48, 3, 64, 20, 30, 16)[0] == 2
    assert layout(L, 48, 1, 15, 3, 16, 24, 30, 5)[0] == 0


# ---- resources of the built kernels (the method of tests/test_kernarg_bytes.py: the gfx950 code objects' notes, read with llvm-readelf)
NEW_KERNELS = {"k_cconv4v6ILi1ELb0ELb0ELi3EE": 96, "k_cconv4v6tILi1ELi3EE": 160}     # -> kernel argument bytes (Dc3Packed, + Dc3Tape)


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
            path = "/tmp/lic360_nets_co_%d.elf" % os.getpid()
            with open(path, "wb") as f:
                f.write(blob[p + eo:p + eo + es])
            notes = subprocess.run([READELF, "--notes", path], capture_output=True, text=True, check=True).stdout
            os.unlink(path)
            for block in notes.split("  - .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", block)
                if name:
                    out[name.group(1)] = "  - .agpr_count:" + block
    return out


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(READELF)), reason="built library or llvm-readelf missing")
def test_three_net_kernels_fit_three_waves_per_simd_without_scratch():
    notes = _kernel_notes()
    for pat, kernarg in NEW_KERNELS.items():
        hits = [n for n in notes if pat in n]
        assert len(hits) == 1, (pat, hits)
        block = notes[hits[0]]
        field = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
        assert field("vgpr_count") + field("agpr_count") <= 168, "three waves per SIMD (twelve-wave workgroups) have 168 registers each"
        assert field("private_segment_fixed_size") == 0, "scratch"
        assert field("group_segment_fixed_size") <= 160 * 1024
        assert field("kernarg_segment_size") <= kernarg and "hidden_" not in block
