"""The sphere-convolution kernels issue global loads from inline asm and wait for them by counted `s_waitcnt vmcnt(N)`: the compiler does not know that
such a load is in flight, and a destination register that no later statement names is free for it to reuse -- a late return then overwrites the new
value (the drain behind b1s2_body's loop once named no register, and the bias address went into an operand register ahead of it).  This compiles
csrc/conv3x3_kernels.hip to assembly and walks every path through every kernel (tools/asm_load_hazards.py): no instruction other than a later load
writes a VGPR that an outstanding load will still write, and no load into a register is outstanding at s_endpgm.  The walker itself is checked on two
small hand-written kernels, one with the fault and one without."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "360-image-compression_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
sys.path.insert(0, os.path.join(ROOT, "tools"))

FAULTY = """_Zfaulty:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tglobal_load_dwordx4 v[4:7], v[0:1], off
\ts_cbranch_scc1 .LBB0_2
\tglobal_load_dword v8, v[0:1], off
.LBB0_2:
\tv_mov_b32_e32 v5, s0
\ts_waitcnt vmcnt(0)
\ts_endpgm
.Lfunc_end0:
"""


def test_the_walker_sees_a_reused_destination_and_a_load_left_in_flight():
    import asm_load_hazards as ah
    lines = FAULTY.splitlines(True)[1:-1]
    assert ah.analyse("faulty", lines) == 1                                                             # v5 is written under the dwordx4 load
    assert ah.analyse("waited", [l for l in lines if "v_mov" not in l]) == 0
    assert ah.analyse("in order", [l.replace("v_mov_b32_e32 v5, s0", "global_load_dword v5, v[2:3], off") for l in lines]) == 0   # a later load returns later
    assert ah.analyse("counted", [l.replace("vmcnt(0)", "vmcnt(1)") for l in lines if "v_mov" not in l]) == 1                  # one load into v8 reaches s_endpgm
    assert ah.analyse("moved", [lines[i] for i in (0, 1, 2, 3, 4, 6, 5, 7)]) == 0                       # the same write behind the wait


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_no_kernel_of_the_sphere_convolutions_writes_under_a_load_in_flight(tmp_path):
    import asm_load_hazards as ah
    out = str(tmp_path / "k.s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-S", "--cuda-device-only",
                           "-c", os.path.join(CSRC, "conv3x3_kernels.hip"), "-o", out], stderr=subprocess.DEVNULL)
    kernels = ah.kernels(out)
    names = [k for k in kernels if "k_sconv" in k]
    assert len([k for k in names if "k_sconv_b1s2" in k]) == 4 and len(names) == 22, names
    bad = {k: n for k in names for n in [ah.analyse(k, kernels[k])] if n}
    assert not bad, bad
