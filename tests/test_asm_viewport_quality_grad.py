"""The kernels of the fused viewport metrics' backward in the device assembly of csrc/viewport_quality_kernels.hip: the four coefficient-storing
forward kernels and the four backward kernels exist under names of their own, beside the four plain forward kernels, and the new ones use no
scratch and spill nothing (the kernel metadata, as tests/test_asm_gate_kernels.py reads it)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "360-image-compression_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    out = str(tmp_path_factory.mktemp("vqgrad") / "k.s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-S", "--cuda-device-only",
                           "-c", os.path.join(CSRC, "viewport_quality_kernels.hip"), "-o", out], stderr=subprocess.DEVNULL)
    found = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_spill_count:\s+(\d+).*?"
                         r"\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", open(out).read(), re.S):
        lds, name, priv, ss, vg, vs = m.groups()
        found[name] = dict(lds=int(lds), scratch=int(priv), spills=int(ss) + int(vs), vgprs=int(vg))
    return found


FORMS = ["ILb0ELi0E", "ILb0ELi11E", "ILb1ELi0E", "ILb1ELi11E"]              # NEAREST x {run-time window, window 11}


def test_the_unit_holds_the_new_kernels_by_name(meta):
    forward = sorted(k for k in meta if "18k_viewport_qualityI" in k)
    backward = sorted(k for k in meta if "27k_viewport_quality_backwardI" in k)
    assert len(forward) == 8 and len(backward) == 4, (forward, backward)
    split = [re.search(r"quality(ILb[01]ELi\d+E)(Lb[01]E)EEv", k).groups() for k in forward]
    for coef in ("Lb0E", "Lb1E"):                                            # the plain kernels and the coefficient-storing ones
        assert sorted(form for form, c in split if c == coef) == FORMS, forward
    assert sorted(re.search(r"backward(ILb[01]ELi\d+E)EEv", k).group(1) for k in backward) == FORMS, backward


def test_the_new_kernels_use_no_scratch_and_spill_nothing(meta):
    new = {k: v for k, v in meta.items() if "27k_viewport_quality_backwardI" in k or ("18k_viewport_qualityI" in k and "Lb1EEEv" in k)}
    assert len(new) == 8, sorted(new)
    for k, v in sorted(new.items()):
        print(k, v)
        assert v["scratch"] == 0 and v["spills"] == 0, (k, v)
        assert v["vgprs"] <= 128 and v["lds"] <= 160 * 1024 // 4, (k, v)      # at least four workgroups of four waves per CU
