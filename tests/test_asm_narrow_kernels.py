"""The narrow-workgroup kernels of csrc/conv3x3_kernels.hip (k_narrow_conv<NT, NQ, RW, KS, PQ>, k_narrow_gate<NT, NQ, RW, PQ>) in the unit's metadata: they exist
under names of their own -- eighteen convolutions (three forms x two kernel sizes x (NQ, RW, PQ) = (2, 4, 4), (1, 2, 4), (1, 2, 2)) and six gates -- use no scratch
and spill nothing, their argument struct is S3Args in a wrapper of their own (the gates': S3GateArgs, S3Args plus one pointer), and the counts the other tests
of this unit rely on still hold: 22 kernels of the k_sconv prefix, 6 of k_gate_sconv, 20 whose argument type is S3Args itself."""
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
    out = str(tmp_path_factory.mktemp("narrow") / "k.s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-S", "--cuda-device-only",
                           "-c", os.path.join(CSRC, "conv3x3_kernels.hip"), "-o", out], stderr=subprocess.DEVNULL)
    m = {}
    for g in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.kernarg_segment_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?"
                         r"\.sgpr_spill_count:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", open(out).read(), re.S):
        lds, ka, name, priv, ss, vg, vs = g.groups()
        m[name] = dict(lds=int(lds), kernarg=int(ka), scratch=int(priv), spills=int(ss) + int(vs), vgprs=int(vg))
    return m


def test_the_unit_holds_the_narrow_kernels(meta):
    conv = sorted(k for k in meta if "k_narrow_conv" in k)
    gate = sorted(k for k in meta if "k_narrow_gate" in k)
    assert len(conv) == 18 and all(k.endswith("12S3NarrowArgs") for k in conv), conv
    assert len(gate) == 6 and all(k.endswith("10S3GateArgs") for k in gate), gate
    shapes = lambda names: sorted(k[k.index("I"):k.index("Ev")] for k in names)
    L = lambda *v: "I" + "".join("Li%dE" % x for x in v)
    assert shapes(conv) == sorted(L(nt, nq, rw, ks, pq) for nt in (0, 3, 1) for ks in (3, 1) for nq, rw, pq in ((2, 4, 4), (1, 2, 4), (1, 2, 2)))
    assert shapes(gate) == sorted(L(nt, nq, rw, 4) for nt in (0, 3, 1) for nq, rw in ((2, 4), (1, 2)))


def test_they_use_no_scratch_no_spills_and_the_argument_bytes_of_s3args(meta):
    wide = {v["kernarg"] for k, v in meta.items() if k.endswith("6S3Args")}
    assert len(wide) == 1
    s3args = wide.pop()
    assert len([k for k in meta if "k_narrow_" in k]) == 24
    for k, v in meta.items():
        if "k_narrow_" in k:
            print(k, v)
            assert v["scratch"] == 0 and v["spills"] == 0 and v["vgprs"] <= 256 and v["lds"] <= 160 * 1024, (k, v)
            assert v["kernarg"] == s3args + (8 if "k_narrow_gate" in k else 0), (k, v, s3args)     # S3Args and nothing else; the gate: plus the trunk pointer


def test_the_counts_of_the_other_tests_still_hold(meta):
    assert len([k for k in meta if "k_sconv" in k]) == 22                   # tests/test_asm_load_hazards.py
    assert len([k for k in meta if "k_gate_sconv" in k]) == 6               # tests/test_asm_gate_kernels.py
    assert len([k for k in meta if k.endswith("6S3Args")]) == 20
    assert not [k for k in meta if "narrow" in k and ("k_sconv" in k or "k_gate_sconv" in k)]
