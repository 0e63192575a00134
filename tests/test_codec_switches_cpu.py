"""The reader of the fused latent codec's environment switches on the CPU (csrc/codec_switches.h): tests/switches_main.cpp, built with
-fsanitize=address,undefined and run as a child process, reads one environment per case and prints the struct the reader fills.  The accepted values
are those each switch had when it was read where it was used, quirks included; the cases state them.  No GPU, no library."""
import os
import re
import shutil
import subprocess

import pytest

import gpu_support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "360-image-compression_amd", "csrc")
DEFAULTS = dict(conv16=0, coder_mode=-1, skip=1, clear=1, dc_tall=1, dc_nb=8, dc_place=1, dc_order_bad=0, dc_order_text="", dc_pack=1, dc_gstep=0,
                dc_nets=1, ec_gbk=16, balance=1)
FIELDS = tuple(DEFAULTS)                                                    # in the order the program prints them


def case(env, **changed):
    return {"LIC360_" + k: v for k, v in env.items()}, dict(DEFAULTS, **changed)


CASES = [
    case({}),
    # every switch at each accepted value
    case({"FUSED_CONV": "16"}, conv16=1),
    case({"HOST_CODER": "0"}, coder_mode=0), case({"HOST_CODER": "1"}, coder_mode=1),
    case({"NOSKIP": "1"}, skip=0), case({"NOCLEAR": "1"}, clear=0), case({"DC_NOTALL": "1"}, dc_tall=0),
    case({"DC_ORDER": "1"}, dc_nb=1, dc_place=0), case({"DC_ORDER": "1p"}, dc_nb=1, dc_place=1), case({"DC_ORDER": "2"}, dc_nb=2, dc_place=1),
    case({"DC_ORDER": "4"}, dc_nb=4, dc_place=1), case({"DC_ORDER": "8"}, dc_nb=8, dc_place=1),
    case({"NOPACK": "1"}, dc_pack=0), case({"DC_GSTEP": "1"}, dc_gstep=1), case({"DC_GSTEP": "3"}, dc_gstep=3), case({"DC_NONETS": "1"}, dc_nets=0),
    case({"EC_GBK": "1"}, ec_gbk=1), case({"EC_GBK": "4"}, ec_gbk=4), case({"EC_GBK": "4096"}, ec_gbk=4096),
    case({"NOBALANCE": "1"}, balance=0),
    # the lenient readings, kept as they are: "set" is set with any value; only the first characters count
    case({"NOSKIP": ""}, skip=0), case({"NOSKIP": "0"}, skip=0),
    case({"HOST_CODER": "2"}, coder_mode=2), case({"HOST_CODER": "x"}, coder_mode=2),
    case({"FUSED_CONV": "1"}), case({"FUSED_CONV": "160"}, conv16=1),
    case({"DC_GSTEP": "2"}),
    case({"EC_GBK": "0"}), case({"EC_GBK": "4097"}), case({"EC_GBK": "-3"}), case({"EC_GBK": "abc"}),
    # not an order: flagged with its text, nb and place left at their defaults (the same list as tests/test_gpu_dc_order.py refuses at create)
] + [case({"DC_ORDER": bad}, dc_order_bad=1, dc_order_text=bad) for bad in ("3", "0", "16", "4p", "p", "")] + [
    case({"NO_SUCH_SWITCH": "1", "NOSKI": "1"}),                            # names the table does not hold are ignored
    case({"NOSKIP": "1", "DC_ORDER": "1p", "EC_GBK": "4", "NOBALANCE": "", "DC_GSTEP": "3x"}, skip=0, dc_nb=1, ec_gbk=4, balance=0, dc_gstep=3),
]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_reader_under_asan_ubsan(tmp_path):
    inp = tmp_path / "envs.txt"
    inp.write_text("".join("".join("%s=%s\n" % kv for kv in env.items()) + "end\n" for env, _ in CASES))
    exe = str(tmp_path / "switches_main")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-Wall", "-I" + CSRC, os.path.join(ROOT, "tests", "switches_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300, env={})
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-500:] + r.stderr[-3000:])
    lines = r.stdout.split("\n")
    assert lines[0].split(" ") == ["names"] + list(gpu_support.SWITCH_NAMES), "tests/gpu_support.py clears the names of the C table"
    n = len(FIELDS) + 1
    assert len(lines) == 1 + n * len(CASES) + 1 and lines[-1] == ""
    for k, (env, want) in enumerate(CASES):
        block = lines[1 + k * n:1 + (k + 1) * n]
        assert block == ["%s=%s" % (f, want[f]) for f in FIELDS] + ["end"], env


def test_the_environment_is_read_in_one_header_only():
    """getenv, and a string literal that names a LIC360_* variable, occur in csrc/codec_switches.h and nowhere else under csrc/"""
    hits = set()
    for name in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, name)
        if os.path.isfile(path):
            text = open(path, errors="replace").read()
            if "getenv" in text or re.search(r'"LIC360_[A-Z_]*', text):
                hits.add(name)
    assert hits == {"codec_switches.h"}
