"""Writes the fixtures of the decode lists' order tests:
  tests/golden/dc_order_counts.npz  -- blocks and records per net of the smooth-mask lists at the bench's main shape (tests/dc_order_cases.py:
                                       smooth_mask_counts; tests/test_dc_order_cpu.py recomputes and compares it);
  tests/golden/dc_order_streams.npz -- the CPU oracle's bitstreams (tests/ref_codec.py:encode_main, image by image) of both batches of every shape of
                                       tests/test_gpu_dc_order.py: 192 images, about a second each, too long for a test that runs with every suite.  The
                                       digests of the batches are stored beside the bytes, and the test checks them before it trusts the bytes.
Run from the repository root once the oracle is built:  python tools/gen_golden_dc_order.py

Not written here: tests/golden/dc_order_parent_lists.npz, the digests (tests/test_gpu_dc_order.py: digest) of the decode lists that the library of the
commit BEFORE the switch built for the same batches.  They were recorded once, on the GPU, from that commit's build; a later library cannot
regenerate them without assuming what the test is there to show."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "360-image-compression_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))

import dc_order_cases as cases                                              # noqa: E402
import ref_codec as rc                                                      # noqa: E402
from util import make_main_params                                           # noqa: E402


def main():
    print(cases.write_golden())
    out = {}
    for shape in cases.GPU_SHAPES:
        G, H, W, B = shape
        layers = make_main_params(cases.weight_seed(shape), G)
        for second in (False, True):
            code, mask = cases.batch(shape, second)
            k = cases.stream_key(shape, second)
            streams = [rc.encode_main(code[i:i + 1], mask[i:i + 1], layers, G) for i in range(B)]
            out[k + "_sha256"] = np.array([hashlib.sha256(code.tobytes()).hexdigest(), hashlib.sha256(mask.tobytes()).hexdigest()])
            out[k + "_lengths"] = np.array([len(s) for s in streams])
            out[k + "_bytes"] = np.frombuffer(b"".join(streams), np.uint8)
            print(k, sum(len(s) for s in streams), flush=True)
    path = os.path.join(ROOT, "tests", "golden", cases.GOLDEN_STREAMS)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
