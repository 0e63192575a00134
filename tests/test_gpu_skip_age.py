"""What the fused latent codec leaves in its activation buffers, call after call ("Why skipping is safe").  The dead-cone skip is safe
only while every dead cell stays finite: live chains read dead cells through zero weights, and 0 * Inf is NaN.  One FusedCodec runs a whole sequence
of tests/skip_age_cases.py -- alternating mask sets whose patches make each call's computed-but-dead cells read what the previous call left in the
tiles it skips, batch sizes that move the planes, one call below the decode-list regime -- under weights scaled so that an activation grows about
9 x (5 x) per layer.  The buffers are zeroed once, before the first call, and never again.  After EVERY call:
  * the bitstreams are the CPU oracle's (the fixture tests/golden/skip_age_streams.npz), the decode of the oracle's bytes gives the symbols, err is 0;
  * no activation buffer holds an Inf or a NaN;
  * no finite cell exceeds M_12 (skip_age_cases.depth_bound: from the weights alone, in fp64), which bounds every cell that is at most 12 layers
    away from real symbols and nothing deeper.
Measured on an MI355X, largest |cell| of e_buf[1] / e_buf[2] after each call (device coder; the host coder's figures are the same):
  * 12 groups (M_12 = 2.78e34), under LIC360_NOCLEAR=1 -- the schedule of the commits before the per-encode clear of the two buffers:
    6.5e8 / 4.6e9, 3.5e13 / 4.2e12, 1.6e18 / 5.2e18, 4.4e22 / 6.0e21, 4.1e26 / 1.2e27, 1.1e31 / 1.7e30, the same after Z, 8.1e32 / 1.0e32 and, after the
    ninth call's encode, 2.7e37 / 8.5e37: past M_12 (the bytes were still right: one more call and the cells are Inf).  This test fails there.
  * 12 groups as shipped: 6.5e8 / 4.6e9 after every X, 5.7e8 / 4.3e9 after every Y and Z; no Inf or NaN in any of the 15 buffers.
  * 48 groups (M_12 = 2.67e36), LIC360_NOCLEAR=1: 1.3e7 / 5.9e7 after the first X, 1.1e7 / 5.7e7 after every Y, 4.6e9 / 6.1e9 after every later X -- one
    call old and no older, as the model says of a latent two tiles wide; as shipped 1.3e7 / 5.9e7 and 1.1e7 / 5.7e7 throughout.  Here the test is a
    regression test of bytes, symbols and finiteness; only the 12-group sequence can show the recurrence."""
import numpy as np
import pytest

import skip_age_cases as cases
from gpu_support import dev  # noqa: F401

pytestmark = pytest.mark.gpu


_batches = {}


def batch_of(name, which):
    """(code, mask, the oracle's streams) of a batch, made once"""
    if (name, which) not in _batches:
        code, mask = cases.batch(name, which)
        _batches[name, which] = (code, mask, cases.golden_streams(name, which, code, mask))
    return _batches[name, which]


def run_sequence(name, coder, check=True):
    """-> [calls] of (absmax [15], nonfinite [15]); check: assert after every call"""
    from lic360_fused import FusedCodec
    cfg = cases.CODECS[name]
    G, H, W = cfg["shape"]
    layers = cases.scaled_params(name)
    bound = cases.depth_bound(layers)
    fc = FusedCodec(G, H, W, max_batch=cfg["max_batch"])
    fc.load_layers(layers)
    fc.set_coder(coder)
    assert fc.skip_active() == 2
    fc.debug_fill(0.0)                                                      # once: what follows is what the codec leaves behind by itself
    series = []

    def curve():
        return "largest |cell| of e_buf[0..2] per call: " + "; ".join(" ".join("%.3g" % v for v in a[:3]) for a, _ in series)

    for k, which in enumerate(cfg["calls"]):
        code, mask, want = batch_of(name, which)
        B = code.shape[0]
        got = fc.encode(dev(code), dev(mask))
        enc_err = int(fc.err[:B].abs().sum().item())
        out = fc.decode(want, dev(mask)).cpu().numpy()                      # (raises unless err is 0 for every image)
        dec_err = int(fc.err[:B].abs().sum().item())
        absmax, bad = fc.debug_absmax()
        series.append((absmax.astype(np.float64), bad))
        if not check:
            continue
        for i in range(B):
            assert got[i] == want[i], "call %d (%s), image %d; %s" % (k, which, i, curve())
        assert np.array_equal(out, code * mask), "call %d (%s); %s" % (k, which, curve())
        assert enc_err == 0 and dec_err == 0
        assert not bad.any(), "call %d (%s): Inf / NaN cells per buffer %s; %s" % (k, which, dict(zip(fc.ABSMAX_BUFFERS, bad.tolist())), curve())
        assert (series[-1][0] <= bound).all(), "call %d (%s): M_12 = %.4g, largest |cell| per buffer %s; %s" % (
            k, which, bound, dict(zip(fc.ABSMAX_BUFFERS, absmax.tolist())), curve())
    return series


@pytest.mark.parametrize("coder", cases.CODERS)
@pytest.mark.parametrize("name", list(cases.CODECS), ids=cases.codec_id)
def test_skipped_cells_stay_bounded_across_calls(name, coder):
    series = run_sequence(name, coder)
    print("\n%s, %s coder, M_12 = %.4g" % (cases.codec_id(name), coder, cases.depth_bound(cases.scaled_params(name))))
    for k, (a, _) in enumerate(series):
        print("  call %2d (%s)  e_buf %s  d_act..d_y max %.4g" % (k, cases.CODECS[name]["calls"][k], " ".join("%.4g" % v for v in a[:3]), a[3:].max()))
    # the hook looks at what the codec wrote: after the first call every buffer holds something (a read-back of zeros would pass everything above)
    assert all((a > 0).all() for a, _ in series)
