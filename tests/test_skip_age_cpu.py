"""The depth model of tests/skip_age_cases.py over the sequences that tests/test_gpu_skip_age.py runs (no GPU, no library):
  * WITHOUT the per-encode clear of e_buf[1] and e_buf[2] -- the schedule of the commits before it, still there under LIC360_NOCLEAR=1 -- the sequence of
    the 12-group codec drives the depth of a skipped cell up with every call, past 12 by the third: the inputs exercise the recurrence.  The 48-group
    codec's latent is two tiles wide, and the model finds that there the recurrence cannot close: the cone of a patch grows by two columns per layer
    towards the left, so the tile on its left is live at layers 1 and 2 and holds this call's values in all three buffers; only a tile on the RIGHT of
    a patch, more than a few columns away, is dead at every layer and keeps an earlier call's.  A cell can be one call old there (depth 19 by the
    third call) and no older.  On the 64-column latent batch X's patch sits in tile column 1 and batch Y's in tile column 3, 20 columns past tile
    column 1: X's tile 1 reads what Y left in tile 2, Y's tile 2 reads what X left in tile 1.
  * with the clear every depth stays <= 12 in every call (11 in fact: the deepest activation is layer 10's);
  * decode order: d_act[l] <= l + 1 and d_y <= 12 whatever the call.
And the weights: the recorded factors follow the stated rule, M_12 is finite in fp32."""
import numpy as np
import pytest

import skip_age_cases as cases


@pytest.fixture(scope="module")
def series():
    return {(name, clear): cases.encode_series(name, clear) for name in cases.CODECS for clear in (False, True)}


def test_without_the_clear_the_depth_grows_with_every_call(series):
    s = [max(c[1], c[2]) for c in series["g12", False]]
    assert s[0] <= 12 and s[2] > 12
    assert all(b > a for a, b in zip(s, s[1:])), s
    assert s[-1] > 6 * 12                                                   # about eight layers per call


def test_two_tile_columns_cannot_close_the_recurrence(series):
    s = [max(c[1], c[2]) for c in series["g48", False]]
    assert s[2] > 12                                                        # one call old ...
    assert max(s) <= 11 + 8                                                 # ... and no older


@pytest.mark.parametrize("name", list(cases.CODECS))
def test_with_the_clear_no_cell_is_deeper_than_12(series, name):
    for call in series[name, True]:
        assert max(call) <= 12, series[name, True]


@pytest.mark.parametrize("name", list(cases.CODECS))
def test_decode_order_is_at_most_one_layer_per_buffer_deep(name):
    for call in cases.decode_series(name):
        assert all(d <= l + 1 for l, d in enumerate(call)), call
    assert call[11] == 12                                                   # (the model is not vacuous: y is 12 layers from the symbols)


def test_the_patches_are_where_the_argument_needs_them():
    cfg = cases.CODECS["g12"]
    W = cfg["shape"][2]
    x, y = 2 * cfg["batches"]["X"][2], 2 * cfg["batches"]["Y"][2]
    assert x // cases.TILE_W == 1 and y // cases.TILE_W == 3
    assert y - 20 > 2 * cases.TILE_W - 1 and y + 1 < W                      # layer 1's cone of Y's patch (20 columns) stops short of tile column 1
    for name, cfg in cases.CODECS.items():
        for which, (B, _seed, _col, _who) in cfg["batches"].items():
            code, mask = cases.batch(name, which)
            G = cfg["shape"][0]
            assert code.shape == mask.shape == (B,) + cfg["shape"] and B <= cfg["max_batch"]
            lv = mask.sum(1)
            assert set(np.unique(lv).tolist()) <= {cfg["background"], G} and (lv == G).sum() in (4 * B, 4 * (B - B // 4))


@pytest.mark.parametrize("name", list(cases.CODECS))
def test_recorded_factors_and_the_bound(name):
    m = cases.BLOCK_MAXIMA[name]
    assert len(m) == 6 and all(b >= 2 * a for a, b in zip(m, m[1:])) and m[-1] < 1e12
    M = cases.depth_bound(cases.scaled_params(name))
    assert np.isfinite(np.float32(M)) and M > m[-1]
    assert cases.depth_bound(cases.scaled_params(name), 13) > M > cases.depth_bound(cases.scaled_params(name), 11)
