"""lic360_models' routing of the fused sphere convolutions against the committed table (tests/golden/sconv_routes.json, the enumeration of
tests/sconv_route_cases.py run on the file as it was before the routing was gathered into _route: the table pins that refactor and every later one), and the one
statement of the launch geometry there (_workgroups) against the three restatements the exact tests use.  No GPU."""
import json
import os

import pytest

import sconv_cases as sc
import sconv_narrow_cases as nc
import sconv_route_cases as rc
import sconv_s2_cases as s2

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sconv_routes.json")


def test_the_enumeration_covers_the_grid():
    want = json.load(open(GOLDEN))
    stride1 = [k for k in want if k.split()[0] in [layer.name for layer in rc.STRIDE1]]
    assert len(stride1) * len(rc.BATCHES) == 7 * 5 * 6 * 3 * 2 == 1260
    tokens = [t for k in stride1 for t in want[k].split()]
    assert len(tokens) == 1260 and sum("_narrow" in t for t in tokens) == 76
    assert sum(k.startswith("gate ") for k in want) == 5 * 3 * 2 and sum("stride2=" in k and not k.startswith("odd") for k in want) == 2 * 5 * 2
    assert {"outside_48 48>48 132x260 bf16x1 narrow", "outside_96_gate 96>96 132x260 bf16x1 narrow", "odd down_conv1 192>192 259x515 stride2=bf16x1",
            "bare v2_conv2 192>192 132x260"} <= set(want)
    assert all(len(v.split()) == len(rc.BATCHES) for v in want.values())


def test_the_routes_are_the_tables():
    import lic360_models
    want, got = json.load(open(GOLDEN)), rc.routes(lic360_models)
    assert sorted(got) == sorted(want)
    wrong = ["%s:\n    table %s\n    now   %s" % (k, want[k], got[k]) for k in sorted(want) if got[k] != want[k]]
    assert not wrong, "%d rows differ (batches %s)\n%s" % (len(wrong), rc.BATCHES, "\n".join(wrong[:20]))


# (launch, kernel size, form, cout, cpw): the wide launch in the fp32 and split-bf16 bodies and both pack blocks; stride 2; the narrow launch in all three forms, both
# widths on the 192-block pack (one and four blocks of it) and 48 on the 96-block pack
GEOMETRY = ([("wide", ks, form, cout, None) for ks in (3, 1) for form in ("fp32", "bf16x3") for cout in (192, 96, 768)]
            + [("stride2", ks, "fp32", cout, None) for ks in (3, 1) for cout in (192, 96, 384)]
            + [("narrow", ks, form, cout, cpw) for ks in (3, 1) for form in nc.FORMS for cout, cpw in ((192, 96), (192, 48), (768, 96), (768, 48), (96, 48))])


@pytest.mark.parametrize("launch,ks,form,cout,cpw", GEOMETRY, ids=lambda v: str(v))
def test_workgroups_counts_as_the_case_files_do(launch, ks, form, cout, cpw):
    """lic360_models._workgroups against branch_of of tests/sconv_cases.py (wide), sconv_s2_cases.py (stride 2) and sconv_narrow_cases.py (narrow): the workgroup
    count and the tall last tile row, window heights 1 .. 80, two windows (a 1-ring one with ragged columns)"""
    import lic360_models as lm
    for nr in range(1, 81):
        for ring, ring_w, ncol in ((2, 2, 40), (1, 2, 33)):
            if launch == "stride2":
                b, got = s2.branch_of(s2._c("t", ks, 32, cout, 3, nr, ncol)), lm._workgroups(3, nr, ncol, cout, ks, stride=2)
                assert not got[1]                                           # no tall tile row at stride 2
            else:
                case = sc._c("t", ks, 32, cout, 3, nr + 2 * ring, ncol + 2 * ring_w, ring=ring, ring_w=ring_w)
                b = sc.branch_of(case, form != "fp32") if launch == "wide" else nc.branch_of(case, form, cpw)
                got = lm._workgroups(3, nr, ncol, cout, ks, cpw=cpw, precision=form)
                assert got[1] is b.tall
            assert got[0] == 3 * b.tiles_y * b.tiles_x * b.blocks_y, (nr, ring, got, b)
