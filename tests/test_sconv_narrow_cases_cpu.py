"""tests/sconv_narrow_cases.py by itself, without a GPU: the case list reaches every body the narrow kernels instantiate, every tile-row branch and every
(pack block, mq slot) with a non-zero slot; the exactness condition holds for every case in every form and tier; and each bug only a narrow kernel can have --
every block on pack slot 0, the channel offset taken from the pack's block size, the wide form's tall-row threshold, a shuffled store without the block's
offset -- changes the reference of at least one case."""
import numpy as np
import pytest

import sconv_narrow_cases as nc
import sconv_gate_cases as gc

SMALL_PARAMS = [p for p in nc.params() if not p[0].case.prod]


def test_the_cases_reach_every_body_and_tile_row_branch():
    bodies, branches = set(), set()
    for n, form, tier, cpw in nc.params():
        bodies |= nc.bodies_of(n.case, form, cpw)
        br = nc.branch_of(n.case, form, cpw)
        if br.ks == 3:
            branches.add((form, br.nq, br.pq, "low" if br.full == 0 else "tall" if br.tall else "exact" if br.rem == 0 else "extra_row"))
    assert bodies == nc.BODIES, (sorted(nc.BODIES - bodies), sorted(bodies - nc.BODIES))
    for form in nc.FORMS:
        for nq, pq in ((2, 4), (1, 4), (1, 2)):
            want = {"low", "extra_row"} | ({"tall"} if nc.has_tall(form, nq, 3) else set())
            assert want <= {b[3] for b in branches if b[:3] == (form, nq, pq)}, (form, nq, pq, branches)
    # the split-bf16 form at cpw 48 runs a remainder of 1 .. 8 rows as a tile row of its own
    assert any(not nc.branch_of(n.case, "bf16x3", 48).tall and 0 < nc.branch_of(n.case, "bf16x3", 48).rem <= 8 and nc.branch_of(n.case, "fp32", 48).tall
               for n in nc.SMALL if 48 in n.cpws and n.case.ks == 3 and nc.supported("bf16x3", 3, n.case.cin, n.case.cout, 48))
    gates = {(f, cpw // 48) for c, f, t, cpw in nc.gate_params()}
    assert gates == nc.GATE_KERNELS
    assert any(c.cout > 192 for c, f, t, cpw in nc.gate_params()) and any(c.name == "g_saturate" for c, f, t, cpw in nc.gate_params())
    assert {c.n > 1 and (c.hp - 2 * c.ring) % 16 != 0 for c in nc.GATE_CASES} == {True, False}


def test_the_cases_reach_every_pack_block_and_slot():
    seen = set()
    for n, form, tier, cpw in SMALL_PARAMS:
        c = n.case
        for blk, slot in nc.slots_of(c, cpw):
            seen.add((form, c.ks, nc.pack_block(c.cout), cpw, min(blk, 1), slot))
    for form in nc.FORMS:
        for ks in (3, 1):
            for pb, cpw, slots in ((192, 96, (0, 2)), (192, 48, (0, 1, 2, 3)), (96, 48, (0, 1))):
                for slot in slots:
                    assert (form, ks, pb, cpw, 0, slot) in seen, (form, ks, pb, cpw, slot)
                    if pb == 192:
                        assert (form, ks, pb, cpw, 1, slot) in seen, (form, ks, pb, cpw, slot)      # and in a later pack block
    # the geometry's own consistency: a launch's blocks cover every channel once
    for n in nc.CASES:
        for cpw in n.cpws:
            chans = [blk * nc.pack_block(n.case.cout) + 48 * slot + j for blk, slot in nc.slots_of(n.case, cpw) for j in range(cpw)]
            assert chans == list(range(n.case.cout)), (n.case.name, cpw)


def test_the_geometry_refuses_what_the_kernels_refuse():
    assert not nc.supported("fp32", 3, 32, 96, 96) and not nc.supported("fp32", 3, 32, 192, 192) and not nc.supported("fp32", 3, 32, 192, 144)
    assert not nc.supported("bf16x3", 3, 16, 96, 48) and nc.supported("fp32", 3, 16, 96, 48) and not nc.supported("fp16", 3, 32, 192, 96)
    assert nc.supported("bf16x1", 1, 32, 768, 48) and not nc.supported("fp32", 1, 16, 192, 96)


@pytest.mark.parametrize("p", SMALL_PARAMS, ids=nc.ident)
def test_exactness_holds_and_the_reference_is_the_wide_one(p):
    n, form, tier, cpw = p
    data, want = nc.shared(n.case, form, tier)
    assert nc.assert_exact_domain(n.case, form, tier, data) < nc.sc.EXACT_BELOW
    assert want.shape == nc.sc.out_shape(n.case)
    assert np.array_equal(nc.reference(n.case, form, data, cpw), want)
    assert np.array_equal(want.astype(np.float32), want)                    # an fp32 number in every cell


@pytest.mark.parametrize("mut", sorted(nc.MUTATIONS))
def test_every_narrow_bug_changes_a_reference(mut):
    hit = {}
    for n, form, tier, cpw in SMALL_PARAMS:
        if tier != nc.TIERS[form][0] or not nc.MUTATIONS[mut](n.case, form, cpw):
            continue
        data, want = nc.shared(n.case, form, tier)
        changed = not np.array_equal(nc.reference(n.case, form, data, cpw, mut), want)
        assert changed, (mut, nc.ident((n, form, tier, cpw)))
        hit.setdefault((form, n.case.ks, cpw), 0)
        hit[form, n.case.ks, cpw] += 1
    for form in nc.FORMS:                                                   # in every form, and at both widths
        assert {cpw for (f, ks, cpw) in hit if f == form} == (set(nc.CPWS) if mut != "wide_tall_threshold" or form != "bf16x3" else {96}), (mut, form, hit)


def test_the_gate_cases_are_the_gate_files():
    for c, form, tier, cpw in nc.gate_params():
        assert c.cout % 192 == 0 and nc.supported(form, 1, c.cin, c.cout, cpw) and tier in gc.TIERS[form]
