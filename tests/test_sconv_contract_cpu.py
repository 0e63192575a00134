"""The sphere convolutions' argument contract against its record (tests/sconv_contract_cases.py, tests/golden/sconv_contract.json): every pure entry point
returns what it returned, and every launch and pack entry point refuses exactly the calls it refused.  The contract is host logic; it is replayed where no device is
visible, because a call that passes it would otherwise launch on the host pointers of the case file."""
import json
import os

import pytest

import sconv_contract_cases as cc


@pytest.fixture(scope="module")
def replay():
    path = os.environ.get("LIC360_LIB") or os.path.join(cc.ROOT, "360-image-compression_amd", "liblic360_hip.so")       # the library `import lic360` loads
    if not os.path.exists(path):
        pytest.skip("the library is not built")
    if cc.device_visible():
        pytest.skip("a device is visible: the passing rows would launch on host pointers")
    return cc.record(cc.load(path)), json.load(open(cc.GOLDEN))


def test_the_record_holds_the_case_files_rows(replay):
    """no row left out on either side, and the counts the case file promises: 17 pure entry points, 15 launch and 6 pack entry points"""
    now, golden = replay
    for part in ("pure", "calls"):
        assert sorted(now[part]) == sorted(golden[part]), part
    assert len(cc.PURE) + 1 == 17 and sorted(k for k, _ in cc.ENTRIES) == sorted(set(k for k, _ in cc.ENTRIES))
    assert sum(kind != "pack" for _, kind in cc.ENTRIES) == 15 and sum(kind == "pack" for _, kind in cc.ENTRIES) == 6
    assert all(len(golden["calls"][cc.key(name, b, fields)]) == len(values) for name, _, b, fields, values in cc.groups())


def test_the_pure_entry_points_return_what_they_returned(replay):
    now, golden = replay
    bad = [k for k in golden["pure"] if now["pure"][k] != golden["pure"][k]]
    assert not bad, bad


def test_every_call_is_refused_or_not_as_it_was(replay):
    now, golden = replay
    bad = [(k, now["calls"][k], golden["calls"][k]) for k in golden["calls"] if now["calls"][k] != golden["calls"][k]]
    assert not bad, bad[:10]
    assert sum(v.count("1") for v in golden["calls"].values()) > 2000 and sum(v.count("0") for v in golden["calls"].values()) > 2000    # both outcomes are pinned
