"""The C-ABI's refusals, pinned without a GPU: every row of tests/capi_refusal_cases.py — each bad
argument of each launching entry point, the empty batch, the ZMPC_ESTATE refusals decided from a
plan's fields, and pairs of them — answers the return code and the message, character for
character, that the library answered before capi.hip's disturbance paths were merged
(tests/golden/capi_refusals.json).  For a pair the record says which of two true messages wins:
the order of an entry point's checks is behaviour."""
import json
import os

import pytest

import capi_refusal_cases as cc
from conftest import GOLDEN

from mpc_bipedal import _native  # noqa: E402

ROWS = cc.rows()
with open(os.path.join(GOLDEN, cc.FILE)) as _f:
    RECORD = json.load(_f)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_native.LIB_PATH):
        pytest.fail("libzmpc.so not built (run __graft_entry__.build())")
    lib = _native.load()
    yield lib
    cc.answer(lib, "zmpc_step", {"B": 0})  # a passing call leaves no message behind


def test_table_and_record_hold_the_same_rows():
    assert sorted(name for name, _, _ in ROWS) == sorted(RECORD)
    # every launching entry point of the header but the plan's own calls
    launching = {s for s in _native.SIGNATURES if not s.startswith("zmpc_plan_")} - \
        {"zmpc_abi_version", "zmpc_last_error"}
    assert {symbol for symbol, _, _ in cc.ENTRIES.values()} == launching


def test_no_recorded_row_reaches_a_device_call():
    for name, _, overrides in ROWS:
        assert cc.reaches_no_device(overrides, RECORD[name]), name


@pytest.mark.parametrize("variant", sorted(cc.ENTRIES))
def test_entry_point_refuses_what_it_refused(lib, variant):
    mine = [(name, o) for name, v, o in ROWS if v == variant]
    assert mine
    wrong = {}
    for name, overrides in mine:
        # (the record is consulted first: a row it does not hold as a refusal is never called)
        assert cc.reaches_no_device(overrides, RECORD[name]), name
        got = cc.answer(lib, variant, overrides)
        if got != RECORD[name]:
            wrong[name] = (got, RECORD[name])
    assert not wrong, wrong
