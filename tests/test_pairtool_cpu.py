"""The six pair tools against tests/records/pairtools.json, the record of what each command line of tests/pairtool_cases.py
printed, how it exited, what it returned, which files it wrote and which calls it made on its context before the tools were
given one front end (pairtool.py).  The record is made by ``python tests/pairtool_cases.py --record``; it is never made from
the code it is held against."""
import json

import pytest

import pairtool_cases as cases


@pytest.fixture(scope="module")
def record():
    with open(cases.RECORD) as fh:
        return json.load(fh)


def test_the_record_has_every_case_and_no_other(record):
    ids = [c["id"] for c in cases.CASES]
    assert len(ids) == len(set(ids)) and sorted(record) == sorted(ids)
    assert all(sorted(entry) == ["calls", "exit", "files", "returned", "stdout"] for entry in record.values())


def test_the_table_covers_every_tool():
    tools = ("supportSpans", "supportEnds", "placeUnplaced", "supportSeats", "polishOrder", "scaffoldLinks")
    for tool in tools:
        mine = [c for c in cases.CASES if c["tool"] == tool]
        assert any(c["args"] == ["--help"] for c in mine) and any(c["setup"] == "six" for c in mine), tool
        assert sum("-refused-two_" in c["id"] for c in mine) >= 2 and sum("-refused-" in c["id"] for c in mine) >= 10, tool
    assert {c["tool"] for c in cases.CASES} == set(tools)


@pytest.mark.parametrize("case", cases.CASES, ids=[c["id"] for c in cases.CASES])
def test_a_case_does_what_the_record_says(case, record, tmp_path):
    got, want = cases.run_case(case, tmp_path), record[case["id"]]
    assert got["exit"] == want["exit"]
    assert got["stdout"] == want["stdout"]
    assert got["calls"] == want["calls"]
    assert got["files"] == want["files"]
    assert got["returned"] == want["returned"]
    if "-refused-" in case["id"]:
        assert isinstance(got["exit"], str) and got["files"] == {}
    elif case["args"] == ["--help"]:
        assert got["exit"] == 0 and got["stdout"].startswith("usage: ") and got["calls"] == [] and got["files"] == {}
    else:
        assert got["exit"] is None and got["files"] and got["returned"]
