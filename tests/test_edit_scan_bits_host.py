"""The host-side twin of tests/test_gpu_edit_scan_bits.py: tests/golden/edit_scan_digests.json covers every case and every output, names
the commit it was recorded from, and its INPUT digests are those of the operands that tests/dense_subst_scan.py /
tests/dense_indel_scan.py build here -- so a mismatch of output digests on the device cannot be blamed on the operands."""
import json
import os
import re
import sys

import pytest

import dense_indel_scan as dis
import dense_subst_scan as dss

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scan_digests as sd      # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "edit_scan_digests.json")) as f:
        return json.load(f)


def test_the_file_covers_every_case_and_output(recorded):
    assert re.fullmatch(r"[0-9a-f]{40}", recorded["commit"])
    assert sd.NAMES == [c[0] for c in dss.CASES] == [c[0] for c in dis.CASES] and len(sd.NAMES) == 12
    assert list(recorded["cases"]) == sd.NAMES
    for name, entry in recorded["cases"].items():
        assert set(entry["outputs"]) == set(sd.OUTPUTS) == {"subst", "scores", "del", "ins"}, name
        assert set(entry["inputs"]) == {"subst", "indel"} and all(set(v) == set(sd.ARRAYS) for v in entry["inputs"].values()), name
        assert all(re.fullmatch(r"[0-9a-f]{64}", d) for d in entry["outputs"].values()), name


@pytest.mark.parametrize("name", sd.NAMES)
def test_the_recorded_operands_are_the_ones_built_here(recorded, name):
    assert sd.input_digests(name) == recorded["cases"][name]["inputs"]
    assert sd.first_difference(recorded, name) is None


def test_a_changed_operand_is_reported_as_such(recorded):
    other = json.loads(json.dumps(recorded))
    other["cases"]["n1"]["inputs"]["indel"]["chi"] = "0" * 64
    assert "operands differ" in sd.first_difference(other, "n1")
    ok = {o: recorded["cases"]["n1"]["outputs"][o] for o in sd.OUTPUTS}
    assert sd.first_difference(recorded, "n1", ok) is None
    assert sd.first_difference(recorded, "n1", dict(ok, ins="0" * 64)) == "n1: output ins differs from the recorded bits"
