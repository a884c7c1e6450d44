"""The three edit-scan operators bit for bit: every output of hipConvTokenSubstScan, hipConvTokenWindowScores and hipConvTokenIndelScan
(both outputs) on every case of tests/dense_subst_scan.py / tests/dense_indel_scan.py has the sha256 that tools/scan_digests.py recorded
in tests/golden/edit_scan_digests.json from the commit named there -- the one before the substitution and indel kernels became one
template.  The dense references hold the operators to a-priori caps; this holds them to the contract of DESIGN.md 3.20 / 3.21: every
output is a bitwise function of its sequence, the table and the weights, so a change that moves a last bit is a change of behaviour.
(tests/test_edit_scan_bits_host.py holds the recorded INPUT digests to what the case builders make, without a device.)"""
import json
import os
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scan_digests as sd      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "edit_scan_digests.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


@pytest.mark.parametrize("name", sd.NAMES)
def test_every_output_has_the_recorded_bits(ext, recorded, name):
    assert sd.first_difference(recorded, name) is None                       # the operands are those of the recording
    got = sd.output_digests(ext, name)
    assert set(got) == set(sd.OUTPUTS) == set(recorded["cases"][name]["outputs"])
    for out in sd.OUTPUTS:
        assert got[out] == recorded["cases"][name]["outputs"][out], f"{name}: output {out} differs from the recorded bits"
