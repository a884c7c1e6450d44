"""The two variance scans do not move.  The substitution scan's quadratic form became a device function shared with the indel variance
scan (sv_quad_body under a row map), and both scans then became one file with one quadratic-form template, one check and one slab loop
(var_scan.inc): tests/golden/subst_var_scan_digests.json holds the sha256 of what xgpr_conv_token_subst_var_scan_f32 wrote for every
case of tests/dense_subst_var_scan.py on the commit before the first step, tests/golden/indel_var_scan_digests.json what ONE call of
xgpr_conv_token_indel_var_scan_f32 wrote into both outputs for every case of tests/dense_indel_var_scan.py on the commit before the
second (tools/var_scan_digests.py).  A case whose operands hash differently (another numpy built them) says nothing about the kernels
and is reported as such."""
import json
import os
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import var_scan_digests as vsd      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "subst_var_scan_digests.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def recorded_indel():
    with open(os.path.join(ROOT, "tests", "golden", "indel_var_scan_digests.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", vsd.NAMES)
def test_the_output_has_the_recorded_bits(recorded, name):
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    assert vsd.first_difference(recorded, name) is None                   # the operands are the recorded ones
    assert vsd.first_difference(recorded, name, vsd.output_digest(ext, name)) is None


@pytest.mark.parametrize("name", vsd.INDEL_NAMES)
def test_both_indel_outputs_have_the_recorded_bits(recorded_indel, name):
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    assert vsd.indel_first_difference(recorded_indel, name) is None       # the operands are the recorded ones
    assert vsd.indel_first_difference(recorded_indel, name, vsd.indel_output_digests(ext, name)) is None
