"""The indel variance scan without a GPU: the brute-force reference of tests/dense_indel_var_scan.py catches every planted mistake
through the comparison the GPU test uses, agrees with the contract's three-term form, and its a-priori caps are at most 1e-2 of the
largest |Q - q~| of every case the GPU test runs, for the deletions and for the insertions; the tenth public header,
include/xgpr_hip_indel_var_scan.h, held to what tests/test_subst_var_scan_host.py holds the ninth; the launcher's argument validation
through the C ABI (nothing reaches a HIP call: device pointers are dummy integers); the shape predicate and the workspace size on
the host; the recorded digests of both variance scans name every case, and the indel file's operands are the ones built here.  (The compiler's resource report of the new
kernels -- no scratch, no spilled vector register -- is held by tests/test_resource_usage.py, which walks every kernel.)"""
import ctypes
import inspect
import json
import os
import re
import shutil
import sys

import numpy as np
import pytest

import dense_indel_scan as dis
import dense_indel_var_scan as div
import dense_subst_var_scan as dv
from dense_reference import LD
from test_cabi import _build_module
from test_subst_var_scan_host import _codes

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))
HEADER = os.path.join(ROOT, "include", "xgpr_hip_indel_var_scan.h")
NAMES = ["xgpr_conv_token_indel_var_scan_f32", "xgpr_conv_token_indel_var_scan_ok", "xgpr_conv_token_indel_var_scan_workspace_bytes"]
CASE_NAMES = [c[0] for c in div.CASES]


def _live(k):
    """(deletions, insertions): the entries that hold a mutant's value."""
    c = k["c"]
    L = c["tokens"].shape[1]
    return (~dis.zero_mask(c["seqlen"], L) & ~np.isnan(np.asarray(k["ref_del"], dtype=np.float64)),
            ~dis.zero_mask(c["seqlen"], L, gaps=True))


def _spreads(k):
    """max |Q - q~_i| over the live deletions and over the live insertions of a case."""
    ld, li = _live(k)
    sd = np.abs(k["ref_del"] - k["ops"]["q_del"][:, None])[ld]
    si = np.abs(k["ref_ins"] - k["ops"]["q_ins"][:, None, None])[li]
    return (float(sd.max()) if sd.size else None), float(si.max())


# ------------------------------------------------------------------------------------------------ 1. the reference and its cap
def test_the_case_list_covers_every_axis():
    assert CASE_NAMES == [c[0] for c in dv.CASES] == [c[0] for c in dis.CASES]       # the twelve operand sets
    assert sorted(nv for _, nv, _, _ in div.CASES) == sorted(nv for _, nv, _, _ in dv.CASES)          # the same nvar list
    assert [pd for _, _, pd, _ in div.CASES] == [pd for _, _, pd, _ in dv.CASES] and any(pd for _, _, pd, _ in div.CASES)
    F = {nm: kw["F"] for nm, kw, _, _ in dis.CASES}
    assert all(nv % 2 == 0 and 2 <= nv <= 2 * F[nm] for nm, nv, _, _ in div.CASES)
    assert {2, 16, 18, 34, 64, 66, 130, 512, 2048} <= {nv for _, nv, _, _ in div.CASES}
    for name in CASE_NAMES:
        c, cw, _, _ = dis.case(name)
        assert int(c["seqlen"].max()) == c["tokens"].shape[1], name                   # the append lands at g = L
    assert dis.case("graph_cw1")[1] == 1 and dis.case("vocab1")[0]["table"].shape[0] == 1
    assert any(int((dis.case(nm)[0]["seqlen"] == dis.case(nm)[1]).sum()) for nm in CASE_NAMES)       # a sequence without a deletion mutant


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_cap_is_two_orders_below_the_spread(name):
    """A condition on the case, not a measurement of the operator: the reference alone."""
    k = div.case(name)
    sd, si = _spreads(k)
    print(name, k["nvar"], "del", k["cap_del"], sd, "ins", k["cap_ins"], si)
    assert 0 < k["cap_ins"] <= 1e-2 * si
    if sd is not None:
        assert 0 < k["cap_del"] <= 1e-2 * sd


def test_the_reference_has_the_contract_s_structure():
    k = div.case("dup_rows")
    c = k["c"]
    L = c["tokens"].shape[1]
    assert (k["ref_del"][dis.zero_mask(c["seqlen"], L)] == 0).all() and (k["ref_ins"][dis.zero_mask(c["seqlen"], L, gaps=True)] == 0).all()
    nan = np.isnan(np.asarray(k["ref_del"], dtype=np.float64))
    want = (c["seqlen"][:, None] == k["cw"]) & (np.arange(L)[None, :] < c["seqlen"][:, None])
    assert np.array_equal(nan, want) and nan.any()
    assert (k["ref_ins"][:, :, 1] == k["ref_ins"][:, :, 3]).all()                     # the duplicated table row
    for which, zeros in (("del", dis.zero_mask(c["seqlen"], L)), ("ins", dis.zero_mask(c["seqlen"], L, gaps=True))):
        ref = k["ref_" + which]
        assert div.check(ref.astype(np.float64), ref, k["cap_" + which], zeros) <= k["cap_" + which]     # passes its own comparison


def test_a_table_of_one_row_still_has_insertions():
    k = div.case("vocab1")
    assert k["ref_ins"].shape[2] == 1 and _spreads(k)[1] > 0 and k["cap_ins"] > 0


PLANT_CASES = ("dup_rows", "w16_c4_cw3", "n65", "n1")       # scaling 1 / 0 / 2 under the intercept, 0 without


@pytest.mark.parametrize("mistake", div.MISTAKES)
def test_a_planted_mistake_is_caught(mistake):
    caught = []
    for name in PLANT_CASES:
        k = div.case(name)
        c = k["c"]
        L = c["tokens"].shape[1]
        bad = div.decomposed(c, k["vm"], k["cw"], k["scaling"], k["icpt"], mistake=mistake)
        for which, got, zeros in (("del", bad[0], dis.zero_mask(c["seqlen"], L)), ("ins", bad[1], dis.zero_mask(c["seqlen"], L, gaps=True))):
            ref, cap = k["ref_" + which], k["cap_" + which]
            ok = ~np.isnan(np.asarray(ref, dtype=np.float64))
            moved = float(np.abs(got - ref)[ok].max()) if ok.any() else 0.0
            print(mistake, name, which, moved, cap)
            if moved > cap:
                with pytest.raises(AssertionError):
                    div.check(got.astype(np.float64), ref, cap, zeros)
                caught.append((name, which))
    assert caught, mistake


def test_every_mistake_has_a_test():
    assert set(div.MISTAKES) == {"old_norm", "no_rescale", "rescale_col0", "junction_short", "del_keeps_covering", "no_cross", "r_once",
                                 "append_past_end", "cos_sin_swapped"}


@pytest.mark.parametrize("name", ["dup_rows", "w128_c21_cw6", "w512_c16_cw20", "n65", "graph_cw1", "vocab1"])
def test_the_three_term_form_is_the_direct_form(name):
    k = div.case(name)
    d, i = div.decomposed(k["c"], k["vm"], k["cw"], k["scaling"], k["icpt"])
    ok = ~np.isnan(np.asarray(k["ref_del"], dtype=np.float64))
    assert np.array_equal(ok, ~np.isnan(np.asarray(d, dtype=np.float64)))
    scale = float(np.abs(k["ref_ins"]).max())
    tol = 64 * k["nvar"] * float(np.finfo(LD).eps) * scale
    assert float(np.abs(i - k["ref_ins"]).max()) <= tol and (not ok.any() or float(np.abs(d - k["ref_del"])[ok].max()) <= tol)


def test_the_recorded_digests_name_every_case():
    """tests/golden/subst_var_scan_digests.json (tools/var_scan_digests.py, recorded on the parent of the commit that moved the
    quadratic form into a shared function): one entry per case of dense_subst_var_scan.CASES, an output digest each."""
    with open(os.path.join(ROOT, "tests", "golden", "subst_var_scan_digests.json")) as f:
        rec = json.load(f)
    assert list(rec["cases"]) == [c[0] for c in dv.CASES] and rec["commit"]
    for name, entry in rec["cases"].items():
        assert re.fullmatch(r"[0-9a-f]{64}", entry["output"]), name
        assert set(entry["inputs"]) == {"tokens", "table", "seqlen", "radem", "chi", "vm", "u64", "q64"}


@pytest.fixture(scope="module")
def indel_digests():
    with open(os.path.join(ROOT, "tests", "golden", "indel_var_scan_digests.json")) as f:
        return json.load(f)


def test_the_indel_digests_name_every_case_and_output(indel_digests):
    """tests/golden/indel_var_scan_digests.json (tools/var_scan_digests.py --op indel, recorded on the parent of the commit that merged
    the two variance scans into var_scan.inc): one entry per case of dense_indel_var_scan.CASES, both outputs of one call each."""
    import var_scan_digests as vsd
    assert re.fullmatch(r"[0-9a-f]{40}", indel_digests["commit"])
    assert list(indel_digests["cases"]) == vsd.INDEL_NAMES == CASE_NAMES and len(CASE_NAMES) == 12
    for name, entry in indel_digests["cases"].items():
        assert set(entry["outputs"]) == set(vsd.INDEL_OUTPUTS) == {"del", "ins"}, name
        assert all(re.fullmatch(r"[0-9a-f]{64}", d) for d in entry["outputs"].values()), name
        assert set(entry["inputs"]) == set(vsd.ARRAYS + vsd.INDEL_DERIVED), name


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_recorded_operands_are_the_ones_built_here(indel_digests, name):
    """... so a mismatch of output digests on the device (tests/test_gpu_subst_var_scan_bits.py) cannot be blamed on the operands."""
    import var_scan_digests as vsd
    assert vsd.indel_input_digests(name) == indel_digests["cases"][name]["inputs"]
    assert vsd.indel_first_difference(indel_digests, name) is None


def test_a_changed_operand_is_reported_as_such(indel_digests):
    import var_scan_digests as vsd
    other = json.loads(json.dumps(indel_digests))
    other["cases"]["n1"]["inputs"]["u_ins"] = "0" * 64
    assert "operands differ (u_ins)" in vsd.indel_first_difference(other, "n1")
    ok = dict(indel_digests["cases"]["n1"]["outputs"])
    assert vsd.indel_first_difference(indel_digests, "n1", ok) is None
    assert vsd.indel_first_difference(indel_digests, "n1", dict(ok, ins="0" * 64)) == "n1: output ins differs from the recorded bits"


# ------------------------------------------------------------------------------------------------ 2. the tenth header
def _declared():
    hdr = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(xgpr_[a-z0-9_]+)\s*\(", hdr)))                # the expression of tests/test_cabi.py


def test_the_header_declares_its_three_entry_points_and_nothing_of_the_other_headers():
    import test_cabi
    import test_cluster_host
    import test_indel_scan_host
    import test_input_grad_host
    import test_pool_header_host
    import test_pool_input_grad_host
    import test_seq_input_grad_host
    import test_subst_scan_host
    import test_subst_var_scan_host
    assert _declared() == NAMES
    assert not set(_declared()) & (set(test_cabi._declared()) | set(test_pool_header_host._declared())
                                   | set(test_input_grad_host._declared()) | set(test_seq_input_grad_host._declared())
                                   | set(test_pool_input_grad_host._declared()) | set(test_cluster_host._declared())
                                   | set(test_subst_scan_host._declared()) | set(test_indel_scan_host._declared())
                                   | set(test_subst_var_scan_host._declared()))


def test_library_exports_every_declared_name():
    bm = _build_module()
    bm.build_extension()
    lib = ctypes.CDLL(bm.LIB)
    for n in _declared():
        assert hasattr(lib, n), f"{n} declared in include/xgpr_hip_indel_var_scan.h but not exported"


def test_ctypes_table_matches_the_header():
    from xgpr_amd import _lib
    assert set(_lib.INDEL_VAR_SCAN_SIGNATURES) == set(_declared())
    assert not set(_lib.INDEL_VAR_SCAN_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.SIZE_FUNCS) | set(_lib.STRING_FUNCS)
                                                      | set(_lib.POOL_SIGNATURES) | set(_lib.INPUT_GRAD_SIGNATURES)
                                                      | set(_lib.SEQ_INPUT_GRAD_SIGNATURES) | set(_lib.POOL_INPUT_GRAD_SIGNATURES)
                                                      | set(_lib.CLUSTER_SIGNATURES) | set(_lib.SUBST_SCAN_SIGNATURES)
                                                      | set(_lib.INDEL_SCAN_SIGNATURES) | set(_lib.SUBST_VAR_SCAN_SIGNATURES))
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, args in _lib.INDEL_VAR_SCAN_SIGNATURES.items():                        # load() applied the table
        fn = getattr(lib, name)
        assert fn.argtypes == args
        sized = name.endswith("_workspace_bytes")
        assert fn.restype is (ctypes.c_size_t if sized else ctypes.c_int), name
        decl = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)", hdr)                 # the tables' lengths are the parameter counts
        assert len(decl.group(2).split(",")) == len(args), name
        assert decl.group(1) == ("size_t" if sized else "int"), name


def test_every_writer_has_a_memory_contract_row():
    import test_gpu_indel_var_scan_memory_contract as table
    writers = {n for n in _declared() if n.endswith("_f32")}
    assert writers == {"xgpr_conv_token_indel_var_scan_f32"}
    assert table.covered_entry_points() == writers


def test_source_id_covers_the_header_and_the_kernels(tmp_path, monkeypatch):
    bm = _build_module()
    assert os.path.samefile(bm.INDEL_VAR_SCAN_HDR, HEADER) and bm.INDEL_VAR_SCAN_HDR in bm.sources()
    assert "var_scan.inc" in [os.path.basename(p) for p in bm.sources()]
    before = bm.source_id()
    copy = tmp_path / "xgpr_hip_indel_var_scan.h"
    shutil.copyfile(HEADER, copy)
    monkeypatch.setattr(bm, "INDEL_VAR_SCAN_HDR", str(copy))
    assert bm.source_id() == before                                                  # name and contents, not the path
    with open(copy, "a") as f:
        f.write("/* changed */\n")
    assert bm.source_id() != before


# ------------------------------------------------------------------------------------------------ 3. launcher validation
A = 0x100000                     # a dummy 4096-byte-aligned address, never dereferenced on these paths
BIG = 1 << 40
ARRAY_DIMS, ARRAY_SIZES, CONV_WIDTH, RFFS_FREQS, SEQLEN, UNSUPPORTED, WORKSPACE = "ARRAY_DIMS", "ARRAY_SIZES", "CONV_WIDTH", "RFFS_FREQS", \
    "SEQLEN_RANGE", "UNSUPPORTED", "WORKSPACE"


def scan(tokens=A, table=A, vm=A, stride=None, u_del=A, q_del=A, u_ins=A, q_ins=A, out_del=A, out_ins=A, radem=A, chi=A, lens=(6, 3, 4),
         seqlen_dev=A, n=3, L=6, vocab=5, C=4, F=40, R=64, nvar=16, cw=3, scaling=1, icpt=1, slab=0, ws=A, wb=BIG):
    from xgpr_amd import _lib
    host = np.asarray(lens, dtype=np.int32) if lens is not None else None
    hp = ctypes.c_void_p(host.ctypes.data) if host is not None else None
    rc = _lib.load().xgpr_conv_token_indel_var_scan_f32(tokens, table, vm, nvar if stride is None else stride, u_del, q_del, u_ins, q_ins,
                                                        out_del, out_ins, radem, chi, hp, seqlen_dev, n, L, vocab, C, F, R, nvar, cw,
                                                        scaling, icpt, slab, ws, wb, None)
    return int(rc), _lib.last_error()


NO_DEL = dict(u_del=None, q_del=None, out_del=None)
NO_INS = dict(u_ins=None, q_ins=None, out_ins=None)

REFUSALS = {
    # in the documented order
    "n < 0": (dict(n=-1), ARRAY_DIMS),
    "L < 1": (dict(L=0), ARRAY_DIMS),
    "C < 1": (dict(C=0), ARRAY_DIMS),
    "scaling 3": (dict(scaling=3), ARRAY_DIMS),
    "conv_width 0": (dict(cw=0), CONV_WIDTH),
    "conv_width > L": (dict(cw=7), CONV_WIDTH),
    "no frequencies": (dict(F=0), RFFS_FREQS),
    "more frequencies than signs": (dict(F=65), RFFS_FREQS),
    "signs not a multiple of the padded width": (dict(R=72), RFFS_FREQS),
    "nvar odd": (dict(nvar=15), ARRAY_DIMS),
    "nvar 0": (dict(nvar=0), ARRAY_DIMS),
    "nvar above 2 F": (dict(nvar=82), ARRAY_DIMS),
    "a short row stride of vm": (dict(stride=14), ARRAY_SIZES),
    "slab_rows 8": (dict(slab=8), ARRAY_DIMS),
    "slab_rows 40": (dict(slab=40), ARRAY_DIMS),
    "slab_rows negative": (dict(slab=-16), ARRAY_DIMS),
    "no host lengths": (dict(lens=None), SEQLEN),
    "a length below conv_width": (dict(lens=(6, 2, 4)), SEQLEN),
    "a length above L": (dict(lens=(6, 3, 7)), SEQLEN),
    "vocab 0": (dict(vocab=0), ARRAY_DIMS),
    "vocab 257": (dict(vocab=257), ARRAY_DIMS),
    "a window of 2048 elements": (dict(L=40, cw=32, C=64, lens=(40, 32, 33), R=2048), UNSUPPORTED),
    "a table of more than 4608 floats": (dict(vocab=256, C=19, R=64), UNSUPPORTED),
    "nvar above one tile": (dict(F=2048, R=2048, nvar=2050), UNSUPPORTED),
    "no workspace": (dict(ws=None), WORKSPACE),
    "short workspace": (dict(wb=8), WORKSPACE),
    "misaligned workspace": (dict(ws=A + 4), WORKSPACE),
    "NULL tokens": (dict(tokens=None), WORKSPACE),
    "NULL table": (dict(table=None), WORKSPACE),
    "NULL vm": (dict(vm=None), WORKSPACE),
    "NULL radem": (dict(radem=None), WORKSPACE),
    "NULL chi": (dict(chi=None), WORKSPACE),
    "NULL device lengths": (dict(seqlen_dev=None), WORKSPACE),
    "NULL u_del alone": (dict(u_del=None), WORKSPACE),
    "NULL q_del alone": (dict(q_del=None), WORKSPACE),
    "NULL out_del alone": (dict(out_del=None), WORKSPACE),
    "NULL u_ins alone": (dict(u_ins=None), WORKSPACE),
    "NULL q_ins alone": (dict(q_ins=None), WORKSPACE),
    "NULL out_ins alone": (dict(out_ins=None), WORKSPACE),
    "NULL out_ins without the deletions": (dict(NO_DEL, out_ins=None), WORKSPACE),
    "both groups NULL": (dict(NO_DEL, **NO_INS), WORKSPACE),
    # two failing checks at once: the first in the documented order is the one reported
    "n < 0 and conv_width 0": (dict(n=-1, cw=0), ARRAY_DIMS),
    "conv_width 0 and nvar odd": (dict(cw=0, nvar=15), CONV_WIDTH),
    "no frequencies and nvar odd": (dict(F=0, nvar=15), RFFS_FREQS),
    "nvar odd and a short stride": (dict(nvar=15, stride=3), ARRAY_DIMS),
    "a short stride and slab_rows 8": (dict(stride=14, slab=8), ARRAY_SIZES),
    "slab_rows 8 and a bad length": (dict(slab=8, lens=(6, 2, 4)), ARRAY_DIMS),
    "a bad length and vocab 257": (dict(lens=(6, 2, 4), vocab=257), SEQLEN),
    "vocab 257 and no workspace": (dict(vocab=257, ws=None), ARRAY_DIMS),
    "an unsupported table and no workspace": (dict(vocab=256, C=19, ws=None), UNSUPPORTED),
    "short workspace and both groups NULL": (dict(NO_DEL, wb=8, **NO_INS), WORKSPACE),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_validation_outcome(name):
    kw, code = REFUSALS[name]
    rc, err = scan(**kw)
    assert rc == _codes()[code] and rc < 0, (rc, err)
    assert err
    if "workspace" in name and "NULL" not in name and code == WORKSPACE:
        assert "xgpr_conv_token_indel_var_scan_workspace_bytes" in err
    if name.startswith("NULL"):
        assert err == "NULL array pointer"
    if name == "both groups NULL":
        assert err.startswith("NULL array pointer") and "both NULL" in err


def test_the_documented_order_is_the_order_of_the_header():
    """The header's list of checks names the codes in the order REFUSALS walks them: the order of the ninth header."""
    doc = open(HEADER).read()
    doc = doc[doc.index("Checks, before anything is launched"):]
    order = re.findall(r"XGPR_ERR_([A-Z_]+)", doc)
    assert order == [ARRAY_DIMS, CONV_WIDTH, RFFS_FREQS, ARRAY_DIMS, ARRAY_SIZES, ARRAY_DIMS, SEQLEN, ARRAY_DIMS, UNSUPPORTED, WORKSPACE,
                     UNSUPPORTED]
    ninth = open(os.path.join(ROOT, "include", "xgpr_hip_subst_var_scan.h")).read()
    assert order == re.findall(r"XGPR_ERR_([A-Z_]+)", ninth[ninth.index("Checks, before anything is launched"):])


def test_one_group_alone_passes_validation():
    """Either group may be NULL as a whole: with n == 0 nothing is launched and the call returns 0 -- but a half-given group is looked at
    only behind n == 0, as the ninth header's NULL arrays are."""
    assert scan(n=0, lens=None, **NO_DEL)[0] == 0 and scan(n=0, lens=None, **NO_INS)[0] == 0


def test_the_position_count_of_one_launch():
    from xgpr_amd import _lib
    for n, code in (((1 << 24) // 7 + 1, _codes()[UNSUPPORTED]),):
        lens = np.full(n, 6, dtype=np.int32)
        rc = _lib.load().xgpr_conv_token_indel_var_scan_f32(A, A, A, 16, A, A, A, A, A, A, A, A, ctypes.c_void_p(lens.ctypes.data), A, n, 6, 5,
                                                            4, 40, 64, 16, 3, 1, 1, 0, A, BIG, None)
        assert rc == code and "n * (L + 1)" in _lib.last_error()


def test_no_sequences():
    none = dict(n=0, lens=None, tokens=None, table=None, vm=None, radem=None, chi=None, seqlen_dev=None, ws=None, wb=0, **NO_DEL, **NO_INS)
    assert scan(**none)[0] == 0
    assert scan(n=0, lens=None, vocab=257)[0] == _codes()[ARRAY_DIMS]                 # ... but the shape is still checked
    assert scan(n=0, lens=None, nvar=15)[0] == _codes()[ARRAY_DIMS]
    assert scan(n=0, lens=None, vocab=256, C=19)[0] == _codes()[UNSUPPORTED]


def test_workspace_bytes():
    from xgpr_amd import _lib
    lib = _lib.load()
    wsb = lambda R, nvar, slab: int(lib.xgpr_conv_token_indel_var_scan_workspace_bytes(R, nvar, slab))
    masks = int(lib.xgpr_rbf_workspace_bytes(64))
    assert wsb(64, 16, 16) == masks + 16 * 16 * 8 and wsb(64, 16, 48) == masks + 48 * 16 * 8
    assert [wsb(64, 16, 8), wsb(64, 16, 24), wsb(64, 16, -16), wsb(64, 15, 16), wsb(64, 0, 16), wsb(0, 16, 16)] == [0] * 6
    for nvar in (2, 16, 130, 512, 2048):                                              # the formula and the default of the ninth header
        for slab in (0, 16, 4096):
            assert wsb(64, nvar, slab) == int(lib.xgpr_conv_token_subst_var_scan_workspace_bytes(64, nvar, slab)) > 0
        rows = (wsb(64, nvar, 0) - masks) // (8 * nvar)
        assert rows % 16 == 0 and rows == min(65536, (128 << 20) // (8 * nvar) // 16 * 16)
    need = wsb(64, 16, 32)                                                            # the advertised size is the bound the launcher checks
    assert scan(slab=32, wb=need - 1)[0] == _codes()[WORKSPACE]


def test_ok_predicate():
    from xgpr_amd import _lib
    lib = _lib.load()
    ok = lambda *a: int(lib.xgpr_conv_token_indel_var_scan_ok(*a))
    assert [ok(1, 1, 1, 1, 2), ok(12, 6, 4, 8, 16), ok(189, 21, 21, 8192, 512), ok(189, 21, 21, 8192, 2048), ok(1008, 5, 21, 1030, 130),
            ok(54, 256, 18, 130, 260)] == [1] * 6
    assert [ok(12, 6, 4, 8, 15), ok(12, 6, 4, 8, 0), ok(12, 6, 4, 8, 18), ok(12, 6, 4, 8, -2), ok(189, 21, 21, 8192, 2050),
            ok(1025, 5, 21, 8, 4), ok(57, 256, 19, 8, 4), ok(12, 6, 4, 0, 2)] == [0] * 8
    for args in ((12, 6, 4, 8, 16), (1008, 5, 21, 1030, 130), (1025, 5, 21, 8, 4), (57, 256, 19, 8, 4), (12, 6, 4, 8, 15)):
        assert ok(*args) == int(lib.xgpr_conv_token_subst_var_scan_ok(*args))         # the predicate of the substitution variance scan
        assert ok(*args[:4], 2) == int(lib.xgpr_conv_token_indel_scan_ok(*args[:4]))


def test_python_wrappers():
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    assert ext.conv_token_indel_var_scan_ok(189, 21, 21, 8192, 512) == 1 and ext.conv_token_indel_var_scan_ok(189, 21, 21, 8192, 511) == 0
    assert ext.conv_token_indel_var_scan_workspace_bytes(64, 16, 16) == ext._LIB.xgpr_rbf_workspace_bytes(64) + 16 * 16 * 8
    sig = inspect.signature(ext.hipConvTokenIndelVarScan)
    assert list(sig.parameters) == ["tokens", "table", "vm", "u_del", "q_del", "u_ins", "q_ins", "deletions", "insertions", "radem", "chi",
                                    "seqlen", "conv_width", "scaling_type", "fit_intercept", "slab_rows", "workspace"]
    assert sig.parameters["slab_rows"].default == 0 and sig.parameters["workspace"].default is None
    from xgpr_amd.kernels import ConvSORFKernel
    from xgpr_amd.models import xGPRegression
    assert callable(ConvSORFKernel.indel_variance_scan) and callable(ConvSORFKernel.indel_variance_scan_composed)
    sig = inspect.signature(xGPRegression.predict_indels)
    assert list(sig.parameters)[:5] == ["self", "input_x", "sequence_lengths", "token_table", "chunk_size"]   # the old positional parameters
    assert sig.parameters["chunk_size"].default == 64 and sig.parameters["get_var"].default is False
    assert "not built" not in xGPRegression.predict_indels.__doc__
    for doc in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "variance of insertions and deletions is not built" not in text and "variance of indels is not built" not in text
