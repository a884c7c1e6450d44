"""The single-deletion / single-insertion scan without a GPU: the brute-force dense reference of tests/dense_indel_scan.py agrees with
the contract's decomposition, catches every planted mistake through the comparison the GPU test uses (and passes it unplanted), and its
a-priori caps are at most 1e-2 of the largest output of every case the GPU test runs; the eighth public header,
include/xgpr_hip_indel_scan.h, held to what tests/test_subst_scan_host.py holds the seventh; the launchers' argument validation
through the C ABI (nothing reaches a HIP call: device pointers are dummy integers); the shape predicate on the host; and the
compiler's resource report for the new kernels."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest

import dense_indel_scan as dis
import dense_reference as dr
from test_cabi import _build_module

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "xgpr_hip_indel_scan.h")
NAMES = ["xgpr_conv_token_indel_scan_f32", "xgpr_conv_token_indel_scan_ok", "xgpr_conv_token_window_scores_f32"]


def _operands(name):
    c, cw, scaling, icpt = dis.case(name)
    return (c["tokens"], c["table"], c["seqlen"], c["w"], c["radem"], c["chi"], cw, scaling, icpt)


def _finite_max(a):
    a = np.asarray(a, dtype=np.float64)
    a = a[np.isfinite(a)]
    return float(np.abs(a).max()) if a.size else 0.0


# ------------------------------------------------------------------------------------------------ 1. the plants
PLANT_CASE = "dup_rows"             # conv_width 4, V = 5 != C = 6, scaling 1, intercept on, lengths L and conv_width (the NaN row)


def test_the_unplanted_reference_passes_its_own_comparison():
    c, cw, _, _, sc, dele, ins, cs, cd, ci = dis.reference(PLANT_CASE)
    n, L = c["tokens"].shape
    assert dis.check(sc.astype(np.float64), sc, cs, dis.zero_mask(c["seqlen"] - cw + 1, L)) <= cs
    assert dis.check(dele.astype(np.float64), dele, cd, dis.zero_mask(c["seqlen"], L)) <= cd
    assert dis.check(ins.astype(np.float64), ins, ci, dis.zero_mask(c["seqlen"], L, gaps=True)) <= ci
    short = c["seqlen"] == cw
    assert short.any() and not short.all()
    for i in range(n):
        s = int(c["seqlen"][i])
        assert np.isnan(dele[i, :s].astype(np.float64)).all() == bool(short[i]) and not np.isnan(dele[i, s:].astype(np.float64)).any()
    assert not np.isnan(ins.astype(np.float64)).any()
    assert (ins[:, :, 1] == ins[:, :, 3]).all()                               # the duplicated table row


def test_the_decomposition_is_the_brute_force():
    """The contract's formulas against every mutant written out, in long double: what the kernels implement is the definition."""
    for name in ("dup_rows", "graph_cw1", "w16_c4_cw3", "n65"):
        _, _, _, _, _, dele, ins, _, _, _ = dis.reference(name)
        dd, ii = dis.decomposed(*_operands(name))
        assert np.array_equal(np.isnan(dd.astype(np.float64)), np.isnan(dele.astype(np.float64)))
        tol = 1e3 * dr.LD_EPS * max(_finite_max(dele), _finite_max(ins))
        assert float(np.nanmax(np.abs(dd - dele))) <= tol and float(np.abs(ii - ins).max()) <= tol


@pytest.mark.parametrize("mistake", dis.MISTAKES)
def test_a_planted_mistake_is_caught(mistake):
    c, cw, _, _, _, dele, ins, _, cd, ci = dis.reference(PLANT_CASE)
    L = c["tokens"].shape[1]
    bd, bi = dis.decomposed(*_operands(PLANT_CASE), mistake=mistake)
    with pytest.raises(AssertionError):
        dis.check(bd.astype(np.float64), dele, cd, dis.zero_mask(c["seqlen"], L))
        dis.check(bi.astype(np.float64), ins, ci, dis.zero_mask(c["seqlen"], L, gaps=True))
    print(mistake, float(np.nanmax(np.abs(bd - dele))), cd, float(np.abs(bi - ins).max()), ci)


def test_every_mistake_has_a_test():
    assert set(dis.MISTAKES) == {"junction_short", "remap_wrong_side", "old_norm", "norm_by_length", "keep_w0", "ins_removes_covering",
                                 "append_past_end"}


def test_the_cases_are_those_of_the_substitution_scan():
    import dense_subst_scan as dss
    assert [c[0] for c in dis.CASES] == [c[0] for c in dss.CASES]
    for mine, theirs in zip(dis.CASES, dss.CASES):                                   # shapes, scalings, intercept flags; lengths may move
        assert mine[2:] == theirs[2:] and {k: v for k, v in mine[1].items() if k != "lengths"} == {k: v for k, v in theirs[1].items() if k != "lengths"}
    names = {c[0] for c in dis.CASES}
    assert {"vocab256_c18", "dup_rows", "n65", "n1", "graph_cw1"} <= names
    for nm in ("w16_c4_cw3", "w128_c21_cw6", "w256_c21_cw9", "w1024_c21_cw48"):      # s == conv_width and s == conv_width + 1
        c, cw, _, _ = dis.case(nm)
        assert (c["seqlen"] == cw).any() and (c["seqlen"] == cw + 1).any(), nm
    c, cw, _, _ = dis.case("graph_cw1")
    assert cw == 1 and (c["seqlen"] == 1).any()


@pytest.mark.parametrize("name", [c[0] for c in dis.CASES])
def test_the_caps_are_two_orders_below_the_outputs(name):
    """A condition on the case, not a measurement of the operator: the reference alone; deletions and insertions separately."""
    _, _, _, _, sc, dele, ins, cs, cd, ci = dis.reference(name)
    for what, cap, ref in (("scores", cs, sc), ("del", cd, dele), ("ins", ci, ins)):
        big = _finite_max(ref)
        print(name, what, cap, big, cap / big if big else None)
        assert big > 0, "every case has something to scan"
        assert 0 < cap <= 1e-2 * big


# ------------------------------------------------------------------------------------------------ 2. identities on the reference
@pytest.mark.parametrize("name", ["dup_rows", "graph_cw1", "w64_onehot21_cw3"])
def test_the_window_scores_sum_to_the_dense_feature_row_times_w(name):
    c, cw, scaling, icpt, sc, _, _, _, _, _ = dis.reference(name)
    F = c["chi"].shape[0]
    z = dr.conv_features(c["table"].astype(dr.LD)[c["tokens"].astype(np.int64) % c["table"].shape[0]], c["seqlen"], c["radem"], c["chi"], cw, scaling)
    w = np.asarray(c["w"], dtype=dr.LD)
    if icpt:
        z[:, 0] = 1                                                          # transform_x: column 0 is the constant
    for i, s in enumerate(c["seqlen"]):
        nk = int(s) - cw + 1
        total = dr.conv_row_scale(F, nk, scaling) * sc[i].sum() + (w[0] if icpt else 0)
        assert abs(float(total - z[i] @ w)) <= 1e3 * dr.LD_EPS * float(np.abs(w).sum())
        assert (sc[i, nk:] == 0).all()


def test_deleting_either_of_two_adjacent_equal_tokens_is_the_same_mutant():
    c, cw, scaling, icpt = dis.case("w16_c4_cw3")
    tokens = c["tokens"].copy()
    tokens[0, 4] = tokens[0, 3]                                              # sequence 0 has the full length 9
    dele, ins = dis.indel_scan(tokens[:1], c["table"], c["seqlen"][:1], c["w"], c["radem"], c["chi"], cw, scaling, icpt)
    assert dele[0, 3] == dele[0, 4] and dele[0, 3] != dele[0, 2]
    # ... and inserting v next to an existing v, on either side
    v = int(tokens[0, 3])
    assert ins[0, 3, v] == ins[0, 4, v] == ins[0, 5, v] and ins[0, 3, v] != ins[0, 2, v]


# ------------------------------------------------------------------------------------------------ 3. the eighth header
def _declared():
    hdr = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(xgpr_[a-z0-9_]+)\s*\(", hdr)))                # the expression of tests/test_cabi.py


def test_the_header_declares_its_three_entry_points_and_nothing_of_the_other_headers():
    import test_cabi
    import test_cluster_host
    import test_input_grad_host
    import test_pool_header_host
    import test_pool_input_grad_host
    import test_seq_input_grad_host
    import test_subst_scan_host
    assert _declared() == NAMES
    assert not set(_declared()) & (set(test_cabi._declared()) | set(test_pool_header_host._declared())
                                   | set(test_input_grad_host._declared()) | set(test_seq_input_grad_host._declared())
                                   | set(test_pool_input_grad_host._declared()) | set(test_cluster_host._declared())
                                   | set(test_subst_scan_host._declared()))


def test_library_exports_every_declared_name():
    bm = _build_module()
    bm.build_extension()
    lib = ctypes.CDLL(bm.LIB)
    for n in _declared():
        assert hasattr(lib, n), f"{n} declared in include/xgpr_hip_indel_scan.h but not exported"


def test_ctypes_table_matches_the_header():
    from xgpr_amd import _lib
    assert set(_lib.INDEL_SCAN_SIGNATURES) == set(_declared())
    assert not set(_lib.INDEL_SCAN_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.SIZE_FUNCS) | set(_lib.STRING_FUNCS)
                                                  | set(_lib.POOL_SIGNATURES) | set(_lib.INPUT_GRAD_SIGNATURES)
                                                  | set(_lib.SEQ_INPUT_GRAD_SIGNATURES) | set(_lib.POOL_INPUT_GRAD_SIGNATURES)
                                                  | set(_lib.CLUSTER_SIGNATURES) | set(_lib.SUBST_SCAN_SIGNATURES))
    lib = _lib.load()
    for name, args in _lib.INDEL_SCAN_SIGNATURES.items():                            # load() applied the table
        fn = getattr(lib, name)
        assert fn.argtypes == args
        assert fn.restype is ctypes.c_int, name
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, args in _lib.INDEL_SCAN_SIGNATURES.items():                            # the tables' lengths are the parameter counts
        decl = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert len(decl.group(2).split(",")) == len(args), name
        assert decl.group(1) == "int", name


def test_every_writer_has_a_memory_contract_row():
    import test_gpu_indel_scan_memory_contract as table
    writers = {n for n in _declared() if n.endswith("_f32")}
    assert writers == {"xgpr_conv_token_window_scores_f32", "xgpr_conv_token_indel_scan_f32"}
    assert table.covered_entry_points() == writers


def test_source_id_covers_the_header(tmp_path, monkeypatch):
    bm = _build_module()
    assert os.path.samefile(bm.INDEL_SCAN_HDR, HEADER) and bm.INDEL_SCAN_HDR in bm.sources()
    names = [os.path.basename(p) for p in bm.sources()]
    assert "edit_scan.inc" in names and "subst_scan.inc" not in names and "indel_scan.inc" not in names
    before = bm.source_id()
    copy = tmp_path / "xgpr_hip_indel_scan.h"
    shutil.copyfile(HEADER, copy)
    monkeypatch.setattr(bm, "INDEL_SCAN_HDR", str(copy))
    assert bm.source_id() == before                                                  # name and contents, not the path
    with open(copy, "a") as f:
        f.write("/* changed */\n")
    assert bm.source_id() != before


# ------------------------------------------------------------------------------------------------ 4. launcher validation
A = 0x100000                     # a dummy 4096-byte-aligned address, never dereferenced on these paths
BIG = 1 << 40
ARRAY_DIMS, CONV_WIDTH, RFFS_FREQS, SEQLEN, UNSUPPORTED, WORKSPACE = "ARRAY_DIMS", "CONV_WIDTH", "RFFS_FREQS", "SEQLEN_RANGE", \
    "UNSUPPORTED", "WORKSPACE"


def _codes():
    """The error codes by name, from include/xgpr_hip.h."""
    hdr = open(os.path.join(ROOT, "include", "xgpr_hip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"XGPR_ERR_([A-Z_]+)\s*=?\s*\(?(-\d+)\)?", hdr)}


def _host(lens):
    host = np.asarray(lens, dtype=np.int32) if lens is not None else None
    return host, (ctypes.c_void_p(host.ctypes.data) if host is not None else None)


def scan(tokens=A, table=A, w=A, scores=A, dele=A, ins=A, radem=A, chi=A, lens=(6, 3, 4), seqlen_dev=A, n=3, L=6, vocab=5, C=4, F=40,
         R=64, cw=3, scaling=1, icpt=1, ws=A, wb=BIG):
    from xgpr_amd import _lib
    host, hp = _host(lens)
    rc = _lib.load().xgpr_conv_token_indel_scan_f32(tokens, table, w, scores, dele, ins, radem, chi, hp, seqlen_dev, n, L, vocab, C, F, R,
                                                    cw, scaling, icpt, ws, wb, None)
    return int(rc), _lib.last_error()


def score(tokens=A, table=A, w=A, scores=A, radem=A, chi=A, lens=(6, 3, 4), seqlen_dev=A, n=3, L=6, vocab=5, C=4, F=40, R=64, cw=3,
          icpt=1, ws=A, wb=BIG):
    from xgpr_amd import _lib
    host, hp = _host(lens)
    rc = _lib.load().xgpr_conv_token_window_scores_f32(tokens, table, w, scores, radem, chi, hp, seqlen_dev, n, L, vocab, C, F, R, cw, icpt,
                                                       ws, wb, None)
    return int(rc), _lib.last_error()


REFUSALS = {
    # in the documented order
    "n < 0": (dict(n=-1), ARRAY_DIMS),
    "L < 1": (dict(L=0), ARRAY_DIMS),
    "C < 1": (dict(C=0), ARRAY_DIMS),
    "scaling 3": (dict(scaling=3), ARRAY_DIMS),
    "scaling -1": (dict(scaling=-1), ARRAY_DIMS),
    "conv_width 0": (dict(cw=0), CONV_WIDTH),
    "conv_width > L": (dict(cw=7), CONV_WIDTH),
    "no frequencies": (dict(F=0), RFFS_FREQS),
    "more frequencies than signs": (dict(F=65), RFFS_FREQS),
    "signs not a multiple of the padded width": (dict(R=72), RFFS_FREQS),
    "no host lengths": (dict(lens=None), SEQLEN),
    "a length below conv_width": (dict(lens=(6, 2, 4)), SEQLEN),
    "a length above L": (dict(lens=(6, 3, 7)), SEQLEN),
    "vocab 0": (dict(vocab=0), ARRAY_DIMS),
    "vocab 257": (dict(vocab=257), ARRAY_DIMS),
    "a window of 2048 elements": (dict(L=40, cw=32, C=64, lens=(40, 32, 33), R=2048), UNSUPPORTED),
    "a table of more than 4608 floats": (dict(vocab=256, C=19, R=64), UNSUPPORTED),
    "no workspace": (dict(ws=None), WORKSPACE),
    "short workspace": (dict(wb=8), WORKSPACE),
    "NULL tokens": (dict(tokens=None), WORKSPACE),
    "NULL table": (dict(table=None), WORKSPACE),
    "NULL w": (dict(w=None), WORKSPACE),
    "NULL scores": (dict(scores=None), WORKSPACE),
    "NULL radem": (dict(radem=None), WORKSPACE),
    "NULL chi": (dict(chi=None), WORKSPACE),
    "NULL device lengths": (dict(seqlen_dev=None), WORKSPACE),
    "both outputs NULL": (dict(dele=None, ins=None), WORKSPACE),
    # two failing checks at once: the first in the documented order is the one reported
    "n < 0 and conv_width 0": (dict(n=-1, cw=0), ARRAY_DIMS),
    "conv_width 0 and no frequencies": (dict(cw=0, F=0), CONV_WIDTH),
    "no frequencies and a bad length": (dict(F=0, lens=(6, 2, 4)), RFFS_FREQS),
    "a bad length and vocab 257": (dict(lens=(6, 2, 4), vocab=257), SEQLEN),
    "vocab 257 and no workspace": (dict(vocab=257, ws=None), ARRAY_DIMS),
    "an unsupported table and no workspace": (dict(vocab=256, C=19, ws=None), UNSUPPORTED),
    "short workspace and NULL scores": (dict(wb=8, scores=None), WORKSPACE),
    "short workspace and both outputs NULL": (dict(wb=8, dele=None, ins=None), WORKSPACE),
}
SCAN_ONLY = ("scaling 3", "scaling -1", "both outputs NULL", "short workspace and both outputs NULL")   # the scores call has neither argument


@pytest.mark.parametrize("call,name", [(c, nm) for nm in sorted(REFUSALS) for c in ("scan", "scores") if c == "scan" or nm not in SCAN_ONLY])
def test_validation_outcome(call, name):
    kw, code = REFUSALS[name]
    rc, err = (scan if call == "scan" else score)(**kw)
    assert rc == _codes()[code] and rc < 0, (rc, err)
    assert err
    if name.startswith("short workspace") or name == "no workspace":
        assert err == "workspace too small (see xgpr_rbf_workspace_bytes)"
    if name.startswith("NULL"):
        assert err == "NULL array pointer"
    if name == "both outputs NULL":
        assert "both NULL" in err


def test_one_output_may_be_null():
    """... as far as validation goes: with the other checks failing later, a single NULL output is not what is reported."""
    for kw in (dict(dele=None), dict(ins=None)):
        rc, err = scan(n=(1 << 24) // 7 + 1, lens=np.full((1 << 24) // 7 + 1, 6, dtype=np.int32), **kw)
        assert rc == _codes()[UNSUPPORTED] and "n * (L + 1)" in err


def test_the_gap_count_of_one_launch():
    n = (1 << 24) // 7 + 1                                                          # n * (L + 1) >= 2^24 at L = 6
    lens = np.full(n, 6, dtype=np.int32)
    for call in (scan, score):
        rc, err = call(n=n, lens=lens)
        assert rc == _codes()[UNSUPPORTED] and "n * (L + 1)" in err
    # (one fewer sequence passes every check and would launch: not called with dummy pointers)
    assert ((1 << 24) // 7) * 7 < (1 << 24)


def test_no_sequences():
    nothing = dict(n=0, lens=None, tokens=None, table=None, w=None, scores=None, radem=None, chi=None, seqlen_dev=None, ws=None, wb=0)
    assert scan(dele=None, ins=None, **nothing)[0] == 0
    assert score(**nothing)[0] == 0
    for call in (scan, score):
        assert call(n=0, lens=None, vocab=257)[0] == _codes()[ARRAY_DIMS]            # ... but the shape is still checked
        assert call(n=0, lens=None, vocab=256, C=19)[0] == _codes()[UNSUPPORTED]


def test_the_advertised_workspace_is_the_bound_the_launchers_check():
    from xgpr_amd import _lib
    need = int(_lib.load().xgpr_rbf_workspace_bytes(64))
    assert need > 0
    for call in (scan, score):
        assert call(wb=need - 1)[0] == _codes()[WORKSPACE]


def test_ok_predicate_is_the_substitution_scans():
    from xgpr_amd import _lib
    lib = _lib.load()
    ok = lambda width, vocab, C, F: int(lib.xgpr_conv_token_indel_scan_ok(width, vocab, C, F))
    assert [ok(1, 1, 1, 1), ok(12, 6, 4, 8), ok(189, 21, 21, 8192), ok(1008, 5, 21, 1030), ok(1024, 4, 128, 1), ok(54, 256, 18, 130)] == [1] * 6
    assert [ok(1025, 5, 21, 8), ok(2048, 4, 64, 8), ok(57, 256, 19, 8), ok(12, 0, 4, 8), ok(12, 257, 4, 8), ok(0, 5, 4, 8),
            ok(12, 6, 4, 0), ok(12, 6, 0, 8)] == [0] * 8
    for width in (0, 1, 12, 16, 189, 1008, 1024, 1025, 2048):
        for vocab, C in ((0, 4), (1, 1), (6, 4), (21, 21), (256, 18), (256, 19), (257, 4), (5, 0)):
            for F in (0, 1, 8192):
                assert ok(width, vocab, C, F) == int(lib.xgpr_conv_token_subst_scan_ok(width, vocab, C, F)), (width, vocab, C, F)


def test_python_wrappers():
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    assert ext.conv_token_indel_scan_ok(189, 21, 21, 8192) == 1 and ext.conv_token_indel_scan_ok(2048, 4, 64, 8) == 0
    assert callable(ext.hipConvTokenWindowScores) and callable(ext.hipConvTokenIndelScan)
    from xgpr_amd.kernels import ConvSORFKernel
    from xgpr_amd.models import xGPRegression
    assert callable(ConvSORFKernel.window_scores) and callable(ConvSORFKernel.indel_scan) and callable(ConvSORFKernel.indel_scan_composed)
    assert callable(xGPRegression.predict_indels) and callable(xGPRegression.predict_window_scores)


# ------------------------------------------------------------------------------------------------ 5. the compiler's report
# Register-limited occupancy (waves per SIMD) of every instantiation, by mode and LOG2P = 1 .. 10: what tools/resource_usage.py reports
# for the kernels this template replaced -- conv_token_indel_scan_kernel<lg, mode> for the modes 0 .. 2 and
# conv_token_subst_scan_kernel<lg> for mode 3 -- at the commit before the merge.  A floor: the merged template may not fall below it.
OCCUPANCY_FLOOR = {
    0: [4, 3, 3, 3, 3, 3, 3, 3, 3, 3],      # window scores
    1: [3, 3, 3, 3, 3, 3, 3, 3, 3, 2],      # deletions
    2: [2] * 10,                            # insertions
    3: [2] * 10,                            # substitutions
}


def test_the_new_kernels_use_no_scratch_and_spill_nothing():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    report = resource_usage.collect()
    rows = [r for r in report if r["name"].startswith("conv_token_edit_scan_kernel<")]
    assert sorted(r["name"] for r in rows) == sorted(f"conv_token_edit_scan_kernel<{lg}, {mode}>" for lg in range(1, 11) for mode in range(4))
    assert not [r["name"] for r in report if re.match(r"conv_token_(subst|indel)_scan_kernel", r["name"])]      # the two templates it replaced
    for r in rows:
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, r
        lg, mode = (int(v) for v in re.fullmatch(r"conv_token_edit_scan_kernel<(\d+), (\d)>", r["name"]).groups())
        assert r["Occupancy"] >= OCCUPANCY_FLOOR[mode][lg - 1], r
