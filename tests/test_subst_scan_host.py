"""The single-substitution scan without a GPU: the dense reference of tests/dense_subst_scan.py catches every planted mistake through
the comparison the GPU test uses (and passes it unplanted), and its a-priori cap is at most 1e-2 of the largest output of every case
the GPU test runs; the seventh public header, include/xgpr_hip_subst_scan.h, held to what tests/test_cluster_host.py holds the
sixth; the launcher's argument validation through the C ABI (nothing reaches a HIP call: device pointers are dummy integers); the
shape predicate on the host; and the compiler's resource report for the new kernels."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest

import dense_subst_scan as dss
from test_cabi import _build_module

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "xgpr_hip_subst_scan.h")
NAMES = ["xgpr_conv_token_subst_scan_f32", "xgpr_conv_token_subst_scan_ok"]


def _ref(name, mistake=None):
    c, cw, scaling, icpt = dss.case(name)
    return c, dss.subst_scan(c["tokens"], c["table"], c["seqlen"], c["w"], c["radem"], c["chi"], cw, scaling, icpt, mistake=mistake), \
        dss.cap_subst_scan(c["table"], c["seqlen"], c["w"], c["chi"], cw, scaling, icpt)


# ------------------------------------------------------------------------------------------------ 1. the plants
PLANT_CASE = "dup_rows"             # conv_width 4, V = 5 != C = 6, scaling 1, intercept on, lengths L, conv_width and between


def test_the_unplanted_reference_passes_its_own_comparison():
    c, ref, cap = _ref(PLANT_CASE)
    assert dss.check(ref.astype(np.float64), ref, cap) <= cap
    n, L = c["tokens"].shape
    for i in range(n):
        s = int(c["seqlen"][i])
        assert (ref[i, s:] == 0).all()
        own = np.abs(ref[i, np.arange(s), c["tokens"][i, :s]])                 # the own token: zero up to the reference's own rounding
        assert float(own.max()) <= 1e-15 * float(np.abs(ref).max())
    assert (ref[:, :, 1] == ref[:, :, 3]).all()                               # the duplicated table row


@pytest.mark.parametrize("mistake", dss.MISTAKES)
def test_a_planted_mistake_is_caught(mistake):
    _, ref, cap = _ref(PLANT_CASE)
    _, bad, _ = _ref(PLANT_CASE, mistake)
    with pytest.raises(AssertionError):
        dss.check(bad.astype(np.float64), ref, cap)
    print(mistake, float(np.abs(bad - ref).max()), cap)


def test_every_mistake_has_a_test():
    assert set(dss.MISTAKES) == {"offset", "first_window", "norm_by_L", "keep_w0", "no_wild", "table_transposed"}


@pytest.mark.parametrize("name", [c[0] for c in dss.CASES if c[0] != "vocab1"])
def test_the_cap_is_two_orders_below_the_outputs(name):
    """A condition on the case, not a measurement of the operator: the reference alone."""
    _, ref, cap = _ref(name)
    big = float(np.abs(ref).max())
    print(name, cap, big, cap / big)
    assert 0 < cap <= 1e-2 * big


def test_a_table_of_one_row_has_nothing_to_substitute():
    _, ref, cap = _ref("vocab1")
    assert ref.shape[2] == 1 and (ref == 0).all() and cap > 0


# ------------------------------------------------------------------------------------------------ 2. the seventh header
def _declared():
    hdr = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(xgpr_[a-z0-9_]+)\s*\(", hdr)))                # the expression of tests/test_cabi.py


def test_the_header_declares_its_two_entry_points_and_nothing_of_the_other_headers():
    import test_cabi
    import test_cluster_host
    import test_input_grad_host
    import test_pool_header_host
    import test_pool_input_grad_host
    import test_seq_input_grad_host
    assert _declared() == NAMES
    assert not set(_declared()) & (set(test_cabi._declared()) | set(test_pool_header_host._declared())
                                   | set(test_input_grad_host._declared()) | set(test_seq_input_grad_host._declared())
                                   | set(test_pool_input_grad_host._declared()) | set(test_cluster_host._declared()))


def test_library_exports_every_declared_name():
    bm = _build_module()
    bm.build_extension()
    lib = ctypes.CDLL(bm.LIB)
    for n in _declared():
        assert hasattr(lib, n), f"{n} declared in include/xgpr_hip_subst_scan.h but not exported"


def test_ctypes_table_matches_the_header():
    from xgpr_amd import _lib
    assert set(_lib.SUBST_SCAN_SIGNATURES) == set(_declared())
    assert not set(_lib.SUBST_SCAN_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.SIZE_FUNCS) | set(_lib.STRING_FUNCS)
                                                  | set(_lib.POOL_SIGNATURES) | set(_lib.INPUT_GRAD_SIGNATURES)
                                                  | set(_lib.SEQ_INPUT_GRAD_SIGNATURES) | set(_lib.POOL_INPUT_GRAD_SIGNATURES)
                                                  | set(_lib.CLUSTER_SIGNATURES))
    lib = _lib.load()
    for name, args in _lib.SUBST_SCAN_SIGNATURES.items():                            # load() applied the table
        fn = getattr(lib, name)
        assert fn.argtypes == args
        assert fn.restype is ctypes.c_int, name
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, args in _lib.SUBST_SCAN_SIGNATURES.items():                            # the tables' lengths are the parameter counts
        decl = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert len(decl.group(2).split(",")) == len(args), name
        assert decl.group(1) == "int", name


def test_every_writer_has_a_memory_contract_row():
    import test_gpu_subst_scan_memory_contract as table
    writers = {n for n in _declared() if n.endswith("_f32")}
    assert writers == {"xgpr_conv_token_subst_scan_f32"}
    assert table.covered_entry_points() == writers


def test_source_id_covers_the_header(tmp_path, monkeypatch):
    bm = _build_module()
    assert os.path.samefile(bm.SUBST_SCAN_HDR, HEADER) and bm.SUBST_SCAN_HDR in bm.sources()
    names = [os.path.basename(p) for p in bm.sources()]
    assert "edit_scan.inc" in names and "subst_scan.inc" not in names and "indel_scan.inc" not in names
    before = bm.source_id()
    copy = tmp_path / "xgpr_hip_subst_scan.h"
    shutil.copyfile(HEADER, copy)
    monkeypatch.setattr(bm, "SUBST_SCAN_HDR", str(copy))
    assert bm.source_id() == before                                                  # name and contents, not the path
    with open(copy, "a") as f:
        f.write("/* changed */\n")
    assert bm.source_id() != before


# ------------------------------------------------------------------------------------------------ 3. launcher validation
A = 0x100000                     # a dummy 4096-byte-aligned address, never dereferenced on these paths
BIG = 1 << 40
ARRAY_DIMS, CONV_WIDTH, RFFS_FREQS, SEQLEN, UNSUPPORTED, WORKSPACE = "ARRAY_DIMS", "CONV_WIDTH", "RFFS_FREQS", "SEQLEN_RANGE", \
    "UNSUPPORTED", "WORKSPACE"


def _codes():
    """The error codes by name, from include/xgpr_hip.h."""
    hdr = open(os.path.join(ROOT, "include", "xgpr_hip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"XGPR_ERR_([A-Z_]+)\s*=?\s*\(?(-\d+)\)?", hdr)}


def scan(tokens=A, table=A, w=A, out=A, radem=A, chi=A, lens=(6, 3, 4), seqlen_dev=A, n=3, L=6, vocab=5, C=4, F=40, R=64, cw=3,
         scaling=1, icpt=1, ws=A, wb=BIG):
    from xgpr_amd import _lib
    host = np.asarray(lens, dtype=np.int32) if lens is not None else None
    hp = ctypes.c_void_p(host.ctypes.data) if host is not None else None
    rc = _lib.load().xgpr_conv_token_subst_scan_f32(tokens, table, w, out, radem, chi, hp, seqlen_dev, n, L, vocab, C, F, R, cw, scaling,
                                                    icpt, ws, wb, None)
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
    "NULL out": (dict(out=None), WORKSPACE),
    "NULL radem": (dict(radem=None), WORKSPACE),
    "NULL chi": (dict(chi=None), WORKSPACE),
    "NULL device lengths": (dict(seqlen_dev=None), WORKSPACE),
    # two failing checks at once: the first in the documented order is the one reported
    "n < 0 and conv_width 0": (dict(n=-1, cw=0), ARRAY_DIMS),
    "conv_width 0 and no frequencies": (dict(cw=0, F=0), CONV_WIDTH),
    "no frequencies and a bad length": (dict(F=0, lens=(6, 2, 4)), RFFS_FREQS),
    "a bad length and vocab 257": (dict(lens=(6, 2, 4), vocab=257), SEQLEN),
    "vocab 257 and no workspace": (dict(vocab=257, ws=None), ARRAY_DIMS),
    "an unsupported table and no workspace": (dict(vocab=256, C=19, ws=None), UNSUPPORTED),
    "short workspace and NULL out": (dict(wb=8, out=None), WORKSPACE),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_validation_outcome(name):
    kw, code = REFUSALS[name]
    rc, err = scan(**kw)
    assert rc == _codes()[code] and rc < 0, (rc, err)
    assert err
    if name in ("no workspace", "short workspace", "short workspace and NULL out"):
        assert err == "workspace too small (see xgpr_rbf_workspace_bytes)"
    if name.startswith("NULL"):
        assert err == "NULL array pointer"


def test_the_position_count_of_one_launch():
    from xgpr_amd import _lib
    n = (1 << 24) // 6 + 1
    lens = np.full(n, 6, dtype=np.int32)
    rc = _lib.load().xgpr_conv_token_subst_scan_f32(A, A, A, A, A, A, ctypes.c_void_p(lens.ctypes.data), A, n, 6, 5, 4, 40, 64, 3, 1, 1, A,
                                                    BIG, None)
    assert rc == _codes()[UNSUPPORTED] and "n * L" in _lib.last_error()


def test_no_sequences():
    assert scan(n=0, lens=None, tokens=None, table=None, w=None, out=None, radem=None, chi=None, seqlen_dev=None, ws=None, wb=0)[0] == 0
    assert scan(n=0, lens=None, vocab=257)[0] == _codes()[ARRAY_DIMS]                 # ... but the shape is still checked
    assert scan(n=0, lens=None, vocab=256, C=19)[0] == _codes()[UNSUPPORTED]


def test_the_advertised_workspace_is_the_bound_the_launcher_checks():
    from xgpr_amd import _lib
    need = int(_lib.load().xgpr_rbf_workspace_bytes(64))
    assert need > 0 and scan(wb=need - 1)[0] == _codes()[WORKSPACE]


def test_ok_predicate():
    from xgpr_amd import _lib
    lib = _lib.load()
    ok = lambda width, vocab, C, F: int(lib.xgpr_conv_token_subst_scan_ok(width, vocab, C, F))
    assert [ok(1, 1, 1, 1), ok(12, 6, 4, 8), ok(189, 21, 21, 8192), ok(1008, 5, 21, 1030), ok(1024, 4, 128, 1), ok(54, 256, 18, 130)] == [1] * 6
    assert [ok(1025, 5, 21, 8), ok(2048, 4, 64, 8), ok(57, 256, 19, 8), ok(12, 0, 4, 8), ok(12, 257, 4, 8), ok(0, 5, 4, 8),
            ok(12, 6, 4, 0), ok(12, 6, 0, 8)] == [0] * 8
    for width, vocab, C in ((12, 6, 4), (1008, 5, 21), (1025, 5, 21), (57, 256, 19)):   # the token gradient's predicate, and a frequency
        assert ok(width, vocab, C, 8) == int(lib.xgpr_conv_token_input_grad_ok(width, vocab, C))


def test_python_wrappers():
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    assert ext.conv_token_subst_scan_ok(189, 21, 21, 8192) == 1 and ext.conv_token_subst_scan_ok(2048, 4, 64, 8) == 0
    assert callable(ext.hipConvTokenSubstScan)
    from xgpr_amd.kernels import ConvSORFKernel
    from xgpr_amd.models import xGPRegression
    assert callable(ConvSORFKernel.substitution_scan) and callable(ConvSORFKernel.substitution_scan_composed)
    assert callable(xGPRegression.predict_substitutions)


# ------------------------------------------------------------------------------------------------ 4. the compiler's report
def test_the_new_kernels_use_no_scratch_and_spill_nothing():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    rows = [r for r in resource_usage.collect() if re.fullmatch(r"conv_token_edit_scan_kernel<\d+, 3>", r["name"])]      # mode 3 = EDIT_SUBST
    assert sorted(r["name"] for r in rows) == sorted(f"conv_token_edit_scan_kernel<{lg}, 3>" for lg in range(1, 11))
    for r in rows:
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, r
