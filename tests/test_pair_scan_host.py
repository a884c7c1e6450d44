"""The pairwise substitution scan without a GPU: the dense reference of tests/dense_pair_scan.py catches every planted mistake through
the comparison the GPU test uses (and passes it unplanted), and its a-priori cap is at most 1e-2 of the largest output of every
non-degenerate case the GPU test runs; the eleventh public header, include/xgpr_hip_pair_scan.h, held to what
tests/test_subst_scan_host.py holds the seventh; the launcher's argument validation through the C ABI (nothing reaches a HIP call:
device pointers are dummy integers); the shape predicate on the host; and the compiler's resource report for the new kernels."""
import ctypes
import inspect
import os
import re
import shutil
import sys

import numpy as np
import pytest

import dense_pair_scan as dp
from test_cabi import _build_module
from test_subst_scan_host import A, ARRAY_DIMS, BIG, CONV_WIDTH, RFFS_FREQS, SEQLEN, UNSUPPORTED, WORKSPACE, _codes

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "xgpr_hip_pair_scan.h")
NAMES = ["xgpr_conv_token_pair_scan_f32", "xgpr_conv_token_pair_scan_ok"]


# ------------------------------------------------------------------------------------------------ 1. the plants
PLANT_CASE = "dup_rows"             # conv_width 4 (a band of 3), V = 5 != C = 6, scaling 1, intercept on, lengths L, conv_width and between


def test_the_unplanted_reference_passes_its_own_comparison():
    c, cw, _, _, ref, cap = dp.reference(PLANT_CASE)
    assert dp.check(ref.astype(np.float64), ref, cap) <= cap
    n, L = c["tokens"].shape
    assert ref.shape == (n, L, cw - 1, 5, 5)
    big = float(np.abs(ref).max())
    for i in range(n):
        s = int(c["seqlen"][i])
        for l1 in range(L):
            for d in range(1, cw):
                blk = ref[i, l1, d - 1]
                if l1 + d >= s:
                    assert (blk == 0).all()
                    continue
                # either own token: zero up to the reference's own rounding
                assert float(np.abs(blk[c["tokens"][i, l1], :]).max()) <= 1e-15 * big
                assert float(np.abs(blk[:, c["tokens"][i, l1 + d]]).max()) <= 1e-15 * big
    assert float(np.abs(ref[:, :, :, 1, :] - ref[:, :, :, 3, :]).max()) <= 1e-15 * big      # the duplicated table row, on both axes
    assert float(np.abs(ref[:, :, :, :, 1] - ref[:, :, :, :, 3]).max()) <= 1e-15 * big


def test_angle_addition_and_direct_trigonometry_give_the_same_reference():
    for name in (PLANT_CASE, "w16_c4_cw3"):
        _, _, _, _, fast, cap = dp.reference(name)
        slow = dp.reference(name, direct=True)[4]
        assert float(np.abs(fast - slow).max()) <= 1e-9 * cap


@pytest.mark.parametrize("mistake", dp.MISTAKES)
def test_a_planted_mistake_is_caught(mistake):
    _, _, _, _, ref, cap = dp.reference(PLANT_CASE)
    bad = dp.reference(PLANT_CASE, mistake)[4]
    with pytest.raises(AssertionError):
        dp.check(bad.astype(np.float64), ref, cap)
    print(mistake, float(np.abs(bad - ref).max()), cap)


def test_every_mistake_has_a_test():
    assert set(dp.MISTAKES) == {"q2_offset", "first_window", "norm_by_L", "keep_w0", "no_singles", "v1_at_l2", "band_shift"}


@pytest.mark.parametrize("name", [c[0] for c in dp.CASES if c[0] not in dp.DEGENERATE])
def test_the_cap_is_two_orders_below_the_outputs(name):
    """A condition on the case, not a measurement of the operator: the reference alone."""
    _, _, _, _, ref, cap = dp.reference(name)
    big = float(np.abs(ref).max())
    print(name, cap, big, cap / big)
    assert 0 < cap <= 1e-2 * big


def test_the_degenerate_cases():
    ref, cap = dp.reference("vocab1")[4:]
    assert ref.shape[3:] == (1, 1) and ref.size > 0 and (ref == 0).all() and cap > 0
    ref = dp.reference("graph_cw1")[4]
    assert ref.shape == (3, 7, 0, 9, 9)


def test_the_case_list_covers_every_axis():
    import dense_reference as dr
    kws = {nm: kw for nm, kw, _, _ in dp.CASES}
    padded = {dr.padded_width(kw["conv_width"] * kw["C"]) for kw in kws.values()}
    assert {16, 64, 128, 256, 512, 1024} <= padded
    assert {(kw["C"], kw["conv_width"]) for kw in kws.values()} >= {(4, 3), (21, 3), (21, 6), (21, 9), (60, 8), (120, 8), (3, 20), (18, 3)}
    assert {kw["n"] for kw in kws.values()} >= {1, 2, 65} and {kw["conv_width"] for kw in kws.values()} >= {1, 20}
    assert {kw["F"] for kw in kws.values()} >= {8, 1030, 5000} and any(kw.get("extra_reps") for kw in kws.values())
    assert {kw["V"] for kw in kws.values()} >= {1, 256}
    assert {(s, i) for _, _, s, i in dp.CASES} == {(s, i) for s in (0, 1, 2) for i in (True, False)}
    for nm in ("w16_c4_cw3", "w128_c21_cw6"):                     # one window, and the full length
        c, cw, _, _ = dp.case(nm)
        assert (c["seqlen"] - cw + 1 == 1).any() and (c["seqlen"] == c["tokens"].shape[1]).any()
    c, cw, _, _ = dp.case("w16_c4_cw3")
    assert (c["seqlen"] == cw + 1).any()
    assert (c["tokens"][np.arange(c["tokens"].shape[1])[None, :] >= c["seqlen"][:, None]] >= c["table"].shape[0]).all()


# ------------------------------------------------------------------------------------------------ 2. the eleventh header
def _declared():
    hdr = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(xgpr_[a-z0-9_]+)\s*\(", hdr)))                # the expression of tests/test_cabi.py


def test_the_header_declares_its_two_entry_points_and_nothing_of_the_other_headers():
    import test_cabi
    import test_cluster_host
    import test_indel_scan_host
    import test_indel_var_scan_host
    import test_input_grad_host
    import test_pool_header_host
    import test_pool_input_grad_host
    import test_seq_input_grad_host
    import test_subst_scan_host
    import test_subst_var_scan_host
    assert _declared() == NAMES
    others = [test_cabi, test_pool_header_host, test_input_grad_host, test_seq_input_grad_host, test_pool_input_grad_host,
              test_cluster_host, test_subst_scan_host, test_indel_scan_host, test_subst_var_scan_host, test_indel_var_scan_host]
    headers = {f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h")}
    assert len(headers) == len(others) + 1 and "xgpr_hip_pair_scan.h" in headers
    for mod in others:
        assert not set(_declared()) & set(mod._declared()), mod.__name__


def test_library_exports_every_declared_name():
    bm = _build_module()
    bm.build_extension()
    lib = ctypes.CDLL(bm.LIB)
    for n in _declared():
        assert hasattr(lib, n), f"{n} declared in include/xgpr_hip_pair_scan.h but not exported"


def test_ctypes_table_matches_the_header():
    from xgpr_amd import _lib
    assert set(_lib.PAIR_SCAN_SIGNATURES) == set(_declared())
    tables = [getattr(_lib, t) for t in dir(_lib) if t.endswith("SIGNATURES") or t in ("SIZE_FUNCS", "STRING_FUNCS")]
    assert len(tables) == 13                                                        # eleven headers' tables, SIZE_FUNCS, STRING_FUNCS
    for tab in tables:
        if tab is not _lib.PAIR_SCAN_SIGNATURES:
            assert not set(_lib.PAIR_SCAN_SIGNATURES) & set(tab)
    lib = _lib.load()
    for name, args in _lib.PAIR_SCAN_SIGNATURES.items():                             # load() applied the table
        fn = getattr(lib, name)
        assert fn.argtypes == args
        assert fn.restype is ctypes.c_int, name
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, args in _lib.PAIR_SCAN_SIGNATURES.items():                             # the tables' lengths are the parameter counts
        decl = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert len(decl.group(2).split(",")) == len(args), name
        assert decl.group(1) == "int", name
    # the operands are those of the substitution scan
    assert _lib.PAIR_SCAN_SIGNATURES["xgpr_conv_token_pair_scan_f32"] == _lib.SUBST_SCAN_SIGNATURES["xgpr_conv_token_subst_scan_f32"]


def test_every_writer_has_a_memory_contract_row():
    import test_gpu_pair_scan_memory_contract as table
    writers = {n for n in _declared() if n.endswith("_f32")}
    assert writers == {"xgpr_conv_token_pair_scan_f32"}
    assert table.covered_entry_points() == writers


def test_source_id_covers_the_header(tmp_path, monkeypatch):
    bm = _build_module()
    assert os.path.samefile(bm.PAIR_SCAN_HDR, HEADER) and bm.PAIR_SCAN_HDR in bm.sources()
    assert "pair_scan.inc" in [os.path.basename(p) for p in bm.sources()]
    before = bm.source_id()
    copy = tmp_path / "xgpr_hip_pair_scan.h"
    shutil.copyfile(HEADER, copy)
    monkeypatch.setattr(bm, "PAIR_SCAN_HDR", str(copy))
    assert bm.source_id() == before                                                  # name and contents, not the path
    with open(copy, "a") as f:
        f.write("/* changed */\n")
    assert bm.source_id() != before


# ------------------------------------------------------------------------------------------------ 3. launcher validation
def scan(tokens=A, table=A, w=A, out=A, radem=A, chi=A, lens=(6, 3, 4), seqlen_dev=A, n=3, L=6, vocab=5, C=4, F=40, R=64, cw=3,
         scaling=1, icpt=1, ws=A, wb=BIG):
    from xgpr_amd import _lib
    host = np.asarray(lens, dtype=np.int32) if lens is not None else None
    hp = ctypes.c_void_p(host.ctypes.data) if host is not None else None
    rc = _lib.load().xgpr_conv_token_pair_scan_f32(tokens, table, w, out, radem, chi, hp, seqlen_dev, n, L, vocab, C, F, R, cw, scaling,
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
    "a graph kernel's bad length": (dict(cw=1, lens=(6, 0, 4)), SEQLEN),             # conv_width 1 returns only after the shape checks
    "a graph kernel's vocab 257": (dict(cw=1, vocab=257, out=None, ws=None), ARRAY_DIMS),
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
    if code == UNSUPPORTED:
        assert err.startswith("the pair scan serves") and "xgpr_conv_token_pair_scan_ok" in err     # the message names this operator


def _many(n, L=6, vocab=5, cw=3):
    from xgpr_amd import _lib
    lens = np.full(n, L, dtype=np.int32)
    rc = _lib.load().xgpr_conv_token_pair_scan_f32(A, A, A, A, A, A, ctypes.c_void_p(lens.ctypes.data), A, n, L, vocab, 4, 40, 64, cw, 1, 1,
                                                   A, BIG, None)
    return int(rc), _lib.last_error()


def test_the_row_count_of_one_launch():
    """n * L * (conv_width - 1) * vocab < 2^24.  (The largest batch inside the bound would be launched: only the refusals are called.)"""
    per = 6 * 2 * 5
    rc, err = _many((1 << 24) // per + 1)
    assert rc == _codes()[UNSUPPORTED] and "n * L * (conv_width - 1) * vocab" in err
    assert ((1 << 24) // per + 1) * 6 < 1 << 24                                       # ... a batch the substitution scan takes
    rc, err = _many((1 << 24) // (6 * 5 * 255) + 1, vocab=255, cw=6)                  # the band and the vocabulary count
    assert rc == _codes()[UNSUPPORTED] and "n * L * (conv_width - 1) * vocab" in err


def test_no_sequences():
    assert scan(n=0, lens=None, tokens=None, table=None, w=None, out=None, radem=None, chi=None, seqlen_dev=None, ws=None, wb=0)[0] == 0
    assert scan(n=0, lens=None, vocab=257)[0] == _codes()[ARRAY_DIMS]                 # ... but the shape is still checked
    assert scan(n=0, lens=None, vocab=256, C=19)[0] == _codes()[UNSUPPORTED]


def test_a_graph_kernel_has_no_pairs():
    """conv_width == 1: the output has no elements; 0 after the shape checks, nothing launched, out may be NULL."""
    assert scan(cw=1, lens=(6, 1, 4), out=None)[0] == 0
    assert scan(cw=1, lens=(6, 1, 4), tokens=None, table=None, w=None, out=None, radem=None, chi=None, seqlen_dev=None, ws=None, wb=0)[0] == 0
    assert _many((1 << 24) // 6 + 1, cw=1)[0] == 0                                    # (no row, no bound)
    assert scan(cw=1, lens=(6, 1, 4), vocab=256, C=19)[0] == _codes()[UNSUPPORTED]


def test_the_advertised_workspace_is_the_bound_the_launcher_checks():
    from xgpr_amd import _lib
    need = int(_lib.load().xgpr_rbf_workspace_bytes(64))
    assert need > 0 and scan(wb=need - 1)[0] == _codes()[WORKSPACE]


def test_ok_predicate():
    from xgpr_amd import _lib
    lib = _lib.load()
    ok = lambda width, vocab, C, F: int(lib.xgpr_conv_token_pair_scan_ok(width, vocab, C, F))
    assert [ok(1, 1, 1, 1), ok(12, 6, 4, 8), ok(189, 21, 21, 8192), ok(1008, 5, 21, 1030), ok(1024, 4, 128, 1), ok(54, 256, 18, 130)] == [1] * 6
    assert [ok(1025, 5, 21, 8), ok(2048, 4, 64, 8), ok(57, 256, 19, 8), ok(12, 0, 4, 8), ok(12, 257, 4, 8), ok(0, 5, 4, 8),
            ok(12, 6, 4, 0), ok(12, 6, 0, 8)] == [0] * 8
    for args in ((12, 6, 4, 8), (1008, 5, 21, 1), (1025, 5, 21, 8), (57, 256, 19, 8), (12, 6, 4, 0)):   # the substitution scan's predicate
        assert ok(*args) == int(lib.xgpr_conv_token_subst_scan_ok(*args))


def test_python_wrappers():
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    assert ext.conv_token_pair_scan_ok(189, 21, 21, 8192) == 1 and ext.conv_token_pair_scan_ok(2048, 4, 64, 8) == 0
    assert list(inspect.signature(ext.hipConvTokenPairScan).parameters) == list(inspect.signature(ext.hipConvTokenSubstScan).parameters)
    from xgpr_amd.kernels import ConvSORFKernel
    from xgpr_amd.models import xGPRegression
    assert callable(ConvSORFKernel.pair_substitution_scan) and callable(ConvSORFKernel.pair_substitution_scan_composed)
    sig = inspect.signature(xGPRegression.predict_substitution_pairs)
    assert sig.parameters["chunk_size"].default == 4
    doc = xGPRegression.predict_substitution_pairs.__doc__
    assert "mean(double) = predict + sub[i, l1, v1] + sub[i, l2, v2]" in doc and "14.5 MB" in doc
    assert 512 * 8 * 21 * 21 * 8 == 14450688                                          # the size the docstring quotes


# ------------------------------------------------------------------------------------------------ 4. the compiler's report
def test_the_new_kernels_use_no_scratch_and_spill_nothing():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    rows = [r for r in resource_usage.collect() if re.fullmatch(r"pair_scan_grid_kernel<\d+>|pair_scan_diff_kernel", r["name"])]
    assert sorted(r["name"] for r in rows) == sorted([f"pair_scan_grid_kernel<{lg}>" for lg in range(1, 11)] + ["pair_scan_diff_kernel"])
    for r in rows:
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, r
