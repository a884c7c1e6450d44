"""The single-edit projection without a GPU: the long-double reference of tests/dense_edit_proj.py -- its contract form against the
direct form, every planted mistake far beyond the a-priori cap, and the cap at most 1e-2 of every column's signal on every case
the GPU test runs (a condition on the cases: the reference alone); the thirteenth public header, include/xgpr_hip/edit_proj.h, held
to what tests/test_pool_edits_host.py holds the twelfth; the launchers' argument validation through the C ABI in the documented
order (nothing reaches a HIP call: device pointers are dummy integers); the predicate and the workspace size on the host; and the
compiler's resource table for the new kernels."""
import ctypes
import glob
import inspect
import os
import re
import shutil
import sys

import numpy as np
import pytest

import dense_edit_proj as dep
import dense_indel_scan as dis
import dense_indel_var_scan as div
import dense_subst_var_scan as dv
from dense_reference import LD
from test_cabi import _build_module
from test_subst_var_scan_host import _codes

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "xgpr_hip", "edit_proj.h")
NAMES = ["xgpr_conv_token_edit_proj_ok", "xgpr_conv_token_edit_proj_workspace_bytes", "xgpr_conv_token_indel_proj_f32",
         "xgpr_conv_token_subst_proj_f32"]
CASE_NAMES = [c[0] for c in dv.CASES]


def _zeros(k, gaps=False):
    c = k["c"]
    return dis.zero_mask(c["seqlen"], c["tokens"].shape[1], gaps=gaps)


def _sets(k):
    """(reference, base b, cap, dead slots) of the row sets a case dict holds."""
    if "ref" in k:
        return [("sub", k["ref"], k["b"], k["cap"], _zeros(k))]
    return [("del", k["ref_del"], k["b_del"], k["cap_del"], _zeros(k)), ("ins", k["ref_ins"], k["b_ins"], k["cap_ins"], _zeros(k, gaps=True))]


# ------------------------------------------------------------------------------------------------ 1. the reference and its cap
@pytest.mark.parametrize("name", ["dup_rows", "w128_c21_cw6", "w512_c16_cw20", "n65", "graph_cw1", "vocab1"])
def test_the_contract_form_is_the_direct_form(name):
    k = dep.subst_case(name)
    direct, _ = dep.subst_proj(k["c"], k["pm"], k["cw"], k["scaling"], k["icpt"], direct=True, z=k["z"])
    tol = 64 * k["nvar"] * float(np.finfo(LD).eps) * float(np.abs(k["ref"]).max())
    assert float(np.abs(direct - k["ref"]).max()) <= tol
    k = dep.indel_case(name)
    dd, di, _, _ = dep.indel_proj(k["c"], k["pm"], k["cw"], k["scaling"], k["icpt"], direct=True, z=k["ops"]["z"])
    tol = 64 * k["nvar"] * float(np.finfo(LD).eps) * float(np.abs(k["ref_ins"]).max())
    nan = np.isnan(np.asarray(k["ref_del"], dtype=np.float64))
    assert np.array_equal(nan, np.isnan(np.asarray(dd, dtype=np.float64)))
    assert float(np.abs(di - k["ref_ins"]).max()) <= tol and (nan.all() or float(np.abs(dd - k["ref_del"])[~nan].max()) <= tol)


def test_the_reference_has_the_contract_s_structure():
    k = dep.subst_case("dup_rows")
    c = k["c"]
    n, L = c["tokens"].shape
    assert (k["ref"][_zeros(k)] == 0).all()
    tol = 64 * k["nvar"] * float(np.finfo(LD).eps) * float(np.abs(k["ref"]).max())
    for i in range(n):                                       # the own token: b[i] itself (the reference re-adds the slot: to rounding)
        for l in range(int(c["seqlen"][i])):
            assert float(np.abs(k["ref"][i, l, c["tokens"][i, l]] - k["b"][i]).max()) <= tol
    assert (k["ref"][:, :, 1] == k["ref"][:, :, 3]).all()    # the duplicated table row
    # pm pm^T = vm: the rows' squared norms are the variance scan's quadratic forms
    quad = (k["ref"] * k["ref"]).sum(axis=-1)
    assert float(np.abs(quad - dv.case("dup_rows")["ref"]).max()) <= 1e-12 * float(np.abs(quad).max())
    k = dep.indel_case("dup_rows")
    nan = np.isnan(np.asarray(k["ref_del"], dtype=np.float64))
    want = (c["seqlen"][:, None] == k["cw"]) & (np.arange(L)[None, :] < c["seqlen"][:, None])
    assert np.array_equal(nan, np.broadcast_to(want[:, :, None], nan.shape)) and nan.any()
    assert (k["ref_del"][_zeros(k)] == 0).all() and (k["ref_ins"][_zeros(k, gaps=True)] == 0).all()
    for which, q in (("del", "ref_del"), ("ins", "ref_ins")):
        quad = (k["ref_" + which] * k["ref_" + which]).sum(axis=-1)
        ref = div.case("dup_rows")[q]
        ok = ~np.isnan(np.asarray(ref, dtype=np.float64))
        assert float(np.abs(quad - ref)[ok].max()) <= 1e-12 * float(np.abs(ref[ok]).max())
    for _, ref, _, cap, zeros in _sets(k) + _sets(dep.subst_case("dup_rows")):
        assert dep.check(ref.astype(np.float64), ref, cap, zeros)[1] <= 1.0          # passes its own comparison


PLANT_CASES = ("dup_rows", "w16_c4_cw3", "n65", "n1")       # scaling 1 / 0 / 2 under the intercept, 0 without


@pytest.mark.parametrize("mistake", sorted(set(dep.SUBST_MISTAKES) | set(dep.INDEL_MISTAKES)))
def test_a_planted_mistake_exceeds_the_cap_a_hundredfold(mistake):
    worst = 0.0
    for name in PLANT_CASES:
        got = []
        if mistake in dep.SUBST_MISTAKES:
            k = dep.subst_case(name)
            got += list(zip(_sets(k), [dep.subst_proj(k["c"], k["pm"], k["cw"], k["scaling"], k["icpt"], mistake=mistake, z=k["z"])[0]]))
        k = dep.indel_case(name)
        got += list(zip(_sets(k), dep.indel_proj(k["c"], k["pm"], k["cw"], k["scaling"], k["icpt"], mistake=mistake, z=k["ops"]["z"])[:2]))
        for (which, ref, _, cap, zeros), bad in got:
            capb = np.asarray(cap).reshape((ref.shape[0],) + (1,) * (ref.ndim - 2) + (ref.shape[-1],))
            live = ~np.isnan(np.asarray(ref, dtype=np.float64)) & ~np.broadcast_to(zeros.reshape(zeros.shape + (1,) * (ref.ndim - 2)), ref.shape)
            ratio = float((np.abs(bad - ref) / np.maximum(np.broadcast_to(capb, ref.shape), 1e-300))[live].max())
            print(f"edit proj {mistake} / {name} / {which}: {ratio:.3g} x the cap")
            if ratio > 1:
                with pytest.raises(AssertionError):
                    dep.check(np.asarray(bad, dtype=np.float64), ref, cap, zeros)
            worst = max(worst, ratio)
    assert worst >= 100, (mistake, worst)


def test_every_mistake_the_issue_names_is_planted():
    assert set(dep.SUBST_MISTAKES) == {"pm_transposed", "r_dropped", "keep_col0"}
    assert set(dep.INDEL_MISTAKES) == set(dep.SUBST_MISTAKES) | {"no_rescale", "old_norm"}


def _worst_ratio(ref, b, cap, zeros):
    """max over sequences and columns of cap[i, k] / max |out[i, ..., k] - b[i, k]| over the sequence's live rows."""
    n, K = ref.shape[0], ref.shape[-1]
    sig = np.abs(np.asarray(ref - np.asarray(b).reshape((n,) + (1,) * (ref.ndim - 2) + (K,)), dtype=np.float64))
    sig[np.broadcast_to(zeros.reshape(zeros.shape + (1,) * (ref.ndim - 2)), ref.shape)] = 0
    sig = np.nan_to_num(sig, nan=0.0).reshape(n, -1, K).max(axis=1)
    has = np.asarray(cap).max(axis=1) > 0                    # (a sequence of conv_width tokens has no deletion)
    return float((np.asarray(cap)[has] / np.maximum(sig[has], 1e-300)).max()), float(sig.max())


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_cap_is_two_orders_below_every_column_s_signal(name):
    """A condition on the cases, not a measurement of the operator: pm = chol(the case's own vm), every sequence, every column."""
    for k in (dep.subst_case(name), dep.indel_case(name)):
        for which, ref, b, cap, zeros in _sets(k):
            ratio, sig = _worst_ratio(ref, b, cap, zeros)
            print(f"edit proj cap {name} {which} nvar {k['nvar']}: cap / signal {ratio:.3g}, largest signal {sig:.3g}")
            if name == "vocab1" and which == "sub":
                assert sig == 0                              # one table row: every substitution is the own token
                continue
            assert 0 < ratio <= 1e-2


# ------------------------------------------------------------------------------------------------ 2. the thirteenth header
def _strip(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _declared(path=HEADER):
    return sorted(set(re.findall(r"\b(xgpr_[a-z0-9_]+)\s*\(", _strip(path))))            # the expression of tests/test_cabi.py


def test_the_header_declares_its_four_entry_points_and_nothing_of_the_other_headers():
    assert _declared() == NAMES
    others = sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))) + [os.path.join(ROOT, "include", "xgpr_hip", "pool_edits.h")]
    assert len(others) >= 12 and HEADER not in others
    for h in others:
        assert not set(_declared()) & set(_declared(h)), h
    assert '#include "../xgpr_hip.h"' in open(HEADER).read()


def test_library_exports_every_declared_name():
    bm = _build_module()
    bm.build_extension()
    lib = ctypes.CDLL(bm.LIB)
    for n in _declared():
        assert hasattr(lib, n), f"{n} declared in include/xgpr_hip/edit_proj.h but not exported"


def test_ctypes_table_matches_the_header():
    from xgpr_amd import _lib
    assert set(_lib.EDIT_PROJ_ABI) == set(_declared())
    others = [getattr(_lib, a) for a in dir(_lib) if a.endswith("SIGNATURES")] + [_lib.SIZE_FUNCS, _lib.POOL_EDITS_ABI]
    assert len(others) >= 13
    for table in others:
        assert not set(_lib.EDIT_PROJ_ABI) & set(table)
    assert not set(_lib.EDIT_PROJ_ABI) & set(_lib.STRING_FUNCS)
    lib = _lib.load()
    for name, args in _lib.EDIT_PROJ_ABI.items():                                    # load() applied the table
        fn = getattr(lib, name)
        assert fn.argtypes == args
        assert fn.restype is (ctypes.c_size_t if name.endswith("_workspace_bytes") else ctypes.c_int)
    hdr = _strip(HEADER)
    for name, args in _lib.EDIT_PROJ_ABI.items():                                    # the tables' lengths are the parameter counts
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert len(params.split(",")) == len(args), name


def test_every_writer_has_a_memory_contract_row():
    import test_gpu_edit_proj_memory_contract as table
    writers = {n for n in _declared() if n.endswith("_f32")}
    assert writers == {"xgpr_conv_token_subst_proj_f32", "xgpr_conv_token_indel_proj_f32"}
    assert table.covered_entry_points() == writers


def test_source_id_covers_the_header_and_the_kernels(tmp_path, monkeypatch):
    bm = _build_module()
    assert os.path.samefile(bm.EDIT_PROJ_HDR, HEADER) and bm.EDIT_PROJ_HDR in bm.sources()
    assert "edit_proj.inc" in [os.path.basename(p) for p in bm.sources()]
    before = bm.source_id()
    copy = tmp_path / "edit_proj.h"
    shutil.copyfile(HEADER, copy)
    monkeypatch.setattr(bm, "EDIT_PROJ_HDR", str(copy))
    assert bm.source_id() == before                                                  # name and contents, not the path
    with open(copy, "a") as f:
        f.write("/* changed */\n")
    assert bm.source_id() != before


def test_the_part_is_included_behind_the_variance_scans():
    src = open(os.path.join(ROOT, "xgpr_amd", "csrc", "xgpr_hip.hip")).read()
    assert src.index('#include "var_scan.inc"') < src.index('#include "edit_proj.inc"') < src.index('#include "pool_input_grad.inc"')


# ------------------------------------------------------------------------------------------------ 3. launcher validation
A = 0x100000                     # a dummy 4096-byte-aligned address, never dereferenced on these paths
BIG = 1 << 40
ARRAY_DIMS, ARRAY_SIZES, CONV_WIDTH, RFFS_FREQS, SEQLEN, UNSUPPORTED, WORKSPACE = "ARRAY_DIMS", "ARRAY_SIZES", "CONV_WIDTH", "RFFS_FREQS", \
    "SEQLEN_RANGE", "UNSUPPORTED", "WORKSPACE"


def proj(indel=False, tokens=A, table=A, pm=A, stride=None, b=A, out=A, b_ins=A, out_ins=A, radem=A, chi=A, lens=(6, 3, 4), seqlen_dev=A,
         n=3, L=6, vocab=5, C=4, F=40, R=64, nvar=16, K=5, cw=3, scaling=1, icpt=1, slab=0, ws=A, wb=BIG):
    """``b`` / ``out``: the substitutions' arrays, or the deletion group of the indel entry point (``b_ins`` / ``out_ins``: its
    insertion group)."""
    from xgpr_amd import _lib
    lib = _lib.load()
    host = np.asarray(lens, dtype=np.int32) if lens is not None else None
    hp = ctypes.c_void_p(host.ctypes.data) if host is not None else None
    stride = K if stride is None else stride
    tail = (radem, chi, hp, seqlen_dev, n, L, vocab, C, F, R, nvar, K, cw, scaling, icpt, slab, ws, wb, None)
    if indel:
        rc = lib.xgpr_conv_token_indel_proj_f32(tokens, table, pm, stride, b, b_ins, out, out_ins, *tail)
    else:
        rc = lib.xgpr_conv_token_subst_proj_f32(tokens, table, pm, stride, b, out, *tail)
    return int(rc), _lib.last_error()


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
    "K 0": (dict(K=0), ARRAY_DIMS),
    "K negative": (dict(K=-3), ARRAY_DIMS),
    "a short row stride of pm": (dict(stride=4), ARRAY_SIZES),
    "slab_rows 8": (dict(slab=8), ARRAY_DIMS),
    "slab_rows negative": (dict(slab=-16), ARRAY_DIMS),
    "no host lengths": (dict(lens=None), SEQLEN),
    "a length below conv_width": (dict(lens=(6, 2, 4)), SEQLEN),
    "a length above L": (dict(lens=(6, 3, 7)), SEQLEN),
    "vocab 0": (dict(vocab=0), ARRAY_DIMS),
    "vocab 257": (dict(vocab=257), ARRAY_DIMS),
    "a window of 2048 elements": (dict(L=40, cw=32, C=64, lens=(40, 32, 33), R=2048), UNSUPPORTED),
    "a table of more than 4608 floats": (dict(vocab=256, C=19, R=64), UNSUPPORTED),
    "nvar above one tile": (dict(F=2048, R=2048, nvar=2050), UNSUPPORTED),
    "K above 2048": (dict(K=2049), UNSUPPORTED),
    "no workspace": (dict(ws=None), WORKSPACE),
    "short workspace": (dict(wb=8), WORKSPACE),
    "misaligned workspace": (dict(ws=A + 4), WORKSPACE),
    "NULL tokens": (dict(tokens=None), WORKSPACE),
    "NULL table": (dict(table=None), WORKSPACE),
    "NULL pm": (dict(pm=None), WORKSPACE),
    "NULL radem": (dict(radem=None), WORKSPACE),
    "NULL chi": (dict(chi=None), WORKSPACE),
    "NULL device lengths": (dict(seqlen_dev=None), WORKSPACE),
    # two failing checks at once: the first in the documented order is the one reported
    "n < 0 and conv_width 0": (dict(n=-1, cw=0), ARRAY_DIMS),
    "conv_width 0 and nvar odd": (dict(cw=0, nvar=15), CONV_WIDTH),
    "nvar odd and K 0": (dict(nvar=15, K=0), ARRAY_DIMS),
    "K 0 and a short stride": (dict(K=0, stride=-1), ARRAY_DIMS),
    "a short stride and slab_rows 8": (dict(stride=4, slab=8), ARRAY_SIZES),
    "slab_rows 8 and a bad length": (dict(slab=8, lens=(6, 2, 4)), ARRAY_DIMS),
    "a bad length and vocab 257": (dict(lens=(6, 2, 4), vocab=257), SEQLEN),
    "vocab 257 and K above 2048": (dict(vocab=257, K=2049), ARRAY_DIMS),
    "K above 2048 and no workspace": (dict(K=2049, ws=None), UNSUPPORTED),
}
SUBST_ONLY = {"NULL b": (dict(b=None), WORKSPACE), "NULL out": (dict(out=None), WORKSPACE)}
NO_DEL, NO_INS = dict(b=None, out=None), dict(b_ins=None, out_ins=None)
INDEL_ONLY = {
    "NULL b_del alone": (dict(b=None), WORKSPACE),
    "NULL out_del alone": (dict(out=None), WORKSPACE),
    "NULL b_ins alone": (dict(b_ins=None), WORKSPACE),
    "NULL out_ins alone": (dict(out_ins=None), WORKSPACE),
    "NULL out_ins without the deletions": (dict(NO_DEL, out_ins=None), WORKSPACE),
    "both groups NULL": (dict(NO_DEL, **NO_INS), WORKSPACE),
    "short workspace and both groups NULL": (dict(NO_DEL, wb=8, **NO_INS), WORKSPACE),
}


def _refused(indel, name, kw, code):
    rc, err = proj(indel=indel, **kw)
    assert rc == _codes()[code] and rc < 0, (rc, err)
    assert err
    if "workspace" in name and "NULL" not in name and code == WORKSPACE:
        assert "xgpr_conv_token_edit_proj_workspace_bytes" in err
    if code == UNSUPPORTED:
        assert "xgpr_conv_token_edit_proj_ok" in err
    if name.startswith("NULL"):
        assert err == "NULL array pointer"


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_validation_outcome_of_both_entry_points(name):
    for indel in (False, True):
        _refused(indel, name, *REFUSALS[name])


@pytest.mark.parametrize("name", sorted(SUBST_ONLY))
def test_validation_outcome_of_the_substitutions(name):
    _refused(False, name, *SUBST_ONLY[name])


@pytest.mark.parametrize("name", sorted(INDEL_ONLY))
def test_validation_outcome_of_the_indels(name):
    _refused(True, name, *INDEL_ONLY[name])
    if name == "both groups NULL":
        assert "both NULL" in proj(indel=True, **INDEL_ONLY[name][0])[1]


def test_the_documented_order_is_the_tenth_header_s_with_the_two_checks_of_pm():
    doc = open(HEADER).read()
    order = re.findall(r"XGPR_ERR_([A-Z_]+)", doc[doc.index("Checks, before anything is launched"):])
    assert order == [ARRAY_DIMS, CONV_WIDTH, RFFS_FREQS, ARRAY_DIMS, ARRAY_DIMS, ARRAY_SIZES, ARRAY_DIMS, SEQLEN, ARRAY_DIMS, UNSUPPORTED,
                     WORKSPACE, UNSUPPORTED]
    tenth = open(os.path.join(ROOT, "include", "xgpr_hip_indel_var_scan.h")).read()
    theirs = re.findall(r"XGPR_ERR_([A-Z_]+)", tenth[tenth.index("Checks, before anything is launched"):])
    assert order[:4] + order[6:] == theirs[:4] + theirs[5:] and theirs[4] == ARRAY_SIZES        # (theirs[4]: vm_stride; no vm here)


def test_one_group_alone_passes_validation_and_no_sequences_launch_nothing():
    assert proj(indel=True, n=0, lens=None, **NO_DEL)[0] == 0 and proj(indel=True, n=0, lens=None, **NO_INS)[0] == 0
    none = dict(n=0, lens=None, tokens=None, table=None, pm=None, radem=None, chi=None, seqlen_dev=None, ws=None, wb=0)
    assert proj(**none, **NO_DEL)[0] == 0 and proj(indel=True, **none, **NO_DEL, **NO_INS)[0] == 0
    for indel in (False, True):                                                       # ... but the shape is still checked
        assert proj(indel=indel, n=0, lens=None, vocab=257)[0] == _codes()[ARRAY_DIMS]
        assert proj(indel=indel, n=0, lens=None, K=0)[0] == _codes()[ARRAY_DIMS]
        assert proj(indel=indel, n=0, lens=None, K=2049)[0] == _codes()[UNSUPPORTED]


def test_the_position_count_of_one_launch():
    from xgpr_amd import _lib
    for indel, n, words in ((False, (1 << 24) // 6 + 1, "n * L"), (True, (1 << 24) // 7 + 1, "n * (L + 1)")):
        rc, err = proj(indel=indel, n=n, lens=np.full(n, 6, dtype=np.int32))
        assert rc == _codes()[UNSUPPORTED] and words in err
    assert proj(indel=True, n=(1 << 24) // 6 + 1, lens=np.full((1 << 24) // 6 + 1, 6, dtype=np.int32))[0] == _codes()[UNSUPPORTED]


def test_workspace_bytes_are_the_variance_scan_s():
    from xgpr_amd import _lib
    lib = _lib.load()
    wsb = lambda R, nvar, slab: int(lib.xgpr_conv_token_edit_proj_workspace_bytes(R, nvar, slab))
    masks = int(lib.xgpr_rbf_workspace_bytes(64))
    assert wsb(64, 16, 16) == masks + 16 * 16 * 8 and wsb(64, 16, 48) == masks + 48 * 16 * 8
    assert [wsb(64, 16, 8), wsb(64, 16, 24), wsb(64, 16, -16), wsb(64, 15, 16), wsb(64, 0, 16), wsb(0, 16, 16)] == [0] * 6
    for nvar in (2, 16, 130, 512, 2048):
        for slab in (0, 16, 4096):
            assert wsb(64, nvar, slab) == int(lib.xgpr_conv_token_subst_var_scan_workspace_bytes(64, nvar, slab)) \
                == int(lib.xgpr_conv_token_indel_var_scan_workspace_bytes(64, nvar, slab)) > 0
    need = wsb(64, 16, 32)                                                            # the advertised size is the bound the launchers check
    for indel in (False, True):
        assert proj(indel=indel, slab=32, wb=need - 1)[0] == _codes()[WORKSPACE]


def test_ok_predicate():
    from xgpr_amd import _lib
    lib = _lib.load()
    ok = lambda *a: int(lib.xgpr_conv_token_edit_proj_ok(*a))
    assert [ok(1, 1, 1, 1, 2, 1), ok(12, 6, 4, 8, 16, 16), ok(189, 21, 21, 8192, 512, 2048), ok(189, 21, 21, 8192, 2048, 1),
            ok(54, 256, 18, 130, 260, 65)] == [1] * 5
    assert [ok(12, 6, 4, 8, 16, 0), ok(12, 6, 4, 8, 16, -1), ok(12, 6, 4, 8, 16, 2049), ok(12, 6, 4, 8, 15, 4), ok(189, 21, 21, 8192, 2050, 4),
            ok(1025, 5, 21, 8, 4, 4), ok(57, 256, 19, 8, 4, 4)] == [0] * 7
    for args in ((12, 6, 4, 8, 16), (1008, 5, 21, 1030, 130), (1025, 5, 21, 8, 4), (57, 256, 19, 8, 4), (12, 6, 4, 8, 15)):
        for K in (1, 2048):
            assert ok(*args, K) == int(lib.xgpr_conv_token_subst_var_scan_ok(*args))


def test_python_surface():
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    assert ext.conv_token_edit_proj_ok(189, 21, 21, 8192, 512, 16) == 1 and ext.conv_token_edit_proj_ok(189, 21, 21, 8192, 512, 0) == 0
    assert ext.conv_token_edit_proj_workspace_bytes(64, 16, 16) == ext._LIB.xgpr_rbf_workspace_bytes(64) + 16 * 16 * 8
    sig = inspect.signature(ext.hipConvTokenSubstProj)
    assert list(sig.parameters) == ["tokens", "table", "pm", "b", "out", "radem", "chi", "seqlen", "conv_width", "scaling_type",
                                    "fit_intercept", "slab_rows", "workspace"]
    assert sig.parameters["slab_rows"].default == 0 and sig.parameters["workspace"].default is None
    sig = inspect.signature(ext.hipConvTokenIndelProj)
    assert list(sig.parameters) == ["tokens", "table", "pm", "b_del", "b_ins", "deletions", "insertions", "radem", "chi", "seqlen",
                                    "conv_width", "scaling_type", "fit_intercept", "slab_rows", "workspace"]
    assert sig.parameters["slab_rows"].default == 0 and sig.parameters["workspace"].default is None
    from xgpr_amd.kernels import Conv1dTwoLayerKernel, ConvSORFKernel
    from xgpr_amd.models import xGPRegression
    for nm in ("substitution_projection_scan", "indel_projection_scan", "substitution_projection_scan_composed",
               "indel_projection_scan_composed"):
        assert callable(getattr(ConvSORFKernel, nm))
    assert inspect.signature(Conv1dTwoLayerKernel.edit_scan).parameters["proj"].default is None
    sig = inspect.signature(xGPRegression.sample_single_edits)
    assert (sig.parameters["n_samples"].default, sig.parameters["random_seed"].default, sig.parameters["chunk_size"].default) == (16, 123, 16)
    sig = inspect.signature(xGPRegression.select_single_edit_batch)
    assert (sig.parameters["batch_size"].default, sig.parameters["beta"].default, sig.parameters["maximize"].default) == (8, 2.0, True)
    assert list(inspect.signature(xGPRegression.single_edit_neighbourhoods).parameters) == ["self", "input_x", "sequence_lengths", "token_table"]
    from xgpr_amd.acquisition import SingleEditPosterior
    assert inspect.signature(SingleEditPosterior.select_batch).parameters["beta"].default == 2.0


def test_a_model_without_a_fit_or_without_variance_refuses():
    from xgpr_amd.models import xGPRegression
    m = xGPRegression(num_rffs=64, variance_rffs=16, kernel_choice="Conv1dRBF", device="cuda")
    for fn in (m.single_edit_neighbourhoods, m.sample_single_edits, m.select_single_edit_batch):
        with pytest.raises(RuntimeError, match="not yet been successfully fitted"):
            fn(np.zeros((1, 4), dtype=np.int64), np.array([4]), token_table=np.eye(3, dtype=np.float32))


# ------------------------------------------------------------------------------------------------ 4. the compiler's table
def test_resource_table_lists_the_new_kernels_without_scratch_or_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    rows = [r for r in resource_usage.collect() if r["name"].startswith("var_proj_kernel<")]
    names = sorted(r["name"].replace("(anonymous namespace)::", "") for r in rows)
    assert names == [f"var_proj_kernel<{m}>" for m in ("DelRowMap", "InsRowMap", "SubstRowMap")]
    for r in rows:
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, r
