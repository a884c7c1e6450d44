"""The two-layer kernel's single-edit pool without a GPU: the index algebra of tests/dense_pool_edits.py against brute force over
written-out mutants, with every planted mistake caught; the twelfth public header, include/xgpr_hip/pool_edits.h, held to what
tests/test_pool_input_grad_host.py holds the fifth; the launchers' argument validation through the C ABI (no call reaches a HIP
launch: device pointers are dummy integers); the _ok predicate at its limits; and the compiler's resource table for the new kernels."""
import ctypes
import glob
import os
import re
import shutil
import sys

import numpy as np
import pytest

import dense_pool_edits as dpe
from test_cabi import _build_module

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "xgpr_hip", "pool_edits.h")
NAMES = ["xgpr_conv_token_maxpool_edits_f32", "xgpr_conv_token_maxpool_edits_ok", "xgpr_conv_token_maxpool_tables_f32"]

# ------------------------------------------------------------------------------------------------ 1. index algebra
L, V, F = 14, 5, 7
CASES = [(cw, s) for cw in (1, 3, 9) for s in (cw, cw + 1, L)]


@pytest.mark.parametrize("mode", dpe.MODES)
@pytest.mark.parametrize("cw,s", CASES)
def test_identity_equals_brute_force(cw, s, mode):
    tokens = dpe.make_tokens(L, V, seed=100 * cw + s)
    got, want = dpe.edit_rows(tokens, s, cw, V, F, mode), dpe.brute(tokens, s, cw, V, F, mode)
    assert dpe.same(got, want)
    slots, _ = dpe.geometry(L, V, mode)
    first_gone = s + 1 if mode == "insertions" else s
    assert (want[first_gone:] == 0).all() and slots - first_gone == L - s
    assert bool(np.isnan(want).any()) == (mode == "deletions" and s == cw)          # NaN: the deletions at nk == 1, and only those
    if mode == "substitutions":                                                      # the own token gives the sequence's own row
        own = dpe.pooled(tokens[:s], cw, F)
        assert all((want[l, tokens[l]] == own).all() for l in range(s))


def test_the_window_function_separates():
    """Integer values of both signs, different for different windows: a wrong window changes a maximum somewhere."""
    a, b = dpe.window_values([1, 2, 3], 64), dpe.window_values([1, 2, 4], 64)
    assert (a == np.round(a)).all() and a.min() < 0 < a.max() and (a != b).any()
    assert (dpe.window_values([1, 2, 3], 64) == a).all()


APPLIES = {"jhi_off_by_one": dpe.MODES, "b_off_by_one": dpe.MODES, "ins_removed_at_g0": ("insertions",),
           "ins_removed_at_gs": ("insertions",), "del_nk1": ("deletions",)}


@pytest.mark.parametrize("mistake", dpe.MISTAKES)
def test_every_planted_mistake_is_caught(mistake):
    assert set(APPLIES) == set(dpe.MISTAKES)
    for mode in APPLIES[mistake]:
        caught = 0
        for cw, s in CASES:
            tokens = dpe.make_tokens(L, V, seed=100 * cw + s)
            caught += not dpe.same(dpe.edit_rows(tokens, s, cw, V, F, mode, mistake=mistake), dpe.brute(tokens, s, cw, V, F, mode))
        print(f"pool edits {mistake} / {mode}: caught in {caught} of {len(CASES)} cases")
        assert caught > 0, (mistake, mode)


def test_del_nk1_is_caught_exactly_where_no_window_is_left():
    for cw, s in CASES:
        tokens = dpe.make_tokens(L, V, seed=100 * cw + s)
        wrong = not dpe.same(dpe.edit_rows(tokens, s, cw, V, F, "deletions", mistake="del_nk1"), dpe.brute(tokens, s, cw, V, F, "deletions"))
        assert wrong == (s == cw)


# ------------------------------------------------------------------------------------------------ 2. the twelfth header
def _strip(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _declared(path=HEADER):
    return sorted(set(re.findall(r"\b(xgpr_[a-z0-9_]+)\s*\(", _strip(path))))            # the expression of tests/test_cabi.py


def test_the_header_declares_its_three_entry_points_and_nothing_of_the_other_headers():
    assert _declared() == NAMES
    others = sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert len(others) >= 11 and HEADER not in others
    for h in others:
        assert not set(_declared()) & set(_declared(h)), h
    assert '#include "../xgpr_hip.h"' in open(HEADER).read()


def test_library_exports_every_declared_name():
    bm = _build_module()
    bm.build_extension()
    lib = ctypes.CDLL(bm.LIB)
    for n in _declared():
        assert hasattr(lib, n), f"{n} declared in include/xgpr_hip/pool_edits.h but not exported"


def test_ctypes_table_matches_the_header():
    from xgpr_amd import _lib
    assert set(_lib.POOL_EDITS_ABI) == set(_declared())
    others = [getattr(_lib, a) for a in dir(_lib) if a.endswith("SIGNATURES")] + [_lib.SIZE_FUNCS]
    assert len(others) >= 12
    for table in others:
        assert not set(_lib.POOL_EDITS_ABI) & set(table)
    assert not set(_lib.POOL_EDITS_ABI) & set(_lib.STRING_FUNCS)
    lib = _lib.load()
    for name, args in _lib.POOL_EDITS_ABI.items():                                   # load() applied the table
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype is ctypes.c_int
    hdr = _strip(HEADER)
    for name, args in _lib.POOL_EDITS_ABI.items():                                   # the tables' lengths are the parameter counts
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert len(params.split(",")) == len(args), name


def test_the_header_s_mode_values_are_the_wrappers():
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    hdr = open(HEADER).read()
    for word, name in (("DEL", "deletions"), ("INS", "insertions"), ("SUBST", "substitutions")):
        assert int(re.search(r"#define XGPR_POOL_EDIT_" + word + r"\s+(\d+)", hdr).group(1)) == ext.POOL_EDIT_MODES[name]


def test_every_writer_has_a_memory_contract_row():
    import test_gpu_pool_edits_memory_contract as table
    writers = {n for n in _declared() if n.endswith("_f32")}                         # (_ok: a predicate, no memory)
    assert writers == {"xgpr_conv_token_maxpool_tables_f32", "xgpr_conv_token_maxpool_edits_f32"}
    assert table.covered_entry_points() == writers


def test_source_id_covers_the_header(tmp_path, monkeypatch):
    bm = _build_module()
    assert os.path.samefile(bm.POOL_EDITS_HDR, HEADER) and bm.POOL_EDITS_HDR in bm.sources()
    before = bm.source_id()
    copy = tmp_path / "pool_edits.h"
    shutil.copyfile(HEADER, copy)
    monkeypatch.setattr(bm, "POOL_EDITS_HDR", str(copy))
    assert bm.source_id() == before                                                  # name and contents, not the path
    with open(copy, "a") as f:
        f.write("/* changed */\n")
    assert bm.source_id() != before


# ------------------------------------------------------------------------------------------------ 3. launcher validation
A = 0x100000                     # a dummy 4096-byte-aligned address, never dereferenced on these paths
BIG = 1 << 30
LENS = (10, 11, 12, 12)
DEL, INS, SUBST = 1, 2, 3


def call(edits=True, tokens=A, table=A, pm=A, sm=A, out=A, radem=A, chi=A, lens=LENS, dev=A, n=4, L=12, vocab=24, C=6, F=64, R=64,
         nseq=4, cw=10, mode=SUBST, lo=0, cnt=48, ws=A, wb=BIG):
    """Defaults: windows of 10 x 6 = 60 elements (padded width 64), 64 filters, four sequences of lengths 10 .. 12, all 48 slots."""
    from xgpr_amd import _lib
    lib = _lib.load()
    host = None if lens is None else np.asarray(lens, dtype=np.int32)
    hp = None if host is None else host.ctypes.data
    if edits:
        rc = lib.xgpr_conv_token_maxpool_edits_f32(tokens, table, pm, sm, out, radem, chi, hp, dev, n, L, vocab, C, F, R, nseq, cw, mode,
                                                   lo, cnt, ws, wb, None)
    else:
        rc = lib.xgpr_conv_token_maxpool_tables_f32(tokens, table, pm, sm, radem, chi, hp, dev, n, L, vocab, C, F, R, nseq, cw, ws, wb, None)
    return int(rc), _lib.last_error()


NO_DATAPOINTS, ODD_OUTPUT, RFFS_FREQS, ARRAY_SIZES, SEQLEN_SIZE, CONV_WIDTH, SEQLEN_RANGE, ARRAY_DIMS = -1, -2, -3, -4, -5, -6, -7, -8
UNSUPPORTED, WORKSPACE = -20, -21
REFUSED = ("the single-edit pool serves windows of up to 1024 elements and tables of up to 4608 floats "
           "(see xgpr_conv_token_maxpool_edits_ok)")
SEQ_RANGE = "All sequence lengths must be >= conv width and < array size."
FREQS = "incorrect number of rffs and or freqs."
VOCAB = "token table: vocab must be 1 .. 256 (uint8 tokens)"
WS_SMALL = "workspace too small (see xgpr_conv_workspace_bytes)"
WIDE = dict(L=200, C=6, cw=171, lens=(171, 180, 200, 200), F=2048, R=2048)      # 1026 elements: padded width 2048

# the checks both entry points make, in the order of xgpr_conv_token_maxpool_f32
SHARED = {
    "vocab 0": (dict(vocab=0), ARRAY_DIMS, VOCAB),
    "vocab 257": (dict(vocab=257), ARRAY_DIMS, VOCAB),
    "C < 1": (dict(C=0), ARRAY_DIMS, "token table: needs at least one column"),
    "no datapoints": (dict(n=0, nseq=0, lens=(), cnt=0), NO_DATAPOINTS, "no datapoints"),
    "an odd number of filters": (dict(F=63), ODD_OUTPUT, "last dim of output must be even number"),
    "no filters": (dict(F=0), ODD_OUTPUT, "last dim of output must be even number"),
    "more filters than signs": (dict(F=66), RFFS_FREQS, FREQS),
    "lengths of another batch": (dict(nseq=3), SEQLEN_SIZE, "wrong array sizes"),
    "conv_width 0": (dict(cw=0), CONV_WIDTH, "invalid conv_width"),
    "conv_width > L": (dict(cw=13), CONV_WIDTH, "invalid conv_width"),
    "signs not whole transforms": (dict(R=96), RFFS_FREQS, FREQS),
    "more signs than the filters' repetitions": (dict(R=128), RFFS_FREQS, FREQS),
    "a length below conv_width": (dict(lens=(10, 9, 12, 12)), SEQLEN_RANGE, SEQ_RANGE),
    "a length beyond L": (dict(lens=(10, 11, 12, 13)), SEQLEN_RANGE, SEQ_RANGE),
    "no host lengths": (dict(lens=None), SEQLEN_RANGE, "seqlen_host is required (sequence lengths are validated on the host)"),
    "NULL device lengths": (dict(dev=None), WORKSPACE, "seqlen_dev (device copy of the sequence lengths) is required"),
    "NULL tokens": (dict(tokens=None), WORKSPACE, "NULL array pointer"),
    "NULL table": (dict(table=None), WORKSPACE, "NULL array pointer"),
    "NULL pm": (dict(pm=None), WORKSPACE, "NULL array pointer"),
    "NULL sm": (dict(sm=None), WORKSPACE, "NULL array pointer"),
    "NULL radem": (dict(radem=None), WORKSPACE, "NULL array pointer"),
    "NULL chi": (dict(chi=None), WORKSPACE, "NULL array pointer"),
    "a table of 4617 floats": (dict(vocab=243, C=19, cw=3, lens=(3, 11, 12, 12)), UNSUPPORTED, REFUSED),
    "padded width 2048": (dict(vocab=4, **WIDE), UNSUPPORTED, REFUSED),
    "short workspace": (dict(wb=8), WORKSPACE, WS_SMALL),
    "no workspace": (dict(ws=None), WORKSPACE, WS_SMALL),
    # two failing checks at once: the first in the documented order is the one reported
    "vocab 0 and no datapoints": (dict(vocab=0, n=0, nseq=0, lens=()), ARRAY_DIMS, VOCAB),
    "odd filters and conv_width 0": (dict(F=63, cw=0), ODD_OUTPUT, "last dim of output must be even number"),
    "conv_width 0 and bad signs": (dict(cw=0, R=96), CONV_WIDTH, "invalid conv_width"),
    "bad signs and a bad length": (dict(R=96, lens=(1, 11, 12, 12)), RFFS_FREQS, FREQS),
    "a bad length and too wide": (dict(WIDE, vocab=4, lens=(170, 180, 200, 200)), SEQLEN_RANGE, SEQ_RANGE),
    "NULL tokens and too wide": (dict(WIDE, vocab=4, tokens=None), WORKSPACE, "NULL array pointer"),
    "too wide and short workspace": (dict(WIDE, vocab=4, wb=8), UNSUPPORTED, REFUSED),
}
MANY = 1398102                   # sequences of 12 positions: 16 777 224 slots, more than 2^24 - 1
EDITS_ONLY = {
    "mode 0": (dict(mode=0), ARRAY_DIMS, "mode must be 1 (deletions), 2 (insertions) or 3 (substitutions)"),
    "mode 4": (dict(mode=4), ARRAY_DIMS, "mode must be 1 (deletions), 2 (insertions) or 3 (substitutions)"),
    "mode 0 and vocab 0": (dict(mode=0, vocab=0), ARRAY_DIMS, "mode must be 1 (deletions), 2 (insertions) or 3 (substitutions)"),
    "NULL out": (dict(out=None), WORKSPACE, "NULL array pointer"),
    "a negative first slot": (dict(lo=-1), ARRAY_SIZES, "slot range outside the n * (L or L + 1) slots of the batch"),
    "slots past the batch": (dict(lo=40, cnt=9), ARRAY_SIZES, "slot range outside the n * (L or L + 1) slots of the batch"),
    "deletions: slots past the batch": (dict(mode=DEL, lo=0, cnt=49), ARRAY_SIZES, "slot range outside the n * (L or L + 1) slots of the batch"),
    "a negative count": (dict(cnt=-1), ARRAY_SIZES, "slot range outside the n * (L or L + 1) slots of the batch"),
    "short workspace and slots past the batch": (dict(wb=8, cnt=49), WORKSPACE, WS_SMALL),
    "too many slots": (dict(n=MANY, nseq=MANY, lens=(12,) * MANY, cnt=1 << 24), UNSUPPORTED, "too many slots for one launch (nslots < 2^24)"),
}
TABLES_ONLY = {
    "too many windows": (dict(n=1 << 23, nseq=1 << 23, lens=(10,) * (1 << 23)), UNSUPPORTED,
                         "too many windows for one launch (n * (L - conv_width + 2) < 2^24)"),
}


@pytest.mark.parametrize("name", sorted(SHARED))
def test_validation_outcome_of_both_entry_points(name):
    kw, code, msg = SHARED[name]
    assert call(edits=True, **kw) == (code, msg)
    assert call(edits=False, **{k: v for k, v in kw.items() if k != "cnt"}) == (code, msg)
    if code == UNSUPPORTED:
        assert "xgpr_conv_token_maxpool_edits_ok" in msg


@pytest.mark.parametrize("name", sorted(EDITS_ONLY))
def test_validation_outcome_of_the_edits(name):
    kw, code, msg = EDITS_ONLY[name]
    assert call(edits=True, **kw) == (code, msg)


@pytest.mark.parametrize("name", sorted(TABLES_ONLY))
def test_validation_outcome_of_the_tables(name):
    kw, code, msg = TABLES_ONLY[name]
    assert call(edits=False, **kw) == (code, msg)


def test_an_empty_slot_range_is_a_no_op():
    """Past every check and in front of the launch: 0; the insertions have 4 (12 + 1) = 52 slots, the other two modes 48."""
    assert call(cnt=0)[0] == 0 and call(lo=48, cnt=0)[0] == 0
    assert call(mode=INS, lo=52, cnt=0)[0] == 0 and call(mode=INS, lo=53, cnt=0)[0] == ARRAY_SIZES
    assert call(cnt=0, wb=8)[0] == WORKSPACE                                         # ... but the arguments are still checked


def test_workspace_bound_is_the_advertised_size():
    from xgpr_amd import _lib
    need = int(_lib.load().xgpr_rbf_workspace_bytes(64))
    assert need <= int(_lib.load().xgpr_conv_workspace_bytes(64, 60, 4, 4))         # the max-pool operator's buffer serves too
    for edits in (True, False):
        assert call(edits=edits, wb=need - 1)[0] == WORKSPACE
    assert call(wb=need, cnt=0)[0] == 0


def test_ok_predicate_at_its_limits():
    from xgpr_amd import _lib
    lib = _lib.load()
    ok = lambda *a: int(lib.xgpr_conv_token_maxpool_edits_ok(*a))
    assert [ok(w, 21, 21, 1024) for w in (21, 189)] == [1, 1] and ok(1, 4, 1, 2) == 1
    assert ok(1024, 4, 4, 64) == 1 and ok(1028, 4, 4, 64) == 0                       # padded width 1024 / 2048
    assert ok(3 * 18, 256, 18, 64) == 1 and ok(3 * 18, 257, 18, 64) == 0             # 4608 floats, 256 rows: the largest table
    assert ok(9 * 19, 243, 19, 64) == 0                                              # 4617 floats
    assert ok(190, 21, 21, 64) == 0                                                  # not whole positions
    assert ok(189, 21, 21, 0) == 0 and ok(189, 21, 21, 1) == 1                       # at least one filter
    for w, v, c in ((189, 21, 21), (1028, 4, 4), (171, 243, 19), (54, 256, 18)):     # the shapes of the input-gradient predicate
        assert ok(w, v, c, 64) == int(lib.xgpr_conv_token_maxpool_input_grad_ok(w, v, c))


# ------------------------------------------------------------------------------------------------ 4. the compiler's table
def test_resource_table_lists_every_new_kernel_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    pat = r"conv_token_maxpool_edits_kernel<\d+, \d+>|conv_token_maxpool_proj_kernel<\d+>|conv_token_maxpool_scan_kernel"
    rows = [r for r in resource_usage.collect() if re.fullmatch(pat, r["name"])]
    want = ([f"conv_token_maxpool_edits_kernel<{lg}, {mode}>" for lg in range(1, 11) for mode in (DEL, INS, SUBST)]
            + [f"conv_token_maxpool_proj_kernel<{lg}>" for lg in range(1, 11)] + ["conv_token_maxpool_scan_kernel"])
    assert sorted(r["name"] for r in rows) == sorted(want)
    for r in rows:                                       # (windows of up to 64 elements park 9 .. 22 scalar registers in vector lanes)
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0, r
        if re.fullmatch(r"conv_token_maxpool_edits_kernel<[789], \d+>|conv_token_maxpool_(proj|scan)_kernel.*", r["name"]):
            assert r.get("SGPRs Spill", 0) == 0, r
