"""The combinatorial site scan without a GPU: the fourteenth public header, include/xgpr_hip/site_scan.h, held to what
tests/test_pair_scan_host.py holds the eleventh; the host layout function against the Python mirror of tests/dense_site_scan.py on
an exhaustive sweep; the launcher's argument validation through the C ABI (nothing reaches a HIP call: device pointers are dummy
integers); the reference's self-checks -- the run decomposition summed equals the definition, every planted mistake moves some case
beyond its cap, the a-priori cap is at most 1e-2 of the largest output of every non-degenerate case the GPU test runs --; the
``SiteLibrary`` class on CPU tensors against brute force; and the compiler's resource report for the new kernels."""
import ctypes
import functools
import inspect
import itertools
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

import dense_site_scan as ds
from test_cabi import _build_module
from xgpr_amd.acquisition import SiteLibrary, site_runs          # (the classes under test: without them nothing here has a subject)
from test_subst_scan_host import A, ARRAY_DIMS, BIG, CONV_WIDTH, RFFS_FREQS, SEQLEN, UNSUPPORTED, WORKSPACE, _codes

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "xgpr_hip", "site_scan.h")
NAMES = ["xgpr_conv_token_site_scan_f32", "xgpr_conv_token_site_scan_layout", "xgpr_conv_token_site_scan_ok",
         "xgpr_conv_token_site_scan_workspace_bytes"]
RETURNS = {"xgpr_conv_token_site_scan_f32": ("int", ctypes.c_int), "xgpr_conv_token_site_scan_layout": ("long", ctypes.c_long),
           "xgpr_conv_token_site_scan_ok": ("int", ctypes.c_int), "xgpr_conv_token_site_scan_workspace_bytes": ("size_t", ctypes.c_size_t)}


# ------------------------------------------------------------------------------------------------ 1. the fourteenth header
def _declared():
    hdr = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(xgpr_[a-z0-9_]+)\s*\(", hdr)))                # the expression of tests/test_cabi.py


def test_the_header_declares_its_four_entry_points_and_nothing_of_the_other_headers():
    assert _declared() == NAMES
    inc = os.path.join(ROOT, "include")
    others = [os.path.join(inc, f) for f in os.listdir(inc) if f.endswith(".h")]
    others += [os.path.join(inc, "xgpr_hip", f) for f in os.listdir(os.path.join(inc, "xgpr_hip")) if f != "site_scan.h"]
    assert len(others) == 13
    for path in others:
        hdr = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
        assert not set(NAMES) & set(re.findall(r"\b(xgpr_[a-z0-9_]+)\s*\(", hdr)), path


def test_library_exports_every_declared_name():
    bm = _build_module()
    bm.build_extension()
    lib = ctypes.CDLL(bm.LIB)
    for n in _declared():
        assert hasattr(lib, n), f"{n} declared in include/xgpr_hip/site_scan.h but not exported"


def test_ctypes_table_matches_the_header():
    from xgpr_amd import _lib
    assert set(_lib.SITE_SCAN_ABI) == set(_declared())
    for t in dir(_lib):
        tab = getattr(_lib, t)
        if (t.endswith("SIGNATURES") or t.endswith("_ABI") or t in ("SIZE_FUNCS", "STRING_FUNCS")) and tab is not _lib.SITE_SCAN_ABI:
            assert not set(_lib.SITE_SCAN_ABI) & set(tab), t
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, args in _lib.SITE_SCAN_ABI.items():                                    # load() applied the table
        fn = getattr(lib, name)
        assert fn.argtypes == args
        assert fn.restype is RETURNS[name][1], name
        decl = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)", hdr)                # the tables' lengths are the parameter counts
        assert len(decl.group(2).split(",")) == len(args), name
        assert decl.group(1) == RETURNS[name][0], name
    # the operands are those of the pair scan, plus the site list and its length after the device lengths
    pair = _lib.PAIR_SCAN_SIGNATURES["xgpr_conv_token_pair_scan_f32"]
    assert _lib.SITE_SCAN_ABI["xgpr_conv_token_site_scan_f32"] == pair[:8] + [ctypes.c_void_p, ctypes.c_int] + pair[8:]


def test_every_writer_has_a_memory_contract_row():
    import test_gpu_site_scan_memory_contract as table
    writers = {n for n in _declared() if n.endswith("_f32")}
    assert writers == {"xgpr_conv_token_site_scan_f32"}
    assert table.covered_entry_points() == writers


def test_source_id_covers_the_header(tmp_path, monkeypatch):
    bm = _build_module()
    assert os.path.samefile(bm.SITE_SCAN_HDR, HEADER) and bm.SITE_SCAN_HDR in bm.sources()
    assert "site_scan.inc" in [os.path.basename(p) for p in bm.sources()]
    src = open(bm.SRC).read()
    assert src.index('#include "pair_scan.inc"') < src.index('#include "site_scan.inc"') < src.index('#include "var_scan.inc"')
    before = bm.source_id()
    copy = tmp_path / "site_scan.h"
    shutil.copyfile(HEADER, copy)
    monkeypatch.setattr(bm, "SITE_SCAN_HDR", str(copy))
    assert bm.source_id() == before                                                  # name and contents, not the path
    with open(copy, "a") as f:
        f.write("/* changed */\n")
    assert bm.source_id() != before


# ------------------------------------------------------------------------------------------------ 2. the layout on the host
def layout(sites, L, cw, vocab, max_runs=None, arrays=True):
    from xgpr_amd import _lib
    s = np.asarray(sites, dtype=np.int32)
    K = len(sites)
    cap = max(2 * K - 1, 1) if max_runs is None else max_runs
    bufs = [np.full(max(cap, 1), -7, dtype=np.int32) for _ in range(4)] + [np.full(max(cap, 1), -7, dtype=np.int64)]
    ptrs = [ctypes.c_void_p(b.ctypes.data) if arrays else None for b in bufs]
    nr = int(_lib.load().xgpr_conv_token_site_scan_layout(ctypes.c_void_p(s.ctypes.data) if sites is not None and K else None, K, L, cw,
                                                          vocab, *ptrs, cap))
    return nr, bufs


def test_the_layout_is_the_python_mirror_on_every_site_subset():
    """Every non-empty subset of the positions of arrays of up to 8 tokens, at every conv_width (255 subsets at L = 8): runs with more
    than four sites included -- the layout describes them, the launcher refuses them."""
    from xgpr_amd.acquisition import site_runs
    count = 0
    for L in (1, 2, 5, 8):
        for cw in range(1, L + 1):
            for K in range(1, L + 1):
                for sites in itertools.combinations(range(L), K):
                    want = ds.site_runs(sites, L, cw)
                    assert site_runs(sites, L, cw) == want                           # (the package's own mirror)
                    offs, T = ds.run_offsets(want, 3)
                    nr, (jlo, jhi, first, g, off) = layout(sites, L, cw, 3)
                    assert nr == len(want) <= 2 * K - 1, (sites, L, cw)
                    got = [(int(jlo[q]), int(jhi[q]), int(first[q]), int(g[q])) for q in range(nr)]
                    assert got == want and [int(o) for o in off[:nr]] == offs, (sites, L, cw)
                    assert (jlo[nr:] == -7).all() and (off[nr:] == -7).all()
                    assert layout(sites, L, cw, 3, arrays=False, max_runs=0)[0] == nr    # the count alone
                    # every window that holds a site lies in exactly one run, with exactly the sites it holds
                    for j in range(L - cw + 1):
                        cov = [k for k, p in enumerate(sites) if j <= p < j + cw]
                        hit = [r for r in want if r[0] <= j <= r[1]]
                        assert (len(hit) == 1 and list(range(hit[0][2], hit[0][2] + hit[0][3])) == cov) if cov else not hit
                    count += 1
    assert count > 1000


def test_the_gb1_layout():
    """The example of DESIGN.md 3.27: sites 38, 39, 40, 53 of 56 residues at conv_width 9 and V = 20."""
    want = ds.site_runs((38, 39, 40, 53), 56, 9)
    assert [(r[1] - r[0] + 1, r[3]) for r in want] == [(1, 1), (1, 2), (7, 3), (1, 2), (1, 1), (3, 1)]
    nr, (jlo, jhi, first, g, off) = layout((38, 39, 40, 53), 56, 9, 20)
    assert nr == 6 and [20 ** int(x) for x in g[:6]] == [20, 400, 8000, 400, 20, 20]
    assert int(off[5]) + 20 == 8860 == ds.run_offsets(want, 20)[1]


def test_the_layouts_refusals():
    codes = _codes()
    assert layout((1, 2), 0, 1, 3)[0] == codes[ARRAY_DIMS]
    assert layout((1, 2), 6, 0, 3)[0] == codes[CONV_WIDTH]
    assert layout((1, 2), 6, 7, 3)[0] == codes[CONV_WIDTH]
    assert layout((1, 2), 6, 3, 0)[0] == codes[ARRAY_DIMS]
    assert layout((1, 2), 6, 3, 257)[0] == codes[ARRAY_DIMS]
    assert layout((), 6, 3, 3)[0] == codes[ARRAY_DIMS]
    assert layout(tuple(range(17)), 40, 3, 3)[0] == codes[ARRAY_DIMS]
    assert layout(tuple(range(16)), 40, 3, 3)[0] > 0
    assert layout((2, 2), 6, 3, 3)[0] == codes[ARRAY_DIMS]
    assert layout((3, 2), 6, 3, 3)[0] == codes[ARRAY_DIMS]
    assert layout((-1, 2), 6, 3, 3)[0] == codes[ARRAY_DIMS]
    assert layout((2, 6), 6, 3, 3)[0] == codes[ARRAY_DIMS]
    assert layout((1, 2, 4), 6, 3, 3, max_runs=2)[0] == codes[ARRAY_DIMS]             # an array too short for the runs
    assert layout(tuple(range(16)), 40, 16, 256)[0] == codes[UNSUPPORTED]            # 256^16 entries
    from xgpr_amd import _lib
    assert _lib.last_error()


# ------------------------------------------------------------------------------------------------ 3. launcher validation
def scan(tokens=A, table=A, w=A, out=A, radem=A, chi=A, lens=(6, 4, 5), seqlen_dev=A, sites=(1, 2, 3), K=None, n=3, L=6, vocab=5, C=4,
         F=40, R=64, cw=3, scaling=1, icpt=1, ws=A, wb=BIG):
    from xgpr_amd import _lib
    host = np.asarray(lens, dtype=np.int32) if lens is not None else None
    hp = ctypes.c_void_p(host.ctypes.data) if host is not None else None
    sh = np.asarray(sites, dtype=np.int32) if sites is not None else None
    sp = ctypes.c_void_p(sh.ctypes.data) if sh is not None and sh.size else None
    K = (len(sites) if sites is not None else 0) if K is None else K
    rc = _lib.load().xgpr_conv_token_site_scan_f32(tokens, table, w, out, radem, chi, hp, seqlen_dev, sp, K, n, L, vocab, C, F, R, cw,
                                                   scaling, icpt, ws, wb, None)
    return int(rc), _lib.last_error()


REFUSALS = {
    # in the documented order: the pair scan's checks down to vocab ...
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
    "a length above L": (dict(lens=(6, 4, 7)), SEQLEN),
    "vocab 0": (dict(vocab=0), ARRAY_DIMS),
    "vocab 257": (dict(vocab=257), ARRAY_DIMS),
    # ... the site list ...
    "no sites": (dict(sites=()), ARRAY_DIMS),
    "K 0 with a list": (dict(K=0), ARRAY_DIMS),
    "NULL site list": (dict(sites=None, K=2), ARRAY_DIMS),
    "17 sites": (dict(sites=tuple(range(17)), L=40, lens=(40, 40, 40)), ARRAY_DIMS),
    "sites not ascending": (dict(sites=(2, 1)), ARRAY_DIMS),
    "a site twice": (dict(sites=(2, 2)), ARRAY_DIMS),
    "a negative site": (dict(sites=(-1, 2)), ARRAY_DIMS),
    "a site at L": (dict(sites=(2, 6)), ARRAY_DIMS),
    "a site past a sequence": (dict(sites=(1, 4)), SEQLEN),
    # ... the predicate ...
    "a window of 2048 elements": (dict(L=40, cw=32, C=64, lens=(40, 32, 33), R=2048), UNSUPPORTED),
    "a table of more than 4608 floats": (dict(vocab=256, C=19, R=64), UNSUPPORTED),
    "five sites in one window": (dict(sites=(0, 1, 2, 3, 4), L=8, cw=5, lens=(8, 5, 6), R=64), UNSUPPORTED),
    # ... the buffers
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
    "a bad length and vocab 257": (dict(lens=(6, 2, 4), vocab=257), SEQLEN),
    "vocab 257 and no sites": (dict(vocab=257, sites=()), ARRAY_DIMS),
    "an unsupported table and sites not ascending": (dict(vocab=256, C=19, sites=(2, 1)), ARRAY_DIMS),
    "an unsupported table and a site past a sequence": (dict(vocab=256, C=19, sites=(1, 4)), SEQLEN),
    "sites not ascending and a site past a sequence": (dict(sites=(5, 4)), ARRAY_DIMS),
    "a site past a sequence and five sites in one window": (dict(sites=(0, 1, 2, 3, 5), L=8, cw=6, lens=(8, 5, 6)), SEQLEN),
    "an unsupported table and no workspace": (dict(vocab=256, C=19, ws=None), UNSUPPORTED),
    "five sites in one window and no workspace": (dict(sites=(0, 1, 2, 3, 4), L=8, cw=5, lens=(8, 5, 6), ws=None), UNSUPPORTED),
    "short workspace and NULL out": (dict(wb=8, out=None), WORKSPACE),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_validation_outcome(name):
    kw, code = REFUSALS[name]
    rc, err = scan(**kw)
    assert rc == _codes()[code] and rc < 0, (rc, err)
    assert err
    if name in ("no workspace", "short workspace", "short workspace and NULL out"):
        assert err == "workspace too small (see xgpr_conv_token_site_scan_workspace_bytes)"
    if name.startswith("NULL") and code == WORKSPACE:
        assert err == "NULL array pointer"
    if name in ("a window of 2048 elements", "a table of more than 4608 floats", "an unsupported table and no workspace"):
        assert err.startswith("the site scan serves windows") and "xgpr_conv_token_site_scan_ok" in err   # the message names this operator
    if name.startswith("five sites"):
        assert err.startswith("the site scan serves up to 4 sites inside one window")


def test_the_row_count_of_one_launch():
    """n * sum over the runs of vocab^(g - 1) < 2^24.  (The largest batch inside the bound would be launched: only the refusals are
    called.)"""
    from xgpr_amd import _lib

    def many(n, sites, vocab, L=6, cw=3):
        lens = np.full(n, L, dtype=np.int32)
        s = np.asarray(sites, dtype=np.int32)
        rc = _lib.load().xgpr_conv_token_site_scan_f32(A, A, A, A, A, A, ctypes.c_void_p(lens.ctypes.data), A, ctypes.c_void_p(s.ctypes.data),
                                                       len(sites), n, L, vocab, 4, 40, 64, cw, 1, 1, A, BIG, None)
        return int(rc), _lib.last_error()
    # sites (1, 2, 3) of 6 positions at conv_width 3: runs of 2, 3, 2, 1 sites -> V + V^2 + V + 1 rows per sequence
    per = 5 + 25 + 5 + 1
    rc, err = many((1 << 24) // per + 1, (1, 2, 3), 5)
    assert rc == _codes()[UNSUPPORTED] and "vocab^(sites - 1)" in err
    rc, err = many(1, (0, 1, 2, 3), 256, cw=4)                                       # one sequence: 256^3 rows in the run of four
    assert rc == _codes()[UNSUPPORTED] and "vocab^(sites - 1)" in err


def test_no_sequences():
    assert scan(n=0, lens=None, tokens=None, table=None, w=None, out=None, radem=None, chi=None, seqlen_dev=None, ws=None, wb=0)[0] == 0
    assert scan(n=0, lens=None, vocab=257)[0] == _codes()[ARRAY_DIMS]                 # ... but the shape is still checked
    assert scan(n=0, lens=None, sites=(2, 1))[0] == _codes()[ARRAY_DIMS]              # ... and the site list
    assert scan(n=0, lens=None, vocab=256, C=19)[0] == _codes()[UNSUPPORTED]


def test_the_advertised_workspace_is_the_bound_the_launcher_checks():
    from xgpr_amd import _lib
    lib = _lib.load()
    masks = int(lib.xgpr_rbf_workspace_bytes(64))
    need = int(lib.xgpr_conv_token_site_scan_workspace_bytes(64, 3, 3))
    assert need == masks + 3 * 5 * 8                                                 # one double per sequence and possible run (2 K - 1)
    assert scan(wb=need - 1)[0] == _codes()[WORKSPACE]
    assert int(lib.xgpr_conv_token_site_scan_workspace_bytes(64, 0, 3)) == masks


def test_ok_predicate():
    from xgpr_amd import _lib
    lib = _lib.load()
    ok = lambda width, vocab, C, F, m: int(lib.xgpr_conv_token_site_scan_ok(width, vocab, C, F, m))
    for args in ((12, 6, 4, 8), (1008, 5, 21, 1), (1025, 5, 21, 8), (57, 256, 19, 8), (12, 6, 4, 0), (189, 21, 21, 8192)):
        base = int(lib.xgpr_conv_token_subst_scan_ok(*args))
        assert [ok(*args, m) for m in (0, 1, 2, 3, 4, 5)] == [0, base, base, base, base, 0]


def test_python_wrappers():
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    assert ext.conv_token_site_scan_ok(189, 21, 21, 8192, 3) == 1 and ext.conv_token_site_scan_ok(189, 21, 21, 8192, 5) == 0
    runs, T = ext.conv_token_site_scan_layout((38, 39, 40, 53), 56, 9, 20)
    assert T == 8860 and [r["sites"] for r in runs] == [1, 2, 3, 2, 1, 1] and runs[2] == dict(
        first_window=32, last_window=38, first_site=0, sites=3, offset=420)
    with pytest.raises(RuntimeError, match="strictly ascending"):
        ext.conv_token_site_scan_layout((3, 3), 56, 9, 20)
    pair, site = (list(inspect.signature(f).parameters) for f in (ext.hipConvTokenPairScan, ext.hipConvTokenSiteScan))
    assert site == pair[:7] + ["sites"] + pair[7:]
    from xgpr_amd.kernels import ConvSORFKernel
    from xgpr_amd.models import xGPRegression
    assert callable(ConvSORFKernel.site_scan) and callable(ConvSORFKernel.site_scan_composed)
    assert ConvSORFKernel.SITE_SCAN_VARIANTS == 1 << 22 and "2^22" in ConvSORFKernel.site_scan_composed.__doc__
    sig = inspect.signature(xGPRegression.predict_site_library)
    assert list(sig.parameters)[1:3] == ["input_x", "sites"] and sig.parameters["chunk_size"].default == 4


# ------------------------------------------------------------------------------------------------ 4. the reference's self-checks
@functools.lru_cache(maxsize=None)
def _ref(name):
    return ds.reference(name)


@functools.lru_cache(maxsize=None)
def _full(name):
    return ds.full_reference(name)


@pytest.mark.parametrize("name", [c[0] for c in ds.CASES])
def test_the_run_tables_summed_are_the_definition(name):
    """The decomposition itself, in long double on both sides: far inside the cap."""
    c, sites, cw, _, _, runs, tables, caps, total = _ref(name)
    V, K = c["table"].shape[0], len(sites)
    full = _full(name)
    got = ds.gather_full(runs, tables, V, K)
    assert got.shape == full.shape == (c["tokens"].shape[0], V ** K)
    err = float(np.abs(got - full).max())
    print(name, err, total)
    assert err <= 1e-6 * total
    assert ds.check(got.astype(np.float64), full, total) <= total                     # the comparison of the GPU test, unplanted
    for i in range(c["tokens"].shape[0]):                                            # the own assignment: zero in every table and in the sum
        own = 0
        for p in sites:
            own = own * V + int(c["tokens"][i, p])
        assert abs(float(full[i, own])) <= 1e-15 * max(float(np.abs(full).max()), 1e-300)


def _dead_runs(name):
    c, sites, cw, _, _, runs, _, _, _ = _ref(name)
    return [(i, q) for i in range(c["tokens"].shape[0]) for q, r in enumerate(runs) if r[0] > int(c["seqlen"][i]) - cw]


def test_the_cases_cover_what_they_are_listed_for():
    import dense_reference as dr
    kws = {nm: (kw, sites) for nm, kw, sites, _, _ in ds.CASES}
    padded = {dr.padded_width(kw["conv_width"] * kw["C"]) for kw, _ in kws.values()}
    assert {16, 64, 128, 512, 1024} <= padded
    cover = {nm: max(g for _, _, _, g in ds.site_runs(sites, kw["L"], kw["conv_width"])) for nm, (kw, sites) in kws.items()}
    assert cover["w16_c4_cw3"] == 3 and cover["g4_cw9"] == 4 and cover["graph_cw1"] == 1 and cover["one_site"] == 1
    assert {kw["V"] for kw, _ in kws.values()} >= {1, 256} and {kw["n"] for kw, _ in kws.values()} >= {1, 65}
    assert _dead_runs("w16_c4_cw3") and _dead_runs("w128_c21_cw6")                    # runs that have no window in a short sequence
    c, sites, cw = ds.case("w512_c60_cw8")[:3]
    assert any(r[0] <= int(s) - cw < r[1] for s in c["seqlen"] for r in ds.site_runs(sites, 10, cw))   # a run cut short by a length
    c, sites, _, _, _ = ds.case("w128_c21_cw6")
    assert sites[0] == 0 and (c["seqlen"] - 1 == sites[-1]).any()                     # position 0 and a last token
    from xgpr_amd.acquisition import SiteLibrary
    kw, sites = kws["two_components"]
    runs = ds.site_runs(sites, kw["L"], kw["conv_width"])
    lib = SiteLibrary(sites, 3, [range(a, a + g) for _, _, a, g in runs], [torch.zeros((1,) + (3,) * g) for _, _, _, g in runs])
    assert lib.components() == [(0, 1), (2, 3)]
    c = ds.case("dup_rows")[0]
    assert (c["table"][1] == c["table"][3]).all()
    for nm, (kw, sites) in kws.items():                                              # every site inside every sequence
        assert sites[-1] < int(ds.case(nm)[0]["seqlen"].min()), nm


@pytest.mark.parametrize("mistake", ds.MISTAKES)
def test_a_planted_mistake_moves_some_case_beyond_its_cap(mistake):
    caught = []
    for name in ("w16_c4_cw3", "dup_rows", "two_components"):
        c, sites, _, _, _, _, _, _, total = _ref(name)
        runs, bad = ds.reference(name, mistake)[5:7]
        got = ds.gather_full(runs, bad, c["table"].shape[0], len(sites))
        err = float(np.abs(got - _full(name)).max())
        print(mistake, name, err, total)
        if err > total:
            with pytest.raises(AssertionError):
                ds.check(got.astype(np.float64), _full(name), total)
            caught.append(name)
    assert caught, mistake


def test_every_mistake_has_a_test():
    assert set(ds.MISTAKES) == {"run_boundary", "swapped_sites", "truncate_at_L", "keep_w0", "no_parent", "strides"}


@pytest.mark.parametrize("name", [c[0] for c in ds.CASES if c[0] not in ds.DEGENERATE])
def test_the_cap_is_two_orders_below_the_outputs(name):
    """A condition on the case, not a measurement of the operator: the reference alone."""
    _, _, _, _, _, runs, tables, caps, total = _ref(name)
    big = float(np.abs(_full(name)).max())
    print(name, total, big, total / big)
    assert 0 < total <= 1e-2 * big
    for q, tb in enumerate(tables):                                                  # ... and run by run
        assert 0 < caps[q] <= 1e-2 * float(np.abs(tb).max()), (q, runs[q])


def test_the_degenerate_case():
    _, _, _, _, _, runs, tables, caps, total = _ref("vocab1")
    assert [tb.shape for tb in tables] == [(2, 1)] * len(runs) and all((tb == 0).all() for tb in tables) and total > 0
    assert (_full("vocab1") == 0).all()


# ------------------------------------------------------------------------------------------------ 5. SiteLibrary on CPU tensors
def _library(seed, n=3, V=4, sites=(2, 3, 4, 9, 10, 20), runs=((0,), (0, 1), (0, 1, 2), (1, 2), (2,), (3,), (3, 4), (4,), (5,)), integer=False):
    from xgpr_amd.acquisition import SiteLibrary
    gen = torch.Generator().manual_seed(seed)
    tables = []
    for r in runs:
        shape = (n,) + (V,) * len(r)
        t = (torch.randint(-2, 3, shape, generator=gen).to(torch.float64) if integer
             else torch.randn(shape, dtype=torch.float64, generator=gen))
        tables.append(t)
    return SiteLibrary(sites, V, runs, tables, base=torch.arange(n, dtype=torch.float64))


def _brute(lib):
    """[n, V^K] by adding, for every assignment, one entry of every table with plain Python indexing."""
    V, K = lib.vocab, len(lib.sites)
    out = torch.zeros((lib.n, V ** K), dtype=torch.float64)
    for flat, a in enumerate(itertools.product(range(V), repeat=K)):
        for r, t in zip(lib.runs, lib.tables):
            out[:, flat] += t[(slice(None),) + tuple(a[k] for k in r)]
    return out


def test_site_library_components_dense_and_gather():
    lib = _library(1)
    assert lib.components() == [(0, 1, 2), (3, 4), (5,)]
    V, K = lib.vocab, len(lib.sites)
    brute = _brute(lib)
    dense = lib.dense()
    assert tuple(dense.shape) == (lib.n,) + (V,) * K
    assert float((dense.reshape(lib.n, -1) - brute).abs().max()) <= 1e-13
    A = torch.tensor(list(itertools.product(range(V), repeat=K)))
    pick = A[torch.randperm(A.shape[0], generator=torch.Generator().manual_seed(2))[:97]]
    got = lib.gather(pick)
    flat = (pick * torch.tensor([V ** (K - 1 - k) for k in range(K)])).sum(dim=1)
    assert tuple(got.shape) == (lib.n, 97) and float((got - brute[:, flat]).abs().max()) <= 1e-13
    assert tuple(lib.gather(pick.numpy()).shape) == (lib.n, 97)
    with pytest.raises(RuntimeError, match="one token per site"):
        lib.gather(pick[:, :-1])
    with pytest.raises(RuntimeError, match="tokens 0"):
        lib.gather(pick + V)
    lib.DENSE_ELEMS = lib.n * V ** K - 1
    with pytest.raises(RuntimeError, match="DENSE_ELEMS"):
        lib.dense()
    from xgpr_amd.acquisition import SiteLibrary
    with pytest.raises(RuntimeError, match="one axis per site"):
        SiteLibrary((1, 2), 3, [(0, 1)], [torch.zeros(2, 3)])
    with pytest.raises(RuntimeError, match="ascending sites"):
        SiteLibrary((1, 2), 3, [(1, 0)], [torch.zeros(2, 3, 3)])


@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("integer", [False, True])
def test_site_library_topk_is_brute_force(largest, integer):
    """Random tables, and small-integer tables where most values tie: the k best with ties to the lower flat index are what a stable
    sort of the dense library gives."""
    lib = _library(3 + integer, integer=integer)
    V, K = lib.vocab, len(lib.sites)
    brute = _brute(lib)                                                              # (integers: exact, so the ties are real)
    for k in (1, 7, 100):
        vals, assign = lib.topk(k, largest=largest)
        assert tuple(vals.shape) == (lib.n, k) and tuple(assign.shape) == (lib.n, k, K)
        order = torch.sort(-brute if largest else brute, dim=1, stable=True)[1][:, :k]
        want = torch.gather(brute, 1, order)
        flat = (assign * torch.tensor([V ** (K - 1 - j) for j in range(K)])).sum(dim=2)
        if integer:
            assert torch.equal(vals, want) and torch.equal(flat, order)
            assert len({float(v) for v in want[0]}) < k or k == 1                    # there WERE ties among the best
        else:
            assert float((vals - want).abs().max()) <= 1e-13 and torch.equal(flat, order)
        assert float((lib.gather(assign[0])[0] - vals[0]).abs().max()) <= 1e-13
    vals, assign = _library(5, V=2, sites=(1, 5), runs=((0,), (1,))).topk(100)        # k above V^K: all of them
    assert tuple(vals.shape) == (3, 4) and tuple(assign.shape) == (3, 4, 2)


def test_site_library_topk_never_forms_the_whole_library():
    """3 + 3 + 2 sites of 20 tokens: 20^8 variants, three components of at most 8000 entries."""
    runs = ((0,), (0, 1), (0, 1, 2), (1, 2), (2,), (3,), (3, 4), (3, 4, 5), (4, 5), (5,), (6,), (6, 7), (7,))
    lib = _library(7, n=1, V=20, sites=(3, 4, 5, 30, 31, 32, 50, 51), runs=runs)
    lib.DENSE_ELEMS = 8000
    vals, assign = lib.topk(5)
    assert float((lib.gather(assign[0])[0] - vals[0]).abs().max()) <= 1e-12 and bool((vals[0, :-1] >= vals[0, 1:]).all())
    best = sum(float(lib._dense_over(c).max()) for c in lib.components())
    assert abs(float(vals[0, 0]) - best) <= 1e-12
    with pytest.raises(RuntimeError, match="DENSE_ELEMS"):
        lib.dense()


# ------------------------------------------------------------------------------------------------ 6. the compiler's report
def test_the_new_kernels_use_no_scratch_and_spill_nothing():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_usage
    rows = [r for r in resource_usage.collect() if r["name"].startswith("site_scan_")]
    assert sorted(r["name"] for r in rows) == sorted([f"site_scan_grid_kernel<{lg}>" for lg in range(1, 11)]
                                                     + ["site_scan_corner_kernel", "site_scan_diff_kernel"])
    for r in rows:
        assert r.get("ScratchSize", 0) == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, r
