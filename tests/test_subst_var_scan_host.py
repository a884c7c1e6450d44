"""The substitution variance scan without a GPU: the dense reference of tests/dense_subst_var_scan.py catches every planted mistake
through the comparison the GPU test uses, its direct form agrees with the operator's three-term expansion, and its a-priori cap is at
most 1e-2 of the largest |Q - q_i| of every case the GPU test runs; the ninth public header, include/xgpr_hip_subst_var_scan.h, held
to what tests/test_subst_scan_host.py holds the seventh; the launcher's argument validation through the C ABI (nothing reaches a HIP
call: device pointers are dummy integers); the shape predicate and the workspace size on the host.  (The compiler's resource report
of the two new kernels -- no scratch, no spilled vector register -- is held by tests/test_resource_usage.py, which walks every kernel
of the library.)"""
import ctypes
import inspect
import os
import re
import shutil

import numpy as np
import pytest

import dense_subst_scan as dss
import dense_subst_var_scan as dv
from dense_reference import LD
from test_cabi import _build_module

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "xgpr_hip_subst_var_scan.h")
NAMES = ["xgpr_conv_token_subst_var_scan_f32", "xgpr_conv_token_subst_var_scan_ok", "xgpr_conv_token_subst_var_scan_workspace_bytes"]
CASE_NAMES = [c[0] for c in dv.CASES]


def _spread(k):
    """max |Q - q_i| over the live entries of a case."""
    c = k["c"]
    live = np.arange(c["tokens"].shape[1])[None, :] < c["seqlen"][:, None]
    return float(np.abs((k["ref"] - k["q"][:, None, None]) * live[:, :, None]).max())


# ------------------------------------------------------------------------------------------------ 1. the reference and its cap
def test_the_case_list_covers_every_axis():
    assert CASE_NAMES == [c[0] for c in dss.CASES]                                   # the twelve operand sets, each with an nvar
    nvars = {nm: nv for nm, nv, _, _ in dv.CASES}
    F = {nm: kw["F"] for nm, kw, _, _ in dss.CASES}
    icpt = {nm: ic for nm, _, _, ic in dss.CASES}
    assert all(nv % 2 == 0 and 2 <= nv <= 2 * F[nm] for nm, nv in nvars.items())
    assert {2, 130, 512, 2048} <= set(nvars.values()) and nvars["w256_c21_cw9"] == 2048
    assert any(nv == 2 * F[nm] for nm, nv in nvars.items())                          # every column
    assert any(nv % 4 and nv % 16 and nv % 64 for nv in nvars.values())
    assert any(icpt[nm] for nm in nvars) and any(not icpt[nm] for nm in nvars)
    assert any(pad > 0 for _, _, pad, _ in dv.CASES)                                  # a row stride of Vm


@pytest.mark.parametrize("name", [n for n in CASE_NAMES if n != "vocab1"])
def test_the_cap_is_two_orders_below_the_spread(name):
    """A condition on the case, not a measurement of the operator: the reference alone."""
    k = dv.case(name)
    big = _spread(k)
    print(name, k["nvar"], k["cap"], big, k["cap"] / big)
    assert 0 < k["cap"] <= 1e-2 * big


def test_a_table_of_one_row_has_nothing_to_substitute():
    k = dv.case("vocab1")
    c = k["c"]
    assert k["ref"].shape[2] == 1 and k["cap"] > 0
    for i, s in enumerate(c["seqlen"]):
        assert float(np.abs(k["ref"][i, :s, 0] - k["q"][i]).max()) <= 1e-17 * max(1.0, abs(float(k["q"][i])))
        assert (k["ref"][i, s:] == 0).all()


def test_the_reference_has_the_contract_s_structure():
    k = dv.case("dup_rows")
    c, ref = k["c"], k["ref"]
    for i, s in enumerate(int(v) for v in c["seqlen"]):
        assert (ref[i, s:] == 0).all()
        own = ref[i, np.arange(s), c["tokens"][i, :s]]                                # the own token: q_i up to the reference's rounding
        assert float(np.abs(own - k["q"][i]).max()) <= 1e-16 * float(np.abs(ref).max())
    assert (ref[:, :, 1] == ref[:, :, 3]).all()                                       # the duplicated table row
    assert dv.check(ref.astype(np.float64), ref, k["cap"]) <= k["cap"]                # the unplanted reference passes its own comparison
    vm = k["vm"]
    assert (vm == vm.T).all() and 0.7 <= vm.diagonal().min() and vm.diagonal().max() <= 1.3
    assert float((np.abs(vm).sum(axis=1) - np.abs(vm.diagonal())).max()) <= 1.0


PLANT_CASES = ("dup_rows", "w16_c4_cw3", "n1")       # intercept on / on with every column / off


@pytest.mark.parametrize("mistake", dv.MISTAKES)
def test_a_planted_mistake_is_caught(mistake):
    caught = []
    for name in PLANT_CASES:
        k = dv.case(name)
        bad = dv.var_scan(k["c"], k["vm"], k["cw"], k["scaling"], k["icpt"], mistake=mistake)[0]
        moved = float(np.abs(bad - k["ref"]).max())
        print(mistake, name, moved, k["cap"])
        if moved > k["cap"]:
            with pytest.raises(AssertionError):
                dv.check(bad.astype(np.float64), k["ref"], k["cap"])
            caught.append(name)
    assert caught, mistake


def test_every_mistake_has_a_test():
    assert set(dv.MISTAKES) == {"no_cross", "r_once", "keep_col0", "first_window", "vm_upper", "cos_sin_swapped"}


@pytest.mark.parametrize("name", ["dup_rows", "w128_c21_cw6", "w512_c16_cw20", "n65"])
def test_the_three_term_expansion_is_the_direct_form(name):
    k = dv.case(name)
    exp = dv.var_scan(k["c"], k["vm"], k["cw"], k["scaling"], k["icpt"], expansion=True)[0]
    scale = float(np.abs(k["ref"]).max())
    assert float(np.abs(exp - k["ref"]).max()) <= 64 * k["nvar"] * float(np.finfo(LD).eps) * scale


def test_the_fixed_point_product_is_the_longdouble_product():
    rng = np.random.default_rng(5)
    a = (rng.standard_normal((7, dv.FIXED_FROM)) / 3).astype(LD) * (LD(1) + LD(2) ** -60)
    b = np.asarray(dv.make_vm(dv.FIXED_FROM), dtype=LD)
    plain, fixed = a @ b, dv._times(a, b)
    assert float(np.abs(plain - fixed).max()) <= dv.FIXED_FROM * 2.0 ** -58 * float(np.abs(a).max() * np.abs(b).max())


# ------------------------------------------------------------------------------------------------ 2. the ninth header
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
    assert _declared() == NAMES
    assert not set(_declared()) & (set(test_cabi._declared()) | set(test_pool_header_host._declared())
                                   | set(test_input_grad_host._declared()) | set(test_seq_input_grad_host._declared())
                                   | set(test_pool_input_grad_host._declared()) | set(test_cluster_host._declared())
                                   | set(test_subst_scan_host._declared()) | set(test_indel_scan_host._declared()))


def test_library_exports_every_declared_name():
    bm = _build_module()
    bm.build_extension()
    lib = ctypes.CDLL(bm.LIB)
    for n in _declared():
        assert hasattr(lib, n), f"{n} declared in include/xgpr_hip_subst_var_scan.h but not exported"


def test_ctypes_table_matches_the_header():
    from xgpr_amd import _lib
    assert set(_lib.SUBST_VAR_SCAN_SIGNATURES) == set(_declared())
    assert not set(_lib.SUBST_VAR_SCAN_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.SIZE_FUNCS) | set(_lib.STRING_FUNCS)
                                                      | set(_lib.POOL_SIGNATURES) | set(_lib.INPUT_GRAD_SIGNATURES)
                                                      | set(_lib.SEQ_INPUT_GRAD_SIGNATURES) | set(_lib.POOL_INPUT_GRAD_SIGNATURES)
                                                      | set(_lib.CLUSTER_SIGNATURES) | set(_lib.SUBST_SCAN_SIGNATURES)
                                                      | set(_lib.INDEL_SCAN_SIGNATURES))
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, args in _lib.SUBST_VAR_SCAN_SIGNATURES.items():                        # load() applied the table
        fn = getattr(lib, name)
        assert fn.argtypes == args
        sized = name.endswith("_workspace_bytes")
        assert fn.restype is (ctypes.c_size_t if sized else ctypes.c_int), name
        decl = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)", hdr)                 # the tables' lengths are the parameter counts
        assert len(decl.group(2).split(",")) == len(args), name
        assert decl.group(1) == ("size_t" if sized else "int"), name


def test_every_writer_has_a_memory_contract_row():
    import test_gpu_subst_var_scan_memory_contract as table
    writers = {n for n in _declared() if n.endswith("_f32")}
    assert writers == {"xgpr_conv_token_subst_var_scan_f32"}
    assert table.covered_entry_points() == writers


def test_source_id_covers_the_header_and_the_kernels(tmp_path, monkeypatch):
    bm = _build_module()
    assert os.path.samefile(bm.SUBST_VAR_SCAN_HDR, HEADER) and bm.SUBST_VAR_SCAN_HDR in bm.sources()
    assert "var_scan.inc" in [os.path.basename(p) for p in bm.sources()]
    before = bm.source_id()
    copy = tmp_path / "xgpr_hip_subst_var_scan.h"
    shutil.copyfile(HEADER, copy)
    monkeypatch.setattr(bm, "SUBST_VAR_SCAN_HDR", str(copy))
    assert bm.source_id() == before                                                  # name and contents, not the path
    with open(copy, "a") as f:
        f.write("/* changed */\n")
    assert bm.source_id() != before


# ------------------------------------------------------------------------------------------------ 3. launcher validation
A = 0x100000                     # a dummy 4096-byte-aligned address, never dereferenced on these paths
BIG = 1 << 40
ARRAY_DIMS, ARRAY_SIZES, CONV_WIDTH, RFFS_FREQS, SEQLEN, UNSUPPORTED, WORKSPACE = "ARRAY_DIMS", "ARRAY_SIZES", "CONV_WIDTH", "RFFS_FREQS", \
    "SEQLEN_RANGE", "UNSUPPORTED", "WORKSPACE"


def _codes():
    """The error codes by name, from include/xgpr_hip.h."""
    hdr = open(os.path.join(ROOT, "include", "xgpr_hip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"XGPR_ERR_([A-Z_]+)\s*=?\s*\(?(-\d+)\)?", hdr)}


def scan(tokens=A, table=A, vm=A, stride=None, u=A, q=A, out=A, radem=A, chi=A, lens=(6, 3, 4), seqlen_dev=A, n=3, L=6, vocab=5, C=4, F=40,
         R=64, nvar=16, cw=3, scaling=1, icpt=1, slab=0, ws=A, wb=BIG):
    from xgpr_amd import _lib
    host = np.asarray(lens, dtype=np.int32) if lens is not None else None
    hp = ctypes.c_void_p(host.ctypes.data) if host is not None else None
    rc = _lib.load().xgpr_conv_token_subst_var_scan_f32(tokens, table, vm, nvar if stride is None else stride, u, q, out, radem, chi, hp,
                                                        seqlen_dev, n, L, vocab, C, F, R, nvar, cw, scaling, icpt, slab, ws, wb, None)
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
    "NULL u": (dict(u=None), WORKSPACE),
    "NULL q": (dict(q=None), WORKSPACE),
    "NULL out": (dict(out=None), WORKSPACE),
    "NULL radem": (dict(radem=None), WORKSPACE),
    "NULL chi": (dict(chi=None), WORKSPACE),
    "NULL device lengths": (dict(seqlen_dev=None), WORKSPACE),
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
    "short workspace and NULL out": (dict(wb=8, out=None), WORKSPACE),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_validation_outcome(name):
    kw, code = REFUSALS[name]
    rc, err = scan(**kw)
    assert rc == _codes()[code] and rc < 0, (rc, err)
    assert err
    if "workspace" in name and "NULL" not in name and code == WORKSPACE:
        assert "xgpr_conv_token_subst_var_scan_workspace_bytes" in err
    if name.startswith("NULL"):
        assert err == "NULL array pointer"


def test_the_documented_order_is_the_order_of_the_header():
    """The header's list of checks names the codes in the order REFUSALS walks them."""
    doc = open(HEADER).read()
    doc = doc[doc.index("Checks, before anything is launched"):]
    order = re.findall(r"XGPR_ERR_([A-Z_]+)", doc)
    assert order == [ARRAY_DIMS, CONV_WIDTH, RFFS_FREQS, ARRAY_DIMS, ARRAY_SIZES, ARRAY_DIMS, SEQLEN, ARRAY_DIMS, UNSUPPORTED, WORKSPACE,
                     UNSUPPORTED]


def test_the_position_count_of_one_launch():
    from xgpr_amd import _lib
    n = (1 << 24) // 6 + 1
    lens = np.full(n, 6, dtype=np.int32)
    rc = _lib.load().xgpr_conv_token_subst_var_scan_f32(A, A, A, 16, A, A, A, A, A, ctypes.c_void_p(lens.ctypes.data), A, n, 6, 5, 4, 40, 64,
                                                        16, 3, 1, 1, 0, A, BIG, None)
    assert rc == _codes()[UNSUPPORTED] and "n * L" in _lib.last_error()


def test_no_sequences():
    none = dict(n=0, lens=None, tokens=None, table=None, vm=None, u=None, q=None, out=None, radem=None, chi=None, seqlen_dev=None, ws=None,
                wb=0)
    assert scan(**none)[0] == 0
    assert scan(n=0, lens=None, vocab=257)[0] == _codes()[ARRAY_DIMS]                 # ... but the shape is still checked
    assert scan(n=0, lens=None, nvar=15)[0] == _codes()[ARRAY_DIMS]
    assert scan(n=0, lens=None, vocab=256, C=19)[0] == _codes()[UNSUPPORTED]


def test_workspace_bytes():
    from xgpr_amd import _lib
    lib = _lib.load()
    wsb = lambda R, nvar, slab: int(lib.xgpr_conv_token_subst_var_scan_workspace_bytes(R, nvar, slab))
    masks = int(lib.xgpr_rbf_workspace_bytes(64))
    assert wsb(64, 16, 16) == masks + 16 * 16 * 8 and wsb(64, 16, 48) == masks + 48 * 16 * 8
    sizes = [wsb(64, 130, s) for s in range(16, 16 * 40, 16)]
    assert all(b > a for a, b in zip(sizes, sizes[1:]))                               # monotone in slab_rows
    assert [wsb(64, 16, 8), wsb(64, 16, 24), wsb(64, 16, -16), wsb(64, 15, 16), wsb(64, 0, 16), wsb(0, 16, 16)] == [0] * 6
    for nvar in (2, 16, 130, 512, 2048):                                              # the default: 128 MiB of rows, 16 .. 65536 rows
        rows = (wsb(64, nvar, 0) - masks) // (8 * nvar)
        assert rows % 16 == 0 and rows == min(65536, (128 << 20) // (8 * nvar) // 16 * 16) and wsb(64, nvar, 0) == wsb(64, nvar, rows)
    # the advertised size is the bound the launcher checks
    need = wsb(64, 16, 32)
    assert scan(slab=32, wb=need - 1)[0] == _codes()[WORKSPACE]


def test_ok_predicate():
    from xgpr_amd import _lib
    lib = _lib.load()
    ok = lambda width, vocab, C, F, nvar: int(lib.xgpr_conv_token_subst_var_scan_ok(width, vocab, C, F, nvar))
    assert [ok(1, 1, 1, 1, 2), ok(12, 6, 4, 8, 16), ok(189, 21, 21, 8192, 512), ok(189, 21, 21, 8192, 2048), ok(1008, 5, 21, 1030, 130),
            ok(54, 256, 18, 130, 260)] == [1] * 6
    assert [ok(12, 6, 4, 8, 15), ok(12, 6, 4, 8, 0), ok(12, 6, 4, 8, 18), ok(12, 6, 4, 8, -2), ok(189, 21, 21, 8192, 2050),
            ok(1025, 5, 21, 8, 4), ok(57, 256, 19, 8, 4), ok(12, 6, 4, 0, 2)] == [0] * 8
    for width, vocab, C, F in ((12, 6, 4, 8), (1008, 5, 21, 1030), (1025, 5, 21, 8), (57, 256, 19, 8)):   # the mean scan's predicate
        assert ok(width, vocab, C, F, 2) == int(lib.xgpr_conv_token_subst_scan_ok(width, vocab, C, F))


def test_python_wrappers():
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    assert ext.conv_token_subst_var_scan_ok(189, 21, 21, 8192, 512) == 1 and ext.conv_token_subst_var_scan_ok(189, 21, 21, 8192, 511) == 0
    assert ext.conv_token_subst_var_scan_workspace_bytes(64, 16, 16) == ext._LIB.xgpr_rbf_workspace_bytes(64) + 16 * 16 * 8
    sig = inspect.signature(ext.hipConvTokenSubstVarScan)
    assert list(sig.parameters) == ["tokens", "table", "vm", "u", "q", "out", "radem", "chi", "seqlen", "conv_width", "scaling_type",
                                    "fit_intercept", "slab_rows", "workspace"]
    assert sig.parameters["slab_rows"].default == 0 and sig.parameters["workspace"].default is None
    from xgpr_amd.kernels import ConvSORFKernel
    from xgpr_amd.models import xGPRegression
    assert callable(ConvSORFKernel.substitution_variance_scan) and callable(ConvSORFKernel.substitution_variance_scan_composed)
    sig = inspect.signature(xGPRegression.predict_substitutions)
    assert list(sig.parameters)[:5] == ["self", "input_x", "sequence_lengths", "token_table", "chunk_size"]   # the old positional parameters
    assert sig.parameters["chunk_size"].default == 64 and sig.parameters["get_var"].default is False
    assert "no per-window decomposition" not in xGPRegression.predict_substitutions.__doc__
