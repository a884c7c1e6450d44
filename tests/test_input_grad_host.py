"""The input gradient of a weighted feature sum without a GPU: the dense reference of tests/dense_input_grad.py against central
differences of the dense feature operator; the sensitivity of its a-priori cap to planted structural mistakes; the third public
header, include/xgpr_hip_input_grad.h, held to what tests/test_pool_header_host.py holds the second; and the launcher's argument
validation through the C ABI (no row reaches a HIP call: pointers are dummy integers, as in tests/test_launcher_validation_host.py)."""
import ctypes
import os
import re
import shutil
from math import ceil

import numpy as np
import pytest

import dense_input_grad as dig
import dense_reference as dr
from dense_reference import LD
from test_cabi import _build_module

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "xgpr_hip_input_grad.h")

# ------------------------------------------------------------------------------------------------ 1. central differences
FD_SHAPES = [(3, 37), (9, 40), (100, 300), (20, 1324)]
H = 1e-5


@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "per-row"])
@pytest.mark.parametrize("intercept", [True, False], ids=["intercept", "no-intercept"])
@pytest.mark.parametrize("d,F", FD_SHAPES)
def test_reference_against_central_differences(d, F, intercept, per_row):
    """f(x) = rbf_features(sigma x) . w (w[0] dropped under the intercept) in long double, (f(x + h e_k) - f(x - h e_k)) / 2h.
    Bound, per row and input column k, from f = sum_f c (a_f cos p_f + b_f sin p_f), p_f = sum_k sigma W[f, k] x_k:
      truncation  h^2 / 6 max |d^3 f / d x_k^3| <= h^2 / 6 sum_f c (|a_f| + |b_f|) |sigma W[f, k]|^3
      rounding    each of the two evaluations is off by at most sum_f c (|a_f| + |b_f|) (dp_f + 3 eps) with dp_f the error of the
                  reference's own projection -- three dense products of P + 2 terms each on a vector of norm ||sigma x||_2, times
                  chi_f: dp_f <= 3 (P + 2) eps |chi_f| ||sigma x||_2 -- so the quotient is off by that over h (eps = longdouble's)."""
    n = 2
    xs, w, radem, chi, sigma = dig.make_case(n, d, F, per_row, seed=1)
    x = xs.astype(LD) / LD(sigma)                                       # the unscaled point the differences are taken at
    xs = x * LD(sigma)
    g = dig.rbf_input_grad(xs, w, radem, chi, sigma, intercept)
    wc, ws = dig.split_weights(w, n, F, intercept)
    wfull = np.zeros((n, 2 * F), dtype=LD)
    wfull[:, 0::2], wfull[:, 1::2] = wc, ws

    def f(xp):
        return (dr.rbf_features(xp * LD(sigma), radem, chi, intercept) * wfull).sum(axis=1)

    W = dr.mini_ard_weights(d, radem, chi)
    P = dr.padded_width(d)
    c = dr.rbf_scale(F, intercept)
    amp = c * (np.abs(wc) + np.abs(ws))                                 # [n, F]
    eps = LD(dr.LD_EPS)
    norms = np.sqrt((xs ** 2).sum(axis=1))
    worst = 0.0
    for k in range(d):
        e = np.zeros((1, d), dtype=LD)
        e[0, k] = LD(H)
        fd = (f(x + e) - f(x - e)) / (2 * LD(H))
        trunc = LD(H) ** 2 / 6 * (amp * np.abs(LD(sigma) * W[:, k]) ** 3).sum(axis=1)
        dp = 3 * (P + 2) * eps * np.abs(chi.astype(LD))[None, :] * norms[:, None]
        bound = trunc + (amp * (dp + 3 * eps)).sum(axis=1) / LD(H)
        err = np.abs(fd - g[:, k])
        assert (err <= bound).all(), (k, err, bound)
        worst = max(worst, float((err / bound).max()))
    print(f"input-grad reference vs central differences d={d} F={F} intercept={intercept} per_row={per_row}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("d,F", FD_SHAPES[:3])
def test_row_form_equals_the_product_with_the_weight_matrix(d, F):
    """rbf_input_grad applies S^T to chi (.) u row by row; sigma (u @ mini_ard_weights) is the same number."""
    xs, w, radem, chi, sigma = dig.make_case(3, d, F, True, seed=2)
    a = dig.rbf_input_grad(xs, w, radem, chi, sigma, True)
    b = dig.rbf_input_grad(xs, w, radem, chi, sigma, True, by_weights=True)
    scale = float(np.abs(b).max())
    assert float(np.abs(a - b).max()) <= 64 * (dr.padded_width(d) + F) * dr.LD_EPS * scale


# ------------------------------------------------------------------------------------------------ 2. sensitivity
#            d     F   intercept  per-row
TABLE = [(3, 37, True, False), (9, 40, False, True), (100, 300, True, False), (100, 1324, True, True), (1000, 1300, True, False),
         (1024, 2048, False, False)]


@pytest.mark.parametrize("d,F,intercept,per_row", TABLE)
def test_every_planted_mistake_exceeds_the_cap(d, F, intercept, per_row):
    n = 2
    xs, w, radem, chi, sigma = dig.make_case(n, d, F, per_row, seed=3)
    good = dig.rbf_input_grad(xs, w, radem, chi, sigma, intercept)
    cap = dig.cap_input_grad(xs, w, radem, chi, sigma, intercept)
    assert 0 < cap < 1e-3
    nrep = ceil(F / dr.padded_width(d))
    for mistake in dig.MISTAKES:
        if mistake == "keep_w0" and not intercept:
            continue
        if mistake == "rep0_signs" and nrep < 2:
            continue
        bad = dig.rbf_input_grad(xs, w, radem, chi, sigma, intercept, mistake=mistake)
        diff = float(np.abs(bad - good).max())
        print(f"input-grad sensitivity d={d} F={F} {mistake}: {diff:.3e} against cap {cap:.3e}")
        assert diff > cap, (mistake, diff, cap)


def test_w_cols_limits_the_columns_and_nan_padding_is_never_read():
    xs, w, radem, chi, sigma = dig.make_case(3, 9, 40, True, seed=4, stride_pad=3)
    full = dig.rbf_input_grad(xs, w, radem, chi, sigma, True)
    assert np.isfinite(full.astype(np.float64)).all()
    cut = w.copy()
    cut[:, 10:80] = 0
    a = dig.rbf_input_grad(xs, w, radem, chi, sigma, True, w_cols=10)
    b = dig.rbf_input_grad(xs, cut, radem, chi, sigma, True)
    assert np.array_equal(a, b) and float(np.abs(a - full).max()) > 1e-3


# ------------------------------------------------------------------------------------------------ 3. the third header
def _declared():
    hdr = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(xgpr_[a-z0-9_]+)\s*\(", hdr)))                # the expression of tests/test_cabi.py


def test_the_header_declares_its_two_entry_points_and_nothing_of_the_other_headers():
    import test_cabi
    import test_pool_header_host
    assert _declared() == ["xgpr_rbf_input_grad_f32", "xgpr_rbf_input_grad_ok"]
    assert not set(_declared()) & (set(test_cabi._declared()) | set(test_pool_header_host._declared()))


def test_library_exports_every_declared_name():
    bm = _build_module()
    bm.build_extension()
    lib = ctypes.CDLL(bm.LIB)
    for n in _declared():
        assert hasattr(lib, n), f"{n} declared in include/xgpr_hip_input_grad.h but not exported"


def test_ctypes_table_matches_the_header():
    from xgpr_amd import _lib
    assert set(_lib.INPUT_GRAD_SIGNATURES) == set(_declared())
    assert not set(_lib.INPUT_GRAD_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.SIZE_FUNCS) | set(_lib.STRING_FUNCS)
                                                  | set(_lib.POOL_SIGNATURES))
    lib = _lib.load()
    for name, args in _lib.INPUT_GRAD_SIGNATURES.items():                            # load() applied the table
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype is ctypes.c_int


def test_every_writer_has_a_memory_contract_row():
    import test_gpu_input_grad_memory_contract as table
    writers = {n for n in _declared() if not n.endswith("_workspace_bytes") and not n.endswith("_ok")}      # (_ok: a predicate, no memory)
    assert writers == {"xgpr_rbf_input_grad_f32"}
    covered = table.covered_entry_points()
    assert covered == writers, (sorted(writers - covered), sorted(covered - writers))


def test_source_id_covers_the_header(tmp_path, monkeypatch):
    bm = _build_module()
    assert os.path.samefile(bm.INPUT_GRAD_HDR, HEADER) and bm.INPUT_GRAD_HDR in bm.sources()
    before = bm.source_id()
    copy = tmp_path / "xgpr_hip_input_grad.h"
    shutil.copyfile(HEADER, copy)
    monkeypatch.setattr(bm, "INPUT_GRAD_HDR", str(copy))
    assert bm.source_id() == before                                                  # name and contents, not the path
    with open(copy, "a") as f:
        f.write("/* changed */\n")
    assert bm.source_id() != before


# ------------------------------------------------------------------------------------------------ 4. launcher validation
A = 0x100000                     # a dummy 4096-byte-aligned address, never dereferenced on these paths
BIG = 1 << 30


def call(x=A, w=A, g=A, radem=A, chi=A, n=4, d=60, stride=0, w_cols=128, F=64, R=64, sigma=1.3, icpt=0, ws=A, wb=BIG):
    from xgpr_amd import _lib
    lib = _lib.load()
    rc = lib.xgpr_rbf_input_grad_f32(x, w, g, radem, chi, n, d, stride, w_cols, F, R, sigma, icpt, ws, wb, None)
    return int(rc), _lib.last_error()


UNSUPPORTED, WORKSPACE, ARRAY_DIMS, ODD_OUTPUT, RFFS_FREQS, ARRAY_SIZES = -20, -21, -8, -2, -3, -4

VALIDATION = {
    "padded width 2048": (dict(d=1025, F=2048, R=2048, w_cols=4096), UNSUPPORTED, "padded width > 1024 on this wave-tile kernel"),
    "short workspace": (dict(wb=8), WORKSPACE, "workspace too small (see xgpr_rbf_workspace_bytes)"),
    "no workspace": (dict(ws=None), WORKSPACE, "workspace too small (see xgpr_rbf_workspace_bytes)"),
    "odd w_cols": (dict(w_cols=127), ODD_OUTPUT, "w_cols must be an even number >= 2"),
    "w_cols 0": (dict(w_cols=0), ODD_OUTPUT, "w_cols must be an even number >= 2"),
    "w_cols beyond the features": (dict(w_cols=130), ARRAY_SIZES, "w_cols exceeds the number of features"),
    "short stride": (dict(stride=126), ARRAY_SIZES, "w_row_stride is shorter than w_cols"),
    "n < 0": (dict(n=-1), ARRAY_DIMS, "incorrect array dims passed"),
    "d < 1": (dict(d=0), ARRAY_DIMS, "incorrect array dims passed"),
    "more frequencies than signs": (dict(F=65, w_cols=130), RFFS_FREQS, "incorrect number of rffs and or freqs."),
    "signs not whole transforms": (dict(R=96), RFFS_FREQS, "incorrect number of rffs and or freqs."),
    "NULL weights": (dict(w=None), WORKSPACE, "NULL array pointer"),
    # two failing checks at once: the first in the documented order is the one reported
    "n < 0 and odd w_cols": (dict(n=-1, w_cols=127), ARRAY_DIMS, "incorrect array dims passed"),
    "odd w_cols and short workspace": (dict(w_cols=127, wb=8), ODD_OUTPUT, "w_cols must be an even number >= 2"),
    "too wide and short workspace": (dict(d=1025, F=2048, R=2048, w_cols=4096, wb=8), UNSUPPORTED,
                                     "padded width > 1024 on this wave-tile kernel"),
}


@pytest.mark.parametrize("name", sorted(VALIDATION))
def test_validation_outcome(name):
    kw, code, msg = VALIDATION[name]
    assert call(**kw) == (code, msg)


def test_no_datapoints_is_a_no_op():
    assert call(n=0)[0] == 0
    assert call(n=0, ws=None, wb=0)[0] == 0                       # nothing to launch: no workspace needed either
    assert call(n=0, w_cols=127)[0] == ODD_OUTPUT                 # ... but the arguments are still checked


def test_workspace_bound_is_the_advertised_size():
    from xgpr_amd import _lib
    need = int(_lib.load().xgpr_rbf_workspace_bytes(64))
    assert call(wb=need - 1)[0] == WORKSPACE


def test_ok_predicate():
    from xgpr_amd import _lib
    lib = _lib.load()
    assert [int(lib.xgpr_rbf_input_grad_ok(d, 64)) for d in (2, 3, 1024)] == [1, 1, 1]
    assert int(lib.xgpr_rbf_input_grad_ok(1025, 64)) == 0
    assert int(lib.xgpr_rbf_input_grad_ok(1, 64)) == 1 and int(lib.xgpr_rbf_input_grad_ok(0, 64)) == 0
