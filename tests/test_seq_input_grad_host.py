"""The input gradient of the sequence / graph kernels' weighted feature sum without a GPU: the dense reference of
tests/dense_seq_input_grad.py against central differences of the dense convolution feature operator; exact zeros past each length; the
sensitivity of its a-priori cap to planted structural mistakes; the fourth public header, include/xgpr_hip_seq_input_grad.h, held to
what tests/test_input_grad_host.py holds the third; and the launchers' argument validation through the C ABI (no sequence reaches a HIP
call: device pointers are dummy integers, as in tests/test_launcher_validation_host.py; the host lengths are real)."""
import ctypes
import os
import re
import shutil

import numpy as np
import pytest

import dense_reference as dr
import dense_seq_input_grad as dsg
from dense_reference import LD
from test_cabi import _build_module

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "xgpr_hip_seq_input_grad.h")
NAMES = ["xgpr_conv_input_grad_f32", "xgpr_conv_input_grad_ok", "xgpr_conv_token_input_grad_f32", "xgpr_conv_token_input_grad_ok"]

# ------------------------------------------------------------------------------------------------ 1. central differences
#             n  L  C  cw  F  scaling intercept
FD_SHAPES = [(3, 7, 3, 3, 37, 1, True), (2, 6, 2, 1, 20, 2, False), (2, 9, 5, 4, 70, 0, True)]
H = 1e-4


def _zeroed_w0(w, intercept):
    w = np.array(w, dtype=LD)
    if intercept:
        w[..., 0] = 0
    return w


@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "per-row"])
@pytest.mark.parametrize("n,L,C,cw,F,scaling,intercept", FD_SHAPES)
def test_reference_against_central_differences(n, L, C, cw, F, scaling, intercept, per_row):
    """f(x) = conv_features(sigma x) . w (w[0] dropped under the intercept) in long double, (f(x + h e) - f(x - h e)) / 2h for every
    position and channel.  f = sum_j sum_f r (a_f cos p_jf + b_f sin p_jf) with p_jf = sum_k sigma W[f, k] win_j[k]; x[l, c] is
    element k_j = (l - j) C + c of the windows j that cover l, and the windows enter f additively.  Bound, per sequence:
      truncation  h^2 / 6 max |d^3 f / d x[l, c]^3| <= h^2 / 6 sum_{j covers l} sum_f r (|a_f| + |b_f|) |sigma W[f, k_j]|^3
      rounding    each of the two evaluations is off by at most sum_f r (|a_f| + |b_f|) (sum_j (dp_jf + 3 eps) + nk (nk + 2 F) eps):
                  dp_jf <= 3 (P + 2) eps |chi_f| ||window j||_2 the error of the reference's own projection (three dense products of
                  P + 2 terms), 3 eps for cos / sin and the product with r, nk eps per term for the sum of nk terms over the k-mers
                  and 2 F eps per term for the product with w -- so the quotient is off by that over h (eps = longdouble's)."""
    xs, seqlen, w, radem, chi, sigma = dsg.make_case(n, L, C, cw, F, per_row, seed=1)
    x = xs.astype(LD) / LD(sigma)                                       # the unscaled point the differences are taken at
    xs = x * LD(sigma)
    g = dsg.seq_input_grad(xs, seqlen, w, radem, chi, sigma, cw, scaling, intercept)
    w0 = _zeroed_w0(w if per_row else np.broadcast_to(w, (n, 2 * F)), intercept)[:, :2 * F]

    def f(xp):
        return (dr.conv_features(xp * LD(sigma), seqlen, radem, chi, cw, scaling) * w0).sum(axis=1)

    W = dr.mini_ard_weights(cw * C, radem, chi)                         # [F, cw C]
    P = dr.padded_width(cw * C)
    eps = LD(dr.LD_EPS)
    chia = np.abs(chi.astype(LD))
    worst = 0.0
    for i in range(n):
        nk = int(seqlen[i]) - cw + 1
        amp = dr.conv_row_scale(F, nk, scaling) * (np.abs(w0[i, 0::2]) + np.abs(w0[i, 1::2]))      # [F]
        wn = np.sqrt((dr._windows(xs[i], seqlen[i], cw) ** 2).sum(axis=1))                         # [nk]
        rounding = (amp * (3 * (P + 2) * eps * chia * wn.sum() + nk * 3 * eps + nk * (nk + 2 * F) * eps)).sum() / LD(H)
        for l in range(L):
            for c in range(C):
                e = np.zeros((n, L, C), dtype=LD)
                e[i, l, c] = LD(H)
                fd = ((f(x + e) - f(x - e)) / (2 * LD(H)))[i]
                trunc = LD(0)
                for j in range(max(0, l - cw + 1), min(l, nk - 1) + 1):
                    trunc += LD(H) ** 2 / 6 * (amp * np.abs(LD(sigma) * W[:, (l - j) * C + c]) ** 3).sum()
                bound = trunc + rounding
                err = abs(fd - g[i, l, c])
                assert err <= bound, (i, l, c, err, bound)
                if l < seqlen[i]:
                    worst = max(worst, float(err / bound))
    print(f"seq input-grad reference vs central differences {(n, L, C, cw, F, scaling, intercept)} per_row={per_row}: "
          f"worst error / bound {worst:.3f}")


def test_positions_past_the_length_are_exactly_zero():
    xs, seqlen, w, radem, chi, sigma = dsg.make_case(4, 9, 3, 3, 37, True, seed=2)
    assert (seqlen < 9).any()
    g = dsg.seq_input_grad(xs, seqlen, w, radem, chi, sigma, 3, 1, True)
    for i, s in enumerate(seqlen):
        assert (g[i, s:] == 0).all() and (np.abs(g[i, :s]).max(axis=1) > 0).all()


# ------------------------------------------------------------------------------------------------ 2. sensitivity
#         n   L   C  cw   F  scaling intercept
TABLE = [(3, 7, 3, 3, 37, 1, True), (2, 6, 2, 1, 20, 2, False), (2, 9, 5, 4, 70, 0, True), (2, 40, 21, 9, 64, 1, True),
         (3, 12, 21, 9, 300, 1, True), (2, 8, 4, 3, 1100, 2, True)]


@pytest.mark.parametrize("n,L,C,cw,F,scaling,intercept", TABLE)
def test_every_planted_mistake_exceeds_the_cap(n, L, C, cw, F, scaling, intercept):
    """Each mistake where it applies: keep_w0 under the intercept and at F <= 300 ONLY (w[0]'s share of the gradient shrinks with
    1 / sqrt(F): measured 1867 x / 83 x / 7.1 x the cap at F = 37 / 64 / 300 in this table; at F = 1100 it can fall below the cap and is
    not asserted); no_norm and
    norm_by_L at scaling != 0 (norm_by_L needs a sequence shorter than L); last_only at conv_width > 1; transpose_window at
    conv_width > 1 and C > 1."""
    xs, seqlen, w, radem, chi, sigma = dsg.make_case(n, L, C, cw, F, False, seed=3, lengths=[L - 1, max(cw + 1, L // 2), L])
    good = dsg.seq_input_grad(xs, seqlen, w, radem, chi, sigma, cw, scaling, intercept)
    cap = dsg.cap_seq_input_grad(xs, seqlen, w, radem, chi, sigma, cw, scaling, intercept)
    assert 0 < cap < 1e-3
    applies = {"keep_w0": intercept and F <= 300, "no_norm": scaling != 0, "norm_by_L": scaling != 0 and (seqlen < L).any(),
               "shift": True, "last_only": cw > 1, "transpose_window": cw > 1 and C > 1}
    assert set(applies) == set(dsg.MISTAKES)
    for mistake in dsg.MISTAKES:
        if not applies[mistake]:
            continue
        bad = dsg.seq_input_grad(xs, seqlen, w, radem, chi, sigma, cw, scaling, intercept, mistake=mistake)
        diff = float(np.abs(bad - good).max())
        print(f"seq input-grad sensitivity {(n, L, C, cw, F, scaling)} {mistake}: {diff:.3e} against cap {cap:.3e} ({diff / cap:.1f} x)")
        assert diff > cap, (mistake, diff, cap)


# ------------------------------------------------------------------------------------------------ 3. the fourth header
def _declared():
    hdr = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(xgpr_[a-z0-9_]+)\s*\(", hdr)))                # the expression of tests/test_cabi.py


def test_the_header_declares_its_four_entry_points_and_nothing_of_the_other_headers():
    import test_cabi
    import test_input_grad_host
    import test_pool_header_host
    assert _declared() == NAMES
    assert not set(_declared()) & (set(test_cabi._declared()) | set(test_pool_header_host._declared()) | set(test_input_grad_host._declared()))


def test_library_exports_every_declared_name():
    bm = _build_module()
    bm.build_extension()
    lib = ctypes.CDLL(bm.LIB)
    for n in _declared():
        assert hasattr(lib, n), f"{n} declared in include/xgpr_hip_seq_input_grad.h but not exported"


def test_ctypes_table_matches_the_header():
    from xgpr_amd import _lib
    assert set(_lib.SEQ_INPUT_GRAD_SIGNATURES) == set(_declared())
    assert not set(_lib.SEQ_INPUT_GRAD_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.SIZE_FUNCS) | set(_lib.STRING_FUNCS)
                                                      | set(_lib.POOL_SIGNATURES) | set(_lib.INPUT_GRAD_SIGNATURES))
    lib = _lib.load()
    for name, args in _lib.SEQ_INPUT_GRAD_SIGNATURES.items():                        # load() applied the table
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype is ctypes.c_int
    # the tables' lengths are the headers' parameter counts
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, args in _lib.SEQ_INPUT_GRAD_SIGNATURES.items():
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert len(params.split(",")) == len(args), name


def test_every_writer_has_a_memory_contract_row():
    import test_gpu_seq_input_grad_memory_contract as table
    writers = {n for n in _declared() if not n.endswith("_workspace_bytes") and not n.endswith("_ok")}      # (_ok: predicates, no memory)
    assert writers == {"xgpr_conv_input_grad_f32", "xgpr_conv_token_input_grad_f32"}
    covered = table.covered_entry_points()
    assert covered == writers, (sorted(writers - covered), sorted(covered - writers))


def test_source_id_covers_the_header(tmp_path, monkeypatch):
    bm = _build_module()
    assert os.path.samefile(bm.SEQ_INPUT_GRAD_HDR, HEADER) and bm.SEQ_INPUT_GRAD_HDR in bm.sources()
    before = bm.source_id()
    copy = tmp_path / "xgpr_hip_seq_input_grad.h"
    shutil.copyfile(HEADER, copy)
    monkeypatch.setattr(bm, "SEQ_INPUT_GRAD_HDR", str(copy))
    assert bm.source_id() == before                                                  # name and contents, not the path
    with open(copy, "a") as f:
        f.write("/* changed */\n")
    assert bm.source_id() != before


# ------------------------------------------------------------------------------------------------ 4. launcher validation
A = 0x100000                     # a dummy 4096-byte-aligned address, never dereferenced on these paths
BIG = 1 << 30
LENS = (10, 11, 12, 12)


def call(token=False, x=A, tokens=A, w=A, g=A, radem=A, chi=A, lens=LENS, dev=A, n=4, L=12, vocab=24, C=6, stride=0, w_cols=128, F=64,
         R=64, sigma=1.3, cw=10, scaling=1, icpt=0, ws=A, wb=BIG):
    """Defaults: windows of 10 x 6 = 60 elements (padded width 64), 64 frequencies, four sequences of lengths 10 .. 12."""
    from xgpr_amd import _lib
    lib = _lib.load()
    host = None if lens is None else np.asarray(lens, dtype=np.int32)
    hp = None if host is None else host.ctypes.data
    tail = (n, L) + ((vocab,) if token else ()) + (C, stride, w_cols, F, R, sigma, cw, scaling, icpt, ws, wb, None)
    if token:
        rc = lib.xgpr_conv_token_input_grad_f32(tokens, x, w, g, radem, chi, hp, dev, *tail)
    else:
        rc = lib.xgpr_conv_input_grad_f32(x, w, g, radem, chi, hp, dev, *tail)
    return int(rc), _lib.last_error()


UNSUPPORTED, WORKSPACE, ARRAY_DIMS, ODD_OUTPUT, RFFS_FREQS, ARRAY_SIZES, CONV_WIDTH, SEQLEN_RANGE = -20, -21, -8, -2, -3, -4, -6, -7
TOO_WIDE = "padded width > 1024 on this wave-tile kernel"
TOKEN_REFUSED = ("token input serves windows of up to 1024 elements and tables of up to 4608 floats "
                 "(see xgpr_conv_token_input_grad_ok)")
SEQ_RANGE = "All sequence lengths must be >= conv width and < array size."
WIDE = dict(L=200, C=6, cw=171, lens=(171, 180, 200, 200), F=2048, R=2048, w_cols=4096)      # 1026 elements: padded width 2048

VALIDATION = {
    "n < 0": (dict(n=-1), ARRAY_DIMS, "incorrect array dims passed"),
    "L < 1": (dict(L=0), ARRAY_DIMS, "incorrect array dims passed"),
    "C < 1": (dict(C=0), ARRAY_DIMS, "incorrect array dims passed"),
    "scaling type 3": (dict(scaling=3), ARRAY_DIMS, "scaling_type must be 0, 1 or 2"),
    "conv_width 0": (dict(cw=0), CONV_WIDTH, "invalid conv_width"),
    "conv_width > L": (dict(cw=13), CONV_WIDTH, "invalid conv_width"),
    "more frequencies than signs": (dict(F=65, w_cols=130), RFFS_FREQS, "incorrect number of rffs and or freqs."),
    "signs not whole transforms": (dict(R=96), RFFS_FREQS, "incorrect number of rffs and or freqs."),
    "odd w_cols": (dict(w_cols=127), ODD_OUTPUT, "w_cols must be an even number >= 2"),
    "w_cols 0": (dict(w_cols=0), ODD_OUTPUT, "w_cols must be an even number >= 2"),
    "w_cols beyond the features": (dict(w_cols=130), ARRAY_SIZES, "w_cols exceeds the number of features"),
    "short stride": (dict(stride=126), ARRAY_SIZES, "w_row_stride is shorter than w_cols"),
    "a length below conv_width": (dict(lens=(10, 9, 12, 12)), SEQLEN_RANGE, SEQ_RANGE),
    "a length beyond L": (dict(lens=(10, 11, 12, 13)), SEQLEN_RANGE, SEQ_RANGE),
    "no host lengths": (dict(lens=None), SEQLEN_RANGE, "seqlen_host is required (sequence lengths are validated on the host)"),
    "padded width 2048": (WIDE, UNSUPPORTED, TOO_WIDE),
    "short workspace": (dict(wb=8), WORKSPACE, "workspace too small (see xgpr_rbf_workspace_bytes)"),
    "no workspace": (dict(ws=None), WORKSPACE, "workspace too small (see xgpr_rbf_workspace_bytes)"),
    "NULL weights": (dict(w=None), WORKSPACE, "NULL array pointer"),
    "NULL device lengths": (dict(dev=None), WORKSPACE, "NULL array pointer"),
    "token: vocab 0": (dict(token=True, vocab=0), ARRAY_DIMS, "token table: vocab must be 1 .. 256 (uint8 tokens)"),
    "token: vocab 257": (dict(token=True, vocab=257), ARRAY_DIMS, "token table: vocab must be 1 .. 256 (uint8 tokens)"),
    "token: table of 4617 floats": (dict(token=True, vocab=243, C=19, cw=3, lens=(3, 11, 12, 12), F=64, R=64), UNSUPPORTED, TOKEN_REFUSED),
    "token: padded width 2048": (dict(token=True, vocab=4, **WIDE), UNSUPPORTED, TOKEN_REFUSED),
    "token: NULL tokens": (dict(token=True, tokens=None), WORKSPACE, "NULL array pointer"),
    # two failing checks at once: the first in the documented order is the one reported
    "n < 0 and conv_width 0": (dict(n=-1, cw=0), ARRAY_DIMS, "incorrect array dims passed"),
    "conv_width 0 and odd w_cols": (dict(cw=0, w_cols=127), CONV_WIDTH, "invalid conv_width"),
    "bad frequencies and odd w_cols": (dict(R=96, w_cols=127), RFFS_FREQS, "incorrect number of rffs and or freqs."),
    "odd w_cols and short stride": (dict(w_cols=127, stride=3), ODD_OUTPUT, "w_cols must be an even number >= 2"),
    "short stride and a bad length": (dict(stride=126, lens=(1, 11, 12, 12)), ARRAY_SIZES, "w_row_stride is shorter than w_cols"),
    "a bad length and too wide": (dict(WIDE, lens=(170, 180, 200, 200)), SEQLEN_RANGE, SEQ_RANGE),
    "token: a bad length and vocab 0": (dict(token=True, vocab=0, lens=(1, 11, 12, 12)), SEQLEN_RANGE, SEQ_RANGE),
    "token: vocab 0 and too wide": (dict(token=True, **dict(WIDE, vocab=0)), ARRAY_DIMS, "token table: vocab must be 1 .. 256 (uint8 tokens)"),
    "too wide and short workspace": (dict(WIDE, wb=8), UNSUPPORTED, TOO_WIDE),
    "short workspace and NULL weights": (dict(wb=8, w=None), WORKSPACE, "workspace too small (see xgpr_rbf_workspace_bytes)"),
}


@pytest.mark.parametrize("name", sorted(VALIDATION))
def test_validation_outcome(name):
    kw, code, msg = VALIDATION[name]
    assert call(**kw) == (code, msg)
    if "token" not in kw and code not in (UNSUPPORTED,):                 # the token form makes the same checks
        assert call(token=True, **kw) == (code, msg)


def test_no_datapoints_is_a_no_op():
    for token in (False, True):
        assert call(token=token, n=0, lens=())[0] == 0
        assert call(token=token, n=0, lens=None, ws=None, wb=0)[0] == 0       # nothing to launch: no lengths, no workspace needed
        assert call(token=token, n=0, lens=(), w_cols=127)[0] == ODD_OUTPUT   # ... but the arguments are still checked
        assert call(token=token, n=0, lens=(), **{k: v for k, v in WIDE.items() if k != "lens"})[0] == UNSUPPORTED


def test_workspace_bound_is_the_advertised_size():
    from xgpr_amd import _lib
    need = int(_lib.load().xgpr_rbf_workspace_bytes(64))
    assert call(wb=need - 1)[0] == WORKSPACE and call(token=True, wb=need - 1)[0] == WORKSPACE


def test_ok_predicates():
    from xgpr_amd import _lib
    lib = _lib.load()
    assert [int(lib.xgpr_conv_input_grad_ok(d, 64)) for d in (1, 2, 189, 1024)] == [1, 1, 1, 1]
    assert int(lib.xgpr_conv_input_grad_ok(1025, 64)) == 0 and int(lib.xgpr_conv_input_grad_ok(0, 64)) == 0
    assert int(lib.xgpr_conv_token_input_grad_ok(189, 21, 21)) == 1
    assert int(lib.xgpr_conv_token_input_grad_ok(9 * 19, 243, 19)) == 0          # 4617 floats: more than the LDS image holds
    assert int(lib.xgpr_conv_token_input_grad_ok(1026, 4, 6)) == 0               # padded width 2048
    assert int(lib.xgpr_conv_token_input_grad_ok(190, 21, 21)) == 0              # not whole positions
