"""The backward of the two-layer kernel's first layer without a GPU: the dense reference of tests/dense_pool_input_grad.py against
central differences of the dense max-pool operator; exact ties go to the first window; the share of ambiguous (sequence, filter)
pairs at the shapes the GPU tests exclude them at; the sensitivity of the a-priori cap to planted structural mistakes; the fifth
public header, include/xgpr_hip_pool_input_grad.h, held to what tests/test_seq_input_grad_host.py holds the fourth; the launchers'
argument validation through the C ABI (no sequence reaches a HIP call: device pointers are dummy integers); and the Linear kernel's
input gradient on the CPU device."""
import ctypes
import os
import re
import shutil

import numpy as np
import pytest

import dense_pool_input_grad as dpg
import dense_reference as dr
from dense_reference import LD
from test_cabi import _build_module

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "xgpr_hip_pool_input_grad.h")
NAMES = ["xgpr_conv_maxpool_input_grad_f32", "xgpr_conv_maxpool_input_grad_ok", "xgpr_conv_token_maxpool_input_grad_f32",
         "xgpr_conv_token_maxpool_input_grad_ok"]

# ------------------------------------------------------------------------------------------------ 1. central differences
#             n  L  C  cw  F   lengths
FD_SHAPES = [(3, 7, 3, 3, 37, [7, 3, 5]),         # nk = 5, 1 (a single window), 3
             (2, 6, 2, 1, 20, [6, 4]),            # conv_width 1: no overlap
             (2, 9, 5, 4, 70, [6, 9])]            # nk = 3 < conv_width, and 6
H = 1e-4


@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "per-row"])
@pytest.mark.parametrize("n,L,C,cw,F,lengths", FD_SHAPES)
def test_reference_against_central_differences(n, L, C, cw, F, lengths, per_row):
    """m(x) = sum_f g_f conv_maxpool(x)_f in long double is piecewise linear in x.  A step of h in one input element moves a
    projection p[j, f] by at most h max_k |W1[f, k]| <= h ||W1 row f||_1, so with g zeroed at the filters whose gap -- or whose
    distance of the maximum from the ReLU's kink at 0 -- is below 4 h max_f ||W1 row f||_1 the winner and its side of the ReLU do not
    change within [x - h, x + h], m is linear there and the central difference is exact up to the rounding of the two evaluations:
    each is off by at most sum_f |g_f| 3 (P + 2) eps |chi_f| max_j ||window j||_2 (the reference's own projection: three dense products
    of P + 2 terms) plus F eps sum_f |g_f q_f| for the sum -- over h (eps = longdouble's)."""
    x32, seqlen, g, radem, chi = dpg.make_case(n, L, C, cw, F, per_row, seed=1, lengths=lengths)
    x = x32.astype(LD)
    W = dr.mini_ard_weights(cw * C, radem, chi)                         # [F, cw C]
    thresh = 4 * H * float(np.abs(W).sum(axis=1).max())
    proj = dr.conv_projections(x, seqlen, radem, chi, cw)
    gz = np.array(np.broadcast_to(np.asarray(g, dtype=LD)[..., :F], (n, F)))
    kept = 0
    for i in range(n):
        _, gap, top = dpg.argmax_and_gap(proj[i], ids=dpg.window_ids(x[i], seqlen[i], cw))
        safe = (gap >= thresh) & (np.abs(top.astype(np.float64)) >= thresh)
        gz[i] = np.where(safe, gz[i], LD(0))
        kept += int(safe.sum())
    assert kept > 0.8 * n * F                                           # the exclusion removes a margin, not the test
    grad, amax, _ = dpg.pool_input_grad(x, seqlen, gz, radem, chi, cw, proj=proj)
    assert (amax >= 0).any() and ((amax < 0).any() or min(lengths) > cw)       # a single window leaves about half the filters inactive

    def m(xp):
        return (dr.conv_maxpool(xp, seqlen, radem, chi, cw)[1] * gz).sum(axis=1)

    P = dr.padded_width(cw * C)
    eps = LD(dr.LD_EPS)
    chia = np.abs(chi.astype(LD))
    q = dr.conv_maxpool(x, seqlen, radem, chi, cw, proj=proj)[1]
    worst = 0.0
    for i in range(n):
        wn = np.sqrt((dr._windows(x[i], seqlen[i], cw) ** 2).sum(axis=1)).max() + LD(H)
        bound = ((np.abs(gz[i]) * 3 * (P + 2) * eps * chia * wn).sum() + F * eps * np.abs(gz[i] * q[i]).sum()) / LD(H)
        for l in range(L):
            for c in range(C):
                e = np.zeros((n, L, C), dtype=LD)
                e[i, l, c] = LD(H)
                fd = ((m(x + e) - m(x - e)) / (2 * LD(H)))[i]
                err = abs(fd - grad[i, l, c])
                assert err <= bound, (i, l, c, err, bound)
                worst = max(worst, float(err / bound))
        assert (grad[i, int(seqlen[i]):] == 0).all()
    print(f"pool input-grad reference vs central differences {(n, L, C, cw, F)} per_row={per_row}: worst error / bound {worst:.3f}, "
          f"{kept} of {n * F} pairs kept")


# ------------------------------------------------------------------------------------------------ 2. ties
def periodic_case(L=6, period=2, cw=2, V=5, C=3, F=37, seed=5):
    """Tokens of period ``period`` over a random table: windows j and j + period are identical, so their projections tie exactly."""
    from scipy.stats import chi as chi_dist
    rng = np.random.default_rng(seed)
    table = rng.standard_normal((V, C)).astype(np.float32)
    tokens = np.tile(rng.permutation(V)[:period], L // period + 1)[:L][None, :].astype(np.uint8)
    P = dr.padded_width(cw * C)
    R = -(-F // P) * P
    radem = rng.choice(np.asarray([-1, 1], dtype=np.int8), size=(3, 1, R))
    chi = chi_dist.rvs(df=P, size=F, random_state=rng).astype(np.float32)
    return tokens, table, np.asarray([L], dtype=np.int32), rng.standard_normal(F), radem, chi


def test_exact_ties_go_to_the_first_window():
    """conv_width 2 over "ABABAB": windows 0, 2, 4 are identical, and 1, 3.  Every active argmax lies below the period, and the
    positions no winning window covers -- at or beyond period + conv_width - 1 -- are exactly 0."""
    tokens, table, seqlen, g, radem, chi = periodic_case()
    x = table[tokens]
    grad, amax, gap = dpg.pool_input_grad(x, seqlen, g, radem, chi, 2)
    assert (amax >= 0).any() and (amax[amax >= 0] < 2).all()
    assert (grad[0, 3:] == 0).all() and (np.abs(grad[0, :3]).max(axis=1) > 0).all()
    _, last, _ = dpg.pool_input_grad(x, seqlen, g, radem, chi, 2, mistake="last_argmax")
    assert (last[last >= 0] >= 3).all()                                 # the planted rule picks the other end of the tie


# ------------------------------------------------------------------------------------------------ 3. the ambiguous share
AMBIGUOUS_CASES = [(5, 12, 4, 3, 37), (3, 40, 21, 9, 300), (2, 20, 2, 1, 64), (2, 70, 16, 64, 1100)]


@pytest.mark.parametrize("one_hot", [False, True], ids=["gaussian", "one-hot"])
@pytest.mark.parametrize("n,L,C,cw,F", AMBIGUOUS_CASES)
def test_ambiguous_share_is_at_most_five_percent(n, L, C, cw, F, one_hot):
    """The share of pairs whose runner-up lies within twice the forward operator's float32 cap of the maximum (the gap to the largest
    strictly smaller projection), or whose maximum lies within that cap of 0, on the long-double reference alone; the seed is fixed
    so that the committed cases hold the 5 % (1 to 14 of the 185 pairs of the small one-hot case over the seeds 5 .. 11).
    One-hot rows over a few letters ALSO produce different windows whose projections coincide exactly in long double -- the same
    +-chi terms summed in another order --, which a float32 operator rounds apart either way (measured on the device: the forward
    operator itself returns 1.4449282 and 1.4449284 for two such windows).  ``ambiguous`` counts those too unless told to be literal;
    the GPU tests, whose operator cases draw Gaussian rows, assert the 5 % on that wider set.  Printed here, not asserted: 21 % and
    25 % of the pairs at the two small one-hot shapes."""
    x, seqlen, g, radem, chi = dpg.make_case(n, L, C, cw, F, False, seed=11, one_hot=one_hot)
    proj = dr.conv_projections(x.astype(LD), seqlen, radem, chi, cw)
    amb = dpg.ambiguous(x, seqlen, radem, chi, cw, proj=proj, literal=True)
    wider = dpg.ambiguous(x, seqlen, radem, chi, cw, proj=proj)
    print(f"ambiguous pairs {(n, L, C, cw, F)} one_hot={one_hot}: {int(amb.sum())} of {amb.size}; with coinciding windows {int(wider.sum())}")
    assert amb.mean() <= 0.05 and (wider | ~amb).all()
    if not one_hot:
        assert wider.mean() <= 0.05


# ------------------------------------------------------------------------------------------------ 4. sensitivity
#         n   L   C  cw   F
TABLE = [(3, 7, 3, 3, 37), (2, 6, 2, 1, 20), (2, 9, 5, 4, 70), (2, 40, 21, 9, 64), (3, 12, 21, 9, 300), (2, 8, 4, 3, 1100)]


@pytest.mark.parametrize("n,L,C,cw,F", TABLE)
def test_every_planted_mistake_exceeds_the_cap(n, L, C, cw, F):
    """Each mistake where it applies: last_argmax changes nothing without exact ties and is asserted on the periodic tokens below;
    transpose_window at conv_width > 1 and C > 1; every other one everywhere (every sequence has more than one k-mer here)."""
    x, seqlen, g, radem, chi = dpg.make_case(n, L, C, cw, F, False, seed=3, lengths=[L - 1, max(cw + 1, L // 2), L])
    good, amax, _ = dpg.pool_input_grad(x, seqlen, g, radem, chi, cw)
    cap = dpg.cap_pool_input_grad(g, amax, seqlen, chi, cw, C)
    assert 0 < cap < 1e-3 * float(np.abs(good).max())
    applies = {"last_argmax": False, "no_relu": (amax < 0).any(), "argmax_of_abs": True, "shift": True, "forward_sign_order": True,
               "transpose_window": cw > 1 and C > 1, "all_windows": True}
    assert set(applies) == set(dpg.MISTAKES)
    for mistake in dpg.MISTAKES:
        if not applies[mistake]:
            continue
        bad = dpg.pool_input_grad(x, seqlen, g, radem, chi, cw, mistake=mistake)[0]
        diff = float(np.abs(bad - good).max())
        print(f"pool input-grad sensitivity {(n, L, C, cw, F)} {mistake}: {diff:.3e} against cap {cap:.3e} ({diff / cap:.1f} x)")
        assert diff > cap, (mistake, diff, cap)


def test_last_argmax_exceeds_the_cap_on_ties():
    tokens, table, seqlen, g, radem, chi = periodic_case()
    x = table[tokens]
    good, amax, _ = dpg.pool_input_grad(x, seqlen, g, radem, chi, 2)
    bad = dpg.pool_input_grad(x, seqlen, g, radem, chi, 2, mistake="last_argmax")[0]
    assert float(np.abs(bad - good).max()) > dpg.cap_pool_input_grad(g, amax, seqlen, chi, 2, table.shape[1])


# ------------------------------------------------------------------------------------------------ 5. the fifth header
def _declared():
    hdr = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(xgpr_[a-z0-9_]+)\s*\(", hdr)))                # the expression of tests/test_cabi.py


def test_the_header_declares_its_four_entry_points_and_nothing_of_the_other_headers():
    import test_cabi
    import test_input_grad_host
    import test_pool_header_host
    import test_seq_input_grad_host
    assert _declared() == NAMES
    assert not set(_declared()) & (set(test_cabi._declared()) | set(test_pool_header_host._declared())
                                   | set(test_input_grad_host._declared()) | set(test_seq_input_grad_host._declared()))


def test_library_exports_every_declared_name():
    bm = _build_module()
    bm.build_extension()
    lib = ctypes.CDLL(bm.LIB)
    for n in _declared():
        assert hasattr(lib, n), f"{n} declared in include/xgpr_hip_pool_input_grad.h but not exported"


def test_ctypes_table_matches_the_header():
    from xgpr_amd import _lib
    assert set(_lib.POOL_INPUT_GRAD_SIGNATURES) == set(_declared())
    assert not set(_lib.POOL_INPUT_GRAD_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.SIZE_FUNCS) | set(_lib.STRING_FUNCS)
                                                       | set(_lib.POOL_SIGNATURES) | set(_lib.INPUT_GRAD_SIGNATURES)
                                                       | set(_lib.SEQ_INPUT_GRAD_SIGNATURES))
    lib = _lib.load()
    for name, args in _lib.POOL_INPUT_GRAD_SIGNATURES.items():                       # load() applied the table
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype is ctypes.c_int
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, args in _lib.POOL_INPUT_GRAD_SIGNATURES.items():                       # the tables' lengths are the parameter counts
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert len(params.split(",")) == len(args), name


def test_every_writer_has_a_memory_contract_row():
    import test_gpu_pool_input_grad_memory_contract as table
    writers = {n for n in _declared() if not n.endswith("_ok")}                      # (_ok: predicates, no memory)
    assert writers == {"xgpr_conv_maxpool_input_grad_f32", "xgpr_conv_token_maxpool_input_grad_f32"}
    covered = table.covered_entry_points()
    assert covered == writers, (sorted(writers - covered), sorted(covered - writers))


def test_source_id_covers_the_header(tmp_path, monkeypatch):
    bm = _build_module()
    assert os.path.samefile(bm.POOL_INPUT_GRAD_HDR, HEADER) and bm.POOL_INPUT_GRAD_HDR in bm.sources()
    before = bm.source_id()
    copy = tmp_path / "xgpr_hip_pool_input_grad.h"
    shutil.copyfile(HEADER, copy)
    monkeypatch.setattr(bm, "POOL_INPUT_GRAD_HDR", str(copy))
    assert bm.source_id() == before                                                  # name and contents, not the path
    with open(copy, "a") as f:
        f.write("/* changed */\n")
    assert bm.source_id() != before


# ------------------------------------------------------------------------------------------------ 6. launcher validation
A = 0x100000                     # a dummy 4096-byte-aligned address, never dereferenced on these paths
BIG = 1 << 30
LENS = (10, 11, 12, 12)


def call(token=False, x=A, tokens=A, g=A, out=A, argmax=A, radem=A, chi=A, lens=LENS, dev=A, n=4, L=12, vocab=24, C=6, stride=0, F=64,
         R=64, cw=10, ws=A, wb=BIG):
    """Defaults: windows of 10 x 6 = 60 elements (padded width 64), 64 filters, four sequences of lengths 10 .. 12."""
    from xgpr_amd import _lib
    lib = _lib.load()
    host = None if lens is None else np.asarray(lens, dtype=np.int32)
    hp = None if host is None else host.ctypes.data
    tail = (n, L) + ((vocab,) if token else ()) + (C, stride, F, R, cw, ws, wb, None)
    if token:
        rc = lib.xgpr_conv_token_maxpool_input_grad_f32(tokens, x, g, out, argmax, radem, chi, hp, dev, *tail)
    else:
        rc = lib.xgpr_conv_maxpool_input_grad_f32(x, g, out, argmax, radem, chi, hp, dev, *tail)
    return int(rc), _lib.last_error()


UNSUPPORTED, WORKSPACE, ARRAY_DIMS, RFFS_FREQS, ARRAY_SIZES, CONV_WIDTH, SEQLEN_RANGE = -20, -21, -8, -3, -4, -6, -7
TOO_WIDE = "padded width > 1024 on this wave-tile kernel"
TOKEN_REFUSED = ("token input serves windows of up to 1024 elements and tables of up to 4608 floats "
                 "(see xgpr_conv_token_maxpool_input_grad_ok)")
SEQ_RANGE = "All sequence lengths must be >= conv width and < array size."
FREQS = "incorrect number of rffs and or freqs."
WIDE = dict(L=200, C=6, cw=171, lens=(171, 180, 200, 200), F=2048, R=2048)      # 1026 elements: padded width 2048

VALIDATION = {
    "n < 0": (dict(n=-1), ARRAY_DIMS, "incorrect array dims passed"),
    "L < 1": (dict(L=0), ARRAY_DIMS, "incorrect array dims passed"),
    "C < 1": (dict(C=0), ARRAY_DIMS, "incorrect array dims passed"),
    "conv_width 0": (dict(cw=0), CONV_WIDTH, "invalid conv_width"),
    "conv_width > L": (dict(cw=13), CONV_WIDTH, "invalid conv_width"),
    "no filters": (dict(F=0), RFFS_FREQS, FREQS),
    "more filters than signs": (dict(F=65), RFFS_FREQS, FREQS),
    "signs not whole transforms": (dict(R=96), RFFS_FREQS, FREQS),
    "more signs than the filters' repetitions": (dict(R=128), RFFS_FREQS, FREQS),
    "short stride": (dict(stride=63), ARRAY_SIZES, "g_row_stride is shorter than num_freqs"),
    "a length below conv_width": (dict(lens=(10, 9, 12, 12)), SEQLEN_RANGE, SEQ_RANGE),
    "a length beyond L": (dict(lens=(10, 11, 12, 13)), SEQLEN_RANGE, SEQ_RANGE),
    "no host lengths": (dict(lens=None), SEQLEN_RANGE, "seqlen_host is required (sequence lengths are validated on the host)"),
    "padded width 2048": (WIDE, UNSUPPORTED, TOO_WIDE),
    "short workspace": (dict(wb=8), WORKSPACE, "workspace too small (see xgpr_rbf_workspace_bytes)"),
    "no workspace": (dict(ws=None), WORKSPACE, "workspace too small (see xgpr_rbf_workspace_bytes)"),
    "NULL g": (dict(g=None), WORKSPACE, "NULL array pointer"),
    "NULL argmax": (dict(argmax=None), WORKSPACE, "NULL array pointer"),
    "NULL device lengths": (dict(dev=None), WORKSPACE, "NULL array pointer"),
    "token: vocab 0": (dict(token=True, vocab=0), ARRAY_DIMS, "token table: vocab must be 1 .. 256 (uint8 tokens)"),
    "token: vocab 257": (dict(token=True, vocab=257), ARRAY_DIMS, "token table: vocab must be 1 .. 256 (uint8 tokens)"),
    "token: table of 4617 floats": (dict(token=True, vocab=243, C=19, cw=3, lens=(3, 11, 12, 12), F=64, R=64), UNSUPPORTED, TOKEN_REFUSED),
    "token: padded width 2048": (dict(token=True, vocab=4, **WIDE), UNSUPPORTED, TOKEN_REFUSED),
    "token: NULL tokens": (dict(token=True, tokens=None), WORKSPACE, "NULL array pointer"),
    # two failing checks at once: the first in the documented order is the one reported
    "n < 0 and conv_width 0": (dict(n=-1, cw=0), ARRAY_DIMS, "incorrect array dims passed"),
    "conv_width 0 and bad frequencies": (dict(cw=0, R=96), CONV_WIDTH, "invalid conv_width"),
    "bad frequencies and short stride": (dict(R=96, stride=3), RFFS_FREQS, FREQS),
    "short stride and a bad length": (dict(stride=63, lens=(1, 11, 12, 12)), ARRAY_SIZES, "g_row_stride is shorter than num_freqs"),
    "a bad length and too wide": (dict(WIDE, lens=(170, 180, 200, 200)), SEQLEN_RANGE, SEQ_RANGE),
    "token: a bad length and vocab 0": (dict(token=True, vocab=0, lens=(1, 11, 12, 12)), SEQLEN_RANGE, SEQ_RANGE),
    "token: vocab 0 and too wide": (dict(token=True, **dict(WIDE, vocab=0)), ARRAY_DIMS, "token table: vocab must be 1 .. 256 (uint8 tokens)"),
    "too wide and short workspace": (dict(WIDE, wb=8), UNSUPPORTED, TOO_WIDE),
    "short workspace and NULL g": (dict(wb=8, g=None), WORKSPACE, "workspace too small (see xgpr_rbf_workspace_bytes)"),
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
        assert call(token=token, n=0, lens=(), stride=63)[0] == ARRAY_SIZES   # ... but the arguments are still checked
        assert call(token=token, n=0, lens=(), **{k: v for k, v in WIDE.items() if k != "lens"})[0] == UNSUPPORTED


def test_workspace_bound_is_the_advertised_size():
    from xgpr_amd import _lib
    need = int(_lib.load().xgpr_rbf_workspace_bytes(64))
    assert call(wb=need - 1)[0] == WORKSPACE and call(token=True, wb=need - 1)[0] == WORKSPACE
    assert call(wb=need, g=None)[0] == WORKSPACE                         # (past the size check: the NULL pointer is what is refused)


def test_ok_predicates():
    from xgpr_amd import _lib
    lib = _lib.load()
    assert [int(lib.xgpr_conv_maxpool_input_grad_ok(d)) for d in (1, 2, 189, 1024)] == [1, 1, 1, 1]
    assert int(lib.xgpr_conv_maxpool_input_grad_ok(1025)) == 0 and int(lib.xgpr_conv_maxpool_input_grad_ok(0)) == 0
    assert int(lib.xgpr_conv_token_maxpool_input_grad_ok(189, 21, 21)) == 1
    assert int(lib.xgpr_conv_token_maxpool_input_grad_ok(9 * 19, 243, 19)) == 0  # 4617 floats: more than the LDS image holds
    assert int(lib.xgpr_conv_token_maxpool_input_grad_ok(1026, 4, 6)) == 0       # padded width 2048
    assert int(lib.xgpr_conv_token_maxpool_input_grad_ok(190, 21, 21)) == 0      # not whole positions


# ------------------------------------------------------------------------------------------------ 7. the Linear kernel
@pytest.mark.parametrize("intercept", [True, False])
def test_linear_kernel_input_gradient(intercept):
    import torch
    from xgpr_amd.kernels import LinearKernel
    k = LinearKernel((5, 7), device="cpu", kernel_spec_parms={"intercept": intercept})
    rng = np.random.default_rng(6)
    x = rng.standard_normal((5, 7))
    M = 7 + int(intercept)
    w = rng.standard_normal(M)
    g = k.input_gradient(x, w)
    assert g.dtype == torch.float64 and tuple(g.shape) == (5, 7)
    assert (g.numpy() == np.broadcast_to(w[int(intercept):], (5, 7))).all()
    fd = (k.transform_x(x + 0.5 * np.eye(7)[2]) @ torch.from_numpy(w) - k.transform_x(x - 0.5 * np.eye(7)[2]) @ torch.from_numpy(w))
    assert np.abs(fd.numpy() - w[int(intercept) + 2]).max() < 1e-6      # (the features are the float32 copy of x)
    wr = rng.standard_normal((5, M + 2))                                # per row, with columns past w_cols
    g = k.input_gradient(x, wr, w_cols=4).numpy()
    first = int(intercept)
    assert (g[:, :4 - first] == wr[:, first:4]).all() and (g[:, 4 - first:] == 0).all()
    with pytest.raises(RuntimeError):
        k.input_gradient(x, rng.standard_normal((4, M)))


def test_predict_gradient_for_linear_on_the_cpu_device():
    """d mean / d x = trainy_std * weights (past the intercept); d variance / d x = trainy_std^2 * 2 lambda^2 (V z)[1:], checked against
    central differences of ``predict`` (the variance is a quadratic: exact up to rounding)."""
    import torch
    from xgpr_amd.kernels import LinearKernel
    from xgpr_amd.models import xGPRegression
    rng = np.random.default_rng(7)
    d = 6
    model = xGPRegression.__new__(xGPRegression)
    model.kernel = LinearKernel((10, d), device="cpu")
    model.kernel_choice, model.device = "Linear", "cpu"
    model.weights = torch.from_numpy(rng.standard_normal(d + 1))
    a = rng.standard_normal((d + 1, d + 1))
    model.var = torch.from_numpy(a @ a.T / d)
    model.trainy_mean, model.trainy_std = 0.7, 1.9
    x = rng.standard_normal((4, d)).astype(np.float32).astype(np.float64)
    gm, gv = model.predict_gradient(x, get_var=True)
    assert gm.shape == gv.shape == (4, d)
    assert np.abs(gm - 1.9 * model.weights.numpy()[None, 1:]).max() < 1e-14
    h = 0.25                                                            # (exact in float32 for these magnitudes: x keeps its bits)
    for k in range(d):
        e = np.zeros(d)
        e[k] = h
        (mp, vp), (mm, vm) = model.predict(x + e, get_var=True), model.predict(x - e, get_var=True)
        assert np.abs((mp - mm) / (2 * h) - gm[:, k]).max() < 1e-5
        assert np.abs((vp - vm) / (2 * h) - gv[:, k]).max() < 1e-5 * max(1.0, float(np.abs(gv).max()))
