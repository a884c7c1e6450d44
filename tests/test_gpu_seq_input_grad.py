"""The per-position input gradient of the sequence / graph kernels on the device (xgpr_conv_input_grad_f32,
xgpr_conv_token_input_grad_f32, ConvSORFKernel.input_gradient, xGPRegression.predict_gradient) against the long-double dense reference
of tests/dense_seq_input_grad.py, within its a-priori cap ``cap_seq_input_grad`` (derived from the operation count;
tests/test_seq_input_grad_host.py shows what it separates) -- or bit for bit where a test says so.  Every comparison prints one
``SEQGRAD`` line with measured error and cap; profiles/seq_input_grad_errors.txt is the collection of those lines from one run."""
import numpy as np
import pytest
import torch

import dense_reference as dr
import dense_seq_input_grad as dsg
from dense_reference import U64
from guarded import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64

# (C, conv_width) -> window d / padded P: graph 2/2; 15/16 the shfl fold below 64; 64/64 d = P; 105/128 the first two-layout width;
# 189/256 BASELINE configs[3]'s window; 1024/1024.
ARMS = [(2, 1), (5, 3), (8, 8), (21, 5), (21, 9), (128, 8)]
FS = [37, 300, 1024, 1324, 4500]            # less than a tile; F < P at the wide arms; an exact tile; a ragged second tile; five tiles
MODES = ["shared", "rows", "rows_pad"]      # one vector; one row per sequence with stride == w_cols; with stride > w_cols and NaN in the pad
WCOLS = ["full", "two", "cut"]              # 2 F; 2; a value ending inside the second tile (F >= 1324 only)
#         C  cw   L  lengths        n    F   scaling intercept mode      w_cols
CASES = [(2, 1, 6, (1, 6, 3), 5, 37, 0, True, "shared", "full"),
         (2, 1, 6, (6, 2), 1, 300, 2, False, "rows", "two"),
         (5, 3, 4, (3, 4), 5, 37, 1, True, "rows_pad", "full"),              # nk = 1, 2 < conv_width: the ring never wraps
         (5, 3, 12, (3, 7, 12), 5, 1324, 2, False, "shared", "cut"),
         (5, 3, 9, (9, 5), 1, 4500, 1, True, "rows", "full"),                # five tiles: a wave owns two (the tile loop's second trip)
         (8, 8, 12, (8, 10, 12), 5, 300, 1, True, "rows", "full"),
         (8, 8, 12, (11,), 1, 1024, 0, False, "shared", "two"),
         (21, 5, 12, (5, 9, 12), 5, 1024, 1, True, "rows_pad", "full"),
         (21, 5, 12, (12, 6), 1, 1324, 0, False, "shared", "cut"),
         (21, 9, 40, (9, 23, 40), 5, 300, 1, True, "shared", "full"),
         (21, 9, 40, (23,), 1, 1324, 2, True, "rows_pad", "cut"),
         (21, 9, 12, (9, 12, 10), 5, 37, 0, False, "rows", "two"),
         (128, 8, 10, (8, 9, 10), 5, 1324, 1, True, "shared", "cut"),
         (128, 8, 10, (10,), 1, 1024, 2, False, "rows", "full")]


def test_the_case_list_covers_every_axis():
    assert {(c[0], c[1]) for c in CASES} == set(ARMS) and {c[5] for c in CASES} == set(FS)
    assert {c[4] for c in CASES} == {1, 5} and {c[6] for c in CASES} == {0, 1, 2} and {c[7] for c in CASES} == {True, False}
    assert {c[8] for c in CASES} == set(MODES) and {c[9] for c in CASES} == set(WCOLS)
    assert (5, 3, 4, (3, 4)) in {c[:4] for c in CASES} and (21, 9, 40, (9, 23, 40)) in {c[:4] for c in CASES}


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def w_cols_of(kind, F):
    return {"full": 2 * F, "two": 2, "cut": 2 * (1024 + 100)}[kind]


def device_weights(w, mode, w_cols):
    if mode == "rows":
        w = np.ascontiguousarray(w[:, :w_cols])
    return torch.from_numpy(np.ascontiguousarray(w)).to(DEV)


def run_operator(ext, xs, seqlen, w, radem, chi, sigma, cw, scaling, icpt, w_cols):
    out = torch.full(xs.shape, float("nan"), dtype=F64, device=DEV)
    ext.hipConvInputGrad(torch.from_numpy(xs).to(DEV), w, out, torch.from_numpy(radem).to(DEV), torch.from_numpy(chi).to(DEV), seqlen,
                         sigma, cw, scaling, icpt, w_cols=w_cols)
    return out


def report(tag, case, got, ref, cap):
    err = float(np.abs(got.astype(dr.LD) - ref).max())
    print(f"SEQGRAD {tag:<10} {str(case):<64} hip-dense {err:.3e}  cap {cap:.3e}  ratio {err / cap:.4f}")
    return err


def zero_past_lengths(got, seqlen):
    return all((got[i, s:] == 0).all() and not np.signbit(got[i, s:]).any() for i, s in enumerate(seqlen))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)).replace(" ", ""))
def test_operator_against_the_dense_reference(ext, case):
    """The output is prefilled with NaN: finite everywhere means fully overwritten; positions >= length are 0.0."""
    C, cw, L, lengths, n, F, scaling, icpt, mode, wk = case
    xs, seqlen, w, radem, chi, sigma = dsg.make_case(n, L, C, cw, F, mode != "shared", seed=7, lengths=list(lengths),
                                                     stride_pad=3 if mode == "rows_pad" else 0)
    w_cols = w_cols_of(wk, F)
    assert ext.conv_input_grad_ok(cw * C, F) == 1
    got = run_operator(ext, xs, seqlen, device_weights(w, mode, w_cols), radem, chi, sigma, cw, scaling, icpt, w_cols).cpu().numpy()
    ref = dsg.seq_input_grad(xs, seqlen, w, radem, chi, sigma, cw, scaling, icpt, w_cols=w_cols)
    cap = dsg.cap_seq_input_grad(xs, seqlen, w, radem, chi, sigma, cw, scaling, icpt, w_cols=w_cols)
    assert np.isfinite(got).all() and zero_past_lengths(got, seqlen)
    assert report("operator", case, got, ref, cap) <= cap
    assert float(np.abs(ref).max()) > 100 * cap                            # (the comparison is not vacuous)


@pytest.mark.parametrize("C,cw,L,F", [(5, 3, 9, 4500), (21, 9, 40, 1324), (128, 8, 10, 1024)])
def test_results_are_bit_identical_and_sequences_are_independent(ext, C, cw, L, F):
    """Two launches give equal bits; a sequence's result depends neither on n nor on its position (sequence 3 of 5 against the same
    sequence alone), nor on whether the weights arrive shared or per row."""
    n = 5
    xs, seqlen, w, radem, chi, sigma = dsg.make_case(n, L, C, cw, F, True, seed=8)
    wd = device_weights(w, "rows", 2 * F)
    a = run_operator(ext, xs, seqlen, wd, radem, chi, sigma, cw, 1, True, 2 * F)
    b = run_operator(ext, xs, seqlen, wd, radem, chi, sigma, cw, 1, True, 2 * F)
    assert same_bits(a, b)
    alone = run_operator(ext, xs[3:4].copy(), seqlen[3:4].copy(), wd[3:4].contiguous(), radem, chi, sigma, cw, 1, True, 2 * F)
    assert same_bits(a[3:4].contiguous(), alone)
    shared = run_operator(ext, xs, seqlen, wd[3].contiguous(), radem, chi, sigma, cw, 1, True, 2 * F)
    assert same_bits(a[3:4].contiguous(), shared[3:4].contiguous())
    repeated = run_operator(ext, xs, seqlen, wd[3:4].repeat(n, 1).contiguous(), radem, chi, sigma, cw, 1, True, 2 * F)
    assert same_bits(shared, repeated)


# ------------------------------------------------------------------------------------------------ tokens
def token_case(table, n, L, lengths, seed):
    """tokens [n, L] uint8 with values past each length drawn anew (garbage the operators never read), the dense array table[tokens]."""
    rng = np.random.default_rng([n, L, seed])
    tokens = rng.integers(0, table.shape[0], size=(n, L)).astype(np.uint8)
    seqlen = np.asarray([lengths[i % len(lengths)] for i in range(n)], dtype=np.int32)
    return tokens, seqlen


@pytest.mark.parametrize("kind", ["one-hot", "random"])
def test_token_form_is_bit_identical_to_the_dense_form(ext, kind):
    rng = np.random.default_rng(9)
    if kind == "one-hot":
        table, cw, L, F, lengths = np.eye(21, dtype=np.float32), 9, 40, 1324, (9, 23, 40)
    else:
        table, cw, L, F, lengths = rng.uniform(-1, 1, size=(24, 5)).astype(np.float32), 3, 12, 300, (3, 7, 12)
    n, C = 5, table.shape[1]
    _, _, w, radem, chi, sigma = dsg.make_case(n, L, C, cw, F, True, seed=9)
    tokens, seqlen = token_case(table, n, L, lengths, 9)
    tab = (table.astype(np.float64) * sigma).astype(np.float32)
    xs = tab[tokens]
    wd = device_weights(w, "rows", 2 * F)
    assert ext.conv_token_input_grad_ok(cw * C, table.shape[0], C) == 1
    dense = run_operator(ext, xs, seqlen, wd, radem, chi, sigma, cw, 1, True, 2 * F)
    garbage = tokens.copy()
    for i, s in enumerate(seqlen):
        garbage[i, s:] = (garbage[i, s:].astype(np.int64) + 1 + i) % table.shape[0]
    for tk in (tokens, garbage):
        out = torch.full(xs.shape, float("nan"), dtype=F64, device=DEV)
        ext.hipConvTokenInputGrad(torch.from_numpy(tk).to(DEV), torch.from_numpy(tab).to(DEV), wd, out, torch.from_numpy(radem).to(DEV),
                                  torch.from_numpy(chi).to(DEV), seqlen, sigma, cw, 1, True)
        assert same_bits(out, dense)
    ref = dsg.seq_input_grad(xs, seqlen, w, radem, chi, sigma, cw, 1, True)
    cap = dsg.cap_seq_input_grad(xs, seqlen, w, radem, chi, sigma, cw, 1, True)
    assert report("tokens", (kind, C, cw, L, F, n), dense.cpu().numpy(), ref, cap) <= cap


def _kernel(choice, n, L, C, cw, M, icpt=True, averaging="sqrt"):
    from xgpr_amd.kernels import ConvSORFKernel
    k = ConvSORFKernel(choice, (n, L, C), M, 123, DEV, {"matern_nu": 5 / 2, "intercept": icpt, "conv_width": cw, "averaging": averaging})
    k.set_hyperparams(np.asarray([0.9, 2.1 / np.sqrt(k.conv_width * C)]), logspace=False)
    return k


def _kernel_operands(k, x):
    """x_scaled as KernelBase.scaled_f32 forms it, and the kernel's own draws, on the host."""
    sigma = float(k.hyperparams[1])
    xs = (x.astype(np.float32).astype(np.float64) * sigma).astype(np.float32)
    return xs, k.radem_diag.cpu().numpy(), k.chi_arr.cpu().numpy(), sigma


def test_a_table_the_lds_image_cannot_hold_goes_through_dense_slices(ext):
    from xgpr_amd.dataset import TokenBatch
    rng = np.random.default_rng(10)
    V, C, cw, L, n, F = 250, 19, 3, 8, 5, 300                             # 4750 floats > 4608
    table = rng.uniform(-1, 1, size=(V, C)).astype(np.float32)
    tokens, seqlen = token_case(table, n, L, (3, 5, 8), 10)
    k = _kernel("Conv1dRBF", n, L, C, cw, 2 * F)
    w = rng.standard_normal(2 * F)
    assert ext.conv_token_input_grad_ok(cw * C, V, C) == 0 and ext.conv_input_grad_ok(cw * C, F) == 1
    out = torch.zeros((n, L, C), dtype=F64, device=DEV)
    with pytest.raises(RuntimeError, match="token input serves windows of up to 1024 elements and tables of up to 4608 floats"):
        ext.hipConvTokenInputGrad(torch.from_numpy(tokens).to(DEV), torch.from_numpy(table).to(DEV), torch.from_numpy(w).to(DEV), out,
                                  k.radem_diag, k.chi_arr, seqlen, 1.0, cw, 1, True)
    assert float(out.abs().max()) == 0.0
    k.CACHE_BUILD_ROWS = 2                                                # three slices
    got = k.input_gradient(TokenBatch(torch.from_numpy(tokens).to(DEV), torch.from_numpy(table).to(DEV)), seqlen, w)
    assert same_bits(got, k.input_gradient(table[tokens], seqlen, w))
    xs, radem, chi, sigma = _kernel_operands(k, table[tokens])
    ref = dsg.seq_input_grad(xs, seqlen, w, radem, chi, sigma, cw, 1, True)
    cap = dsg.cap_seq_input_grad(xs, seqlen, w, radem, chi, sigma, cw, 1, True)
    assert report("slices", (V, C, cw, L, F, n), got.cpu().numpy(), ref, cap) <= cap


# ------------------------------------------------------------------------------------------------ the composed route
def test_operator_against_the_composed_route_and_the_composed_route_beyond_1024(ext):
    rng = np.random.default_rng(11)
    # C 21, conv_width 9, F 300: both routes, within the sum of their caps (the composed route's rows go through
    # xgpr_rbf_input_grad_f32: window by window the same cap)
    n, L, C, cw, F = 5, 12, 21, 9, 300
    k = _kernel("Conv1dRBF", n, L, C, cw, 2 * F)
    x = rng.uniform(-1, 1, size=(n, L, C))
    seqlen = np.asarray([9, 12, 10, 11, 12], dtype=np.int32)
    w = rng.standard_normal((n, 2 * F))
    xs, radem, chi, sigma = _kernel_operands(k, x)
    wd = torch.from_numpy(w).to(DEV)
    op = k.input_gradient(x, seqlen, wd).cpu().numpy()
    fb = k.input_gradient_composed(torch.from_numpy(xs).to(DEV), seqlen, wd, 2 * F).cpu().numpy()
    cap = dsg.cap_seq_input_grad(xs, seqlen, w, radem, chi, sigma, cw, 1, True)
    ref = dsg.seq_input_grad(xs, seqlen, w, radem, chi, sigma, cw, 1, True)
    report("op-vs-fb", (C, cw, L, F, n), op, fb.astype(dr.LD), 2 * cap)
    assert float(np.abs(op - fb).max()) <= 2 * cap
    assert report("composed", (C, cw, L, F, n), fb, ref, cap) <= cap
    assert zero_past_lengths(fb, seqlen)
    # a window of 9 x 128 = 1152 elements (P = 2048): the operator refuses, the kernel object takes the composed route
    n, L, C, cw, F = 2, 10, 128, 9, 64
    k = _kernel("Conv1dRBF", n, L, C, cw, 2 * F, icpt=False)
    x = rng.uniform(-1, 1, size=(n, L, C))
    seqlen = np.asarray([9, 10], dtype=np.int32)
    w = rng.standard_normal(2 * F)
    xs, radem, chi, sigma = _kernel_operands(k, x)
    assert ext.conv_input_grad_ok(cw * C, F) == 0
    with pytest.raises(RuntimeError, match="padded width > 1024"):
        run_operator(ext, xs, seqlen, torch.from_numpy(w).to(DEV), radem, chi, sigma, cw, 1, False, 2 * F)
    got = k.input_gradient(x, seqlen, w).cpu().numpy()
    ref = dsg.seq_input_grad(xs, seqlen, w, radem, chi, sigma, cw, 1, False)
    cap = dsg.cap_seq_input_grad(xs, seqlen, w, radem, chi, sigma, cw, 1, False)
    assert report("composed", (C, cw, L, F, n), got, ref, cap) <= cap and zero_past_lengths(got, seqlen)


@pytest.mark.parametrize("choice", ["Conv1dRBF", "Conv1dMatern", "Conv1dCauchy", "GraphRBF"])
def test_kernel_input_gradient(choice):
    n, L, C, cw, M = 4, 9, 6, 4, 600
    k = _kernel(choice, n, L, C, cw, M, averaging="full" if choice == "GraphRBF" else "sqrt")
    cw = k.conv_width                                                      # (1 for the graph kernel)
    rng = np.random.default_rng(12)
    x = rng.uniform(-1, 1, size=(n, L, C))
    seqlen = np.asarray([9, 4, 6, 8], dtype=np.int32)
    w = rng.standard_normal(M)
    xs, radem, chi, sigma = _kernel_operands(k, x)
    got = k.input_gradient(x, seqlen, w)
    assert got.dtype == F64 and tuple(got.shape) == (n, L, C) and got.is_cuda
    ref = dsg.seq_input_grad(xs, seqlen, w, radem, chi, sigma, cw, k.scaling_type, True)
    cap = dsg.cap_seq_input_grad(xs, seqlen, w, radem, chi, sigma, cw, k.scaling_type, True)
    assert report("kernel", (choice, C, cw, L, M // 2, n), got.cpu().numpy(), ref, cap) <= cap
    with pytest.raises(RuntimeError):
        k.input_gradient(x, seqlen, w, w_cols=7)
    with pytest.raises(RuntimeError, match="sequence_length is required"):
        k.input_gradient(x, None, w)


# ------------------------------------------------------------------------------------------------ predict_gradient end to end
N, L_, C_, CW, V_ = 60, 12, 4, 3, 6


@pytest.fixture(scope="module")
def fitted():
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.models import xGPRegression
    rng = np.random.default_rng(13)
    table = rng.uniform(-1, 1, size=(V_, C_)).astype(np.float32)
    tokens = rng.integers(0, V_, size=(N, L_)).astype(np.uint8)
    seqlen = rng.integers(CW, L_ + 1, size=N).astype(np.int32)
    x = table[tokens].astype(np.float64)
    y = np.asarray([x[i, :s, 0].sum() - x[i, :s, 1].mean() for i, s in enumerate(seqlen)]) + 3.0 + 0.05 * rng.standard_normal(N)
    ds = build_regression_dataset(x, y * 2.5, sequence_lengths=seqlen, chunk_size=25, device=DEV)
    model = xGPRegression(num_rffs=128, variance_rffs=32, kernel_choice="Conv1dRBF", device=DEV, verbose=False,
                          kernel_settings={"conv_width": CW, "averaging": "sqrt", "intercept": True})
    model.set_hyperparams(np.log(np.asarray([0.3, 0.6])), ds)
    model.fit(ds, mode="exact")
    return model, ds, x, seqlen, tokens, table


def test_predict_gradient(fitted):
    model, _, x, seqlen, tokens, table = fitted
    k = model.kernel
    xs, radem, chi, sigma = _kernel_operands(k, x)
    std = float(model.trainy_std)
    gm, gv = model.predict_gradient(x, get_var=True, chunk_size=16, sequence_lengths=seqlen)
    assert isinstance(gm, np.ndarray) and gm.shape == (N, L_, C_) and gv.shape == (N, L_, C_)
    assert np.array_equal(gm, model.predict_gradient(x, chunk_size=16, sequence_lengths=seqlen))
    assert zero_past_lengths(gm, seqlen) and zero_past_lengths(gv, seqlen)
    case = ("Conv1dRBF", C_, CW, L_, 64, N)
    # mean
    w = model.weights.cpu().numpy()
    ref = dsg.seq_input_grad(xs, seqlen, w, radem, chi, sigma, CW, 1, True) * std
    cap = dsg.cap_seq_input_grad(xs, seqlen, w, radem, chi, sigma, CW, 1, True) * std
    assert report("mean", case, gm, ref, cap) <= cap + 4 * U64 * float(np.abs(ref).max())
    # variance: per-sequence weights 2 lambda^2 V z_v formed on the host from transform_x
    lam = float(k.get_lambda())
    var = model.var.cpu().numpy()
    nvar = var.shape[0]
    assert nvar == 32
    zv = k.transform_x(x, seqlen)[:, :nvar].cpu().numpy()
    wv = 2.0 * lam ** 2 * (zv @ var)
    ref = dsg.seq_input_grad(xs, seqlen, wv, radem, chi, sigma, CW, 1, True, w_cols=nvar) * std ** 2
    cap = dsg.cap_seq_input_grad(xs, seqlen, wv, radem, chi, sigma, CW, 1, True, w_cols=nvar) * std ** 2
    assert report("variance", case, gv, ref, cap) <= cap + 4 * U64 * float(np.abs(ref).max())
    assert float(np.abs(gm).max()) > 0 and float(np.abs(gv).max()) > 0
    # the same problem given as tokens: the dense result bit for bit
    tm, tv = model.predict_gradient(tokens, get_var=True, chunk_size=16, sequence_lengths=seqlen, token_table=table)
    assert np.array_equal(tm, gm) and np.array_equal(tv, gv)


def test_predict_gradient_refusals(fitted):
    from xgpr_amd.models import xGPRegression
    model, ds, x, seqlen, _, _ = fitted
    with pytest.raises(RuntimeError, match="sequence_lengths is required"):
        model.predict_gradient(x[:3])
    fresh = xGPRegression(num_rffs=128, variance_rffs=32, kernel_choice="Conv1dRBF", device=DEV, verbose=False,
                          kernel_settings={"conv_width": CW, "averaging": "sqrt", "intercept": True})
    with pytest.raises(RuntimeError, match="not yet been successfully fitted"):
        fresh.predict_gradient(x[:3], sequence_lengths=seqlen[:3])
    two = xGPRegression(num_rffs=128, variance_rffs=32, kernel_choice="Conv1dTwoLayer", device=DEV, verbose=False,
                        kernel_settings={"conv_width": CW, "init_rffs": 64, "intercept": True})
    two.set_hyperparams(dataset=ds)
    two.weights = torch.zeros(128, dtype=F64, device=DEV)                  # (the refusal is about the kernel, not the fit)
    with pytest.raises(RuntimeError, match="RBF, Matern and Cauchy"):
        two.predict_gradient(x[:3], sequence_lengths=seqlen[:3])
