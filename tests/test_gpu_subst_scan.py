"""The single-substitution scan of the sequence / graph kernels on the device (xgpr_conv_token_subst_scan_f32,
ConvSORFKernel.substitution_scan / substitution_scan_composed, xGPRegression.predict_substitutions) against the long-double dense
reference of tests/dense_subst_scan.py, within its a-priori cap ``cap_subst_scan`` (derived from the operation count;
tests/test_subst_scan_host.py holds the cap to 1e-2 of every case's largest output and shows what it separates) -- or bit for bit where
a test says so.  No element is excused.  Every comparison prints one ``SUBST`` line with measured error and cap."""
import functools

import numpy as np
import pytest
import torch

import dense_reference as dr
import dense_subst_scan as dss
from dense_reference import U32
from guarded import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


@functools.lru_cache(maxsize=None)
def reference(name):
    """(operands, conv_width, scaling, intercept, dense reference, cap) of a case: computed once, shared, left unchanged."""
    c, cw, scaling, icpt = dss.case(name)
    ref = dss.subst_scan(c["tokens"], c["table"], c["seqlen"], c["w"], c["radem"], c["chi"], cw, scaling, icpt)
    ref.setflags(write=False)
    return c, cw, scaling, icpt, ref, dss.cap_subst_scan(c["table"], c["seqlen"], c["w"], c["chi"], cw, scaling, icpt)


def run_operator(ext, c, cw, scaling, icpt, rows=None):
    """The ext call on the case's sequences (``rows``: a subset, in that order); the output starts as NaN."""
    rows = np.arange(c["tokens"].shape[0]) if rows is None else np.asarray(rows)
    tokens = np.ascontiguousarray(c["tokens"][rows])
    out = torch.full((tokens.shape[0], tokens.shape[1], c["table"].shape[0]), float("nan"), dtype=F64, device=DEV)
    ext.hipConvTokenSubstScan(torch.from_numpy(tokens).to(DEV), torch.from_numpy(c["table"]).to(DEV), torch.from_numpy(c["w"]).to(DEV), out,
                              torch.from_numpy(c["radem"]).to(DEV), torch.from_numpy(c["chi"]).to(DEV),
                              np.ascontiguousarray(c["seqlen"][rows]), cw, scaling, icpt)
    return out


def report(tag, case, got, ref, cap):
    err = float(np.abs(got.astype(dr.LD) - ref).max()) if ref.size else 0.0
    print(f"SUBST {tag:<10} {str(case):<40} hip-dense {err:.3e}  cap {cap:.3e}  ratio {err / cap:.4f}  max|ref| {float(np.abs(ref).max()):.3e}")
    return err


def exact_zeros(got, tokens, seqlen):
    """+0.0, bitwise, at every sequence's own token and at every position past its length."""
    for i, s in enumerate(seqlen):
        own = got[i, np.arange(s), tokens[i, :s]]
        for z in (own, got[i, s:]):
            if (z != 0).any() or np.signbit(z).any():
                return False
    return True


def test_the_case_list_covers_every_axis():
    kws = {nm: kw for nm, kw, _, _ in dss.CASES}
    padded = {dr.padded_width(kw["conv_width"] * kw["C"]) for kw in kws.values()}
    assert {16, 64, 128, 256, 512, 1024} <= padded
    assert {(kw["C"], kw["conv_width"]) for kw in kws.values()} >= {(4, 3), (21, 3), (21, 6), (21, 9), (21, 48)}
    assert {kw["n"] for kw in kws.values()} >= {1, 3, 65} and {kw["conv_width"] for kw in kws.values()} >= {1}
    assert {kw["F"] for kw in kws.values()} >= {8, 1030, 5000} and any(kw.get("extra_reps") for kw in kws.values())
    assert {kw["V"] for kw in kws.values()} >= {1, 256} and kws["vocab256_c18"]["C"] == 18
    assert {(s, i) for _, _, s, i in dss.CASES} == {(s, i) for s in (0, 1, 2) for i in (True, False)}
    for nm in ("w16_c4_cw3", "w128_c21_cw6", "w256_c21_cw9"):      # one window, the full length, and nk < conv_width
        c, cw, _, _ = dss.case(nm)
        nk = c["seqlen"] - cw + 1
        assert (nk == 1).any() and (c["seqlen"] == c["tokens"].shape[1]).any() and ((nk > 1) & (nk < cw)).any()
        assert (c["tokens"][np.arange(c["tokens"].shape[1])[None, :] >= c["seqlen"][:, None]] >= c["table"].shape[0]).all()


@pytest.mark.parametrize("name", [c[0] for c in dss.CASES])
def test_operator_against_the_dense_reference(ext, name):
    c, cw, scaling, icpt, ref, cap = reference(name)
    out = run_operator(ext, c, cw, scaling, icpt)
    got = out.cpu().numpy()
    assert report("operator", name, got, ref, cap) <= cap
    assert dss.check(got, ref, cap) <= cap
    assert exact_zeros(got, c["tokens"], c["seqlen"])
    assert same_bits(out, run_operator(ext, c, cw, scaling, icpt)), "two runs differ"
    if name == "vocab1":
        assert (got == 0).all()
    else:
        assert float(np.abs(got).max()) > 0


def test_two_identical_table_rows_give_bit_equal_columns(ext):
    c, cw, scaling, icpt, _, _ = reference("dup_rows")
    assert (c["table"][1] == c["table"][3]).all()
    out = run_operator(ext, c, cw, scaling, icpt)
    assert same_bits(out[:, :, 1].contiguous(), out[:, :, 3].contiguous())
    assert not same_bits(out[:, :, 1].contiguous(), out[:, :, 2].contiguous())


@pytest.mark.parametrize("name", ["w256_c21_cw9", "w1024_c21_cw48", "n65"])
def test_a_sequence_alone_and_inside_a_batch(ext, name):
    c, cw, scaling, icpt, _, _ = reference(name)
    n = c["tokens"].shape[0]
    whole = run_operator(ext, c, cw, scaling, icpt)
    for i in sorted({0, n // 2, n - 1}):
        assert same_bits(run_operator(ext, c, cw, scaling, icpt, rows=[i])[0], whole[i]), i
    back = run_operator(ext, c, cw, scaling, icpt, rows=np.arange(n)[::-1])      # every sequence at another index
    assert same_bits(back.flip(0).contiguous(), whole)


# ------------------------------------------------------------------------------------------------ the kernel object
def _kernel(choice, n, L, C, cw, M, icpt=True, averaging="sqrt"):
    from xgpr_amd.kernels import ConvSORFKernel
    k = ConvSORFKernel(choice, (n, L, C), M, 123, DEV, {"matern_nu": 5 / 2, "intercept": icpt, "conv_width": cw, "averaging": averaging})
    k.set_hyperparams(np.asarray([0.9, 2.1 / np.sqrt(C)]), logspace=False)
    return k


def _kernel_case(k, n, L, V, seed, lengths):
    """Tokens, an unscaled table, lengths and weights for kernel object k; the scaled table as KernelBase.scaled_f32 forms it."""
    rng = np.random.default_rng(seed)
    C = k._xdim[2]
    table = rng.uniform(-1, 1, size=(V, C)).astype(np.float32)
    tokens = rng.integers(0, V, size=(n, L)).astype(np.uint8)
    seqlen = np.asarray([lengths[i % len(lengths)] for i in range(n)], dtype=np.int32)
    w = rng.standard_normal(k.num_rffs) * (1.0 + rng.permutation(k.num_rffs)) ** -1.5
    scaled = (table.astype(np.float64) * float(k.hyperparams[1])).astype(np.float32)
    return tokens, table, scaled, seqlen, w


def _dense(k, tokens, scaled, seqlen, w):
    radem, chi = k.radem_diag.cpu().numpy(), k.chi_arr.cpu().numpy()
    ref = dss.subst_scan(tokens, scaled, seqlen, w, radem, chi, k.conv_width, k.scaling_type, k.fit_intercept)
    return ref, dss.cap_subst_scan(scaled, seqlen, w, chi, k.conv_width, k.scaling_type, k.fit_intercept)


@pytest.mark.parametrize("choice", ["Conv1dRBF", "Conv1dMatern", "Conv1dCauchy", "GraphRBF"])
def test_kernel_substitution_scan_is_the_ext_call_bit_for_bit(ext, choice):
    from xgpr_amd.dataset import TokenBatch
    n, L, C, cw, M, V = 4, 9, 6, 4, 600, 5
    k = _kernel(choice, n, L, C, cw, M, averaging="full" if choice == "GraphRBF" else "sqrt")
    tokens, table, scaled, seqlen, w = _kernel_case(k, n, L, V, 31, (9, 4, 6, 8) if k.conv_width > 1 else (9, 1, 6, 8))
    batch = TokenBatch(torch.from_numpy(tokens).to(DEV), torch.from_numpy(table).to(DEV))
    got = k.substitution_scan(batch, seqlen, w)
    assert got.dtype == F64 and tuple(got.shape) == (n, L, V) and got.is_cuda
    out = torch.full((n, L, V), float("nan"), dtype=F64, device=DEV)
    ext.hipConvTokenSubstScan(batch.tokens, torch.from_numpy(scaled).to(DEV), torch.from_numpy(w).to(DEV), out, k.radem_diag, k.chi_arr,
                              seqlen, k.conv_width, k.scaling_type, k.fit_intercept)
    assert same_bits(got, out)
    ref, cap = _dense(k, tokens, scaled, seqlen, w)
    assert report("kernel", (choice, C, k.conv_width, L, M // 2, n), got.cpu().numpy(), ref, cap) <= cap
    assert exact_zeros(got.cpu().numpy(), tokens, seqlen)
    with pytest.raises(RuntimeError, match="sequence_length is required"):
        k.substitution_scan(batch, None, w)
    with pytest.raises(RuntimeError, match="num_rffs"):
        k.substitution_scan(batch, seqlen, w[:-2])
    with pytest.raises(RuntimeError, match="TokenBatch"):
        k.substitution_scan(table[tokens], seqlen, w)


def _composed_cap(k, tokens, scaled, seqlen, w):
    """The composed route: float32 feature rows of a mutant and of the sequence (each entry within cap_conv with u_out = U32 of
    exact), each multiplied by the weights in float64 -- twice sum|w| cap_conv, over the windows of every mutant."""
    n, L = tokens.shape
    V = scaled.shape[0]
    mut = np.repeat(tokens, L * V, axis=0).reshape(n, L, V, L)
    for l in range(L):
        mut[:, l, :, l] = np.arange(V)[None, :]
    lens = np.repeat(seqlen, L * V)
    x = scaled[mut.reshape(-1, L) % V]                           # (positions past a length hold 255: never part of a window)
    row = dr.cap_conv(np.float32, x, lens, k.chi_arr.cpu().numpy(), k.conv_width, k.scaling_type, u_out=U32)
    sw = float(np.abs(w[1:] if k.fit_intercept else w).sum())
    return 2 * sw * row


def test_the_composed_route_against_the_dense_reference_and_beyond_the_operator(ext):
    from xgpr_amd.dataset import TokenBatch
    n, L, C, cw, M, V = 3, 8, 6, 3, 400, 5
    k = _kernel("Conv1dRBF", n, L, C, cw, M)
    tokens, table, scaled, seqlen, w = _kernel_case(k, n, L, V, 32, (8, 3, 5))
    batch = TokenBatch(torch.from_numpy(tokens).to(DEV), torch.from_numpy(table).to(DEV))
    ref, cap = _dense(k, tokens, scaled, seqlen, w)
    k.COMPOSED_SCAN_ELEMS = 37 * M                               # several slices, the last one ragged
    fb = k.substitution_scan_composed(batch, seqlen, w).cpu().numpy()
    ccap = _composed_cap(k, tokens, scaled, seqlen, w)
    assert report("composed", (C, cw, L, M // 2, n), fb, ref, ccap) <= ccap
    assert exact_zeros(fb, tokens, seqlen)
    op = k.substitution_scan(batch, seqlen, w).cpu().numpy()
    assert float(np.abs(op - fb).max()) <= cap + ccap
    # a window of 9 x 128 = 1152 elements (P = 2048): the operator refuses, the kernel object takes the composed route
    n, L, C, cw, M, V = 2, 10, 128, 9, 128, 4
    k = _kernel("Conv1dRBF", n, L, C, cw, M, icpt=False)
    tokens, table, scaled, seqlen, w = _kernel_case(k, n, L, V, 33, (9, 10))
    assert ext.conv_token_subst_scan_ok(cw * C, V, C, M // 2) == 0
    out = torch.zeros((n, L, V), dtype=F64, device=DEV)
    with pytest.raises(RuntimeError, match="the substitution scan serves windows of up to 1024 elements"):
        ext.hipConvTokenSubstScan(torch.from_numpy(tokens).to(DEV), torch.from_numpy(scaled).to(DEV), torch.from_numpy(w).to(DEV), out,
                                  k.radem_diag, k.chi_arr, seqlen, cw, 1, False)
    assert float(out.abs().max()) == 0.0
    batch = TokenBatch(torch.from_numpy(tokens).to(DEV), torch.from_numpy(table).to(DEV))
    got = k.substitution_scan(batch, seqlen, w).cpu().numpy()
    ref, _ = _dense(k, tokens, scaled, seqlen, w)
    ccap = _composed_cap(k, tokens, scaled, seqlen, w)
    assert report("composed", (C, cw, L, M // 2, n), got, ref, ccap) <= ccap and exact_zeros(got, tokens, seqlen)
    # tokens that are not contiguous take the composed route as well
    wide = torch.from_numpy(np.concatenate([tokens, tokens], axis=1)).to(DEV)
    assert not wide[:, :L].is_contiguous()
    again = k.substitution_scan(TokenBatch(wide[:, :L], batch.table), seqlen, w).cpu().numpy()
    assert np.array_equal(again, got)


# ------------------------------------------------------------------------------------------------ predict_substitutions end to end
N, L_, C_, CW, V_ = 40, 12, 4, 3, 5


def _fit(choice):
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.models import xGPRegression
    rng = np.random.default_rng(34)
    table = rng.uniform(-1, 1, size=(V_, C_)).astype(np.float32)
    tokens = rng.integers(0, V_, size=(N, L_)).astype(np.uint8)
    seqlen = rng.integers(CW, L_ + 1, size=N).astype(np.int32)
    seqlen[:3] = (L_, CW, 7)
    x = table[tokens].astype(np.float64)
    y = np.asarray([x[i, :s, 0].sum() - x[i, :s, 1].mean() for i, s in enumerate(seqlen)]) + 3.0 + 0.05 * rng.standard_normal(N)
    ds = build_regression_dataset(x, y * 2.5, sequence_lengths=seqlen, chunk_size=25, device=DEV)
    settings = {"averaging": "sqrt", "intercept": True}
    if choice.startswith("Conv1d"):
        settings["conv_width"] = CW
    model = xGPRegression(num_rffs=128, variance_rffs=32, kernel_choice=choice, device=DEV, verbose=False, kernel_settings=settings)
    model.set_hyperparams(np.log(np.asarray([0.3, 0.6])), ds)
    model.fit(ds, mode="exact")
    return model, ds, x, seqlen, tokens, table


@pytest.fixture(scope="module")
def fitted():
    return _fit("Conv1dRBF")


def _check_model(model, seqlen, tokens, table):
    k = model.kernel
    std = float(model.trainy_std)
    got = model.predict_substitutions(tokens, sequence_lengths=seqlen, token_table=table, chunk_size=16)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (N, L_, V_)
    assert exact_zeros(got, tokens, seqlen) and float(np.abs(got).max()) > 0
    # all L V mutants of three sequences through predict
    three = tokens[:3]
    mut = np.repeat(three, L_ * V_, axis=0).reshape(3, L_, V_, L_)
    for l in range(L_):
        mut[:, l, :, l] = np.arange(V_, dtype=np.uint8)[None, :]
    lens = np.repeat(seqlen[:3], L_ * V_)
    pm = model.predict(mut.reshape(-1, L_), sequence_lengths=lens, token_table=table).reshape(3, L_, V_)
    p0 = model.predict(three, sequence_lengths=seqlen[:3], token_table=table)
    want = pm - p0[:, None, None]
    want[np.arange(L_)[None, :] >= seqlen[:3, None]] = 0.0       # (a mutation past the length changes nothing: predict agrees, up to rounding)
    scaled = (table.astype(np.float64) * float(k.hyperparams[1])).astype(np.float32)
    w = model.weights.cpu().numpy()
    chi = k.chi_arr.cpu().numpy()
    cap = dss.cap_subst_scan(scaled, seqlen[:3], w, chi, k.conv_width, k.scaling_type, True)
    row = dr.cap_conv(np.float32, scaled[mut.reshape(-1, L_)], lens, chi, k.conv_width, k.scaling_type, u_out=U32)
    bound = (cap + 2 * float(np.abs(w).sum()) * row) * std
    err = float(np.abs(got[:3] - want).max())
    print(f"SUBST model      {model.kernel_choice:<40} scan-predict {err:.3e}  bound {bound:.3e}  max|want| {float(np.abs(want).max()):.3e}")
    assert err <= bound
    # ... and the dense reference itself, in the units of y
    ref = dss.subst_scan(tokens[:3], scaled, seqlen[:3], w, k.radem_diag.cpu().numpy(), chi, k.conv_width, k.scaling_type, True) * std
    assert report("model", model.kernel_choice, got[:3], ref, cap * std) <= cap * std + dr.U64 * float(np.abs(ref).max())   # (the product with std)
    # a TokenBatch is the same input
    from xgpr_amd.dataset import TokenBatch
    tb = TokenBatch(torch.from_numpy(tokens), torch.from_numpy(table))
    assert np.array_equal(model.predict_substitutions(tb, sequence_lengths=seqlen), got)


def test_predict_substitutions_conv1d(fitted):
    model, _, _, seqlen, tokens, table = fitted
    _check_model(model, seqlen, tokens, table)


def test_predict_substitutions_graph():
    model, _, _, seqlen, tokens, table = _fit("GraphRBF")
    assert model.kernel.conv_width == 1
    _check_model(model, seqlen, tokens, table)


def test_predict_substitutions_refusals(fitted):
    from xgpr_amd.models import xGPRegression
    model, ds, x, seqlen, tokens, table = fitted
    with pytest.raises(RuntimeError, match="sequence_lengths is required"):
        model.predict_substitutions(tokens[:3], token_table=table)
    with pytest.raises(RuntimeError, match="needs token input"):
        model.predict_substitutions(x[:3], sequence_lengths=seqlen[:3])
    fresh = xGPRegression(num_rffs=128, variance_rffs=32, kernel_choice="Conv1dRBF", device=DEV, verbose=False,
                          kernel_settings={"conv_width": CW, "averaging": "sqrt", "intercept": True})
    with pytest.raises(RuntimeError, match="not yet been successfully fitted"):
        fresh.predict_substitutions(tokens[:3], sequence_lengths=seqlen[:3], token_table=table)
    two = xGPRegression(num_rffs=128, variance_rffs=32, kernel_choice="Conv1dTwoLayer", device=DEV, verbose=False,
                        kernel_settings={"conv_width": CW, "init_rffs": 64, "intercept": True})
    two.set_hyperparams(dataset=ds)
    two.weights = torch.zeros(128, dtype=F64, device=DEV)                  # (the refusal is about the kernel, not the fit)
    with pytest.raises(RuntimeError, match="Conv1dRBF, Conv1dMatern"):
        two.predict_substitutions(tokens[:3], sequence_lengths=seqlen[:3], token_table=table)
    from xgpr_amd.dataset import build_regression_dataset
    flat = build_regression_dataset(x[:, 0, :], np.arange(N, dtype=np.float64), chunk_size=25, device=DEV)
    for choice in ("RBF", "Linear", "MiniARD"):
        settings = {"intercept": True}
        if choice == "MiniARD":
            settings["split_points"] = [2]
        other = xGPRegression(num_rffs=128, variance_rffs=32, kernel_choice=choice, device=DEV, verbose=False, kernel_settings=settings)
        other.set_hyperparams(dataset=flat)
        other.weights = torch.zeros(128, dtype=F64, device=DEV)
        with pytest.raises(RuntimeError, match="Conv1dRBF, Conv1dMatern"):
            other.predict_substitutions(tokens[:3], sequence_lengths=seqlen[:3], token_table=table)
