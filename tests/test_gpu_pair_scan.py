"""The pairwise substitution (epistasis) scan of the sequence / graph kernels on the device (xgpr_conv_token_pair_scan_f32,
ConvSORFKernel.pair_substitution_scan / pair_substitution_scan_composed, xGPRegression.predict_substitution_pairs) against the
long-double dense reference of tests/dense_pair_scan.py, within its a-priori cap ``cap_pair_scan`` (derived from the operation count;
tests/test_pair_scan_host.py holds the cap to 1e-2 of every case's largest output and shows what it separates) -- or bit for bit where
a test says so.  No element is excused.  Every comparison prints one ``PAIR`` line with measured error and cap."""
import functools

import numpy as np
import pytest
import torch

import dense_pair_scan as dp
import dense_reference as dr
import dense_subst_scan as dss
from dense_reference import U32
from guarded import same_bits
from test_gpu_subst_scan import _fit, _kernel, _kernel_case

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
    got = dp.reference(name)
    got[4].setflags(write=False)
    return got


def run_operator(ext, c, cw, scaling, icpt, rows=None):
    """The ext call on the case's sequences (``rows``: a subset, in that order); the output starts as NaN."""
    rows = np.arange(c["tokens"].shape[0]) if rows is None else np.asarray(rows)
    tokens = np.ascontiguousarray(c["tokens"][rows])
    V = c["table"].shape[0]
    out = torch.full((tokens.shape[0], tokens.shape[1], cw - 1, V, V), float("nan"), dtype=F64, device=DEV)
    ext.hipConvTokenPairScan(torch.from_numpy(tokens).to(DEV), torch.from_numpy(c["table"]).to(DEV), torch.from_numpy(c["w"]).to(DEV), out,
                             torch.from_numpy(c["radem"]).to(DEV), torch.from_numpy(c["chi"]).to(DEV),
                             np.ascontiguousarray(c["seqlen"][rows]), cw, scaling, icpt)
    return out


def report(tag, case, got, ref, cap):
    err = float(np.abs(got.astype(dr.LD) - ref).max()) if ref.size else 0.0
    big = float(np.abs(ref).max()) if ref.size else 0.0
    print(f"PAIR {tag:<10} {str(case):<40} hip-dense {err:.3e}  cap {cap:.3e}  ratio {err / cap:.4f}  max|ref| {big:.3e}")
    return err


def exact_zeros(got, tokens, seqlen):
    """+0.0, bitwise, on both own-token planes of every slot inside a sequence and on every slot with a position past its length."""
    n, L, band = got.shape[:3]
    for i in range(n):
        s = int(seqlen[i])
        for l1 in range(L):
            for d in range(1, band + 1):
                blk = got[i, l1, d - 1]
                z = blk if l1 + d >= s else np.concatenate([blk[tokens[i, l1], :], blk[:, tokens[i, l1 + d]]])
                if (z != 0).any() or np.signbit(z).any():
                    return False
    return True


@pytest.mark.parametrize("name", [c[0] for c in dp.CASES])
def test_operator_against_the_dense_reference(ext, name):
    c, cw, scaling, icpt, ref, cap = reference(name)
    out = run_operator(ext, c, cw, scaling, icpt)               # (pre-filled with NaN: overwritten as a whole)
    got = out.cpu().numpy()
    assert got.shape == ref.shape
    assert report("operator", name, got, ref, cap) <= cap
    assert dp.check(got, ref, cap) <= cap
    assert exact_zeros(got, c["tokens"], c["seqlen"])
    assert same_bits(out, run_operator(ext, c, cw, scaling, icpt)), "two runs differ"
    if name in dp.DEGENERATE:
        assert (got == 0).all()
    else:
        assert float(np.abs(got).max()) > 0


def test_two_identical_table_rows_give_bit_equal_slices_on_both_token_axes(ext):
    c, cw, scaling, icpt, _, _ = reference("dup_rows")
    assert (c["table"][1] == c["table"][3]).all()
    out = run_operator(ext, c, cw, scaling, icpt)
    assert same_bits(out[:, :, :, 1, :].contiguous(), out[:, :, :, 3, :].contiguous())
    assert same_bits(out[:, :, :, :, 1].contiguous(), out[:, :, :, :, 3].contiguous())
    assert not same_bits(out[:, :, :, 1, :].contiguous(), out[:, :, :, 2, :].contiguous())
    assert not same_bits(out[:, :, :, :, 1].contiguous(), out[:, :, :, :, 2].contiguous())


@pytest.mark.parametrize("name", ["w128_c21_cw6", "w1024_c120_cw8", "n65"])
def test_a_sequence_alone_and_inside_a_batch(ext, name):
    c, cw, scaling, icpt, _, _ = reference(name)
    n = c["tokens"].shape[0]
    whole = run_operator(ext, c, cw, scaling, icpt)
    for i in sorted({0, n // 2, n - 1}):
        assert same_bits(run_operator(ext, c, cw, scaling, icpt, rows=[i])[0], whole[i]), i
    back = run_operator(ext, c, cw, scaling, icpt, rows=np.arange(n)[::-1])      # every sequence at another index
    assert same_bits(back.flip(0).contiguous(), whole)


# ------------------------------------------------------------------------------------------------ the kernel object
def _dense(k, tokens, scaled, seqlen, w):
    radem, chi = k.radem_diag.cpu().numpy(), k.chi_arr.cpu().numpy()
    ref = dp.pair_scan(tokens, scaled, seqlen, w, radem, chi, k.conv_width, k.scaling_type, k.fit_intercept)
    return ref, dp.cap_pair_scan(scaled, seqlen, w, chi, k.conv_width, k.scaling_type, k.fit_intercept)


@pytest.mark.parametrize("choice", ["Conv1dRBF", "Conv1dMatern", "Conv1dCauchy", "GraphRBF"])
def test_kernel_pair_substitution_scan_is_the_ext_call_bit_for_bit(ext, choice):
    from xgpr_amd.dataset import TokenBatch
    n, L, C, cw, M, V = 4, 9, 6, 4, 600, 5
    k = _kernel(choice, n, L, C, cw, M, averaging="full" if choice == "GraphRBF" else "sqrt")
    tokens, table, scaled, seqlen, w = _kernel_case(k, n, L, V, 41, (9, 4, 6, 8) if k.conv_width > 1 else (9, 1, 6, 8))
    batch = TokenBatch(torch.from_numpy(tokens).to(DEV), torch.from_numpy(table).to(DEV))
    got = k.pair_substitution_scan(batch, seqlen, w)
    band = k.conv_width - 1
    assert got.dtype == F64 and tuple(got.shape) == (n, L, band, V, V) and got.is_cuda
    out = torch.full((n, L, band, V, V), float("nan"), dtype=F64, device=DEV)
    ext.hipConvTokenPairScan(batch.tokens, torch.from_numpy(scaled).to(DEV), torch.from_numpy(w).to(DEV), out, k.radem_diag, k.chi_arr,
                             seqlen, k.conv_width, k.scaling_type, k.fit_intercept)
    assert same_bits(got, out)
    ref, cap = _dense(k, tokens, scaled, seqlen, w)
    assert report("kernel", (choice, C, k.conv_width, L, M // 2, n), got.cpu().numpy(), ref, cap) <= cap
    assert exact_zeros(got.cpu().numpy(), tokens, seqlen)
    # a batch beyond one launch's rows goes to the operator in slices: the same bits
    k.PAIR_SCAN_ROWS = 2 * L * max(band, 1) * V + 1
    assert same_bits(k.pair_substitution_scan(batch, seqlen, w), out)
    with pytest.raises(RuntimeError, match="sequence_length is required"):
        k.pair_substitution_scan(batch, None, w)
    with pytest.raises(RuntimeError, match="num_rffs"):
        k.pair_substitution_scan(batch, seqlen, w[:-2])
    with pytest.raises(RuntimeError, match="TokenBatch"):
        k.pair_substitution_scan(table[tokens], seqlen, w)


def _double_mutants(tokens, V, cw_band):
    """Every double mutant of the band written out: uint8 [n, L, band, V, V, L] (the second position clamped into the array: those
    slots lie past every length that reaches them) -- with the two single mutants and the sequence itself, the rows the composed
    route forms."""
    n, L = tokens.shape
    mut = np.broadcast_to(tokens[:, None, None, None, None, :], (n, L, cw_band, V, V, L)).copy()
    for l1 in range(L):
        for d in range(1, cw_band + 1):
            mut[:, l1, d - 1, :, :, l1] = np.arange(V, dtype=np.uint8)[None, :, None]
            if l1 + d < L:
                mut[:, l1, d - 1, :, :, l1 + d] = np.arange(V, dtype=np.uint8)[None, None, :]
    return mut


def _composed_cap(k, tokens, scaled, seqlen, w):
    """The composed route: four float32 feature rows -- the double mutant, the two single mutants, the sequence (each entry within
    cap_conv with u_out = U32 of exact) --, each multiplied by the weights in float64: four times sum|w| cap_conv, as
    tests/test_gpu_subst_scan.py forms it for two, over the windows of every double mutant (a single mutant and the sequence itself
    are among them: the planes of the own tokens)."""
    n, L = tokens.shape
    V, band = scaled.shape[0], k.conv_width - 1
    mut = _double_mutants(tokens, V, band)
    lens = np.repeat(seqlen, L * band * V * V)
    x = scaled[mut.reshape(-1, L) % V]                           # (positions past a length hold 255: never part of a window)
    row = dr.cap_conv(np.float32, x, lens, k.chi_arr.cpu().numpy(), k.conv_width, k.scaling_type, u_out=U32)
    sw = float(np.abs(w[1:] if k.fit_intercept else w).sum())
    return 4 * sw * row


def test_the_composed_route_against_the_dense_reference_and_beyond_the_operator(ext):
    from xgpr_amd.dataset import TokenBatch
    n, L, C, cw, M, V = 3, 8, 6, 3, 400, 5
    k = _kernel("Conv1dRBF", n, L, C, cw, M)
    tokens, table, scaled, seqlen, w = _kernel_case(k, n, L, V, 42, (8, 3, 5))
    batch = TokenBatch(torch.from_numpy(tokens).to(DEV), torch.from_numpy(table).to(DEV))
    ref, cap = _dense(k, tokens, scaled, seqlen, w)
    k.COMPOSED_SCAN_ELEMS = 37 * M                               # several slices, the last one ragged
    fb = k.pair_substitution_scan_composed(batch, seqlen, w).cpu().numpy()
    ccap = _composed_cap(k, tokens, scaled, seqlen, w)
    assert report("composed", (C, cw, L, M // 2, n), fb, ref, cap + ccap) <= cap + ccap
    assert exact_zeros(fb, tokens, seqlen)
    op = k.pair_substitution_scan(batch, seqlen, w).cpu().numpy()
    assert float(np.abs(op - fb).max()) <= 2 * cap + ccap
    # a window of 9 x 128 = 1152 elements (P = 2048): the operator refuses, the kernel object takes the composed route
    n, L, C, cw, M, V = 2, 10, 128, 9, 128, 3
    k = _kernel("Conv1dRBF", n, L, C, cw, M, icpt=False)
    tokens, table, scaled, seqlen, w = _kernel_case(k, n, L, V, 43, (9, 10))
    assert ext.conv_token_pair_scan_ok(cw * C, V, C, M // 2) == 0
    out = torch.zeros((n, L, cw - 1, V, V), dtype=F64, device=DEV)
    with pytest.raises(RuntimeError, match="the pair scan serves windows of up to 1024 elements"):
        ext.hipConvTokenPairScan(torch.from_numpy(tokens).to(DEV), torch.from_numpy(scaled).to(DEV), torch.from_numpy(w).to(DEV), out,
                                 k.radem_diag, k.chi_arr, seqlen, cw, 1, False)
    assert float(out.abs().max()) == 0.0                         # nothing is written
    batch = TokenBatch(torch.from_numpy(tokens).to(DEV), torch.from_numpy(table).to(DEV))
    got = k.pair_substitution_scan(batch, seqlen, w).cpu().numpy()
    ref, cap = _dense(k, tokens, scaled, seqlen, w)
    ccap = _composed_cap(k, tokens, scaled, seqlen, w)
    assert report("composed", (C, cw, L, M // 2, n), got, ref, cap + ccap) <= cap + ccap and exact_zeros(got, tokens, seqlen)
    # tokens that are not contiguous take the composed route as well
    wide = torch.from_numpy(np.concatenate([tokens, tokens], axis=1)).to(DEV)
    assert not wide[:, :L].is_contiguous()
    again = k.pair_substitution_scan(TokenBatch(wide[:, :L], batch.table), seqlen, w).cpu().numpy()
    assert np.array_equal(again, got)


# ------------------------------------------------------------------------------------------------ predict_substitution_pairs end to end
N, L_, C_, CW, V_ = 40, 12, 4, 3, 5          # the shape of tests/test_gpu_subst_scan.py's _fit


@pytest.fixture(scope="module")
def fitted():
    return _fit("Conv1dRBF")


def test_predict_substitution_pairs_conv1d(fitted):
    """predict(double mutant) - predict(sequence) = sub + sub + pairs for ALL position pairs of three sequences: inside the band, and
    at distance >= conv_width, where the pairs term is absent."""
    model, _, _, seqlen, tokens, table = fitted
    k = model.kernel
    std = float(model.trainy_std)
    pairs = model.predict_substitution_pairs(tokens, sequence_lengths=seqlen, token_table=table)
    assert isinstance(pairs, np.ndarray) and pairs.dtype == np.float64 and pairs.shape == (N, L_, CW - 1, V_, V_)
    assert exact_zeros(pairs, tokens, seqlen) and float(np.abs(pairs).max()) > 0
    sub = model.predict_substitutions(tokens[:3], sequence_lengths=seqlen[:3], token_table=table)
    three = tokens[:3]
    ps = [(l1, l2) for l1 in range(L_) for l2 in range(l1 + 1, L_)]
    mut = np.broadcast_to(three[:, None, None, None, :], (3, len(ps), V_, V_, L_)).copy()
    for p, (l1, l2) in enumerate(ps):
        mut[:, p, :, :, l1] = np.arange(V_, dtype=np.uint8)[None, :, None]
        mut[:, p, :, :, l2] = np.arange(V_, dtype=np.uint8)[None, None, :]
    lens = np.repeat(seqlen[:3], len(ps) * V_ * V_)
    pm = model.predict(mut.reshape(-1, L_), sequence_lengths=lens, token_table=table).reshape(3, len(ps), V_, V_)
    p0 = model.predict(three, sequence_lengths=seqlen[:3], token_table=table)
    want = pm - p0[:, None, None, None]
    got = np.zeros_like(want)
    for p, (l1, l2) in enumerate(ps):
        got[:, p] = sub[:, l1, :, None] + sub[:, l2, None, :]
        if l2 - l1 < CW:
            got[:, p] += pairs[:3, l1, l2 - l1 - 1]
    assert any(l2 - l1 >= CW for l1, l2 in ps) and any(l2 - l1 < CW for l1, l2 in ps)
    # the bound of test_gpu_subst_scan._check_model, extended to four rows: the two single scans and the pair scan within their caps,
    # predict's float32 rows of the double mutant and of the sequence within cap_conv each
    scaled = (table.astype(np.float64) * float(k.hyperparams[1])).astype(np.float32)
    w = model.weights.cpu().numpy()
    chi = k.chi_arr.cpu().numpy()
    cap1 = dss.cap_subst_scan(scaled, seqlen[:3], w, chi, k.conv_width, k.scaling_type, True)
    cap2 = dp.cap_pair_scan(scaled, seqlen[:3], w, chi, k.conv_width, k.scaling_type, True)
    row = dr.cap_conv(np.float32, scaled[mut.reshape(-1, L_)], lens, chi, k.conv_width, k.scaling_type, u_out=U32)
    bound = (2 * cap1 + cap2 + 2 * float(np.abs(w).sum()) * row) * std
    # (a position past the length is never read: predict sees the mutant with the other substitution alone, and so does the sum)
    err = float(np.abs(got - want).max())
    print(f"PAIR model      {model.kernel_choice:<40} scans-predict {err:.3e}  bound {bound:.3e}  max|want| {float(np.abs(want).max()):.3e}"
          f"  max|pairs| {float(np.abs(pairs[:3]).max()):.3e}")
    assert err <= bound
    assert float(np.abs(pairs[:3]).max()) > 100 * bound          # the term the identity needs is far above what the check resolves
    # ... and the dense reference itself, in the units of y
    ref = dp.pair_scan(tokens[:3], scaled, seqlen[:3], w, k.radem_diag.cpu().numpy(), chi, k.conv_width, k.scaling_type, True) * std
    assert report("model", model.kernel_choice, pairs[:3], ref, cap2 * std) <= cap2 * std + dr.U64 * float(np.abs(ref).max())
    # a TokenBatch is the same input, and so is another chunking
    from xgpr_amd.dataset import TokenBatch
    tb = TokenBatch(torch.from_numpy(tokens), torch.from_numpy(table))
    assert np.array_equal(model.predict_substitution_pairs(tb, sequence_lengths=seqlen, chunk_size=7), pairs)


def test_predict_substitution_pairs_graph():
    model, _, _, seqlen, tokens, table = _fit("GraphRBF")
    assert model.kernel.conv_width == 1
    pairs = model.predict_substitution_pairs(tokens, sequence_lengths=seqlen, token_table=table)
    assert pairs.shape == (N, L_, 0, V_, V_) and pairs.dtype == np.float64


def test_predict_substitution_pairs_refusals(fitted):
    from xgpr_amd.models import xGPRegression
    model, ds, x, seqlen, tokens, table = fitted
    with pytest.raises(RuntimeError, match="sequence_lengths is required"):
        model.predict_substitution_pairs(tokens[:3], token_table=table)
    with pytest.raises(RuntimeError, match="needs token input"):
        model.predict_substitution_pairs(x[:3], sequence_lengths=seqlen[:3])
    with pytest.raises(RuntimeError, match="shape\\[0\\] of sequence_lengths"):
        model.predict_substitution_pairs(tokens[:3], sequence_lengths=seqlen[:2], token_table=table)
    fresh = xGPRegression(num_rffs=128, variance_rffs=32, kernel_choice="Conv1dRBF", device=DEV, verbose=False,
                          kernel_settings={"conv_width": CW, "averaging": "sqrt", "intercept": True})
    with pytest.raises(RuntimeError, match="not yet been successfully fitted"):
        fresh.predict_substitution_pairs(tokens[:3], sequence_lengths=seqlen[:3], token_table=table)
    two = xGPRegression(num_rffs=128, variance_rffs=32, kernel_choice="Conv1dTwoLayer", device=DEV, verbose=False,
                        kernel_settings={"conv_width": CW, "init_rffs": 64, "intercept": True})
    two.set_hyperparams(dataset=ds)
    two.weights = torch.zeros(128, dtype=F64, device=DEV)                  # (the refusal is about the kernel, not the fit)
    with pytest.raises(RuntimeError, match="predict_substitution_pairs is available for the sequence and graph kernels Conv1dRBF, Conv1dMatern"):
        two.predict_substitution_pairs(tokens[:3], sequence_lengths=seqlen[:3], token_table=table)


def test_the_operators_refusals(ext):
    c, cw, scaling, icpt, _, _ = reference("w16_c4_cw3")
    n, L = c["tokens"].shape
    V = c["table"].shape[0]
    dev = {k: torch.from_numpy(c[k]).to(DEV) for k in ("tokens", "table", "w", "radem", "chi")}
    out = torch.zeros((n, L, cw - 1, V, V), dtype=F64, device=DEV)

    def call(**kw):
        a = dict(dev, out=out, seqlen=c["seqlen"], cw=cw)
        a.update(kw)
        ext.hipConvTokenPairScan(a["tokens"], a["table"], a["w"], a["out"], a["radem"], a["chi"], a["seqlen"], a["cw"], scaling, icpt)

    with pytest.raises(RuntimeError, match="Wrong array sizes"):
        call(out=torch.zeros((n, L, cw, V, V), dtype=F64, device=DEV))     # the band is conv_width - 1
    with pytest.raises(TypeError, match="5 dims"):
        call(out=torch.zeros((n, L, V), dtype=F64, device=DEV))
    with pytest.raises(TypeError, match="dtype"):
        call(out=out.float())
    with pytest.raises(RuntimeError, match="Wrong array sizes"):
        call(w=dev["w"][:-2].contiguous())
    with pytest.raises(RuntimeError):
        call(seqlen=np.asarray([9, 2, 4], dtype=np.int32))                 # a length below conv_width
    with pytest.raises(RuntimeError):
        call(seqlen=c["seqlen"][:2].copy())
    assert float(out.abs().max()) == 0.0                                   # no refusal wrote anything
