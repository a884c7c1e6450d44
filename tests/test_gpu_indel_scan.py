"""The window scores and the single-deletion / single-insertion scan of the sequence / graph kernels on the device
(xgpr_conv_token_window_scores_f32, xgpr_conv_token_indel_scan_f32, ConvSORFKernel.window_scores / indel_scan / indel_scan_composed,
xGPRegression.predict_indels / predict_window_scores) against the long-double brute-force reference of tests/dense_indel_scan.py,
within its a-priori caps (derived from the operation count; tests/test_indel_scan_host.py holds them to 1e-2 of every case's largest
output and shows what they separate) -- or bit for bit where a test says so.  No element is excused: zeros are +0.0 bitwise, NaNs sit
exactly where the contract puts them.  Every comparison prints one ``INDEL`` line with measured error and cap."""
import numpy as np
import pytest
import torch

import dense_indel_scan as dis
import dense_reference as dr
from dense_reference import U32
from guarded import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def run_operator(ext, c, cw, scaling, icpt, rows=None, want=("del", "ins")):
    """The two ext calls on the case's sequences (``rows``: a subset, in that order); the outputs start as NaN (scores, ins) / 1.0
    (del, whose contract has NaNs of its own).  -> (scores, del or None, ins or None)."""
    rows = np.arange(c["tokens"].shape[0]) if rows is None else np.asarray(rows)
    tokens = np.ascontiguousarray(c["tokens"][rows])
    n, L = tokens.shape
    lens = np.ascontiguousarray(c["seqlen"][rows])
    dev = [torch.from_numpy(a).to(DEV) for a in (tokens, c["table"], c["w"])]
    radem, chi = torch.from_numpy(c["radem"]).to(DEV), torch.from_numpy(c["chi"]).to(DEV)
    scores = torch.full((n, L), float("nan"), dtype=F64, device=DEV)
    ext.hipConvTokenWindowScores(*dev, scores, radem, chi, lens, cw, icpt)
    dele = torch.full((n, L), 1.0, dtype=F64, device=DEV) if "del" in want else None
    ins = torch.full((n, L + 1, c["table"].shape[0]), float("nan"), dtype=F64, device=DEV) if "ins" in want else None
    ext.hipConvTokenIndelScan(*dev, scores, dele, ins, radem, chi, lens, cw, scaling, icpt)
    return scores, dele, ins


def report(tag, case, what, got, ref, cap):
    fin = np.isfinite(np.asarray(ref, dtype=np.float64))
    err = float(np.abs(np.asarray(got)[fin].astype(dr.LD) - ref[fin]).max()) if fin.any() else 0.0
    big = float(np.abs(ref[fin]).max()) if fin.any() else 0.0
    print(f"INDEL {tag:<9} {what:<6} {str(case):<40} hip-dense {err:.3e}  cap {cap:.3e}  ratio {err / cap:.4f}  max|ref| {big:.3e}")
    return err


def compare(tag, case, seqlen, cw, got, refs, caps):
    """scores, del, ins (numpy; None skips) against the reference: within the caps, zeros and NaNs exact."""
    L = refs[0].shape[1]
    masks = (dis.zero_mask(seqlen - cw + 1, L), dis.zero_mask(seqlen, L), dis.zero_mask(seqlen, L, gaps=True))
    for what, g, ref, cap, zeros in zip(("scores", "del", "ins"), got, refs, caps, masks):
        if g is None:
            continue
        assert report(tag, case, what, g, ref, cap) <= cap
        assert dis.check(g, ref, cap, zeros) <= cap


@pytest.mark.parametrize("name", [c[0] for c in dis.CASES])
def test_operator_against_the_dense_reference(ext, name):
    c, cw, scaling, icpt, sc, dele, ins, cs, cd, ci = dis.reference(name)
    out = run_operator(ext, c, cw, scaling, icpt)
    compare("operator", name, c["seqlen"], cw, [o.cpu().numpy() for o in out], (sc, dele, ins), (cs, cd, ci))
    again = run_operator(ext, c, cw, scaling, icpt)
    assert all(same_bits(a, b) for a, b in zip(out, again)), "two runs differ"
    assert float(out[0].abs().max()) > 0 and float(out[2].abs().max()) > 0
    # the scores' identity: r(nk) sum_j scores (+ w[0]) is the feature row times w
    F = c["chi"].shape[0]
    z = dr.conv_features(c["table"].astype(dr.LD)[c["tokens"].astype(np.int64) % c["table"].shape[0]], c["seqlen"], c["radem"], c["chi"], cw, scaling)
    w = np.asarray(c["w"], dtype=dr.LD)
    if icpt:
        z[:, 0] = 1
    got = out[0].cpu().numpy().astype(dr.LD)
    for i, s in enumerate(c["seqlen"]):
        nk = int(s) - cw + 1
        r = dr.conv_row_scale(F, nk, scaling)
        assert abs(float(r * got[i].sum() + (w[0] if icpt else 0) - z[i] @ w)) <= float(r) * nk * cs * (1 + 1e-9)


def test_two_identical_table_rows_give_bit_equal_insertion_columns(ext):
    c, cw, scaling, icpt = dis.reference("dup_rows")[:4]
    assert (c["table"][1] == c["table"][3]).all()
    _, _, ins = run_operator(ext, c, cw, scaling, icpt)
    assert same_bits(ins[:, :, 1].contiguous(), ins[:, :, 3].contiguous())
    assert not same_bits(ins[:, :, 1].contiguous(), ins[:, :, 2].contiguous())


@pytest.mark.parametrize("name", ["w256_c21_cw9", "w1024_c21_cw48", "n65"])
def test_a_sequence_alone_and_inside_a_batch(ext, name):
    c, cw, scaling, icpt = dis.case(name)
    n = c["tokens"].shape[0]
    whole = run_operator(ext, c, cw, scaling, icpt)
    for i in sorted({0, n // 2, n - 1}):
        alone = run_operator(ext, c, cw, scaling, icpt, rows=[i])
        assert all(same_bits(a[0], b[i]) for a, b in zip(alone, whole)), i
    back = run_operator(ext, c, cw, scaling, icpt, rows=np.arange(n)[::-1])      # every sequence at another index
    assert all(same_bits(a.flip(0).contiguous(), b) for a, b in zip(back, whole))


@pytest.mark.parametrize("name", ["dup_rows", "w128_c21_cw6"])
def test_either_output_may_be_left_out(ext, name):
    c, cw, scaling, icpt = dis.case(name)
    _, dele, ins = run_operator(ext, c, cw, scaling, icpt)
    _, d_only, none = run_operator(ext, c, cw, scaling, icpt, want=("del",))
    assert none is None and same_bits(d_only, dele)
    _, none, i_only = run_operator(ext, c, cw, scaling, icpt, want=("ins",))
    assert none is None and same_bits(i_only, ins)
    with pytest.raises(RuntimeError, match="both NULL"):
        run_operator(ext, c, cw, scaling, icpt, want=())


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
    """-> (scores, del, ins), (cap_scores, cap_del, cap_ins) for kernel object k."""
    radem, chi = k.radem_diag.cpu().numpy(), k.chi_arr.cpu().numpy()
    a = (tokens, scaled, seqlen, w, radem, chi, k.conv_width)
    dele, ins = dis.indel_scan(*a, k.scaling_type, k.fit_intercept)
    return (dis.window_scores(*a, k.fit_intercept), dele, ins), \
        (dis.cap_window_scores(scaled, w, chi, k.conv_width, k.fit_intercept),
         *dis.cap_indel_scan(scaled, seqlen, w, chi, k.conv_width, k.scaling_type, k.fit_intercept))


@pytest.mark.parametrize("choice", ["Conv1dRBF", "Conv1dMatern", "Conv1dCauchy", "GraphRBF"])
def test_kernel_indel_scan_is_the_ext_call_bit_for_bit(ext, choice):
    from xgpr_amd.dataset import TokenBatch
    n, L, C, cw, M, V = 4, 9, 6, 4, 600, 5
    k = _kernel(choice, n, L, C, cw, M, averaging="full" if choice == "GraphRBF" else "sqrt")
    tokens, table, scaled, seqlen, w = _kernel_case(k, n, L, V, 31, (9, 4, 5, 8) if k.conv_width > 1 else (9, 1, 2, 8))
    batch = TokenBatch(torch.from_numpy(tokens).to(DEV), torch.from_numpy(table).to(DEV))
    dele, ins = k.indel_scan(batch, seqlen, w)
    scores = k.window_scores(batch, seqlen, w)
    assert all(t.dtype == F64 and t.is_cuda for t in (dele, ins, scores))
    assert tuple(dele.shape) == (n, L) and tuple(ins.shape) == (n, L + 1, V) and tuple(scores.shape) == (n, L)
    c = dict(tokens=tokens, table=scaled, w=w, radem=k.radem_diag.cpu().numpy(), chi=k.chi_arr.cpu().numpy(), seqlen=seqlen)
    want = run_operator(ext, c, k.conv_width, k.scaling_type, k.fit_intercept)
    assert same_bits(scores, want[0]) and same_bits(dele, want[1]) and same_bits(ins, want[2])
    refs, caps = _dense(k, tokens, scaled, seqlen, w)
    compare("kernel", (choice, C, k.conv_width, L, M // 2, n), seqlen, k.conv_width, [t.cpu().numpy() for t in (scores, dele, ins)], refs, caps)
    with pytest.raises(RuntimeError, match="sequence_length is required"):
        k.indel_scan(batch, None, w)
    with pytest.raises(RuntimeError, match="num_rffs"):
        k.indel_scan(batch, seqlen, w[:-2])
    with pytest.raises(RuntimeError, match="TokenBatch"):
        k.window_scores(table[tokens], seqlen, w)


def _mutants(tokens, seqlen, V):
    """Every deletion and insertion mutant the contract defines, written into arrays of L + 1 positions -> (rows [m, L + 1] uint8,
    lengths [m]); deletions first (i, p), then insertions (i, g, v)."""
    n, L = tokens.shape
    rows, lens = [], []
    for i in range(n):
        s = int(seqlen[i])
        t = list(tokens[i, :s])
        for p in range(s):
            rows.append(t[:p] + t[p + 1:])
            lens.append(s - 1)
    for i in range(n):
        s = int(seqlen[i])
        t = list(tokens[i, :s])
        for g in range(s + 1):
            for v in range(V):
                rows.append(t[:g] + [v] + t[g:])
                lens.append(s + 1)
    out = np.zeros((len(rows), L + 1), dtype=np.uint8)
    for r, row in enumerate(rows):
        out[r, :len(row)] = row
    return out, np.asarray(lens, dtype=np.int32)


def _composed_cap(k, tokens, scaled, seqlen, w):
    """The composed route: float32 feature rows of a mutant and of the sequence (each entry within cap_conv with u_out = U32 of
    exact), each multiplied by the weights in float64 -- twice sum|w| cap_conv, over the windows of every mutant that has one (and of the
    sequences themselves).  Derived as tests/test_gpu_subst_scan.py derives its own."""
    cw = k.conv_width
    mut, lens = _mutants(tokens, seqlen, scaled.shape[0])
    keep = lens >= cw
    base = np.concatenate([tokens, np.zeros((tokens.shape[0], 1), dtype=np.uint8)], axis=1)
    base[np.arange(base.shape[1])[None, :] >= seqlen[:, None]] = 0              # (positions past a length: never part of a window)
    x = scaled[np.concatenate([mut[keep], base])]
    row = dr.cap_conv(np.float32, x, np.concatenate([lens[keep], seqlen]), k.chi_arr.cpu().numpy(), cw, k.scaling_type, u_out=U32)
    sw = float(np.abs(w[1:] if k.fit_intercept else w).sum())
    return 2 * sw * row


def test_the_composed_route_against_the_dense_reference_and_beyond_the_operator(ext):
    from xgpr_amd.dataset import TokenBatch
    n, L, C, cw, M, V = 3, 8, 6, 3, 400, 5
    k = _kernel("Conv1dRBF", n, L, C, cw, M)
    tokens, table, scaled, seqlen, w = _kernel_case(k, n, L, V, 32, (8, 3, 4))
    tokens[np.arange(L)[None, :] >= seqlen[:, None]] = 255                        # a row the table does not have: never read
    batch = TokenBatch(torch.from_numpy(tokens).to(DEV), torch.from_numpy(table).to(DEV))
    refs, caps = _dense(k, tokens, scaled, seqlen, w)
    k.COMPOSED_SCAN_ELEMS = 37 * M                               # several slices, the last one ragged
    fd, fi = (t.cpu().numpy() for t in k.indel_scan_composed(batch, seqlen, w))
    ccap = _composed_cap(k, tokens, scaled, seqlen, w)
    compare("composed", (C, cw, L, M // 2, n), seqlen, cw, [None, fd, fi], refs, (None, ccap, ccap))
    od, oi = (t.cpu().numpy() for t in k.indel_scan(batch, seqlen, w))
    fin = np.isfinite(od)
    assert np.array_equal(fin, np.isfinite(fd))
    assert float(np.abs(od - fd)[fin].max()) <= caps[1] + ccap and float(np.abs(oi - fi).max()) <= caps[2] + ccap
    # a window of 9 x 128 = 1152 elements (P = 2048): the operator refuses, the kernel object takes the composed route
    n, L, C, cw, M, V = 2, 10, 128, 9, 128, 3
    k = _kernel("Conv1dRBF", n, L, C, cw, M, icpt=False)
    tokens, table, scaled, seqlen, w = _kernel_case(k, n, L, V, 33, (9, 10))
    assert ext.conv_token_indel_scan_ok(cw * C, V, C, M // 2) == 0
    c = dict(tokens=tokens, table=scaled, w=w, radem=k.radem_diag.cpu().numpy(), chi=k.chi_arr.cpu().numpy(), seqlen=seqlen)
    with pytest.raises(RuntimeError, match="the indel scan serves windows of up to 1024 elements"):
        run_operator(ext, c, cw, 1, False)
    batch = TokenBatch(torch.from_numpy(tokens).to(DEV), torch.from_numpy(table).to(DEV))
    gd, gi = (t.cpu().numpy() for t in k.indel_scan(batch, seqlen, w))
    gs = k.window_scores(batch, seqlen, w).cpu().numpy()
    refs, caps = _dense(k, tokens, scaled, seqlen, w)
    ccap = _composed_cap(k, tokens, scaled, seqlen, w)
    # (a window's score from a float32 row of one window: sum|w| cap_conv of that row, divided by the row's constant sqrt(1 / F))
    wins = np.stack([scaled[tokens[i, j:j + cw]] for i in range(n) for j in range(L - cw + 1)])
    scap = float(np.abs(w).sum()) * dr.cap_conv(np.float32, wins, np.full(wins.shape[0], cw), k.chi_arr.cpu().numpy(), cw,
                                                k.scaling_type, u_out=U32) / float(np.sqrt(1.0 / k.num_freqs))
    compare("composed", (C, cw, L, M // 2, n), seqlen, cw, [gs, gd, gi], refs, (scap, ccap, ccap))
    # tokens that are not contiguous take the composed route as well
    wide = torch.from_numpy(np.concatenate([tokens, tokens], axis=1)).to(DEV)
    assert not wide[:, :L].is_contiguous()
    ad, ai = k.indel_scan(TokenBatch(wide[:, :L], batch.table), seqlen, w)
    assert np.array_equal(ad.cpu().numpy(), gd, equal_nan=True) and np.array_equal(ai.cpu().numpy(), gi)


# ------------------------------------------------------------------------------------------------ predict_indels end to end
N, L_, C_, CW, V_ = 40, 12, 4, 3, 5


def _fit(choice):
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.models import xGPRegression
    rng = np.random.default_rng(34)
    table = rng.uniform(-1, 1, size=(V_, C_)).astype(np.float32)
    tokens = rng.integers(0, V_, size=(N, L_)).astype(np.uint8)
    seqlen = rng.integers(CW, L_ + 1, size=N).astype(np.int32)
    seqlen[:3] = (L_ - 1, CW, 7)
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
    cw, std = k.conv_width, float(model.trainy_std)
    dele, ins = model.predict_indels(tokens, sequence_lengths=seqlen, token_table=table, chunk_size=16)
    ws = model.predict_window_scores(tokens, sequence_lengths=seqlen, token_table=table, chunk_size=16)
    assert all(isinstance(a, np.ndarray) and a.dtype == np.float64 for a in (dele, ins, ws))
    assert dele.shape == (N, L_) and ins.shape == (N, L_ + 1, V_) and ws.shape == (N, L_)
    for got, zeros in ((dele, dis.zero_mask(seqlen, L_)), (ins, dis.zero_mask(seqlen, L_, gaps=True)), (ws, dis.zero_mask(seqlen - cw + 1, L_))):
        assert (got[zeros] == 0).all() and not np.signbit(got[zeros]).any()
    assert np.array_equal(np.isnan(dele), (np.arange(L_)[None, :] < seqlen[:, None]) & (seqlen[:, None] == cw))
    assert not np.isnan(ins).any() and float(np.abs(ins).max()) > 0
    # explicitly built mutants of three sequences (no longer than L: predict takes arrays of L positions) through predict
    scaled = (table.astype(np.float64) * float(k.hyperparams[1])).astype(np.float32)
    w = model.weights.cpu().numpy()
    chi = k.chi_arr.cpu().numpy()
    cd, ci = dis.cap_indel_scan(scaled, seqlen[:3], w, chi, cw, k.scaling_type, True)
    p0 = model.predict(tokens[:3], sequence_lengths=seqlen[:3], token_table=table)
    sw = float(np.abs(w).sum())
    checked = 0
    for i in range(3):
        s = int(seqlen[i])
        t = list(tokens[i, :s])
        edits = [("del", p, None, t[:p] + t[p + 1:]) for p in (0, s // 2, s - 1) if s > cw]
        edits += [("ins", g, v, t[:g] + [v] + t[g:]) for g, v in ((0, 1), (s // 2, 4), (s, 2)) if s < L_]
        for kind, at, v, mt in edits:
            row = np.zeros((1, L_), dtype=np.uint8)
            row[0, :len(mt)] = mt
            lens = np.asarray([len(mt)], dtype=np.int32)
            want = float(model.predict(row, sequence_lengths=lens, token_table=table)[0] - p0[i])
            got = float(dele[i, at] if kind == "del" else ins[i, at, v])
            both = np.concatenate([scaled[row], scaled[tokens[i:i + 1]]])
            rowcap = dr.cap_conv(np.float32, both, np.asarray([len(mt), s]), chi, cw, k.scaling_type, u_out=U32)
            bound = ((cd if kind == "del" else ci) + 2 * sw * rowcap) * std
            print(f"INDEL model     {kind:<6} {model.kernel_choice:<12} seq {i} at {at} v {v}  scan-predict {abs(got - want):.3e}  bound {bound:.3e}")
            assert abs(got - want) <= bound
            checked += 1
    assert checked >= 6
    # the window scores sum to predict, minus the offsets
    pall = model.predict(tokens, sequence_lengths=seqlen, token_table=table)
    offset = float(model.trainy_mean) + float(w[0]) * std
    cs = dis.cap_window_scores(scaled, w, chi, cw, True)
    for i in range(N):
        nk = int(seqlen[i]) - cw + 1
        r = float(dr.conv_row_scale(chi.shape[0], nk, k.scaling_type))
        rowcap = dr.cap_conv(np.float32, scaled[tokens[i:i + 1] % V_], seqlen[i:i + 1], chi, cw, k.scaling_type, u_out=U32)
        assert abs(ws[i].sum() + offset - pall[i]) <= (r * nk * cs + sw * rowcap) * std + 8 * dr.U64 * (abs(pall[i]) + abs(offset))
    # a TokenBatch is the same input
    from xgpr_amd.dataset import TokenBatch
    tb = TokenBatch(torch.from_numpy(tokens), torch.from_numpy(table))
    d2, i2 = model.predict_indels(tb, sequence_lengths=seqlen)
    assert np.array_equal(d2, dele, equal_nan=True) and np.array_equal(i2, ins)


def test_predict_indels_conv1d(fitted):
    model, _, _, seqlen, tokens, table = fitted
    _check_model(model, seqlen, tokens, table)


def test_predict_indels_graph():
    model, _, _, seqlen, tokens, table = _fit("GraphRBF")
    assert model.kernel.conv_width == 1
    _check_model(model, seqlen, tokens, table)


def test_predict_indels_refusals(fitted):
    from xgpr_amd.models import xGPRegression
    model, ds, x, seqlen, tokens, table = fitted
    for method in (model.predict_indels, model.predict_window_scores):
        with pytest.raises(RuntimeError, match="sequence_lengths is required"):
            method(tokens[:3], token_table=table)
        with pytest.raises(RuntimeError, match="needs token input"):
            method(x[:3], sequence_lengths=seqlen[:3])
    fresh = xGPRegression(num_rffs=128, variance_rffs=32, kernel_choice="Conv1dRBF", device=DEV, verbose=False,
                          kernel_settings={"conv_width": CW, "averaging": "sqrt", "intercept": True})
    two = xGPRegression(num_rffs=128, variance_rffs=32, kernel_choice="Conv1dTwoLayer", device=DEV, verbose=False,
                        kernel_settings={"conv_width": CW, "init_rffs": 64, "intercept": True})
    two.set_hyperparams(dataset=ds)
    two.weights = torch.zeros(128, dtype=F64, device=DEV)                  # (the refusal is about the kernel, not the fit)
    from xgpr_amd.dataset import build_regression_dataset
    flat = build_regression_dataset(x[:, 0, :], np.arange(N, dtype=np.float64), chunk_size=25, device=DEV)
    rbf = xGPRegression(num_rffs=128, variance_rffs=32, kernel_choice="RBF", device=DEV, verbose=False, kernel_settings={"intercept": True})
    rbf.set_hyperparams(dataset=flat)
    rbf.weights = torch.zeros(128, dtype=F64, device=DEV)
    for name in ("predict_indels", "predict_window_scores"):
        with pytest.raises(RuntimeError, match="not yet been successfully fitted"):
            getattr(fresh, name)(tokens[:3], sequence_lengths=seqlen[:3], token_table=table)
        for other in (two, rbf):
            with pytest.raises(RuntimeError, match="Conv1dRBF, Conv1dMatern"):
                getattr(other, name)(tokens[:3], sequence_lengths=seqlen[:3], token_table=table)
