"""The backward of the two-layer kernel's first layer on the device (xgpr_conv_maxpool_input_grad_f32,
xgpr_conv_token_maxpool_input_grad_f32, Conv1dTwoLayerKernel.first_layer_gradient / input_gradient, xGPRegression.predict_gradient)
against the long-double dense reference of tests/dense_pool_input_grad.py, within its a-priori cap ``cap_pool_input_grad`` (derived from
the operation count; tests/test_pool_input_grad_host.py shows what it separates) -- or bit for bit where a test says so.

The winner of a max-pool is not continuous in the input: at an *ambiguous* (sequence, filter) pair -- the runner-up within twice the
float32 forward operator's cap of the maximum, or the maximum within that cap of the ReLU's kink -- a float32 operator may legitimately
pick another window or another side of the ReLU.  g is zeroed at those pairs (so they contribute nothing, whatever the device picks),
``argmax`` is compared everywhere else, and the ambiguous share of a case is asserted to be at most 5 %: a condition on the test's own
inputs, not a tolerance.  The consistency checks against the forward operator exclude nothing.  Every comparison prints one
``POOLGRAD`` line with measured error and cap; profiles/two_layer_input_grad_errors.txt is the collection of those lines from one run."""
import numpy as np
import pytest
import torch

import dense_input_grad as dig
import dense_pool_input_grad as dpg
import dense_reference as dr
from dense_reference import U64
from guarded import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64

# (C, conv_width) -> window d / padded P: 2/2 (conv_width 1); 12/16; 64/64 d = P; 105/128 the first two-layout width;
# 189/256 BASELINE configs[3]'s window; 1024/1024.
ARMS = [(2, 1), (4, 3), (8, 8), (21, 5), (21, 9), (128, 8)]
FS = [37, 300, 1024, 1324, 4500]            # a partial tile (F < P at the wider arms); ...; an exact tile; a ragged second tile; five tiles
MODES = ["shared", "rows", "rows_pad"]      # one vector; one row per sequence with stride == F; with stride > F and NaN in the pad
#         C  cw   L  lengths        n    F   mode
CASES = [(2, 1, 6, (1, 6, 3), 5, 37, "shared"),
         (2, 1, 6, (6, 2), 1, 300, "rows"),
         (4, 3, 5, (3, 4, 5), 5, 300, "rows_pad"),               # nk = 1, 2 < conv_width: the ring never wraps
         (4, 3, 9, (9, 5), 1, 4500, "rows"),                     # five tiles: a wave owns two (the tile loops' second trip)
         (8, 8, 12, (8, 10, 12), 5, 1024, "rows"),
         (21, 5, 12, (5, 9, 12), 5, 1324, "shared"),
         (21, 9, 40, (9, 23, 40), 5, 1324, "rows_pad"),
         (21, 9, 12, (9, 12, 10), 5, 37, "rows"),                # F < P
         (128, 8, 10, (8, 9, 10), 5, 37, "shared"),              # F < P at the full width
         (128, 8, 10, (10,), 1, 1324, "rows_pad")]


def test_the_case_list_covers_every_axis():
    assert {(c[0], c[1]) for c in CASES} == set(ARMS) and {c[5] for c in CASES} == set(FS)
    assert {c[4] for c in CASES} == {1, 5} and {c[6] for c in CASES} == set(MODES)
    assert any(min(c[3]) == c[1] for c in CASES) and any(c[1] > 1 and min(c[3]) - c[1] + 1 < c[1] for c in CASES)


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_operator(ext, x, seqlen, g, radem, chi, cw):
    """out prefilled with NaN, argmax with garbage: finite / in range everywhere means fully overwritten."""
    out = torch.full(x.shape, float("nan"), dtype=F64, device=DEV)
    argmax = torch.full((x.shape[0], chi.shape[0]), -77, dtype=torch.int32, device=DEV)
    ext.hipConvMaxpoolInputGrad(dev(x), g if isinstance(g, torch.Tensor) else dev(g), out, argmax, dev(radem), dev(chi), seqlen, cw)
    return out, argmax


def run_tokens(ext, tokens, table, seqlen, g, radem, chi, cw):
    out = torch.full(tokens.shape + (table.shape[1],), float("nan"), dtype=F64, device=DEV)
    argmax = torch.full((tokens.shape[0], chi.shape[0]), -77, dtype=torch.int32, device=DEV)
    ext.hipConvTokenMaxpoolInputGrad(dev(tokens), dev(table), g if isinstance(g, torch.Tensor) else dev(g), out, argmax, dev(radem),
                                     dev(chi), seqlen, cw)
    return out, argmax


def report(tag, case, got, ref, cap):
    err = float(np.abs(got.astype(dr.LD) - ref).max())
    print(f"POOLGRAD {tag:<10} {str(case):<56} hip-dense {err:.3e}  cap {cap:.3e}  ratio {err / cap:.4f}")
    return err


def zero_past_lengths(got, seqlen):
    return all((got[i, s:] == 0).all() and not np.signbit(got[i, s:]).any() for i, s in enumerate(seqlen))


def excluded(g, amb, F):
    """g with zeros at the ambiguous pairs (a shared vector: at every filter that is ambiguous in any sequence); the pad stays NaN."""
    gz = np.array(g, dtype=np.float64)
    if gz.ndim == 1:
        gz[:F][amb.any(axis=0)] = 0.0
    else:
        gz[:, :F][amb] = 0.0
    return gz


def projections_and_ambiguous(x, seqlen, radem, chi, cw):
    proj = dr.conv_projections(x.astype(dr.LD), seqlen, radem, chi, cw)
    return proj, dpg.ambiguous(x, seqlen, radem, chi, cw, proj=proj)


def against_reference(tag, case, x, seqlen, g, radem, chi, cw, got, got_arg, proj, amb):
    """The per-case checks of the module docstring (g already zeroed at the ambiguous pairs) -> the reference's argmax."""
    F, C = chi.shape[0], x.shape[2]
    print(f"POOLGRAD {tag:<10} {str(case):<56} ambiguous pairs {int(amb.sum())} of {amb.size}")
    assert amb.mean() <= 0.05
    ref, ref_arg, _ = dpg.pool_input_grad(x, seqlen, g, radem, chi, cw, proj=proj)
    cap = dpg.cap_pool_input_grad(g, ref_arg, seqlen, chi, cw, C)
    assert np.isfinite(got).all() and zero_past_lengths(got, seqlen)
    assert (got_arg >= -1).all() and (got_arg <= (seqlen - cw)[:, None]).all()
    assert (got_arg == ref_arg)[~amb].all()
    assert report(tag, case, got, ref, cap) <= cap
    assert float(np.abs(ref).max()) > 100 * cap                            # (the comparison is not vacuous)
    return ref_arg


def pooled_forward(ext, x, seqlen, radem, chi, cw):
    """hipConv1dMaxpool into zero-filled rows.  The forward operator takes an even number of filters: an odd F gets one more filter
    behind the others (the signs reach that far: F is not a multiple of the even padded width) -- filter f keeps its place in its
    tile, so its bits do not change -- and the first F columns are returned."""
    F = chi.shape[0]
    if F % 2:
        assert radem.shape[2] > F
        chi = np.append(chi, np.float32(1.0))
    out = torch.zeros((x.shape[0], chi.shape[0]), dtype=torch.float32, device=DEV)
    ext.hipConv1dMaxpool(dev(x), out, dev(radem), dev(chi), seqlen, cw)
    return out[:, :F].contiguous()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)).replace(" ", ""))
def test_operator_against_the_dense_reference_and_the_forward_operator(ext, case):
    C, cw, L, lengths, n, F, mode = case
    x, seqlen, g, radem, chi = dpg.make_case(n, L, C, cw, F, mode != "shared", seed=7, lengths=list(lengths),
                                             stride_pad=3 if mode == "rows_pad" else 0)
    assert ext.conv_maxpool_input_grad_ok(cw * C) == 1
    proj, amb = projections_and_ambiguous(x, seqlen, radem, chi, cw)
    gz = excluded(g, amb, F)
    if mode == "rows_pad":
        assert gz.shape[1] > F and np.isnan(gz[:, F:]).all()
    out, argmax = run_operator(ext, x, seqlen, gz, radem, chi, cw)
    ref_arg = against_reference("operator", case, x, seqlen, gz, radem, chi, cw, out.cpu().numpy(), argmax.cpu().numpy(),
                                proj, amb)
    if min(lengths) == cw:                                                 # one window: about half the filters are ReLU-inactive
        share = float((ref_arg[seqlen == cw] < 0).mean())
        assert 0.25 < share < 0.75, share
    # ---- consistency with the forward operator, nothing excluded
    pooled = pooled_forward(ext, x, seqlen, radem, chi, cw)
    assert bool(((argmax >= 0) == (pooled > 0)).all())
    nkmax = L - cw + 1
    wins = dev(x).unfold(1, cw, 1).permute(0, 1, 3, 2).reshape(n * nkmax, cw, C).contiguous()
    single = pooled_forward(ext, wins.cpu().numpy(), np.full(n * nkmax, cw, dtype=np.int32), radem, chi, cw).view(n, nkmax, F)
    winner = torch.gather(single, 1, argmax.clamp(min=0).long()[:, None, :])[:, 0, :]
    winner = torch.where(argmax >= 0, winner, torch.zeros_like(winner))
    assert same_bits(winner.contiguous(), pooled)                          # the winning window alone reproduces the pooled value


def test_exact_ties_go_to_the_first_window(ext):
    from test_pool_input_grad_host import periodic_case
    tokens, table, seqlen, g, radem, chi = periodic_case()
    x = table[tokens]
    for out, argmax in (run_operator(ext, x, seqlen, g, radem, chi, 2), run_tokens(ext, tokens, table, seqlen, g, radem, chi, 2)):
        a, o = argmax.cpu().numpy(), out.cpu().numpy()
        assert (a >= 0).any() and (a[a >= 0] < 2).all()
        assert (o[0, 3:] == 0).all() and (np.abs(o[0, :3]).max(axis=1) > 0).all()
        ref, ref_arg, _ = dpg.pool_input_grad(x, seqlen, g, radem, chi, 2)
        amb = dpg.ambiguous(x, seqlen, radem, chi, 2)
        assert (a == ref_arg)[~amb].all()               # ("AB" and "BA" coincide at a filter or two: ambiguous, see the helper)
        gz = excluded(g, amb, chi.shape[0])
        oz = (run_operator(ext, x, seqlen, gz, radem, chi, 2)[0]).cpu().numpy()
        ref = dpg.pool_input_grad(x, seqlen, gz, radem, chi, 2)[0]
        cap = dpg.cap_pool_input_grad(gz, ref_arg, seqlen, chi, 2, table.shape[1])
        assert report("ties", ("ABABAB", table.shape[1], 2, 6, chi.shape[0]), oz, ref, cap) <= cap


# ------------------------------------------------------------------------------------------------ tokens
def token_case(table, n, L, lengths, seed):
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
    _, _, g, radem, chi = dpg.make_case(n, L, C, cw, F, True, seed=9)
    tokens, seqlen = token_case(table, n, L, lengths, 9)
    assert ext.conv_token_maxpool_input_grad_ok(cw * C, table.shape[0], C) == 1
    gd = dev(g)
    dense, dense_arg = run_operator(ext, table[tokens], seqlen, gd, radem, chi, cw)
    garbage = tokens.copy()
    for i, s in enumerate(seqlen):
        garbage[i, s:] = (garbage[i, s:].astype(np.int64) + 1 + i) % table.shape[0]
    for tk in (tokens, garbage):                                           # other tokens past each length: never read
        out, argmax = run_tokens(ext, tk, table, seqlen, gd, radem, chi, cw)
        assert same_bits(out, dense) and same_bits(argmax, dense_arg)
    assert bool(torch.isfinite(dense).all()) and float(dense.abs().max()) > 0


@pytest.mark.parametrize("C,cw,L,F", [(4, 3, 9, 4500), (21, 9, 40, 1324), (128, 8, 10, 1024)])
def test_results_are_bit_identical_and_sequences_are_independent(ext, C, cw, L, F):
    """Two launches give equal bits; a sequence's result depends neither on n nor on its position (sequence 3 of 5 against the same
    sequence alone), nor on whether g arrives shared or per row."""
    n = 5
    x, seqlen, g, radem, chi = dpg.make_case(n, L, C, cw, F, True, seed=8)
    gd = dev(g)
    a, aa = run_operator(ext, x, seqlen, gd, radem, chi, cw)
    b, ba = run_operator(ext, x, seqlen, gd, radem, chi, cw)
    assert same_bits(a, b) and same_bits(aa, ba)
    alone, alone_arg = run_operator(ext, x[3:4].copy(), seqlen[3:4].copy(), gd[3:4].contiguous(), radem, chi, cw)
    assert same_bits(a[3:4].contiguous(), alone) and same_bits(aa[3:4].contiguous(), alone_arg)
    shared, _ = run_operator(ext, x, seqlen, gd[3].contiguous(), radem, chi, cw)
    assert same_bits(a[3:4].contiguous(), shared[3:4].contiguous())
    repeated, _ = run_operator(ext, x, seqlen, gd[3:4].repeat(n, 1).contiguous(), radem, chi, cw)
    assert same_bits(shared, repeated)


# ------------------------------------------------------------------------------------------------ the kernel object
def _kernel(n, L, C, cw, init_rffs, M=128, icpt=True):
    from xgpr_amd.kernels import Conv1dTwoLayerKernel
    k = Conv1dTwoLayerKernel((n, L, C), M, 123, DEV, {"conv_width": cw, "init_rffs": init_rffs, "intercept": icpt})
    k.set_hyperparams(np.asarray([0.9, 0.35]), logspace=False)
    return k


def test_operator_against_the_composed_route_and_the_composed_route_beyond_1024(ext):
    rng = np.random.default_rng(11)
    # C 21, conv_width 9, F 300: both routes read the same float32 projections, so their argmax is EQUAL everywhere; the composed route
    # does the backward in float64, within the same cap a fortiori: the two are within the sum of their caps
    n, L, C, cw, F = 5, 12, 21, 9, 300
    k = _kernel(n, L, C, cw, F)
    x = rng.standard_normal((n, L, C)).astype(np.float32)
    seqlen = np.asarray([9, 12, 10, 11, 12], dtype=np.int32)
    g = rng.standard_normal((n, F))
    radem, chi = k.radem_diag1.cpu().numpy(), k.chi_arr1.cpu().numpy()
    op, op_arg = k.first_layer_gradient(x, seqlen, g, return_argmax=True)
    fb, fb_arg = k.first_layer_gradient_composed(dev(x), seqlen, dev(g))
    assert same_bits(op_arg, fb_arg)
    cap = dpg.cap_pool_input_grad(g, op_arg.cpu().numpy(), seqlen, chi, cw, C)
    report("op-vs-fb", (C, cw, L, F, n), op.cpu().numpy(), fb.cpu().numpy().astype(dr.LD), 2 * cap)
    assert float((op - fb).abs().max()) <= 2 * cap
    proj, amb = projections_and_ambiguous(x, seqlen, radem, chi, cw)
    gz = excluded(g, amb, F)
    fbz, fbz_arg = k.first_layer_gradient_composed(dev(x), seqlen, dev(gz))
    against_reference("composed", (C, cw, L, F, n), x, seqlen, gz, radem, chi, cw, fbz.cpu().numpy(), fbz_arg.cpu().numpy(), proj, amb)
    # a window of 9 x 128 = 1152 elements (P = 2048): the operator refuses, the kernel object takes the composed route
    n, L, C, cw, F = 2, 10, 128, 9, 64
    k = _kernel(n, L, C, cw, F, icpt=False)
    x = rng.standard_normal((n, L, C)).astype(np.float32)
    seqlen = np.asarray([9, 10], dtype=np.int32)
    radem, chi = k.radem_diag1.cpu().numpy(), k.chi_arr1.cpu().numpy()
    assert ext.conv_maxpool_input_grad_ok(cw * C) == 0
    with pytest.raises(RuntimeError, match="padded width > 1024"):
        run_operator(ext, x, seqlen, rng.standard_normal(F), radem, chi, cw)
    proj, amb = projections_and_ambiguous(x, seqlen, radem, chi, cw)
    gz = excluded(rng.standard_normal(F), amb, F)
    got, got_arg = k.first_layer_gradient(x, seqlen, gz, return_argmax=True)
    against_reference("composed", (C, cw, L, F, n), x, seqlen, gz, radem, chi, cw, got.cpu().numpy(), got_arg.cpu().numpy(), proj, amb)


def test_a_table_the_lds_image_cannot_hold_goes_through_dense_slices(ext, monkeypatch):
    from xgpr_amd.dataset import TokenBatch
    from xgpr_amd.kernels import ConvSORFKernel
    rng = np.random.default_rng(10)
    V, C, cw, L, n, F = 250, 19, 3, 8, 5, 300                             # 4750 floats > 4608
    table = rng.uniform(-1, 1, size=(V, C)).astype(np.float32)
    tokens, seqlen = token_case(table, n, L, (3, 5, 8), 10)
    k = _kernel(n, L, C, cw, F)
    g = rng.standard_normal((n, F))
    assert ext.conv_token_maxpool_input_grad_ok(cw * C, V, C) == 0 and ext.conv_maxpool_input_grad_ok(cw * C) == 1
    monkeypatch.setattr(ConvSORFKernel, "CACHE_BUILD_ROWS", 2)             # three slices
    got, got_arg = k.first_layer_gradient(TokenBatch(dev(tokens), dev(table)), seqlen, g, return_argmax=True)
    want, want_arg = k.first_layer_gradient(table[tokens], seqlen, g, return_argmax=True)
    assert same_bits(got, want) and same_bits(got_arg, want_arg)


# ------------------------------------------------------------------------------------------------ predict_gradient end to end
N, L_, C_, CW, V_, INIT = 60, 12, 4, 3, 6, 64


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
    model = xGPRegression(num_rffs=128, variance_rffs=32, kernel_choice="Conv1dTwoLayer", device=DEV, verbose=False,
                          kernel_settings={"conv_width": CW, "init_rffs": INIT, "intercept": True})
    model.set_hyperparams(np.log(np.asarray([0.3, 0.25])), ds)
    model.fit(ds, mode="exact")
    return model, ds, x, seqlen, tokens, table


def _end_to_end(tag, k, x32, seqlen, pooled, w, w_cols, got, dev_arg, factor):
    """The second layer's reference at the float32 pooled values the device produced; its cap pushed through the first layer under the
    device's argmax (asserted to agree with the reference's off the ambiguous set by the caller); cap_pool_input_grad added."""
    sigma = float(k.hyperparams[1])
    xs2 = (pooled.astype(np.float64) * sigma).astype(np.float32)
    radem2, chi2 = k.radem_diag.cpu().numpy(), k.chi_arr.cpu().numpy()
    radem1, chi1 = k.radem_diag1.cpu().numpy(), k.chi_arr1.cpu().numpy()
    g_ref = dig.rbf_input_grad(xs2, w, radem2, chi2, sigma, True, w_cols=w_cols)
    cap2 = dig.cap_input_grad(xs2, w, radem2, chi2, sigma, True, w_cols=w_cols)
    ref = dpg.pool_input_grad(x32, seqlen, g_ref, radem1, chi1, CW, argmax=dev_arg)[0] * factor
    cap = (dpg.push_bound(cap2, dev_arg, seqlen, radem1, chi1, CW, L_, C_)
           + dpg.cap_pool_input_grad(np.abs(g_ref) + cap2, dev_arg, seqlen, chi1, CW, C_)) * factor
    assert report(tag, ("Conv1dTwoLayer", C_, CW, L_, INIT, N), got, ref, cap) <= cap + 4 * U64 * float(np.abs(ref).max())
    assert float(np.abs(ref).max()) > 100 * cap


def test_kernel_input_gradient_and_predict_gradient(fitted):
    model, _, x, seqlen, tokens, table = fitted
    k = model.kernel
    x32 = x.astype(np.float32)
    radem1, chi1 = k.radem_diag1.cpu().numpy(), k.chi_arr1.cpu().numpy()
    std = float(model.trainy_std)
    pooled = k.pool(x, seqlen)
    # the device's argmax agrees with the reference's off the ambiguous set
    _, dev_arg = k.first_layer_gradient(x, seqlen, np.ones(INIT), return_argmax=True)
    dev_arg = dev_arg.cpu().numpy()
    amb = dpg.ambiguous(x32, seqlen, radem1, chi1, CW)
    ref_arg = dpg.pool_input_grad(x32, seqlen, np.zeros(INIT), radem1, chi1, CW)[1]
    print(f"POOLGRAD end-to-end ambiguous pairs {int(amb.sum())} of {amb.size}")
    assert amb.mean() <= 0.05 and (dev_arg == ref_arg)[~amb].all()
    # the kernel object
    w = model.weights.cpu().numpy()
    got = k.input_gradient(x, seqlen, model.weights)
    assert got.dtype == F64 and tuple(got.shape) == (N, L_, C_) and got.is_cuda
    _end_to_end("kernel", k, x32, seqlen, pooled.cpu().numpy(), w, None, got.cpu().numpy(), dev_arg, 1.0)
    assert same_bits(got, k.input_gradient(x, seqlen, model.weights, pooled=pooled))
    with pytest.raises(ValueError, match="sequence_length is required"):
        k.input_gradient(x, None, w)
    # the model
    gm, gv = model.predict_gradient(x, get_var=True, chunk_size=16, sequence_lengths=seqlen, subgradient=True)
    assert isinstance(gm, np.ndarray) and gm.shape == (N, L_, C_) and gv.shape == (N, L_, C_)
    assert np.array_equal(gm, model.predict_gradient(x, chunk_size=16, sequence_lengths=seqlen, subgradient=True))
    assert zero_past_lengths(gm, seqlen) and zero_past_lengths(gv, seqlen)
    _end_to_end("mean", k, x32, seqlen, pooled.cpu().numpy(), w, None, gm, dev_arg, std)
    lam = float(k.get_lambda())
    var = model.var.cpu().numpy()
    nvar = var.shape[0]
    assert nvar == 32
    zv = k.transform_x(x, seqlen)[:, :nvar].cpu().numpy()
    wv = 2.0 * lam ** 2 * (zv @ var)
    _end_to_end("variance", k, x32, seqlen, pooled.cpu().numpy(), wv, nvar, gv, dev_arg, std ** 2)
    assert float(np.abs(gm).max()) > 0 and float(np.abs(gv).max()) > 0
    # the same problem given as tokens: the dense result bit for bit
    tm, tv = model.predict_gradient(tokens, get_var=True, chunk_size=16, sequence_lengths=seqlen, token_table=table,
                                      subgradient=True)
    assert np.array_equal(tm, gm) and np.array_equal(tv, gv)


def test_predict_gradient_for_linear_and_the_remaining_refusal(fitted):
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.models import xGPRegression
    model, _, x, seqlen, _, _ = fitted
    with pytest.raises(RuntimeError, match="sequence_lengths is required"):
        model.predict_gradient(x[:3], subgradient=True)
    with pytest.raises(RuntimeError, match="with subgradient=True for Conv1dTwoLayer"):      # the convention is asked for by name
        model.predict_gradient(x[:3], sequence_lengths=seqlen[:3])
    rng = np.random.default_rng(14)
    xf = rng.standard_normal((50, 7))
    y = xf @ rng.standard_normal(7) + 0.1 * rng.standard_normal(50)
    ds = build_regression_dataset(xf, y, chunk_size=25, device=DEV)
    lin = xGPRegression(num_rffs=8, variance_rffs=8, kernel_choice="Linear", device=DEV, verbose=False)
    lin.set_hyperparams(np.log(np.asarray([0.5])), ds)
    lin.fit(ds, mode="exact")
    gm, gv = lin.predict_gradient(xf[:9], get_var=True)
    assert gm.shape == gv.shape == (9, 7)
    assert np.abs(gm - float(lin.trainy_std) * lin.weights.cpu().numpy()[None, 1:]).max() < 1e-12
    e = np.zeros(7)
    e[2] = 0.25
    (mp, vp), (mm, vm) = lin.predict(xf[:9] + e, get_var=True), lin.predict(xf[:9] - e, get_var=True)
    assert np.abs((mp - mm) / 0.5 - gm[:, 2]).max() < 1e-4 * max(1.0, float(np.abs(gm).max()))
    assert np.abs((vp - vm) / 0.5 - gv[:, 2]).max() < 1e-4 * max(1.0, float(np.abs(gv).max()))
    ard = xGPRegression(num_rffs=64, variance_rffs=16, kernel_choice="MiniARD", device=DEV, verbose=False,
                        kernel_settings={"split_points": [3], "intercept": True})
    ard.set_hyperparams(dataset=ds)
    ard.weights = torch.zeros(64, dtype=F64, device=DEV)                   # (the refusal is about the kernel, not the fit)
    with pytest.raises(RuntimeError, match="RBF, Matern and Cauchy.*MiniARD is not supported"):
        ard.predict_gradient(xf[:3])
