"""GPU tests of the exact NMLL gradient of the sequence, graph and two-layer kernels from float32 feature and gradient rows: the
rows writer (hipConvGradRows / xgpr_conv_grad_rows_f32) against ``gradient_x`` bit for bit on every code path, its error codes,
the host route of nmll.calc_gradient_terms against an exact model and against the float64 formulation of the same kernel, and
a tuning run end to end.

Tolerances.  Writer: none -- each entry is the float64 k-mer sum of the gradient operator rounded once to float32, so
(double)rows == (double)(float)gradient_x.  Route against the exact model: both sides are float64 sums of the SAME float64
products (a product of two widened float32 values is exact in float64), so only the summation order differs: 1e-12 x max|.|,
as argued in the header of tests/test_gpu_nmll_grad_rows.py.  Route against the float64 formulation: the difference is the
float32 rounding of the float64 k-mer sums (2^-24 relative per entry), amplified by the conditioning of the solve.  What the
rounding alone costs was measured on neither route -- exact_nmll_reg_grad fed with the terms of unrounded and of rounded
gradient_x outputs (tools/seq_grad_rows_timing.py: terms_from_gradient_x) -- by the test itself, at its shapes and its two
hyperparameter settings, and printed; the score and gradient bars are ten times that, to cover the conditioning of other draws.
One recorded run, Conv1dRBF at lambda = 0.7, sigma = 0.45 (n = 2051, M = 256): rounding alone 2.430e-10 on the score and 1.640e-08
of the largest gradient entry, bars 2.430e-09 / 1.640e-07; the route differed from the float64 formulation by 2.430e-10 /
1.640e-08.  The other three cases and the timing of tools/seq_grad_rows_timing.py have not been recorded: profiles/seq_grad_rows.json
holds this one case."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

pytestmark = pytest.mark.gpu
DEV = "cuda"

BAR_FACTOR = 10.0     # bars = BAR_FACTOR x what the rounding alone costs (measured in the test, on neither route)


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def _forbid(monkeypatch, ext, *names):
    calls = []

    def raiser(*a, **k):
        calls.append(1)
        raise AssertionError("a float64 gradient operator was called on the rows route")
    for nm in names:
        monkeypatch.setattr(ext, nm, raiser)
    return calls


# ---------------------------------------------------------------------------------------------- writer contract
def _writer_case(name, n, L, Cc, cw, m, averaging, icpt, seed=0, radem_offset=0):
    from xgpr_amd.kernels import make_kernel
    rng = np.random.default_rng(seed + n + L * Cc + m)
    x = torch.from_numpy(rng.standard_normal((n, L, Cc)).astype(np.float32)).to(DEV)
    sl = rng.integers(cw, L + 1, size=n).astype(np.int32)
    sl[0], sl[1] = cw, L                              # one k-mer; the whole array
    parms = {"averaging": averaging, "intercept": icpt, "matern_nu": 2.5}
    if not name.startswith("Graph"):
        parms["conv_width"] = cw
    kern = make_kernel(name, (n, L, Cc), m, 123, DEV, parms)
    kern.set_hyperparams(np.array([0.5, 0.8]), logspace=False)
    if radem_offset:                                  # the same signs in a view the wave tiles cannot read 16 bytes at a time
        buf = torch.zeros(kern.radem_diag.numel() + radem_offset, dtype=torch.int8, device=DEV)
        buf[radem_offset:] = kern.radem_diag.reshape(-1)
        kern.radem_diag = buf[radem_offset:].view(kern.radem_diag.shape)
        assert kern.radem_diag.data_ptr() % 16 == radem_offset and kern.radem_diag.is_contiguous()
    return kern, x, sl


def _check_writer(ext, kern, x, sl, icpt):
    n, m = x.shape[0], kern.num_rffs
    out, grad = kern.gradient_x(x, sl)                # hipConvGrad into zeroed float64 arrays + the host's intercept fix-up
    zrows = torch.full((n, m), float("nan"), dtype=torch.float32, device=DEV)      # overwritten: no zero fill needed
    grows = torch.full((n, m), float("nan"), dtype=torch.float32, device=DEV)
    assert ext.hipConvGradRows(x, zrows, grows, kern.radem_diag, kern.chi_arr, sl, float(kern.hyperparams[1]), kern.conv_width,
                               kern.scaling_type, icpt) == 0
    assert torch.equal(zrows.double(), out.float().double())
    assert torch.equal(grows.double(), grad[:, :, 0].float().double())
    if icpt:
        assert bool((zrows[:, 0] == 1.0).all()) and bool((grows[:, 0] == 0.0).all())
    assert float(grows.abs().max()) > 0.0
    z2, g2 = torch.zeros_like(zrows), torch.zeros_like(grows)                      # through the kernel class; same bits again
    kern.fill_grad_rows(x, z2, g2, sl)
    assert torch.equal(z2, zrows) and torch.equal(g2, grows)


# (kernel, L, C, conv_width): one window shape per code path -- graph nodes of 21 features (padded 32: rows layout), 9 x 21 (256:
# transposed columns), 5 x 100 (512: layout C), 3 x 500 (2048) and 3 x 1000 (4096) on the wide wave tiles, 2 x 2500 (8192) staged
WINDOWS = [("GraphRBF", 30, 21, 1), ("Conv1dRBF", 30, 21, 9), ("Conv1dMatern", 30, 100, 5), ("Conv1dRBF", 30, 500, 3),
           ("Conv1dCauchy", 30, 1000, 3), ("Conv1dRBF", 30, 2500, 2)]


@pytest.mark.parametrize("averaging,icpt", [("none", True), ("sqrt", False), ("full", True)])
@pytest.mark.parametrize("name,L,Cc,cw", WINDOWS)
def test_rows_equal_gradient_x_rounded_once_bit_for_bit(ext, name, L, Cc, cw, averaging, icpt):
    kern, x, sl = _writer_case(name, 37, L, Cc, cw, 256, averaging, icpt)
    _check_writer(ext, kern, x, sl, icpt)


@pytest.mark.parametrize("name,L,Cc,cw,n,m", [("Conv1dRBF", 30, 21, 9, 70, 256),          # 70 sequences: the longest-first order runs
                                              ("GraphCauchy", 30, 21, 1, 70, 256),
                                              ("Conv1dRBF", 30, 100, 5, 37, 2 * 1300),    # a ragged second tile (1300 frequencies)
                                              ("Conv1dRBF", 30, 500, 3, 37, 2 * 1300)])   # ... on the wide wave tiles: tile 2 stores 276
def test_rows_with_the_order_and_with_a_ragged_second_tile(ext, name, L, Cc, cw, n, m):
    kern, x, sl = _writer_case(name, n, L, Cc, cw, m, "sqrt", True, seed=3)
    _check_writer(ext, kern, x, sl, True)


@pytest.mark.parametrize("Cc,cw", [(500, 3), (1000, 3)])
def test_rows_are_staged_for_a_rademacher_view_the_wave_tiles_cannot_read(ext, Cc, cw):
    """Windows of 2048 / 4096 elements with the Rademacher array 8 bytes into its allocation: the float64 operator leaves the wave
    tiles for the any-width path, and the writer stages it -- same bits as ``gradient_x`` on the same view."""
    kern, x, sl = _writer_case("Conv1dRBF", 37, 30, Cc, cw, 256, "sqrt", True, seed=5, radem_offset=8)
    _check_writer(ext, kern, x, sl, True)


def test_staged_rows_in_several_slices_and_without_room(ext):
    """The staged route with a workspace that holds 5 sequences per float64 array (slices of 5 x 7 + 2: same bits), and
    XGPR_ERR_WORKSPACE -- no launch -- when it holds none."""
    from xgpr_amd import _lib
    lib = _lib.load()
    kern, x, sl = _writer_case("Conv1dRBF", 37, 30, 2500, 2, 256, "none", True, seed=7)
    n, m, R = 37, 256, kern.radem_diag.shape[2]
    out, grad = kern.gradient_x(x, sl)
    full = int(lib.xgpr_conv_grad_rows_workspace_bytes(R, 5000, m, n))
    base = full - 2 * n * m * 8
    sld = torch.from_numpy(sl).to(DEV)

    def call(nbytes, z, g):
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=DEV)
        return lib.xgpr_conv_grad_rows_f32(
            C.c_void_p(x.data_ptr()), C.c_void_p(z.data_ptr()), C.c_void_p(g.data_ptr()), C.c_void_p(kern.radem_diag.data_ptr()),
            C.c_void_p(kern.chi_arr.data_ptr()), C.c_void_p(sl.ctypes.data), C.c_void_p(sld.data_ptr()), n, 30, 2500, m, m // 2, R, n,
            float(kern.hyperparams[1]), 2, 0, 1, C.c_void_p(ws.data_ptr()), C.c_size_t(nbytes),
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    z = torch.full((n, m), float("nan"), dtype=torch.float32, device=DEV)
    g = torch.full((n, m), float("nan"), dtype=torch.float32, device=DEV)
    assert call(base + 2 * 5 * m * 8, z, g) == 0, _lib.last_error()
    assert torch.equal(z.double(), out.float().double()) and torch.equal(g.double(), grad[:, :, 0].float().double())
    z.fill_(7.0)
    g.fill_(7.0)
    assert call(base, z, g) == -21 and "workspace" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((z == 7.0).all()) and bool((g == 7.0).all())


def test_two_layer_rows_equal_gradient_x_bit_for_bit(ext, monkeypatch):
    from xgpr_amd.kernels import make_kernel
    n, L, Cc, m = 37, 30, 21, 256
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.standard_normal((n, L, Cc)).astype(np.float32)).to(DEV)
    sl = rng.integers(3, L + 1, size=n).astype(np.int32)
    sl[0], sl[1] = 3, L
    kern = make_kernel("Conv1dTwoLayer", (n, L, Cc), m, 123, DEV, {"conv_width": 3, "init_rffs": 64, "intercept": True})
    kern.set_hyperparams(np.array([0.5, 0.8]), logspace=False)
    assert kern.grad_rows_ok()
    out, grad = kern.gradient_x(x, sl)
    zrows = torch.full((n, m), float("nan"), dtype=torch.float32, device=DEV)
    grows = torch.full((n, m), float("nan"), dtype=torch.float32, device=DEV)
    _forbid(monkeypatch, ext, "hipRBFGrad", "cudaRBFGrad")
    kern.fill_grad_rows(x, zrows, grows, sl)
    assert torch.equal(zrows.double(), out) and torch.equal(grows.double(), grad[:, :, 0])       # that operator widens float values
    assert bool((zrows[:, 0] == 1.0).all()) and bool((grows[:, 0] == 0.0).all()) and float(grows.abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------- error codes
def test_writer_error_codes_launch_nothing(ext):
    from xgpr_amd import _lib
    lib = _lib.load()
    n, L, Cc, cw, m = 8, 12, 8, 3, 256
    kern, x, sl = _writer_case("Conv1dRBF", n, L, Cc, cw, m, "none", True)
    R = kern.radem_diag.shape[2]
    sentinel = 7.0
    z = torch.full((n, m), sentinel, dtype=torch.float32, device=DEV)
    g = torch.full((n, m), sentinel, dtype=torch.float32, device=DEV)
    flat = torch.full((n * m + 1,), sentinel, dtype=torch.float32, device=DEV)
    ws = torch.empty(int(lib.xgpr_conv_grad_rows_workspace_bytes(R, cw * Cc, m, n)), dtype=torch.uint8, device=DEV)

    def raw(zptr, gptr, lens):
        sld = torch.from_numpy(lens).to(DEV)
        return lib.xgpr_conv_grad_rows_f32(
            C.c_void_p(x.data_ptr()), C.c_void_p(zptr), C.c_void_p(gptr), C.c_void_p(kern.radem_diag.data_ptr()),
            C.c_void_p(kern.chi_arr.data_ptr()), C.c_void_p(lens.ctypes.data), C.c_void_p(sld.data_ptr()), n, L, Cc, m, m // 2, R, n,
            0.8, cw, 0, 1, C.c_void_p(ws.data_ptr()), C.c_size_t(ws.numel()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert raw(flat.data_ptr() + 4, g.data_ptr(), sl) == -21           # XGPR_ERR_WORKSPACE: a 4-byte-aligned zrows
    assert raw(z.data_ptr(), flat.data_ptr() + 4, sl) == -21           # ... a 4-byte-aligned grows
    short, long_ = sl.copy(), sl.copy()
    short[3], long_[0] = cw - 1, L + 1
    assert raw(z.data_ptr(), g.data_ptr(), short) != 0 and raw(z.data_ptr(), g.data_ptr(), long_) != 0
    with pytest.raises(RuntimeError, match="sequence lengths must be >= conv width"):
        ext.hipConvGradRows(x, z, g, kern.radem_diag, kern.chi_arr, short, 0.8, cw, 0, True)
    with pytest.raises(RuntimeError, match="sequence lengths"):
        ext.hipConvGradRows(x, z, g, kern.radem_diag, kern.chi_arr, long_, 0.8, cw, 0, True)
    with pytest.raises(RuntimeError, match="8-byte aligned"):
        ext.hipConvGradRows(x, flat[1:].view(n, m), g, kern.radem_diag, kern.chi_arr, sl, 0.8, cw, 0, True)
    with pytest.raises(TypeError):
        ext.hipConvGradRows(x, z.double(), g, kern.radem_diag, kern.chi_arr, sl, 0.8, cw, 0, True)
    with pytest.raises(RuntimeError, match="no datapoints"):
        ext.hipConvGradRows(x, z[:-1], g[:-1], kern.radem_diag, kern.chi_arr, sl, 0.8, cw, 0, True)
    torch.cuda.synchronize()
    for t in (z, g, flat):
        assert bool((t == sentinel).all())                              # never a launch
    assert raw(z.data_ptr(), g.data_ptr(), sl) == 0
    assert bool((z[:, 0] == 1.0).all()) and bool((g[:, 0] == 0.0).all()) and not bool((z[:, 1:] == sentinel).any())


# ---------------------------------------------------------------------------------------------- host route
_ROUTE = {}


def _route_case(name):
    """(dataset, kernel, {hyperparameters: (exact-model terms, terms of the unrounded outputs)}), computed once per kernel and left
    unchanged: the float64 torch accumulation of ``gradient_x`` outputs, cast to float32 and back / as they are."""
    import seq_grad_rows_timing as tool
    if name not in _ROUTE:
        ds, kern = tool.route_problem(name, DEV)
        refs = {}
        for hp in tool.HPARAMS:
            kern.set_hyperparams(np.array(hp), logspace=False)
            refs[hp] = (tool.terms_from_gradient_x(ds, kern, True), tool.terms_from_gradient_x(ds, kern, False))
        _ROUTE[name] = (ds, kern, refs)
    return _ROUTE[name]


@pytest.mark.parametrize("name", ["Conv1dRBF", "GraphMatern"])
def test_route_equals_the_exact_model_over_three_windows(name, monkeypatch):
    """n = 2051 sequences in chunks of 500, windows forced to 800 rows: 800, 800 and 451."""
    import seq_grad_rows_timing as tool
    from xgpr_amd import nmll
    ds, kern, refs = _route_case(name)
    hp = tool.HPARAMS[0]
    kern.set_hyperparams(np.array(hp), logspace=False)
    assert kern.grad_rows_ok() and nmll._grad_rows_route(ds, kern)
    filled = []
    orig_fill = type(kern).fill_grad_rows

    def counting_fill(self, x, zr, gr, lens):
        filled.append((x.shape[0], len(lens)))
        return orig_fill(self, x, zr, gr, lens)
    monkeypatch.setattr(type(kern), "fill_grad_rows", counting_fill)
    monkeypatch.setattr(nmll, "_grad_window_rows", lambda m: 800)
    rows = nmll.calc_gradient_terms(ds, kern)
    assert filled == [(800, 800), (800, 800), (451, 451)]
    for i, (r, f) in enumerate(zip(rows[:5], refs[hp][0])):
        r, f = torch.as_tensor(r), torch.as_tensor(f)
        bar = 1e-12 * float(f.abs().max())
        err = float((r.to(f.device) - f).abs().max())
        print(name, "term", i, "err", err, "bar", bar)
        assert err <= bar, (i, err, bar)
    assert torch.equal(rows[4][:, :, 0], rows[4][:, :, 0].T)            # symmetric bit for bit
    assert rows[5] == 2051


@pytest.mark.parametrize("hp_index", [0, 1])
@pytest.mark.parametrize("name", ["Conv1dRBF", "GraphMatern"])
def test_route_against_the_float64_formulation(name, hp_index, monkeypatch):
    """Score and gradient of the rows route against ``grad_rows_ok`` forced false (the chunked float64 formulation), within ten
    times what the rounding alone costs, measured here first and printed (header)."""
    import seq_grad_rows_timing as tool
    from xgpr_amd import nmll
    ds, kern, refs = _route_case(name)
    hp = tool.HPARAMS[hp_index]
    kern.set_hyperparams(np.array(hp), logspace=False)
    hpv = kern.get_hyperparams(logspace=False)
    model = []
    for t in refs[hp]:
        s, g, _ = nmll.exact_nmll_reg_grad(t[0].clone(), t[1], t[2], hpv, 2051, t[3], t[4])
        model.append((float(s), np.asarray(g)))
    (s_rnd, g_rnd), (s_unr, g_unr) = model
    score_cost, grad_cost = abs(s_rnd - s_unr) / abs(s_unr), float(np.abs(g_rnd - g_unr).max() / np.abs(g_unr).max())
    SCORE_BAR, GRAD_BAR = BAR_FACTOR * score_cost, BAR_FACTOR * grad_cost
    print(name, hp, "rounding alone: score rel", score_cost, "grad rel", grad_cost)
    assert nmll._grad_rows_route(ds, kern)
    score_r, grad_r = nmll.exact_nmll_gradient(kern, ds)
    monkeypatch.setattr(type(kern), "grad_rows_ok", lambda self: False)
    assert not nmll._grad_rows_route(ds, kern)
    score_f, grad_f = nmll.exact_nmll_gradient(kern, ds)
    ds_rel = abs(score_r - score_f) / abs(score_f)
    dg_rel = float(np.abs(grad_r - grad_f).max() / np.abs(grad_f).max())
    print(name, hp, "route against float64 formulation: score rel", ds_rel, "bar", SCORE_BAR, "grad rel", dg_rel, "bar", GRAD_BAR)
    assert np.isfinite(score_r) and np.all(np.isfinite(grad_r))
    assert ds_rel <= SCORE_BAR, (ds_rel, SCORE_BAR)
    assert dg_rel <= GRAD_BAR, (dg_rel, GRAD_BAR)


@pytest.mark.parametrize("name", ["Conv1dRBF", "GraphMatern"])
def test_route_does_not_call_the_float64_operator(ext, name, monkeypatch):
    from xgpr_amd import nmll
    ds, kern, _ = _route_case(name)
    calls = _forbid(monkeypatch, ext, "hipConvGrad", "cudaConvGrad")
    score, grad = nmll.exact_nmll_gradient(kern, ds)
    assert np.isfinite(score) and np.all(np.isfinite(grad)) and not calls
    monkeypatch.setattr(type(kern), "grad_rows_ok", lambda self: False)
    with pytest.raises(AssertionError):
        nmll.calc_gradient_terms(ds, kern)
    assert calls


def test_two_layer_route_does_not_call_the_float64_operator(ext, monkeypatch):
    """The two-layer kernel over 700 sequences: the route's terms equal the float64 formulation's to summation order (its rows are
    ``gradient_x`` exactly), and hipRBFGrad is not called."""
    from xgpr_amd import nmll
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.kernels import make_kernel
    n, L, Cc, m = 700, 16, 8, 128
    rng = np.random.default_rng(17)
    x = rng.standard_normal((n, L, Cc)).astype(np.float32)
    sl = rng.integers(3, L + 1, size=n).astype(np.int32)
    y = np.sin(x[:, 0, :3].sum(axis=1)) + 0.1 * rng.standard_normal(n)
    ds = build_regression_dataset(x, y, sl, chunk_size=300, device=DEV)
    kern = make_kernel("Conv1dTwoLayer", x.shape, m, 123, DEV, {"conv_width": 3, "init_rffs": 64, "intercept": True})
    kern.set_hyperparams(np.array([0.7, 0.45]), logspace=False)
    f64 = None
    with monkeypatch.context() as mp:
        mp.setattr(type(kern), "grad_rows_ok", lambda self: False)
        f64 = nmll.calc_gradient_terms(ds, kern)
    assert nmll._grad_rows_route(ds, kern)
    calls = _forbid(monkeypatch, ext, "hipRBFGrad", "cudaRBFGrad")
    rows = nmll.calc_gradient_terms(ds, kern)
    score, grad = nmll.exact_nmll_gradient(kern, ds)
    assert np.isfinite(score) and np.all(np.isfinite(grad)) and not calls
    for i, (r, f) in enumerate(zip(rows[:5], f64[:5])):
        r, f = torch.as_tensor(r), torch.as_tensor(f)
        assert float((r - f).abs().max()) <= 1e-12 * float(f.abs().max()), i
    assert rows[5] == f64[5] == n


# ---------------------------------------------------------------------------------------------- end to end
def test_tuning_with_lbfgs_runs_on_the_rows_route(ext, monkeypatch):
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.models import xGPRegression
    n, L, Cc = 300, 20, 8
    rng = np.random.default_rng(23)
    x = rng.standard_normal((n, L, Cc)).astype(np.float32)
    sl = rng.integers(5, L + 1, size=n).astype(np.int32)
    w = rng.standard_normal(Cc)
    y = np.sin(2.0 * np.array([x[i, :sl[i]].mean(axis=0) @ w for i in range(n)])) + 0.05 * rng.standard_normal(n)
    ds = build_regression_dataset(x, y, sl, chunk_size=128, device=DEV)
    calls = _forbid(monkeypatch, ext, "hipConvGrad", "cudaConvGrad")
    mod = xGPRegression(num_rffs=256, kernel_choice="Conv1dRBF", device=DEV, kernel_settings={"conv_width": 5, "averaging": "sqrt"},
                        verbose=False)
    hp, nfev, best = mod.tune_hyperparams(ds, tuning_method="L-BFGS-B", max_iter=3)
    assert np.all(np.isfinite(hp)) and np.isfinite(best) and nfev >= 1
    assert not calls
