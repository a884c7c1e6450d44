"""Float32 feature rows of the sequence kernels (hipConvFeatureRows / xgpr_conv_feature_rows_f32): the operator's bit-for-bit
contract with the float64 operator's rounded output, its argument checks, the cache built from it, and the solver's passes
over resident or regenerated rows -- with the float64 convolution operator switched off, and against the same passes on
float64 Z materialised chunk by chunk (the route forced by switching the predicates off).  Tolerances of the route
comparisons are the ones tests/test_gpu_wide_rows.py fixes for the same comparisons on the fixed-vector kernels."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return float(np.abs(a - b).max() / np.abs(b).max())


def _lengths(rng, n, L, cw, mode):
    if mode == "min":
        return np.full(n, cw, dtype=np.int32)          # one k-mer per sequence
    if mode == "max":
        return np.full(n, L, dtype=np.int32)
    return rng.integers(cw, L + 1, size=n).astype(np.int32)


def _rows_and_reference(ext, name, n, L, Cc, rffs, cw, averaging, icpt, lens_mode, seed=0):
    from xgpr_amd.kernels import make_kernel, scale_input
    rng = np.random.default_rng(seed + n + L * Cc + rffs)
    x = rng.standard_normal((n, L, Cc)).astype(np.float32)
    sl = _lengths(rng, n, L, cw, lens_mode)
    parms = {"averaging": averaging, "intercept": icpt, "matern_nu": 2.5}
    if not name.startswith("Graph"):
        parms["conv_width"] = cw
    kern = make_kernel(name, x.shape, rffs, 123, DEV, parms)
    kern.set_hyperparams(np.array([0.5, 0.8]), logspace=False)
    ref = kern.transform_x(x, sl).to(torch.float32)
    xs = scale_input(dev(x), kern.hyperparams[1])
    rows = torch.full((n, rffs), float("nan"), dtype=torch.float32, device=DEV)      # garbage beforehand: the operator overwrites
    ext.hipConvFeatureRows(xs, rows, kern.radem_diag, kern.chi_arr, sl, kern.conv_width, kern.scaling_type, icpt)
    return kern, xs, sl, rows, ref


# (kernel, n, L, C, rffs, conv_width): padded windows 2, 32, 64, 256 (9 x 21), 1024, 2048, 4096 and one any-width window (8192);
# frequency counts that are no multiple of 1024, one above 16384
SHAPES = [("GraphRBF", 70, 12, 2, 64, 1), ("GraphMatern", 200, 24, 32, 4096, 1), ("Conv1dRBF", 90, 20, 16, 3000, 4),
          ("Conv1dRBF", 130, 60, 21, 2048, 9), ("Conv1dCauchy", 40, 30, 21, 33000, 9), ("Conv1dMatern", 66, 24, 64, 2500, 16),
          ("Conv1dRBF", 30, 26, 100, 4100, 20), ("Conv1dRBF", 21, 44, 100, 8192, 40), ("Conv1dRBF", 9, 54, 100, 16386, 50),
          ("GraphCauchy", 64, 9, 100, 1026, 1)]


@pytest.mark.parametrize("name,n,L,Cc,rffs,cw", SHAPES)
@pytest.mark.parametrize("averaging,icpt,lens_mode", [("none", True, "mixed"), ("sqrt", False, "mixed"), ("full", True, "min"),
                                                      ("sqrt", True, "max")])
def test_rows_equal_the_rounded_float64_operator_bit_for_bit(ext, name, n, L, Cc, rffs, cw, averaging, icpt, lens_mode):
    if name.startswith("Graph"):
        cw = 1
    kern, xs, sl, rows, ref = _rows_and_reference(ext, name, n, L, Cc, rffs, cw, averaging, icpt, lens_mode)
    assert torch.equal(rows, ref)
    if icpt:
        assert bool(torch.all(rows[:, 0] == 1.0))
    # determinism: a second call gives the same bits
    rows2 = torch.zeros_like(rows)
    ext.hipConvFeatureRows(xs, rows2, kern.radem_diag, kern.chi_arr, sl, kern.conv_width, kern.scaling_type, icpt)
    assert torch.equal(rows, rows2)


@pytest.mark.parametrize("name,L,Cc,rffs,cw", [("GraphRBF", 12, 32, 2048, 1), ("Conv1dRBF", 40, 21, 2048, 9),
                                               ("Conv1dRBF", 30, 100, 2048, 20), ("Conv1dRBF", 54, 100, 2048, 50)])
def test_one_sequence(ext, name, L, Cc, rffs, cw):
    kern, xs, sl, rows, ref = _rows_and_reference(ext, name, 1, L, Cc, rffs, cw, "sqrt", True, "mixed")
    assert torch.equal(rows, ref)
    # the same rows through transform_x with a float32 target
    out = torch.full_like(rows, float("nan"))
    assert kern.transform_x(xs, sl, rows_out=out, pre_scaled=True) is out and torch.equal(out, ref)


@pytest.mark.parametrize("L,Cc,cw,rffs", [(60, 21, 9, 2048), (30, 100, 20, 2048)])
def test_same_rows_with_and_without_room_for_the_order(ext, L, Cc, cw, rffs):
    """The longest-first order needs the workspace of xgpr_conv_feature_rows_workspace_bytes; with the masks alone the operator
    runs in the caller's order.  Same bits."""
    from xgpr_amd import _lib
    lib = _lib.load()
    n = 300
    kern, xs, sl, rows, ref = _rows_and_reference(ext, "Conv1dRBF", n, L, Cc, rffs, cw, "sqrt", True, "mixed", seed=5)
    R = kern.radem_diag.shape[2]
    small = int(lib.xgpr_sorf_workspace_bytes(R, cw * Cc, 4))
    full = int(lib.xgpr_conv_feature_rows_workspace_bytes(R, cw * Cc, rffs, n))
    assert full >= small + 4 * n
    sld = dev(sl)
    for nbytes in (small, full):
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=DEV)
        out = torch.full_like(rows, float("nan"))
        rc = lib.xgpr_conv_feature_rows_f32(
            C.c_void_p(xs.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(kern.radem_diag.data_ptr()),
            C.c_void_p(kern.chi_arr.data_ptr()), C.c_void_p(sl.ctypes.data), C.c_void_p(sld.data_ptr()), n, L, Cc, rffs,
            rffs // 2, R, n, cw, 1, 1, C.c_void_p(ws.data_ptr()), C.c_size_t(nbytes),
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, _lib.last_error()
        assert torch.equal(out, ref)


def test_any_width_window_needs_the_staging_workspace(ext):
    """Windows beyond 4096 elements are staged through a float64 slice of the workspace: in several slices when the workspace
    holds only a few rows (same bits), and XGPR_ERR_WORKSPACE -- no launch -- when it holds none."""
    from xgpr_amd import _lib
    lib = _lib.load()
    n, L, Cc, cw, rffs = 23, 54, 100, 50, 1024
    kern, xs, sl, rows, ref = _rows_and_reference(ext, "Conv1dRBF", n, L, Cc, rffs, cw, "none", True, "mixed", seed=9)
    R = kern.radem_diag.shape[2]
    full = int(lib.xgpr_conv_feature_rows_workspace_bytes(R, cw * Cc, rffs, n))
    base = full - ((n * rffs * 8 + 255) // 256) * 256
    sld = dev(sl)

    def call(nbytes, out):
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=DEV)
        return lib.xgpr_conv_feature_rows_f32(
            C.c_void_p(xs.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(kern.radem_diag.data_ptr()),
            C.c_void_p(kern.chi_arr.data_ptr()), C.c_void_p(sl.ctypes.data), C.c_void_p(sld.data_ptr()), n, L, Cc, rffs,
            rffs // 2, R, n, cw, 0, 1, C.c_void_p(ws.data_ptr()), C.c_size_t(nbytes),
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    out = torch.full_like(rows, float("nan"))
    assert call(base + 5 * rffs * 8, out) == 0          # slices of 5, 5, 5, 5, 3 sequences
    assert torch.equal(out, ref)
    untouched = torch.full_like(rows, 7.0)
    assert call(base, untouched) != 0 and "workspace" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool(torch.all(untouched == 7.0))


def test_golden_fixtures_rounded_to_float32(ext):
    """The reference's own values (tests/golden/g3_conv.npz, g17_cfg4_conv.npz) rounded to float32, at the tolerance
    tests/test_gpu_ops.py / test_gpu_cfg_shapes.py use for the float64 operator on the same fixtures."""
    from xgpr_amd.kernels import make_kernel, scale_input
    from test_gpu_cfg_shapes import cfg4_inputs
    g = load_golden("g3_conv.npz")
    for si in range(int(g["n_settings"])):
        x32, radem, chi32, sl = g[f"x_{si}"], g[f"radem_{si}"], g[f"chi_{si}"], g[f"seqlen_{si}"]
        cw, sc = int(g[f"conv_width_{si}"]), int(g[f"scaling_{si}"])
        F = chi32.shape[0]
        kmax = int(sl.max()) - cw + 1
        scale = np.sqrt(1.0 / F) * {0: kmax, 1: np.sqrt(kmax), 2: 1.0}[sc]
        ref = g[f"out32_{si}"]
        rows = torch.full(ref.shape, float("nan"), dtype=torch.float32, device=DEV)
        ext.hipConvFeatureRows(dev(x32), rows, dev(radem), dev(chi32), sl, cw, sc, False)
        got = rows.cpu().numpy().astype(np.float64)
        # 4e-7 * scale as for the float64 operator, plus the one rounding to float32 (2^-24 relative) of the stored value
        err = np.abs(got - ref.astype(np.float32).astype(np.float64)).max()
        print(f"g3 setting {si}: max abs err {err:.3e}, bound {4e-7 * scale:.3e}")
        assert err <= 4e-7 * scale
        assert np.allclose(got, ref, rtol=1e-5, atol=1e-5 * scale)
    g = load_golden("g17_cfg4_conv.npz")
    x, seqlen = cfg4_inputs()
    for averaging in ("none", "sqrt", "full"):
        kern = make_kernel("Conv1dRBF", x.shape, int(g["num_rffs"]), 123, DEV,
                           {"conv_width": int(g["conv_width"]), "averaging": averaging})
        kern.set_hyperparams(g["hyperparams"], logspace=False)
        rows = torch.empty((x.shape[0], int(g["num_rffs"])), dtype=torch.float32, device=DEV)
        kern.fill_feature_rows(scale_input(dev(x), kern.hyperparams[1]), seqlen, rows)
        z = rows.cpu().numpy().astype(np.float64)
        ref = g[f"z_{averaging}"].astype(np.float32).astype(np.float64)
        nk = (seqlen - int(g["conv_width"]) + 1).astype(np.float64)
        scaler = np.sqrt(1.0 / (int(g["num_rffs"]) // 2)) / {"none": np.ones_like(nk), "sqrt": np.sqrt(nk), "full": nk}[averaging]
        bound = 4e-7 * nk * scaler
        err = np.abs(z - ref)
        err[:, 0] = 0.0
        assert np.array_equal(z[:, 0], ref[:, 0])
        print(f"g17 {averaging}: row errors {err.max(axis=1)}, bounds {bound}")
        assert np.all(err.max(axis=1) <= bound), (err.max(axis=1), bound)
        assert np.allclose(z, ref, rtol=1e-5, atol=1e-5 * scaler.max())


def test_argument_checks(ext):
    from xgpr_amd.kernels import make_kernel
    n, L, Cc, cw, rffs = 8, 12, 8, 3, 64
    kern = make_kernel("Conv1dRBF", (n, L, Cc), rffs, 123, DEV, {"conv_width": cw})
    x = torch.ones((n, L, Cc), dtype=torch.float32, device=DEV)
    sl = np.full(n, L, dtype=np.int32)
    rows = torch.full((n, rffs), 7.0, dtype=torch.float32, device=DEV)
    args = (kern.radem_diag, kern.chi_arr)
    with pytest.raises(TypeError):                                           # wrong dtypes
        ext.hipConvFeatureRows(x, rows.double(), *args, sl, cw, 0, True)
    with pytest.raises(TypeError):
        ext.hipConvFeatureRows(x.double(), rows, *args, sl, cw, 0, True)
    with pytest.raises(TypeError):
        ext.hipConvFeatureRows(x, rows, *args, sl.astype(np.int64), cw, 0, True)
    with pytest.raises(RuntimeError, match="no datapoints"):                 # wrong row count
        ext.hipConvFeatureRows(x, rows[:-1], *args, sl, cw, 0, True)
    with pytest.raises(RuntimeError, match="wrong array sizes"):
        ext.hipConvFeatureRows(x, rows, *args, sl[:-1], cw, 0, True)
    with pytest.raises(RuntimeError, match="incorrect number of rffs"):
        ext.hipConvFeatureRows(x, torch.empty((n, rffs + 2), dtype=torch.float32, device=DEV), *args, sl, cw, 0, True)
    short = sl.copy()
    short[3] = cw - 1
    with pytest.raises(RuntimeError, match="sequence lengths must be >= conv width"):
        ext.hipConvFeatureRows(x, rows, *args, short, cw, 0, True)
    long = sl.copy()
    long[0] = L + 1
    with pytest.raises(RuntimeError, match="sequence lengths"):
        ext.hipConvFeatureRows(x, rows, *args, long, cw, 0, True)
    with pytest.raises(RuntimeError, match="conv_width"):
        ext.hipConvFeatureRows(x, rows, *args, sl, L + 1, 0, True)
    flat = torch.full((n * rffs + 1,), 7.0, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="8-byte aligned"):                # a view that starts 4 bytes into an allocation
        ext.hipConvFeatureRows(x, flat[1:].view(n, rffs), *args, sl, cw, 0, True)
    torch.cuda.synchronize()
    assert bool(torch.all(rows == 7.0)) and bool(torch.all(flat == 7.0))     # never a launch
    ext.hipConvFeatureRows(x, rows, *args, sl, cw, 0, True)
    assert bool(torch.all(rows[:, 0] == 1.0)) and not bool(torch.any(rows[:, 1:] == 7.0))


def _seq_problem(name, n, L, Cc, seed, lo_len=None):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, L, Cc)).astype(np.float32)
    cw = 1 if name.startswith("Graph") else 5
    sl = rng.integers(lo_len or cw, L + 1, size=n).astype(np.int32)
    w = rng.standard_normal(Cc)
    mean = np.array([x[i, :sl[i]].mean(axis=0) @ w for i in range(n)])
    y = np.sin(2.0 * mean) + 0.05 * rng.standard_normal(n)
    return x, sl, y, mean, rng


def _kernel(name, xshape, m, sigma=0.6):
    from xgpr_amd.kernels import make_kernel
    parms = {"averaging": "sqrt"}
    if not name.startswith("Graph"):
        parms["conv_width"] = 5
    kern = make_kernel(name, xshape, m, 123, DEV, parms)
    kern.set_hyperparams(np.array([0.4, sigma]), logspace=False)
    return kern


def test_cache_equals_rounded_transform_x_over_a_large_shard(ext, monkeypatch):
    """More than 8192 sequences (the slice the cache used to be built in): one launch, same bits as the rounding of transform_x."""
    from xgpr_amd.dataset import build_regression_dataset
    n, L, Cc, m = 9000, 16, 8, 512
    x, sl, y, _, _ = _seq_problem("Conv1dRBF", n, L, Cc, 3)
    ds = build_regression_dataset(x, y, sl, chunk_size=1024, device=DEV)
    kern = _kernel("Conv1dRBF", x.shape, m)
    launches = []
    orig = kern.fill_feature_rows
    kern.fill_feature_rows = lambda xs, lens, out: (launches.append((xs.shape[0], out.shape)), orig(xs, lens, out))[1]
    with monkeypatch.context() as mp:
        _forbid_float64_operator(mp, ext)
        zc = ds.feature_cache(kern)
    kern.fill_feature_rows = orig
    assert launches == [(n, (n, m))]                 # one launch of the rows operator over the whole shard, into the cache itself
    assert zc.dtype == torch.float32 and zc.shape == (n, m)
    for lo in range(0, n, 3000):
        assert torch.equal(zc[lo:lo + 3000], kern.transform_x(x[lo:lo + 3000], sl[lo:lo + 3000]).to(torch.float32))
    out = torch.full((100, m), float("nan"), dtype=torch.float32, device=DEV)      # a float32 target from the unscaled input
    assert kern.transform_x(x[:100], sl[:100], rows_out=out) is out and torch.equal(out, zc[:100])


def _forbid_float64_operator(monkeypatch, ext):
    def raiser(*a, **k):
        raise AssertionError("the float64 convolution feature operator was called")
    monkeypatch.setattr(ext, "hipConv1dFGen", raiser)
    monkeypatch.setattr(ext, "cudaConv1dFGen", raiser)


@pytest.mark.parametrize("name", ["Conv1dRBF", "GraphRBF"])
def test_no_pass_materialises_float64_z(ext, monkeypatch, name):
    """With the float64 operator raising and cache_features=False: z^T y, both preconditioner builds, the k = 1 solve, the
    k = 26 block matvec, the approximate NMLL, exact weights and variance, the predicted mean, and a classifier fit and its
    probabilities all run to completion on float32 rows."""
    from xgpr_amd.dataset import build_regression_dataset, build_classification_dataset
    from xgpr_amd.preconditioner import RandNysPreconditioner
    from xgpr_amd.cg import cg_fit_lib_internal, calc_zty, ConjugateGrad, holds_cache
    from xgpr_amd import nmll
    from xgpr_amd.exact import calc_weights_exact, calc_variance_exact, predict_mean
    from xgpr_amd.classification import fit_classifier, predict_proba
    n, L, Cc, m = 1500, 14, 10, 512
    x, sl, y, mean, rng = _seq_problem(name, n, L, Cc, 11)
    ds = build_regression_dataset(x, y, sl, chunk_size=400, device=DEV)
    cds = build_classification_dataset(x, np.digitize(mean, [-0.2, 0.2]).astype(np.int64), sl, chunk_size=400, device=DEV)
    kern = _kernel(name, x.shape, m)
    assert kern.seq_rows_ok() and not kern.fused_ok()
    _forbid_float64_operator(monkeypatch, ext)
    zty, yty = calc_zty(ds, kern)
    assert torch.isfinite(zty).all() and yty > 0
    for method in ("srht", "srht_2"):
        pre = RandNysPreconditioner(kern, ds, 64, False, 123, method, cache_features=False)
        assert rel(pre.get_zty(), zty) < 1e-10
    w, niter, _ = cg_fit_lib_internal(kern, ds, 1e-7, 300, pre, False, cache_features=False)
    assert torch.isfinite(w).all() and niter < 300
    vec = torch.from_numpy(rng.standard_normal((m, 26))).to(DEV)
    mv = torch.zeros_like(vec)
    ConjugateGrad(cache_features=False)._matvec(ds, kern, vec, mv, add_ridge=False)
    assert torch.isfinite(mv).all()
    assert not holds_cache(ds, kern)                     # nothing above built the resident cache
    val = nmll.approximate_nmll(kern, ds, pre, {"nsamples": 25, "nmll_iter": 300, "nmll_tol": 1e-6}, 123, cache_features=False)
    assert np.isfinite(val)
    from xgpr_amd import cg as cgmod
    monkeypatch.setattr(cgmod, "_resolve_cache_mode", lambda *a, **k: False)      # exact mode: windows, not the "auto" cache
    we, _, _ = calc_weights_exact(ds, kern)
    var = calc_variance_exact(kern, ds, 128)
    pm = predict_mean(kern, we, dev(x[:200]), ds.get_ymean(), ds.get_ystd(), sl[:200], chunk_size=64)
    assert torch.isfinite(we).all() and torch.isfinite(var).all() and torch.isfinite(pm).all()
    assert not holds_cache(ds, kern)
    ckern = _kernel(name, x.shape, m)
    cpre = RandNysPreconditioner(ckern, cds, 64, False, 123, "srht", is_regression=False, cache_features=False)
    cw_, gamma, _, losses = fit_classifier(ckern, cds, cpre, tol=1e-2, max_iter=100, cache_features=False)
    probs = predict_proba(ckern, cw_, gamma, dev(x[:200]), sl[:200], chunk_size=64)
    assert losses[-1] < losses[0] and torch.allclose(probs.sum(dim=1), torch.ones(200, dtype=torch.float64, device=DEV))
    assert not holds_cache(cds, ckern)


def _f64_route(monkeypatch):
    from xgpr_amd.kernels import ConvSORFKernel
    for nm in ("seq_rows_ok", "cache_ok", "block_ok"):
        monkeypatch.setattr(ConvSORFKernel, nm, lambda self: False)


@pytest.mark.parametrize("name,method", [("Conv1dRBF", "srht"), ("GraphRBF", "srht_2")])
def test_fit_on_rows_equals_the_materialised_float64_path(name, method, monkeypatch):
    """z^T y, the preconditioner, the k = 1 solve, the k = 26 and k = 1 matvecs on the resident cache, on regenerated windows
    and on float64 Z materialised chunk by chunk (predicates off).  The windows leg runs with the window sizes at their
    minimum: the solver's passes see nine windows of sequences (the last one ragged: 1024 x 8 + 808), the preconditioner's two
    (8192 + 808), so its partial sums are partitioned differently from the resident leg's."""
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.preconditioner import RandNysPreconditioner
    from xgpr_amd.cg import cg_fit_lib_internal, calc_zty, ConjugateGrad, holds_cache
    from xgpr_amd import cg as cgmod, preconditioner as premod
    n, L, Cc, m = 9000, 14, 10, 1024
    x, sl, y, _, _ = _seq_problem(name, n, L, Cc, 21)
    vec = torch.from_numpy(np.random.default_rng(1).standard_normal((m, 26))).to(DEV)
    out = {}
    for route in ("resident", "windows", "f64"):
        ds = build_regression_dataset(x, y, sl, chunk_size=1000, device=DEV)
        kern = _kernel(name, x.shape, m)
        if route == "f64":
            _f64_route(monkeypatch)
            assert not kern.cache_ok() and not kern.block_ok() and not kern.seq_rows_ok()
        else:
            assert not kern.fused_ok() and kern.seq_rows_ok() and kern.cache_ok() and kern.block_ok()
        cache = route == "resident"
        nwin = []
        if route == "windows":
            monkeypatch.setattr(ConjugateGrad, "BLOCK_WINDOW_BYTES", 1)
            monkeypatch.setattr(premod, "ROW_WINDOW_BYTES", 1)
            real = cgmod.window_ranges

            def counted(*a, **k):
                got = list(real(*a, **k))
                nwin.append(len(got))
                return iter(got)
            monkeypatch.setattr(cgmod, "window_ranges", counted)
            monkeypatch.setattr(premod, "window_ranges", counted)
        zty, yty = calc_zty(ds, kern)
        pre = RandNysPreconditioner(kern, ds, 128, False, 123, method, cache_features=cache)
        if route == "windows":
            assert nwin[0] == 9 and set(nwin[1:]) == {2}          # z^T y: 9 windows; every preconditioner pass: 2
        w, niter, _ = cg_fit_lib_internal(kern, ds, 1e-7, 300, pre, False, cache_features=cache)
        assert holds_cache(ds, kern) == cache
        if cache:
            zty_res, _ = calc_zty(ds, kern)              # now from the resident rows
            assert rel(zty_res, zty) < 1e-12
        mv = torch.zeros_like(vec)
        ConjugateGrad(cache_features=cache)._matvec(ds, kern, vec, mv, add_ridge=False)
        mv1 = torch.zeros((m, 1), dtype=torch.float64, device=DEV)
        ConjugateGrad(cache_features=cache)._matvec(ds, kern, vec[:, :1].contiguous(), mv1, add_ridge=False)
        if route == "windows":
            assert nwin.count(9) >= 3 + niter              # z^T y, both matvecs and every CG iteration went window by window
        out[route] = (zty, yty, w, niter, mv, mv1)
        monkeypatch.undo()
    zb, yb, wb, nb, mb, m1b = out["f64"]
    for route in ("resident", "windows"):
        za, ya, wa, na, ma, m1a = out[route]
        print(route, "zty", rel(za, zb), "niter", na, nb, "w", rel(wa, wb), "mv", rel(ma, mb), rel(m1a, m1b))
        assert rel(za, zb) < 1e-7 and abs(ya - yb) <= 1e-12 * abs(yb)
        assert abs(na - nb) <= 1
        assert rel(wa, wb) < 1e-5
        assert rel(ma, mb) < 1e-6 and rel(m1a, m1b) < 1e-6
    print("resident vs windows: niter", out["resident"][3], out["windows"][3], "w", rel(out["resident"][2], out["windows"][2]),
          "zty", rel(out["resident"][0], out["windows"][0]))
    assert out["resident"][3] == out["windows"][3]
    assert rel(out["resident"][2], out["windows"][2]) < 1e-6
    assert rel(out["resident"][0], out["windows"][0]) < 1e-12


def test_windows_with_a_ragged_last_window(monkeypatch):
    """The k = 1 matvec and z^T y over several regenerated windows (the last one short) equal the single-window result; the
    windowed matvec twice gives identical bits."""
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.cg import ConjugateGrad, calc_zty
    n, L, Cc, m = 2500, 14, 10, 2048
    x, sl, y, _, rng = _seq_problem("Conv1dRBF", n, L, Cc, 31)
    ds = build_regression_dataset(x, y, sl, chunk_size=1000, device=DEV)
    kern = _kernel("Conv1dRBF", x.shape, m)
    vec = torch.from_numpy(rng.standard_normal((m, 1))).to(DEV)
    one = torch.zeros_like(vec)
    ConjugateGrad(cache_features=False)._matvec(ds, kern, vec, one, add_ridge=False)
    zty1, _ = calc_zty(ds, kern)
    monkeypatch.setattr(ConjugateGrad, "BLOCK_WINDOW_BYTES", 1024 * 4 * m)      # windows of 1024 sequences: 1024, 1024, 452
    many, again = torch.zeros_like(vec), torch.zeros_like(vec)
    ConjugateGrad(cache_features=False)._matvec(ds, kern, vec, many, add_ridge=False)
    ConjugateGrad(cache_features=False)._matvec(ds, kern, vec, again, add_ridge=False)
    zty3, _ = calc_zty(ds, kern)
    assert rel(many, one) < 1e-12 and rel(zty3, zty1) < 1e-12
    assert torch.equal(many, again)


def test_nmll_exact_predict_and_classifier_equal_the_float64_path(monkeypatch):
    """The approximate NMLL (k = 26 probes), the exact-mode fit, variance and predicted mean, and a small classifier agree with
    the same computations on float64 Z (predicates off), at the tolerances of the fixed-vector test of the same name."""
    from xgpr_amd.dataset import build_regression_dataset, build_classification_dataset
    from xgpr_amd import nmll
    from xgpr_amd.exact import calc_weights_exact, calc_variance_exact, predict_mean, gram_route
    from xgpr_amd.preconditioner import RandNysPreconditioner
    from xgpr_amd.classification import fit_classifier, predict_proba
    name, n, L, Cc, m = "Conv1dRBF", 3000, 14, 10, 1024
    x, sl, y, mean, _ = _seq_problem(name, n, L, Cc, 41)
    xtest, sltest = dev(x[:300] + 0.01), sl[:300]
    labels = np.digitize(mean, [-0.2, 0.2]).astype(np.int64)
    res = {}
    for f64 in (False, True):
        ds = build_regression_dataset(x, y, sl, chunk_size=1000, device=DEV)
        cds = build_classification_dataset(x, labels, sl, chunk_size=1000, device=DEV)
        if f64:
            _f64_route(monkeypatch)
        kern = _kernel(name, x.shape, m)
        det = {}
        pre = RandNysPreconditioner(kern, ds, 256, False, 123, "srht_2", cache_features=False)
        approx = nmll.approximate_nmll(kern, ds, pre, {"nsamples": 25, "nmll_iter": 500, "nmll_tol": 1e-6}, 123,
                                       cache_features=False, details=det)
        assert (gram_route(ds, kern, m) is None) == f64
        w, _, _ = calc_weights_exact(ds, kern)
        var = calc_variance_exact(kern, ds, 128)
        pm = predict_mean(kern, w, xtest, ds.get_ymean(), ds.get_ystd(), sltest)
        ckern = _kernel(name, x.shape, m)
        cpre = RandNysPreconditioner(ckern, cds, 256, False, 123, "srht", is_regression=False, cache_features=False)
        cw_, gamma, cniter, closses = fit_classifier(ckern, cds, cpre, tol=1e-2, max_iter=500, cache_features=False)
        probs = predict_proba(ckern, cw_, gamma, xtest, sltest)
        res[f64] = (approx, det, w, var, pm, cw_, cniter, closses, probs)
        monkeypatch.undo()
    (a0, d0, w0, v0, p0, c0, n0, l0, pr0), (a1, d1, w1, v1, p1, c1, n1, l1, pr1) = res[False], res[True]
    print("nmll", a0, a1, "niter", d0["niter"], d1["niter"], "logdet", d0["logdet"], d1["logdet"], "w", rel(w0, w1), "var", rel(v0, v1),
          "classifier", n0, n1, rel(c0, c1))
    assert np.isclose(a0, a1, rtol=1e-6)
    assert abs(d0["niter"] - d1["niter"]) <= 1
    assert np.isclose(d0["logdet"], d1["logdet"], rtol=1e-5)
    assert rel(w0, w1) < 1e-5 and rel(v0, v1) < 1e-5
    assert np.allclose(p0.cpu().numpy(), p1.cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert n0 == n1 and np.allclose(l0, l1, rtol=1e-5)
    assert rel(c0, c1) < 1e-4
    assert np.allclose(pr0.cpu().numpy(), pr1.cpu().numpy(), rtol=1e-4, atol=1e-6)
