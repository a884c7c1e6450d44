"""The resident feature cache as IEEE binary16 rows (cache_features="half"): the packer against torch's own rounding bit for bit,
the streaming matvec against the float64 product of the same widened rows, the dataset's binary16 cache, and the solve, the
model and the fall-back built on them.  No test asks how far a half-mode solution is from a float32-mode one: that is the
effect of rounding the features and depends on the problem (DESIGN.md section 3.14 reports it)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def _rbf_kernel(n, d, m, icpt=True, lam=0.1):
    from xgpr_amd.kernels import make_kernel
    k = make_kernel("RBF", (n, d), m, 123, DEV, {"intercept": icpt})
    k.set_hyperparams(np.array([lam, 1.0]), logspace=False)
    return k


def _half_rows(ext, d, m, icpt, n):
    """(kernel, binary16 rows [n, m]) from hipRBFFeatureCache followed by hipRowsToHalf."""
    k = _rbf_kernel(n, d, m, icpt)
    g = torch.Generator(device=DEV).manual_seed(d + m + n)
    x = torch.randn(n, d, generator=g, device=DEV, dtype=torch.float32) / np.sqrt(d)
    zc = torch.empty((n, m), dtype=torch.float32, device=DEV)
    ext.hipRBFFeatureCache(x, zc, k.radem_diag, k.chi_arr)
    zc16 = torch.empty((n, m), dtype=torch.float16, device=DEV)
    ext.hipRowsToHalf(zc, zc16)
    assert torch.equal(zc16.view(torch.int16), zc.half().view(torch.int16))
    return k, zc16


# ---- 1. the packer
SPECIAL = [0.0, -0.0, 1.0, -1.0, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11]


@pytest.mark.parametrize("count", [2, 8, 1022, 64 * 1024 + 6])
def test_pack_equals_torch_half_bit_for_bit(ext, count):
    g = torch.Generator(device=DEV).manual_seed(count)
    for src in (torch.rand(100_000, generator=g, device=DEV) * 2 - 1,                 # [-1, 1]
                (torch.rand(100_000, generator=g, device=DEV) * 2 - 1) * 1e-4,        # binary16 subnormals
                torch.tensor(SPECIAL + [-v for v in SPECIAL], dtype=torch.float32, device=DEV).repeat(4000)):
        for rows in (src[:count].contiguous(), src):
            out = torch.full(rows.shape, float("nan"), dtype=torch.float16, device=DEV)
            ext.hipRowsToHalf(rows, out)
            assert torch.equal(out.view(torch.int16), rows.half().view(torch.int16))     # the bits: -0 stays -0
    # the special values one by one, ties to even and the smallest subnormal included
    sp = torch.tensor(SPECIAL, dtype=torch.float32, device=DEV)
    out = torch.empty(len(SPECIAL), dtype=torch.float16, device=DEV)
    ext.hipRowsToHalf(sp, out)
    want = torch.tensor([0.0, -0.0, 1.0, -1.0, 2.0 ** -24, 0.0, 2.0 ** -23, 1.0, 1.0 + 2.0 ** -9], dtype=torch.float16, device=DEV)
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))


# ---- 2. the matvec: (d, M, intercept, n), the smallest shapes that reach each arm
SHAPES = [(3, 2, False, 1), (7, 10, True, 33),
          (16, 12, True, 40),               # num_freqs even and no multiple of 4: 8-byte loads
          (20, 64, False, 9001),            # one tile, 8 slots per workgroup, n beyond ring x slots: the ring refills
          (100, 3000, True, 777),           # partial tile
          (64, 6146, True, 5),              # rows not 16-byte aligned: 4-byte loads
          (256, 4096, True, 3000), (1024, 8192, True, 1500),
          (512, 16384, False, 300)]         # eight tiles, one slot


def _reference(zc16, v, scale, icpt):
    zz = zc16.double() * scale
    if icpt:
        zz[:, 0] = 1.0
    return zz.T @ (zz @ v)


@pytest.mark.parametrize("d,m,icpt,n", SHAPES)
def test_matvec_equals_the_float64_product_of_the_widened_rows(ext, d, m, icpt, n):
    k, zc16 = _half_rows(ext, d, m, icpt, n)
    g = torch.Generator(device=DEV).manual_seed(m)
    v = torch.randn(m, generator=g, device=DEV, dtype=torch.float64)
    ws = torch.empty(k.workspace_bytes(), dtype=torch.uint8, device=DEV)
    _, scale = k.row_cache_params()
    out = torch.full((m,), float("nan"), dtype=torch.float64, device=DEV)
    ext.hipZCacheMatvecHalf(zc16, v, out, icpt, ws)
    ref = _reference(zc16, v, scale, icpt)
    err, top = float((out - ref).abs().max()), float(ref.abs().max())
    print(f"half matvec d={d} M={m} n={n}: max err {err:.3e}, bound {1e-12 * top:.3e}")
    assert err <= 1e-12 * top
    out2 = torch.zeros_like(out)
    ext.hipZCacheMatvecHalf(zc16, v, out2, icpt, ws)
    assert torch.equal(out, out2)
    ext.hipZCacheMatvecHalfScaled(zc16, v, out2, 0.37, ws)
    ref = _reference(zc16, v, 0.37, False)
    assert float((out2 - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    k.ztz_matvec_cached_f16(zc16, v, out2, ws)
    assert torch.equal(out, out2)


# ---- 3. additivity
def test_matvec_is_additive_over_a_ragged_split_of_the_rows(ext):
    d, m, icpt, n = 256, 4096, True, 3000
    k, zc16 = _half_rows(ext, d, m, icpt, n)
    v = torch.randn(m, generator=torch.Generator(device=DEV).manual_seed(5), device=DEV, dtype=torch.float64)
    ws = torch.empty(k.workspace_bytes(), dtype=torch.uint8, device=DEV)
    w, wa, wb = (torch.empty(m, dtype=torch.float64, device=DEV) for _ in range(3))
    h = n // 3
    ext.hipZCacheMatvecHalf(zc16, v, w, icpt, ws)
    ext.hipZCacheMatvecHalf(zc16[:h], v, wa, icpt, ws)
    ext.hipZCacheMatvecHalf(zc16[h:], v, wb, icpt, ws)
    assert float((wa + wb - w).abs().max() / w.abs().max()) < 1e-12


# ---- 4. argument checks
def test_argument_checks(ext):
    n = 4
    ws = torch.empty(ext.ztz_workspace_bytes(16386, 8192), dtype=torch.uint8, device=DEV)
    wide = torch.zeros((n, 16386), dtype=torch.float16, device=DEV)
    vw = torch.zeros(16386, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="8192"):
        ext.hipZCacheMatvecHalf(wide, vw, torch.empty_like(vw), True, ws)
    m = 128
    v = torch.zeros(m, dtype=torch.float64, device=DEV)
    out = torch.empty_like(v)
    flat = torch.zeros(n * m + 1, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="aligned"):
        ext.hipZCacheMatvecHalf(flat[1:].view(n, m), v, out, True, ws)
    zc16 = flat[:n * m].view(n, m)
    with pytest.raises(RuntimeError, match="workspace"):
        ext.hipZCacheMatvecHalf(zc16, v, out, True, ws[:256])
    with pytest.raises(TypeError):
        ext.hipZCacheMatvecHalf(torch.zeros((n, m), dtype=torch.float32, device=DEV), v, out, True, ws)
    with pytest.raises(TypeError):
        ext.hipZCacheMatvecHalf(zc16, v[:m - 2], out, True, ws)
    with pytest.raises(TypeError):
        ext.hipZCacheMatvecHalfScaled(zc16, v, out[:m - 2], 1.0, ws)
    with pytest.raises(RuntimeError, match="scale"):
        ext.hipZCacheMatvecHalfScaled(zc16, v, out, 0.0, ws)
    with pytest.raises(TypeError):
        ext.hipRowsToHalf(torch.zeros((n, m), dtype=torch.float32, device=DEV), torch.zeros((n, m + 2), dtype=torch.float16, device=DEV))
    with pytest.raises(TypeError):
        ext.hipRowsToHalf(torch.zeros((n, m), dtype=torch.float64, device=DEV), zc16)


# ---- 5.-8. the dataset's cache, the solve, the model, the fall-back
def _rbf_problem(n=6000, d=20, m=1024):
    from xgpr_amd.dataset import build_regression_dataset
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(n, d, generator=g, device=DEV, dtype=torch.float32)
    y = torch.sin(x @ torch.randn(d, generator=g, device=DEV)).double() + 0.1 * torch.randn(n, generator=g, device=DEV, dtype=torch.float64)
    return x, y, build_regression_dataset(x, y, chunk_size=2000, device=DEV), _rbf_kernel(n, d, m)


def _seq_problem(n=300, L=40, Cc=8, cw=5, m=512):
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.kernels import make_kernel
    rng = np.random.default_rng(3)
    x = rng.standard_normal((n, L, Cc)).astype(np.float32)
    sl = rng.integers(cw, L + 1, size=n).astype(np.int32)
    y = np.tanh(x[:, :cw, 0].sum(axis=1)) + 0.1 * rng.standard_normal(n)
    ds = build_regression_dataset(x, y, sl, chunk_size=128, device=DEV)
    k = make_kernel("Conv1dRBF", x.shape, m, 123, DEV, {"conv_width": cw})
    k.set_hyperparams(np.array([0.1, 0.8]), logspace=False)
    return ds, k


def _bits(t):
    return t.view(torch.int16)


def test_dataset_cache_f16_equals_the_rounded_float32_cache(monkeypatch):
    from xgpr_amd.dataset import DeviceDataset, build_regression_dataset
    from xgpr_amd.cg import holds_cache
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    n, d, m = 2500, 20, 512
    x = torch.randn(n, d, generator=torch.Generator(device=DEV).manual_seed(2), device=DEV, dtype=torch.float32)
    y = x[:, 0].double()
    monkeypatch.setattr(DeviceDataset, "HALF_WINDOW_BYTES", 1024 * 4 * m)           # three windows: 1024, 1024, 452 rows
    packed = []
    orig = ext.hipRowsToHalf
    monkeypatch.setattr(ext, "hipRowsToHalf", lambda src, dst: (packed.append(src.shape[0]), orig(src, dst))[1])
    for make in (lambda: (build_regression_dataset(x, y, chunk_size=1000, device=DEV), _rbf_kernel(n, d, m)), lambda: _seq_problem()):
        ds, k = make()
        nrows = ds.get_local_ndatapoints()
        assert k.half_cache_ok() and ds.feature_cache_f16_bytes(k) == nrows * m * 2
        del packed[:]
        z16 = ds.feature_cache_f16(k)
        assert packed == ([1024, 1024, 452] if nrows == n else [nrows])
        assert not holds_cache(ds, k) and getattr(ds, "_zcache", None) is None     # built with no float32 cache, and made none
        assert z16.dtype == torch.float16 and tuple(z16.shape) == (nrows, m) and ds.feature_cache_f16(k) is z16
        want = ds.feature_cache(k).half()
        assert torch.equal(_bits(z16), _bits(want))
        # once more, packed from the resident float32 cache (a new kernel object: a new key)
        ds2, k2 = make()
        ds2.feature_cache(k2)
        del packed[:]
        assert holds_cache(ds2, k2) and torch.equal(_bits(ds2.feature_cache_f16(k2)), _bits(want))
        assert packed == [nrows]
        # a new sigma rebuilds it
        k2.set_hyperparams(np.array([0.1, 0.5]), logspace=False)
        z16b = ds2.feature_cache_f16(k2)
        assert torch.equal(_bits(z16b), _bits(ds2.feature_cache(k2).half())) and not torch.equal(_bits(z16b), _bits(want))


def _residual(ds, k, w, b):
    """||A w - b|| / ||b|| with A = Zh^T Zh + lambda^2 I in float64 from the dataset's binary16 rows."""
    z16 = ds.feature_cache_f16(k)
    assert z16.dtype == torch.float16 and tuple(z16.shape) == (ds.get_local_ndatapoints(), k.get_num_rffs())
    zh = k.cache_rows_to_features(z16)          # widen, times the kernel's scale, intercept column: float64
    aw = zh.T @ (zh @ w) + k.get_lambda() ** 2 * w
    return float(torch.linalg.norm(aw - b) / torch.linalg.norm(b))


@pytest.fixture(scope="module")
def rbf_solve():
    """The RBF problem solved once in half mode with a rank-128 preconditioner (shared by the solve and the model test)."""
    from xgpr_amd.cg import cg_fit_lib_internal, holds_cache
    from xgpr_amd.preconditioner import RandNysPreconditioner
    x, y, ds, k = _rbf_problem()
    pre = RandNysPreconditioner(k, ds, 128, False, 123, "srht")
    before = holds_cache(ds, k)
    w, niter, _ = cg_fit_lib_internal(k, ds, 1e-6, 500, pre, False, cache_features="half")
    return dict(x=x, y=y, ds=ds, k=k, pre=pre, w=w, niter=niter, before=before)


def test_solve_satisfies_the_normal_equations_of_the_rounded_features(rbf_solve):
    from xgpr_amd.cg import cg_fit_lib_internal, calc_zty, holds_cache
    s = rbf_solve
    ds, k = s["ds"], s["k"]
    assert getattr(ds, "_zcache16", None) is not None and ds._zcache16.dtype == torch.float16
    assert holds_cache(ds, k) == s["before"]
    r = _residual(ds, k, s["w"], s["pre"].get_zty())
    print(f"half solve, rank-128 preconditioner: {s['niter']} iterations, residual {r:.3e}")
    assert r < 1e-5
    # no preconditioner: the right-hand side is calc_zty's
    _, _, ds2, k2 = _rbf_problem()
    before = holds_cache(ds2, k2)
    w2, niter2, _ = cg_fit_lib_internal(k2, ds2, 1e-6, 500, None, False, cache_features="half")
    assert holds_cache(ds2, k2) == before and ds2._zcache16.dtype == torch.float16
    r2 = _residual(ds2, k2, w2, calc_zty(ds2, k2)[0])
    print(f"half solve, no preconditioner: {niter2} iterations, residual {r2:.3e}")
    assert r2 < 1e-5


def test_sequence_solve_satisfies_the_normal_equations_of_the_rounded_features():
    from xgpr_amd.cg import cg_fit_lib_internal, calc_zty, holds_cache
    ds, k = _seq_problem()
    before = holds_cache(ds, k)
    w, niter, _ = cg_fit_lib_internal(k, ds, 1e-6, 500, None, False, cache_features="half")
    assert holds_cache(ds, k) == before
    r = _residual(ds, k, w, calc_zty(ds, k)[0])
    print(f"half solve, Conv1dRBF: {niter} iterations, residual {r:.3e}")
    assert r < 1e-5


def test_model_fit_passes_the_mode_through(rbf_solve):
    from xgpr_amd.models import xGPRegression
    s = rbf_solve
    model = xGPRegression(num_rffs=s["k"].get_num_rffs(), variance_rffs=64, kernel_choice="RBF", device=DEV, verbose=False, random_seed=123)
    model.set_hyperparams(None, s["ds"])
    model.kernel.set_hyperparams(np.array([0.1, 1.0]), logspace=False)       # the very values of the solve above, not exp(log(.))
    model.fit(s["ds"], preconditioner=s["pre"], cache_features="half", suppress_var=True)
    assert torch.equal(model.weights, s["w"])                  # the path is deterministic
    assert s["ds"]._zcache16_key[0] == id(model.kernel)
    pred = model.predict(s["x"][:100].cpu().numpy())
    assert pred.shape == (100,) and np.isfinite(pred).all()


def test_unsupported_width_falls_back_to_the_float32_cache():
    from xgpr_amd.cg import cg_fit_lib_internal, _resolve_cache_mode
    n, d, m = 200, 8, 16388
    sols = {}
    for mode in ("half", True):
        g = torch.Generator(device=DEV).manual_seed(1)
        x = torch.randn(n, d, generator=g, device=DEV, dtype=torch.float32)
        y = x[:, 0].double() + 0.1 * torch.randn(n, generator=g, device=DEV, dtype=torch.float64)
        from xgpr_amd.dataset import build_regression_dataset
        ds = build_regression_dataset(x, y, chunk_size=100, device=DEV)
        k = _rbf_kernel(n, d, m)
        assert not k.half_cache_ok() and _resolve_cache_mode(mode, k, ds) is True
        sols[mode], _, _ = cg_fit_lib_internal(k, ds, 1e-6, 50, None, False, cache_features=mode)
        assert getattr(ds, "_zcache16", None) is None
    assert torch.equal(sols["half"], sols[True])
