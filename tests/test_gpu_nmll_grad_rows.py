"""GPU tests of the exact NMLL gradient from float32 feature and gradient rows: the rows writer (hipRBFGradRows) against the
float64 gradient operator bit for bit, the symmetrised two-operand Gram (hipCrossGram) against a float64 product, the host
route of nmll.calc_gradient_terms against the float64 formulation of the same kernel and against the reference's own numbers
(tests/golden/g10_nmll.npz), and the ``subsample`` argument (reference nmll_gradient_tools.py:37-86).

Tolerances.  Writer: none -- every entry of hipRBFGrad's outputs is a float32 value widened at the store.  Cross Gram and the
route's terms: both sides are float64 sums of the SAME float64 products (a product of two widened float32 values is exact in
float64), so only the summation order differs: 1e-12 x max|.| (a sum of n <= 1e5 terms of partial-sum size s carries
~ sqrt(n) x 1.1e-16 x s of order-dependent rounding, three to four orders below the bar at these shapes)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _kernel(name, d, m, icpt, n=37):
    from xgpr_amd.kernels import make_kernel
    parms = {"intercept": icpt}
    if name == "Matern":
        parms["matern_nu"] = 1.5
    kern = make_kernel(name, (n, d), m, 123, DEV, parms)
    kern.set_hyperparams(np.array([0.7, 0.45]), logspace=False)
    return kern


# ---------------------------------------------------------------------------------------------- writer contract
# (d, num_rffs): padded widths 16, 128, 1024 with two tiles, 2048, 4096, 8192; and one ragged tile shape (1300 frequencies:
# one full tile + 276 of the second) at padded width 1024
WRITER_SHAPES = [(9, 256), (84, 384), (1000, 2048), (1500, 512), (3000, 512), (5000, 256), (1000, 2 * 1300)]


@pytest.mark.parametrize("icpt", [True, False])
@pytest.mark.parametrize("d,m", WRITER_SHAPES)
def test_rows_equal_the_float64_gradient_operator_bit_for_bit(d, m, icpt):
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    n = 37
    rng = np.random.default_rng(d + m)
    x = torch.from_numpy(rng.uniform(-1, 1, size=(n, d)).astype(np.float32)).to(DEV)
    kern = _kernel("RBF", d, m, icpt)
    out, grad = kern.gradient_x(x)                  # hipRBFGrad + the host's intercept fix-up
    zrows = torch.full((n, m), float("nan"), dtype=torch.float32, device=DEV)      # overwritten: no zero fill needed
    grows = torch.full((n, m), float("nan"), dtype=torch.float32, device=DEV)
    assert ext.hipRBFGradRows(x, zrows, grows, kern.radem_diag, kern.chi_arr, float(kern.hyperparams[1]), icpt) == 0
    assert torch.equal(zrows.double(), out)
    assert torch.equal(grows.double(), grad[:, :, 0])
    if icpt:
        assert bool((zrows[:, 0] == 1.0).all()) and bool((grows[:, 0] == 0.0).all())
    assert float(grows.abs().max()) > 0.0


def _raw_grad_rows(kern, x, zptr, gptr, m):
    from xgpr_amd import _lib
    lib = _lib.load()
    ws = torch.empty(int(lib.xgpr_sorf_workspace_bytes(kern.radem_diag.shape[2], x.shape[1], 4)) + 256, dtype=torch.uint8, device=DEV)
    return lib.xgpr_rbf_grad_rows_f32(
        C.c_void_p(x.data_ptr()), C.c_void_p(zptr), C.c_void_p(gptr), C.c_void_p(kern.radem_diag.data_ptr()),
        C.c_void_p(kern.chi_arr.data_ptr()), x.shape[0], x.shape[1], m, m // 2, kern.radem_diag.shape[2],
        float(kern.hyperparams[1]), 1, C.c_void_p(ws.data_ptr()), C.c_size_t(ws.numel()),
        C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_writer_error_codes_launch_nothing():
    n, m = 5, 256
    sentinel = 7.0
    # padded width 16384: the code the float32 cache writer uses for a shape it has no plan for (XGPR_ERR_UNSUPPORTED = -20)
    kern = _kernel("RBF", 9000, m, True, n)
    x = torch.zeros((n, 9000), dtype=torch.float32, device=DEV)
    z = torch.full((n, m), sentinel, dtype=torch.float32, device=DEV)
    g = torch.full((n, m), sentinel, dtype=torch.float32, device=DEV)
    assert _raw_grad_rows(kern, x, z.data_ptr(), g.data_ptr(), m) == -20
    assert not kern.grad_rows_ok()
    # a 4-byte-aligned output view: XGPR_ERR_WORKSPACE = -21, as xgpr_conv_feature_rows_f32
    kern = _kernel("RBF", 9, m, True, n)
    x = torch.zeros((n, 9), dtype=torch.float32, device=DEV)
    flat = torch.full((n * m + 1,), sentinel, dtype=torch.float32, device=DEV)
    assert _raw_grad_rows(kern, x, flat.data_ptr() + 4, g.data_ptr(), m) == -21
    assert _raw_grad_rows(kern, x, z.data_ptr(), flat.data_ptr() + 4, m) == -21
    torch.cuda.synchronize()
    for t in (z, g, flat):
        assert bool((t == sentinel).all())
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    with pytest.raises(RuntimeError):
        ext.hipRBFGradRows(x, flat[1:].view(n, m), g, kern.radem_diag, kern.chi_arr, 0.45, True)


# ---------------------------------------------------------------------------------------------- cross Gram
_AB = {}


def _operands(n, m):
    """Random float32 operands and the float64 reference A^T B + (A^T B)^T, computed once per shape."""
    if (n, m) not in _AB:
        gen = torch.Generator(device="cpu").manual_seed(1000 * m + n)
        a = torch.randn((n, m), generator=gen, dtype=torch.float32).to(DEV)
        b = torch.randn((n, m), generator=gen, dtype=torch.float32).to(DEV)
        atb = a.double().T @ b.double()
        _AB[(n, m)] = (a, b, atb + atb.T)
    return _AB[(n, m)]


def _check_cross_gram(n, m, accumulate):
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    a, b, ref = _operands(n, m)
    ldc = m + 6
    bar = 1e-12 * float(ref.abs().max())
    pad = -3.0
    base = None
    if accumulate:
        s = torch.randn((m, m), dtype=torch.float64, device=DEV)
        base = s + s.T                                   # symmetric on entry, so symmetric on exit
    outs = []
    for _ in range(2):
        buf = torch.full((m, ldc), pad, dtype=torch.float64, device=DEV)
        view = buf[:, :m]                                # a view with ldc > M
        if accumulate:
            view.copy_(base)
        ext.hipCrossGram(a, b, view, accumulate=accumulate)
        assert bool((buf[:, m:] == pad).all())           # the padding columns stay untouched
        outs.append(view.clone())
    got = outs[0]
    want = ref + base if accumulate else ref
    err = float((got - want).abs().max())
    assert err <= bar, (err, bar)
    assert torch.equal(outs[0], outs[1])                 # two launches, identical bits
    assert torch.equal(got, got.T)                       # symmetric bit for bit


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("m", [128, 256, 384])
@pytest.mark.parametrize("n", [5, 16, 333, 2051])
def test_cross_gram_equals_the_float64_product(n, m, accumulate):
    """n = 5: tail only; 16: one chunk; 333 and 2051: chunks plus tail."""
    _check_cross_gram(n, m, accumulate)


def test_cross_gram_stream_k_spill_and_fixup():
    """A launch whose workgroups start inside a tile, so that the spill slabs and the fix-up run, with segments long enough for
    the six-way unrolled chunk loop and one segment that spans the two halves of the unit sequence.  The launcher's plan for
    M = 128, n = 49365 on 256 compute units: 1 tile of 2 x 3085 = 6170 units on 512 workgroup slots -> 13 units per workgroup,
    475 workgroups; every workgroup but the first starts inside the tile (474 slabs); workgroup 237 holds units 3081 .. 3093
    and crosses from the (A, B) half into the (B, A) half at unit 3085; 5 rows are left to the tail kernel.  The numbers are
    re-derived from the library's own workspace size below, so another device's plan is checked for the same properties."""
    from xgpr_amd import _lib
    n, m = 49365, 128
    slots = int(_lib.load().xgpr_cross_gram_workspace_bytes(m, n)) // (128 * 128 * 8)
    nchunks, tiles = n // 16, 1
    total = tiles * 2 * nchunks
    upw = -(-total // slots)
    assert upw >= 7 and (2 * nchunks) % upw != 0 and nchunks % upw != 0
    _check_cross_gram(n, m, False)
    _check_cross_gram(n, m, True)


def test_cross_gram_rejects_bad_arguments():
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    a = torch.zeros((16, 192), dtype=torch.float32, device=DEV)          # not a multiple of 128
    assert not ext.cross_gram_ok(192)
    with pytest.raises(RuntimeError):
        ext.hipCrossGram(a, a, torch.zeros((192, 192), dtype=torch.float64, device=DEV))
    a = torch.zeros((16, 128), dtype=torch.float32, device=DEV)
    with pytest.raises(TypeError):
        ext.hipCrossGram(a, a[:8], torch.zeros((128, 128), dtype=torch.float64, device=DEV))
    with pytest.raises(TypeError):
        ext.hipCrossGram(a, a, torch.zeros((128, 128), dtype=torch.float32, device=DEV))


# ---------------------------------------------------------------------------------------------- host route
def _route_case(name, d, n=2051, m=256):
    from xgpr_amd.dataset import build_regression_dataset
    rng = np.random.default_rng(d)
    x = rng.uniform(-1, 1, size=(n, d)).astype(np.float32)
    y = np.sin(x[:, :5].sum(axis=1)) + 0.1 * rng.standard_normal(n)
    ds = build_regression_dataset(x, y, chunk_size=500, device=DEV)
    return ds, _kernel(name, d, m, True, n)


@pytest.mark.parametrize("d", [9, 1500])
@pytest.mark.parametrize("name", ["RBF", "Matern"])
def test_route_equals_the_float64_formulation(name, d, monkeypatch):
    from xgpr_amd import nmll
    ds, kern = _route_case(name, d)
    assert kern.grad_rows_ok()
    rows = nmll.calc_gradient_terms(ds, kern)
    score_r, grad_r = nmll.exact_nmll_gradient(kern, ds)
    monkeypatch.setattr(type(kern), "grad_rows_ok", lambda self: False)
    f64 = nmll.calc_gradient_terms(ds, kern)
    score_f, grad_f = nmll.exact_nmll_gradient(kern, ds)
    for i, (r, f) in enumerate(zip(rows[:5], f64[:5])):
        r, f = torch.as_tensor(r), torch.as_tensor(f)
        bar = 1e-12 * float(f.abs().max())
        err = float((r - f).abs().max())
        assert err <= bar, (i, err, bar)
    assert rows[5] == f64[5] == 2051
    assert torch.equal(rows[4][:, :, 0], rows[4][:, :, 0].T)
    assert np.isclose(score_r, score_f, rtol=1e-9, atol=0.0)
    assert np.allclose(grad_r, grad_f, rtol=1e-9, atol=0.0)


def test_route_over_several_windows_with_a_ragged_last_one(monkeypatch):
    """n = 2051 in windows of 800 rows: 800, 800 and 451 (the last: 28 chunks + 3 tail rows) -- a second window with lo > 0, a
    shorter last window, the three workspaces reused across windows of different size, accumulation across launches.  Same bars
    as the one-window test."""
    from xgpr_amd import nmll
    ds, kern = _route_case("RBF", 9)
    filled = []
    orig_fill = type(kern).fill_grad_rows

    def counting_fill(self, x, zr, gr):
        filled.append(x.shape[0])
        return orig_fill(self, x, zr, gr)
    monkeypatch.setattr(type(kern), "fill_grad_rows", counting_fill)
    monkeypatch.setattr(nmll, "_grad_window_rows", lambda m: 800)
    rows = nmll.calc_gradient_terms(ds, kern)
    assert filled == [800, 800, 451]
    score_r, grad_r = nmll.exact_nmll_gradient(kern, ds)
    monkeypatch.setattr(type(kern), "grad_rows_ok", lambda self: False)
    f64 = nmll.calc_gradient_terms(ds, kern)
    score_f, grad_f = nmll.exact_nmll_gradient(kern, ds)
    for i, (r, f) in enumerate(zip(rows[:5], f64[:5])):
        r, f = torch.as_tensor(r), torch.as_tensor(f)
        bar = 1e-12 * float(f.abs().max())
        err = float((r - f).abs().max())
        assert err <= bar, (i, err, bar)
    assert torch.equal(rows[4][:, :, 0], rows[4][:, :, 0].T)
    assert np.isclose(score_r, score_f, rtol=1e-9, atol=0.0)
    assert np.allclose(grad_r, grad_f, rtol=1e-9, atol=0.0)


def test_route_is_not_taken_for_a_shard_the_writer_cannot_read():
    """A hand-built dataset whose x is float64 keeps the float64 formulation (which converts each chunk), as before."""
    from xgpr_amd import nmll
    from xgpr_amd.dataset import DeviceDataset
    ds, kern = _route_case("RBF", 9, n=300, m=128)
    ds64 = DeviceDataset(ds.get_xdata().double(), ds._ydata, None, 500, ds.get_ymean(), ds.get_ystd(), device=DEV)
    assert nmll._grad_rows_route(ds, kern) and not nmll._grad_rows_route(ds64, kern)
    a, b = nmll.calc_gradient_terms(ds, kern), nmll.calc_gradient_terms(ds64, kern)
    for r, f in zip(a[:5], b[:5]):
        r, f = torch.as_tensor(r), torch.as_tensor(f)
        assert float((r - f).abs().max()) <= 1e-12 * float(f.abs().max())


def test_route_does_not_call_the_float64_operator(monkeypatch):
    from xgpr_amd import nmll
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    ds, kern = _route_case("RBF", 9, n=700, m=128)

    def boom(*args, **kwargs):
        raise AssertionError("hipRBFGrad called on the rows route")
    monkeypatch.setattr(ext, "hipRBFGrad", boom)
    score, grad = nmll.exact_nmll_gradient(kern, ds)
    assert np.isfinite(score) and np.all(np.isfinite(grad))
    monkeypatch.setattr(type(kern), "grad_rows_ok", lambda self: False)
    with pytest.raises(AssertionError):
        nmll.calc_gradient_terms(ds, kern)


@pytest.mark.parametrize("tag", ["easy", "hard"])
def test_reference_gradient_fixture_through_the_rows_route(tag, monkeypatch):
    """The reference's own exact_nmll_gradient numbers (tests/golden/g10_nmll.npz, loaded as tests/test_gpu_nmll.py loads them)
    with that test's tolerances, on the rows route -- hipRBFGrad raises, so the float64 operator cannot have produced them."""
    from xgpr_amd.kernels import make_kernel
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd import nmll
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    g8, g = load_golden("g8_e2e.npz"), load_golden("g10_nmll.npz")
    x, y = g8["xtrain"], g8["ytrain"]
    ds = build_regression_dataset(x, y, chunk_size=2000, device=DEV)
    kern = make_kernel("RBF", x.shape, 512, 123, DEV, {"intercept": True})
    kern.set_hyperparams(g[f"{tag}_hparam_log"], logspace=True)
    assert kern.grad_rows_ok()

    def boom(*args, **kwargs):
        raise AssertionError("hipRBFGrad called on the rows route")
    monkeypatch.setattr(ext, "hipRBFGrad", boom)
    nll, grad = nmll.exact_nmll_gradient(kern, ds)
    assert np.isclose(nll, float(g[f"{tag}_grad_nmll"]), rtol=1e-6)
    assert np.allclose(grad, g[f"{tag}_grad"], rtol=2e-4, atol=1e-4)


# ---------------------------------------------------------------------------------------------- subsample
def test_subsample_equals_the_terms_of_the_drawn_rows():
    """subsample = 0.25: one generator seeded with 123, one choice without replacement per chunk in chunk order
    (nmll_gradient_tools.py:72-76), reproduced here; the dataset built from the drawn rows (standardised with the FULL
    dataset's mean and std, one chunk per original chunk) must give the same terms, score and gradient."""
    from xgpr_amd import nmll
    from xgpr_amd.dataset import DeviceDataset
    ds, kern = _route_case("RBF", 9, n=1234, m=128)          # chunks of 500, 500, 234 rows
    rng = np.random.default_rng(123)
    picks = []
    for lo in range(0, 1234, 500):
        rows = min(500, 1234 - lo)
        picks.append(lo + rng.choice(rows, max(1, int(0.25 * rows)), replace=False))
    assert [len(p) for p in picks] == [125, 125, 58]
    terms = nmll.calc_gradient_terms(ds, kern, subsample=0.25)
    assert terms[5] == 308
    want = None
    for p in picks:                                          # chunk by chunk, in the order the route adds them
        idx = torch.from_numpy(p).to(DEV)
        sub = DeviceDataset(ds.get_xdata()[idx], ds._ydata[idx], None, 500, ds.get_ymean(), ds.get_ystd(), device=DEV)
        t = nmll.calc_gradient_terms(sub, kern, subsample=1)
        if want is None:
            want = [torch.as_tensor(v, dtype=torch.float64).clone() for v in t[:5]]
        else:
            for acc, v in zip(want, t[:5]):
                acc += torch.as_tensor(v, dtype=torch.float64).to(acc.device)
    for i, (got, ref) in enumerate(zip(terms[:5], want)):
        got = torch.as_tensor(got, dtype=torch.float64).to(ref.device)
        bar = 1e-12 * float(ref.abs().max())
        assert float((got - ref).abs().max()) <= bar, i
    score, grad = nmll.exact_nmll_gradient(kern, ds, subsample=0.25)
    hp = kern.get_hyperparams(logspace=False)
    sc_ref, gr_ref, _ = nmll.exact_nmll_reg_grad(want[0], want[1], float(want[2]), hp, 308, want[3], want[4])
    assert np.isclose(score, sc_ref, rtol=1e-9) and np.allclose(grad, gr_ref, rtol=1e-9, atol=0.0)


def test_subsample_range_and_identity():
    from xgpr_amd import nmll
    from xgpr_amd.models import xGPRegression
    import inspect
    ds, kern = _route_case("RBF", 9, n=700, m=128)
    for bad in (0.005, 1.5, 0.0):
        with pytest.raises(RuntimeError, match="Subsample must be in the range"):
            nmll.exact_nmll_gradient(kern, ds, subsample=bad)
    s0, g0 = nmll.exact_nmll_gradient(kern, ds)
    s1, g1 = nmll.exact_nmll_gradient(kern, ds, subsample=1)
    assert s0 == s1 and np.array_equal(g0, g1)
    assert "subsample" in inspect.signature(xGPRegression.exact_nmll_gradient).parameters
