"""The CPU oracle against the dense-matrix reference (tests/dense_reference.py): every float32 and float64 oracle operator
stays within the reference's a-priori forward-error cap at the shapes the GPU leg uses (tests/test_gpu_dense_reference.py
imports the case tables below), and every structural mistake planted in the reference moves its output by at least 100 x
the cap, so the shapes cannot hide one.  Inputs are the same numbers in both precisions (float32 values widened), so one
dense reference per case serves both."""
import functools
from math import ceil

import numpy as np
import pytest

import dense_reference as dr
from conftest import load_golden

# (n, d, num_rffs): padded widths 2; 64 (one repetition, several with a ragged last one); 128; 1024 (1022: rows that are no
# multiple of 4 floats); 2048; 4096; 8192; 16384
FIXED = [(3, 1, 2), (4, 50, 128), (3, 60, 1000), (4, 100, 300), (3, 1000, 4100), (2, 1022, 8192), (2, 1025, 4096),
         (2, 4000, 8200), (2, 4100, 16400), (1, 9000, 32770)]
SCALES = (1.0, 30.0)            # row norm: cos / sin arguments ~ N(0, scale^2)
GRAD_FIXED = [(4, 50, 128), (3, 60, 1000), (3, 1000, 4100), (2, 1022, 8192), (2, 4000, 8200)]      # padded widths 64, 1024, 4096
SIGMA = 1.3
GRAD_SCALE = 1.0                # the gradient's cap grows with |p| dp ~ scale^2: at scale 30 in float32 it leaves no room for the
                                # 100-fold margin of the sensitivity test at the ragged shapes, so the gradients run at scale 1
# (n, L, C, conv_width, num_rffs): padded windows 2 (graph: conv_width 1), 64, 256, 1024, 2048, 4096, 8192.  Rows: sequence
# lengths conv_width (one k-mer), L, and values in between -- three rows at least, so the two-row shapes carry a third
SEQ = [(3, 12, 2, 1, 64), (4, 20, 16, 4, 300), (3, 23, 21, 9, 1000), (3, 30, 48, 21, 1030), (2, 26, 100, 11, 2100),
       (2, 44, 100, 40, 4100), (2, 54, 100, 50, 8200)]
GRAD_SEQ = [(4, 20, 16, 4, 300), (3, 30, 48, 21, 1030), (2, 44, 100, 40, 4100)]                     # 64, 1024, 4096
TRANSFORM = [(3, 2), (3, 64), (2, 1024), (2, 2048), (2, 8192), (1, 16384)]                          # (rows, P) of the FHT / SRHT
# One launch of every arm of the launchers' width dispatch (tests/test_gpu_dispatch_arms.py): each padded width 2^lg, lg = 1 .. 13, with
# rows of exactly 2^lg numbers and of one fewer (16-byte-aligned rows and rows fetched float by float); three rows; 4096 features up to
# 1024 (two tiles per row: the three-wave feature plan is reachable), one transform's worth beyond.  Sequences: conv_width 1, C = d,
# L = 3, lengths 1, 2, 3 -- the window pads to 2^lg and the rows carry one, two and three k-mers.
DISPATCH_LG = range(1, 14)
DISPATCH_FIXED = [(3, d, 4096 if lg <= 10 else 2 << lg) for lg in DISPATCH_LG for d in (1 << lg, max(1, (1 << lg) - 1))]
DISPATCH_SEQ = [(3, 3, d, 1, rffs) for _, d, rffs in DISPATCH_FIXED]
DISPATCH_SEQLEN = (1, 2, 3)
# MiniARD gradient operator, (n, d, F, nl, map kind).  The HIP kernel tiles 64 frequencies x 4 datapoints and stages d in slices of
# 64: d and F below, at and above one slice / tile (63, 64, 65), two slices and a bit (129 x 130), several blocks both ways (9 x 192),
# the smallest problem, and the widest d of the fixture test; one group, the most the kernel unrolls (8), groups in blocks, interleaved
# (k % nl), in blocks of uneven sizes with groups of one column on both sides of the slice edges 64 and 128, and a map that
# never takes one of its values.
ARD = [(1, 1, 1, 1, "block"), (5, 63, 63, 2, "block"), (4, 64, 64, 8, "interleaved"), (6, 65, 65, 3, "block"),
       (3, 129, 130, 8, "uneven"), (9, 200, 192, 5, "interleaved"), (3, 128, 70, 4, "absent"), (2, 2049, 48, 3, "block")]
ARD_UNEVEN_SPLITS = (1, 3, 64, 65, 100, 127, 128)        # d = 129, eight groups of 1, 2, 61, 1, 35, 27, 1, 1 columns
ARD_ABSENT = 2


def _signs(rng, size):
    return rng.choice(np.asarray([-1, 1], dtype=np.int8), size=size)


class FixedCase:
    def __init__(self, n, d, rffs, scale):
        rng = np.random.default_rng([n, d, rffs, int(scale)])
        self.n, self.d, self.rffs, self.scale, self.F = n, d, rffs, scale, rffs // 2
        self.P = dr.padded_width(d)
        self.x = (rng.standard_normal((n, d)) * (scale / np.sqrt(d))).astype(np.float32)
        self.radem = _signs(rng, (3, 1, ceil(self.F / self.P) * self.P))
        self.chi = np.sqrt(rng.chisquare(self.P, size=self.F)).astype(np.float32)

    @functools.cached_property
    def proj(self):
        return dr.projections(self.x, self.radem, self.chi)

    @functools.cached_property
    def pmax(self):
        return float(np.abs(self.proj).max())

    def typed(self, dtype):
        return self.x.astype(dtype), self.chi.astype(dtype)

    def __repr__(self):
        return f"fixed(n={self.n}, d={self.d}, rffs={self.rffs}, scale={self.scale:g})"


class SeqCase:
    def __init__(self, n, L, C, cw, rffs, seqlen=None):
        rng = np.random.default_rng([n, L, C, cw, rffs])
        self.n, self.L, self.C, self.cw, self.rffs, self.F = max(n, 3), L, C, cw, rffs, rffs // 2
        self.M = self.F + (self.F & 1)               # the max-pool operator wants an even number of outputs
        self.P = dr.padded_width(cw * C)
        self.x = (rng.standard_normal((self.n, L, C)) * (2.0 / np.sqrt(cw * C))).astype(np.float32)      # window norm ~ 2
        self.seqlen = np.asarray([cw, L, min(L, cw + 2), (cw + L) // 2][:self.n] if seqlen is None else seqlen, dtype=np.int32)
        self.radem = _signs(rng, (3, 1, ceil(self.M / self.P) * self.P))
        self.chi_all = np.sqrt(rng.chisquare(self.P, size=self.M)).astype(np.float32)
        self.chi = np.ascontiguousarray(self.chi_all[:self.F])

    @functools.cached_property
    def proj_all(self):
        return dr.conv_projections(self.x, self.seqlen, self.radem, self.chi_all, self.cw)

    @property
    def proj(self):
        return [p[:, :self.F] for p in self.proj_all]

    @functools.cached_property
    def pmax(self):
        return float(max(np.abs(p).max() for p in self.proj_all))

    def typed(self, dtype):
        return self.x.astype(dtype), self.chi.astype(dtype), self.chi_all.astype(dtype)

    def __repr__(self):
        return f"seq(n={self.n}, L={self.L}, C={self.C}, cw={self.cw}, rffs={self.rffs})"


class ArdCase:
    """x: float32 values of row norm about 1; sigma per group in [0.5, 2], none of them 1 (0.5 + 1.5 (r + 1/2) / nl, r a seeded
    permutation of the groups); W from the definition with seeded signs and chi, rounded to the type under test so that operator
    and reference receive the same weights (``typed``); one dense reference per type and intercept setting, computed once."""

    def __init__(self, n, d, F, nl, kind):
        rng = np.random.default_rng([n, d, F, nl])
        self.n, self.d, self.F, self.nl, self.kind, self.rffs = n, d, F, nl, kind, 2 * F
        self.P = dr.padded_width(d)
        self.x = (rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32)
        self.radem = _signs(rng, (3, 1, ceil(F / self.P) * self.P))
        self.chi = np.sqrt(rng.chisquare(self.P, size=F)).astype(np.float32)
        cols = np.arange(d)
        if kind == "block":
            smap = cols * nl // d
        elif kind == "interleaved":
            smap = cols % nl
        elif kind == "uneven":
            assert d == 129 and nl == len(ARD_UNEVEN_SPLITS) + 1
            smap = np.searchsorted(np.asarray(ARD_UNEVEN_SPLITS), cols, side="right")
        else:
            assert kind == "absent" and nl > ARD_ABSENT + 1
            present = np.asarray([g for g in range(nl) if g != ARD_ABSENT])
            smap = present[cols * (nl - 1) // d]
        self.sigma_map = smap.astype(np.int32)
        self.sigma = 0.5 + 1.5 * (rng.permutation(nl) + 0.5) / nl
        self.sigma_vals = self.sigma[self.sigma_map].astype(np.float64)
        self.weights = dr.mini_ard_weights(d, self.radem, self.chi)
        self._refs = {}

    def typed(self, dtype):
        return self.x.astype(dtype), np.ascontiguousarray(self.weights.astype(dtype))

    def ref(self, dtype, icpt, mistake=None):
        """-> (features, grad) of the dense reference for the weights as the type under test holds them."""
        key = (np.dtype(dtype), bool(icpt), mistake)
        if key not in self._refs:
            x, w = self.typed(dtype)
            self._refs[key] = dr.mini_ard_grad(x, w, self.sigma_map, self.sigma_vals, icpt, self.nl, mistake)
        return self._refs[key]

    def caps(self, dtype, icpt):
        x, w = self.typed(dtype)
        return dr.cap_mini_ard(dtype, x, w, self.sigma_map, self.sigma_vals, icpt, self.nl)

    def __repr__(self):
        return f"ard(n={self.n}, d={self.d}, F={self.F}, nl={self.nl}, {self.kind})"


@functools.lru_cache(maxsize=None)
def ard_case(n, d, F, nl, kind):
    return ArdCase(n, d, F, nl, kind)


@functools.lru_cache(maxsize=None)
def fixed_case(n, d, rffs, scale):
    return FixedCase(n, d, rffs, scale)


@functools.lru_cache(maxsize=None)
def seq_case(n, L, C, cw, rffs, seqlen=None):
    return SeqCase(n, L, C, cw, rffs, seqlen)


def maxerr(got, ref):
    return float(np.abs(np.asarray(got, dtype=dr.LD) - ref).max())


def report(what, case, dtype, err, cap, hip=None):
    """One line per case: HIP against dense (GPU leg only), oracle against dense, the a-priori cap."""
    hip_txt = "" if hip is None else f"hip-dense {hip:.3e}  "
    print(f"DENSE {what:<14} {case!r:<52} {np.dtype(dtype).name}  {hip_txt}oracle-dense {err:.3e}  cap {cap:.3e}")


@pytest.fixture(scope="module")
def orc(oracle):
    return oracle


# ---------------------------------------------------------------------------------------------------- self-checks
def test_hadamard_self_checks():
    for P in (1, 2, 8, 64, 256):
        h = dr.hadamard(P)
        assert np.array_equal(h @ h, P * np.eye(P, dtype=dr.LD))
        assert np.array_equal(h, h.T) and np.all(np.abs(h) == 1)
    assert np.array_equal(dr.hadamard(2), [[1, 1], [1, -1]])
    rng = np.random.default_rng(0)
    x = rng.standard_normal((3, 1024))
    dense, kron = dr.apply_hadamard_dense(x), dr.apply_hadamard_kron(x)
    # integers: both forms exact
    xi = rng.integers(-1000, 1000, size=(3, 1024)).astype(dr.LD)
    assert np.array_equal(dr.apply_hadamard_dense(xi), dr.apply_hadamard_kron(xi))
    assert np.abs(dense - kron).max() <= 1024 * dr.ULD * np.abs(x).sum(axis=1).max()
    x3 = rng.integers(-9, 9, size=(2, 3, 4096)).astype(dr.LD)          # 3-D input, Kronecker form: H (H x) = P x
    assert np.array_equal(dr.fht(dr.fht(x3)), 4096 * x3)
    try:
        from scipy.linalg import hadamard as scipy_hadamard
    except ImportError:
        return
    for P in (2, 16, 512):
        assert np.array_equal(dr.hadamard(P), scipy_hadamard(P))


# ---------------------------------------------------------------------------------------------------- oracle vs dense
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("rows,P", TRANSFORM)
def test_oracle_fht_and_srht(orc, rows, P, dtype):
    rng = np.random.default_rng(P + rows)
    x = rng.standard_normal((rows, P)).astype(np.float32).astype(dtype)
    radem = _signs(rng, P)
    got = x.copy()
    orc.cpuFastHadamardTransform2D(got)
    err, cap = maxerr(got, dr.fht(x)), dr.cap_fht(dtype, x)
    report("fht2d", (rows, P), dtype, err, cap)
    assert err <= cap
    x3 = x.reshape(rows, 2, P // 2).copy() if P > 2 else x.reshape(rows, 1, P).copy()
    got3 = x3.copy()
    orc.cpuFastHadamardTransform(got3)
    err, cap = maxerr(got3, dr.fht(x3)), dr.cap_fht(dtype, x3)
    report("fht3d", x3.shape, dtype, err, cap)
    assert err <= cap
    got = x.copy()
    orc.cpuSRHT(got, radem)
    err, cap = maxerr(got, dr.srht(x, radem)), dr.cap_srht(dtype, x)
    report("srht", (rows, P), dtype, err, cap)
    assert err <= cap


def oracle_rbf(orc, case, dtype, icpt):
    x, chi = case.typed(dtype)
    out = np.zeros((case.n, case.rffs))
    orc.cpuRBFFeatureGen(x, out, case.radem, chi, icpt)
    return out


def oracle_rbf_grad(orc, case, dtype, icpt):
    x, chi = case.typed(dtype)
    out, grad = np.zeros((case.n, case.rffs)), np.zeros((case.n, case.rffs, 1))
    orc.cpuRBFGrad(x, out, grad, case.radem, chi, SIGMA, icpt)
    return out, grad[:, :, 0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("n,d,rffs", FIXED)
def test_oracle_rbf_features(orc, n, d, rffs, scale, icpt, dtype):
    case = fixed_case(n, d, rffs, scale)
    ref = dr.rbf_features(case.x, case.radem, case.chi, icpt, proj=case.proj)
    err, cap = maxerr(oracle_rbf(orc, case, dtype, icpt), ref), dr.cap_rbf(dtype, case.x, case.chi, icpt)
    report(f"rbf icpt={int(icpt)}", case, dtype, err, cap)
    assert err <= cap


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("n,d,rffs", GRAD_FIXED)
def test_oracle_rbf_grad(orc, n, d, rffs, icpt, dtype):
    case = fixed_case(n, d, rffs, GRAD_SCALE)
    rf, rg = dr.rbf_grad(case.x, case.radem, case.chi, SIGMA, icpt, proj=case.proj)
    of, og = oracle_rbf_grad(orc, case, dtype, icpt)
    capf, capg = dr.cap_rbf_grad(dtype, case.x, case.chi, SIGMA, icpt, case.pmax)
    report(f"rbfgrad.f i={int(icpt)}", case, dtype, maxerr(of, rf), capf)
    report(f"rbfgrad.g i={int(icpt)}", case, dtype, maxerr(og, rg), capg)
    assert maxerr(of, rf) <= capf and maxerr(og, rg) <= capg


def oracle_conv(orc, case, dtype, scaling):
    x, chi, _ = case.typed(dtype)
    out = np.zeros((case.n, case.rffs))
    orc.cpuConv1dFGen(x, out, case.radem, chi, case.seqlen, case.cw, scaling)
    return out


def oracle_conv_grad(orc, case, dtype, scaling):
    x, chi, _ = case.typed(dtype)
    out, grad = np.zeros((case.n, case.rffs)), np.zeros((case.n, case.rffs, 1))
    orc.cpuConvGrad(x, out, case.radem, chi, case.seqlen, grad, SIGMA, case.cw, scaling)
    return out, grad[:, :, 0]


def oracle_maxpool(orc, case, dtype):
    x, _, chi_all = case.typed(dtype)
    out = np.zeros((case.n, case.M), dtype=np.float32)
    orc.cpuConv1dMaxpool(x, out, case.radem, chi_all, case.seqlen, case.cw)
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,L,C,cw,rffs", SEQ)
def test_oracle_conv_features_and_maxpool(orc, n, L, C, cw, rffs, dtype):
    case = seq_case(n, L, C, cw, rffs)
    for scaling in (0, 1, 2):
        ref = dr.conv_features(case.x, case.seqlen, case.radem, case.chi, cw, scaling, proj=case.proj)
        err, cap = maxerr(oracle_conv(orc, case, dtype, scaling), ref), dr.cap_conv(dtype, case.x, case.seqlen, case.chi, cw, scaling)
        report(f"conv sc={scaling}", case, dtype, err, cap)
        assert err <= cap
    _, ref = dr.conv_maxpool(case.x, case.seqlen, case.radem, case.chi_all, cw, proj=case.proj_all)
    err, cap = maxerr(oracle_maxpool(orc, case, dtype), ref), dr.cap_conv_maxpool(dtype, case.x, case.seqlen, case.chi_all, cw, case.pmax)
    report("maxpool", case, dtype, err, cap)
    assert err <= cap


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,L,C,cw,rffs", GRAD_SEQ)
def test_oracle_conv_grad(orc, n, L, C, cw, rffs, dtype):
    case = seq_case(n, L, C, cw, rffs)
    for scaling in (0, 1, 2):
        rf, rg = dr.conv_grad(case.x, case.seqlen, case.radem, case.chi, SIGMA, cw, scaling, proj=case.proj)
        of, og = oracle_conv_grad(orc, case, dtype, scaling)
        capf, capg = dr.cap_conv_grad(dtype, case.x, case.seqlen, case.chi, SIGMA, cw, scaling, case.pmax)
        report(f"convgrad.f sc={scaling}", case, dtype, maxerr(of, rf), capf)
        report(f"convgrad.g sc={scaling}", case, dtype, maxerr(og, rg), capg)
        assert maxerr(of, rf) <= capf and maxerr(og, rg) <= capg


def oracle_mini_ard(orc, case, dtype, icpt):
    x, w = case.typed(dtype)
    out, grad = np.zeros((case.n, case.rffs)), np.zeros((case.n, case.rffs, case.nl))
    orc.cpuMiniARDGrad(x, out, w, case.sigma_map, case.sigma_vals, grad, icpt)
    return out, grad


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("n,d,F,nl,kind", ARD)
def test_oracle_mini_ard_grad(orc, n, d, F, nl, kind, icpt, dtype):
    case = ard_case(n, d, F, nl, kind)
    rf, rg = case.ref(dtype, icpt)
    of, og = oracle_mini_ard(orc, case, dtype, icpt)
    capf, capg = case.caps(dtype, icpt)
    report(f"mini_ard.f i={int(icpt)}", case, dtype, maxerr(of, rf), capf)
    report(f"mini_ard.g i={int(icpt)}", case, dtype, maxerr(og, rg), capg)
    assert maxerr(of, rf) <= capf and maxerr(og, rg) <= capg


@pytest.mark.parametrize("n,d,F,nl,kind", [c for c in ARD if c[1] <= 200])
def test_mini_ard_weights_row_form_equals_the_definition(n, d, F, nl, kind):
    """mini_ard_weights builds W row by row (S^T e_j); the definition, projections of the unit rows e_k, column by column.  Both
    are three rounds of dense longdouble products of length P and one product with chi on unit vectors: each within
    3 (P + 2) u_ld chi_max of the exact numbers."""
    case = ard_case(n, d, F, nl, kind)
    by_def = dr.mini_ard_weights(d, case.radem, case.chi, by_definition=True)
    assert case.weights.shape == by_def.shape == (F, d)
    assert maxerr(case.weights, by_def) <= 2 * 3 * (case.P + 2) * dr.ULD * float(case.chi.max())


# (d, num_rffs, split points): F = 33 is no multiple of P = 32; two full blocks of P = 64; d = P = 64 with eight groups
ARD_KERNELS = [(20, 66, [7]), (50, 256, [10, 30]), (64, 128, [1, 2, 3, 4, 5, 6, 7])]


def ard_weight_cap(dtype, d, chi, ref):
    """The kernel objects build W by three float64 FHT rounds on the identity (rows of norm 1) and one product with chi, then store
    it in their own type: the float64 projection cap, plus one rounding to float32 where that is the type."""
    cap = dr._projection_cap(dr.U64, dr.padded_width(d), 1.0, float(np.abs(chi).max()))
    return cap if np.dtype(dtype) == np.float64 else cap + dr.U32 * (float(np.abs(ref).max()) + cap)


@pytest.mark.parametrize("dp", [False, True])
@pytest.mark.parametrize("d,rffs,splits", ARD_KERNELS)
def test_oracle_mini_ard_precomputed_weights(orc, d, rffs, splits, dp):
    from oracle import oracle as omod
    kern = omod.OracleMiniARDKernel(rffs, (10, d), splits, None, 123, double_precision=dp, ops=orc)
    kern.precompute_weights()
    dtype = np.float64 if dp else np.float32
    assert kern.precomputed_weights.dtype == dtype and kern.precomputed_weights.shape == (rffs // 2, d)
    ref = dr.mini_ard_weights(d, kern.radem_diag, kern.chi_arr)
    err, cap = maxerr(kern.precomputed_weights, ref), ard_weight_cap(dtype, d, kern.chi_arr, ref)
    report("mini_ard.W", (d, rffs), dtype, err, cap)
    assert err <= cap


# The NMLL gradient of a MiniARD kernel (shared with tests/test_gpu_mini_ard.py): n = 300, d = 12, three groups, 128 RFFs
NMLL_ARD = dict(n=300, d=12, splits=[4, 9], rffs=128, chunk=128, hparams=np.array([0.45, 0.8, 1.3, 0.6]), eps=1e-3)


def nmll_ard_problem():
    p = NMLL_ARD
    rng = np.random.default_rng(300)
    x = rng.uniform(-1, 1, size=(p["n"], p["d"])).astype(np.float32).astype(np.float64)
    y = np.sin(2 * x[:, 0]) + x[:, 5] * x[:, 6] + 0.5 * x[:, 10] + 0.1 * rng.standard_normal(p["n"])
    return x, y


def central_difference(fun, hparams, eps):
    """d fun / d log(hparams[i]) by central differences of width eps in log space."""
    out = np.zeros(hparams.shape[0])
    for i in range(hparams.shape[0]):
        up, down = np.log(hparams), np.log(hparams)
        up[i] += eps
        down[i] -= eps
        out[i] = (fun(np.exp(up)) - fun(np.exp(down))) / (2 * eps)
    return out


def test_oracle_mini_ard_nmll_gradient_against_central_difference(orc):
    """The oracle's exact_nmll_gradient of a multi-lengthscale kernel against a central difference of its exact_nmll in every
    hyperparameter (lambda included), float64 kernel.  The printed deviation is the difference quotient's own error (its
    truncation error, eps^2 / 6 times the third derivative): tests/test_gpu_mini_ard.py takes its tolerance from it.  Asserted
    here: the deviation stays within twice the change of the quotient itself from eps to eps / 2 (which is 3/4 of the truncation
    error at eps), plus the rounding of the quotient, 1e-12 |nmll| / eps."""
    from oracle import oracle as omod
    p = NMLL_ARD
    x, y = nmll_ard_problem()
    ds = omod.OracleDataset(x, y, None, chunk_size=p["chunk"])

    def kernel(hp):
        return omod.OracleMiniARDKernel(p["rffs"], x.shape, p["splits"], hp, 123, double_precision=True, ops=orc)

    def value(hp):
        return omod.exact_nmll(kernel(hp), ds)

    nll, grad = omod.exact_nmll_gradient(kernel(p["hparams"]), ds)
    assert np.isclose(nll, value(p["hparams"]), rtol=1e-12)
    fd, fd_half = central_difference(value, p["hparams"], p["eps"]), central_difference(value, p["hparams"], p["eps"] / 2)
    dev = np.abs(grad - fd)
    print(f"NMLLFD mini_ard oracle: gradient {grad}  central difference {fd}")
    print(f"NMLLFD mini_ard oracle: largest absolute deviation {dev.max():.3e}  largest relative deviation {(dev / np.abs(fd)).max():.3e}")
    assert np.all(dev <= 2 * np.abs(fd - fd_half) + 1e-12 * abs(nll) / p["eps"]), (dev, np.abs(fd - fd_half))


# ---------------------------------------------------------------------------------------------------- the dispatch shapes
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("n,d,rffs", DISPATCH_FIXED)
def test_oracle_dispatch_shapes_fixed(orc, n, d, rffs, icpt, dtype):
    case = fixed_case(n, d, rffs, GRAD_SCALE)
    ref = dr.rbf_features(case.x, case.radem, case.chi, icpt, proj=case.proj)
    err, cap = maxerr(oracle_rbf(orc, case, dtype, icpt), ref), dr.cap_rbf(dtype, case.x, case.chi, icpt)
    report(f"rbf icpt={int(icpt)}", case, dtype, err, cap)
    assert err <= cap
    rf, rg = dr.rbf_grad(case.x, case.radem, case.chi, SIGMA, icpt, proj=case.proj)
    of, og = oracle_rbf_grad(orc, case, dtype, icpt)
    capf, capg = dr.cap_rbf_grad(dtype, case.x, case.chi, SIGMA, icpt, case.pmax)
    report(f"rbfgrad.f i={int(icpt)}", case, dtype, maxerr(of, rf), capf)
    report(f"rbfgrad.g i={int(icpt)}", case, dtype, maxerr(og, rg), capg)
    assert maxerr(of, rf) <= capf and maxerr(og, rg) <= capg


DISPATCH_SCALING = 1            # rows divided by sqrt(nkmers): the three k-mer counts give three row constants


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,L,C,cw,rffs", DISPATCH_SEQ)
def test_oracle_dispatch_shapes_sequences(orc, n, L, C, cw, rffs, dtype):
    case = seq_case(n, L, C, cw, rffs, DISPATCH_SEQLEN)
    sc = DISPATCH_SCALING
    ref = dr.conv_features(case.x, case.seqlen, case.radem, case.chi, cw, sc, proj=case.proj)
    err, cap = maxerr(oracle_conv(orc, case, dtype, sc), ref), dr.cap_conv(dtype, case.x, case.seqlen, case.chi, cw, sc)
    report(f"conv sc={sc}", case, dtype, err, cap)
    assert err <= cap
    rf, rg = dr.conv_grad(case.x, case.seqlen, case.radem, case.chi, SIGMA, cw, sc, proj=case.proj)
    of, og = oracle_conv_grad(orc, case, dtype, sc)
    capf, capg = dr.cap_conv_grad(dtype, case.x, case.seqlen, case.chi, SIGMA, cw, sc, case.pmax)
    report(f"convgrad.f sc={sc}", case, dtype, maxerr(of, rf), capf)
    report(f"convgrad.g sc={sc}", case, dtype, maxerr(og, rg), capg)
    assert maxerr(of, rf) <= capf and maxerr(og, rg) <= capg
    _, ref = dr.conv_maxpool(case.x, case.seqlen, case.radem, case.chi_all, cw, proj=case.proj_all)
    err, cap = maxerr(oracle_maxpool(orc, case, dtype), ref), dr.cap_conv_maxpool(dtype, case.x, case.seqlen, case.chi_all, cw, case.pmax)
    report("maxpool", case, dtype, err, cap)
    assert err <= cap


# ---------------------------------------------------------------------------------------------------- sensitivity
# Which planted mistake applies to which operator (and where):
#   swap02       sign rows 0 and 2 swapped               every SORF operator: rbf, rbf-grad, conv, conv-grad, max-pool; not the shape
#                                                        (3, 1, 2), where the swap is the identity (see test_sensitivity_fixed)
#   offset       rep * P -> rep * F_tile - 1             the same operators, shapes with more than one repetition (F > P)
#   kmer_more    one k-mer too many                      conv, conv-grad, max-pool
#   kmer_fewer   one k-mer too few                       conv, conv-grad, max-pool
#   F_for_Fhalf  sqrt(1/F) where sqrt(1/(F-1/2)) is due  rbf, rbf-grad with the intercept.  The relative change is 1/(4F); the
#                float32 cap is at least 3 (k + 2) u32 |chi| ||x|| relative, so in float32 it is resolvable 100-fold only at the two
#                smallest shapes (F <= 64) at scale 1; asserted against the float64 cap everywhere, against the float32 cap there
#   deinterleave cos block | sin block                   rbf, rbf-grad, conv, conv-grad; needs more than one frequency (F > 1)
#   pad_last     pad = last element, not zero            every SORF operator, shapes whose width is below the padded width
#   scaling1for2 divide by sqrt(nkmers), not nkmers      conv, conv-grad at scaling 2 (a row with more than one k-mer: every shape)
# The bare FHT and the SRHT have none of these degrees of freedom (no offsets, no padding, no pairs, no k-mers).
FACTOR = 100.0
F32_RESOLVES_F = 64


def _assert_moved(what, case, mistake, ref, bad, caps):
    diff = maxerr(bad, ref)
    for dtype, cap in caps.items():
        print(f"SENS {what:<10} {mistake:<12} {case!r:<52} {np.dtype(dtype).name}  moved {diff:.3e}  {FACTOR:g} x cap {FACTOR * cap:.3e}")
        assert diff >= FACTOR * cap, (what, mistake, case, dtype, diff, cap)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("n,d,rffs", FIXED)
def test_sensitivity_fixed(n, d, rffs, scale):
    case = fixed_case(n, d, rffs, scale)
    grad_too = (n, d, rffs) in GRAD_FIXED and scale == GRAD_SCALE
    both = (np.float32, np.float64)
    for icpt in (False, True):
        ref = dr.rbf_features(case.x, case.radem, case.chi, icpt, proj=case.proj)
        caps = {dt: dr.cap_rbf(dt, case.x, case.chi, icpt) for dt in both}
        if grad_too:
            gref = dr.rbf_grad(case.x, case.radem, case.chi, SIGMA, icpt, proj=case.proj)
            gcaps = {dt: dr.cap_rbf_grad(dt, case.x, case.chi, SIGMA, icpt, case.pmax) for dt in both}
        variants = {}
        if d > 1 or case.F > 1:        # one input, one output: only entry [0, 0] of the SORF matrix is seen, and H D3 H D2 H D1 transposes
            variants["swap02"] = dict(radem=np.ascontiguousarray(case.radem[::-1]))      # into H D1 H D2 H D3 with the same [0, 0]
        if case.F > case.P:
            variants["offset"] = dict(mistake="offset")
        if d < case.P:
            variants["pad_last"] = dict(mistake="pad_last")
        for name, kw in variants.items():
            radem = kw.get("radem", case.radem)
            bad_proj = dr.projections(case.x, radem, case.chi, kw.get("mistake"))
            _assert_moved("rbf", case, name, ref, dr.rbf_features(case.x, radem, case.chi, icpt, proj=bad_proj), caps)
            if grad_too:
                bf, bg = dr.rbf_grad(case.x, radem, case.chi, SIGMA, icpt, proj=bad_proj)
                _assert_moved("rbfgrad.f", case, name, gref[0], bf, {dt: c[0] for dt, c in gcaps.items()})
                _assert_moved("rbfgrad.g", case, name, gref[1], bg, {dt: c[1] for dt, c in gcaps.items()})
        if case.F > 1:
            _assert_moved("rbf", case, "deinterleave", ref, dr.deinterleaved(ref), caps)
            if grad_too:
                _assert_moved("rbfgrad.g", case, "deinterleave", gref[1], dr.deinterleaved(gref[1]), {dt: c[1] for dt, c in gcaps.items()})
        if icpt:
            which = both if case.F <= F32_RESOLVES_F and scale == 1.0 else (np.float64,)
            bad = dr.rbf_features(case.x, case.radem, case.chi, False, proj=case.proj)
            _assert_moved("rbf", case, "F_for_Fhalf", ref, bad, {dt: caps[dt] for dt in which})
            if grad_too:
                bf, bg = dr.rbf_grad(case.x, case.radem, case.chi, SIGMA, False, proj=case.proj)
                _assert_moved("rbfgrad.g", case, "F_for_Fhalf", gref[1], bg, {dt: gcaps[dt][1] for dt in which})


@pytest.mark.parametrize("n,L,C,cw,rffs", SEQ)
def test_sensitivity_sequences(n, L, C, cw, rffs):
    case = seq_case(n, L, C, cw, rffs)
    grad_too = (n, L, C, cw, rffs) in GRAD_SEQ
    both = (np.float32, np.float64)
    variants = {"swap02": dict(radem=np.ascontiguousarray(case.radem[::-1])), "kmer_more": dict(mistake="kmer_more"),
                "kmer_fewer": dict(mistake="kmer_fewer")}
    if case.F > case.P:
        variants["offset"] = dict(mistake="offset")
    if cw * C < case.P:
        variants["pad_last"] = dict(mistake="pad_last")
    bad_projs = {name: dr.conv_projections(case.x, case.seqlen, kw.get("radem", case.radem), case.chi_all, cw, kw.get("mistake"))
                 for name, kw in variants.items()}
    mp_ref = dr.conv_maxpool(case.x, case.seqlen, case.radem, case.chi_all, cw, proj=case.proj_all)[1]
    mp_caps = {dt: dr.cap_conv_maxpool(dt, case.x, case.seqlen, case.chi_all, cw, case.pmax) for dt in both}
    for name, bp in bad_projs.items():
        if name == "offset" and case.M <= case.P:
            continue
        _assert_moved("maxpool", case, name, mp_ref, dr.conv_maxpool(case.x, case.seqlen, case.radem, case.chi_all, cw, proj=bp)[1], mp_caps)
    for scaling in (0, 1, 2):
        ref = dr.conv_features(case.x, case.seqlen, case.radem, case.chi, cw, scaling, proj=case.proj)
        caps = {dt: dr.cap_conv(dt, case.x, case.seqlen, case.chi, cw, scaling) for dt in both}
        if grad_too:
            gref = dr.conv_grad(case.x, case.seqlen, case.radem, case.chi, SIGMA, cw, scaling, proj=case.proj)
            gcaps = {dt: dr.cap_conv_grad(dt, case.x, case.seqlen, case.chi, SIGMA, cw, scaling, case.pmax) for dt in both}
        for name, bp in bad_projs.items():
            bp = [p[:, :case.F] for p in bp]
            _assert_moved(f"conv sc={scaling}", case, name, ref, dr.conv_features(case.x, case.seqlen, case.radem, case.chi, cw, scaling, proj=bp), caps)
            if grad_too:
                bg = dr.conv_grad(case.x, case.seqlen, case.radem, case.chi, SIGMA, cw, scaling, proj=bp)[1]
                _assert_moved(f"convgrad sc={scaling}", case, name, gref[1], bg, {dt: c[1] for dt, c in gcaps.items()})
        _assert_moved(f"conv sc={scaling}", case, "deinterleave", ref, dr.deinterleaved(ref), caps)
        if scaling == 2:
            bad = dr.conv_features(case.x, case.seqlen, case.radem, case.chi, cw, 1, proj=case.proj)
            _assert_moved("conv sc=2", case, "scaling1for2", ref, bad, caps)
            if grad_too:
                bg = dr.conv_grad(case.x, case.seqlen, case.radem, case.chi, SIGMA, cw, 1, proj=case.proj)[1]
                _assert_moved("convgrad sc=2", case, "scaling1for2", gref[1], bg, {dt: c[1] for dt, c in gcaps.items()})


# MiniARD gradient operator (features f, gradient g).  Which planted mistake applies where, and on which output it is asserted:
#   group_edge    every column takes its left neighbour's group   g; more than one group (nl > 1)
#   drop_last     column d - 1 left out of the sums                f and g; every shape (at d = 1 nothing is left: a = 0, G = 0)
#   sigma_in_grad G_l weighted by sigma                            g; every shape (no sigma is 1)
#   swap_partner  the gradient's cos and sin partners exchanged    g; every shape
#   layout        grad laid out [n, nl, 2F], then reshaped         g; nl > 1
#   no_half       sqrt(1/F) with the intercept                     f; with the intercept.  (The gradient changes by the same
#                 relative 1/(4F), but G is a signed sum while its cap grows with the sum of magnitudes B: not asserted there.)
ARD_MISTAKES = {"group_edge": "g", "drop_last": "fg", "sigma_in_grad": "g", "swap_partner": "g", "layout": "g", "no_half": "f"}


def ard_mistake_applies(mistake, case, icpt):
    if mistake in ("group_edge", "layout"):
        return case.nl > 1
    return icpt if mistake == "no_half" else True


@pytest.mark.parametrize("n,d,F,nl,kind", ARD)
def test_sensitivity_mini_ard(n, d, F, nl, kind):
    case = ard_case(n, d, F, nl, kind)
    for icpt in (False, True):
        for mistake, where in ARD_MISTAKES.items():
            if not ard_mistake_applies(mistake, case, icpt):
                continue
            for dtype in (np.float32, np.float64):         # each type has its own weights, hence its own reference
                (rf, rg), (bf, bg), (capf, capg) = case.ref(dtype, icpt), case.ref(dtype, icpt, mistake), case.caps(dtype, icpt)
                if "f" in where:
                    _assert_moved(f"ard.f i={int(icpt)}", case, mistake, rf, bf, {dtype: capf})
                if "g" in where:
                    _assert_moved(f"ard.g i={int(icpt)}", case, mistake, rg, bg, {dtype: capg})


# ---------------------------------------------------------------------------------------------------- g19: the reference's slow path
# tests/golden/g19_slow_path.npz: outputs of the reference project's own verbose "ground truth" helpers (make_golden.py
# g19_slow_path), in its float and double modes.  Tolerances: the reference's own (its test_conv1d_fht.py check_results: float
# rtol 1e-5 / atol 1e-5, double np.allclose defaults; test_maxpool_rfgen.py check_results: float rtol 1e-6 / atol 1e-6).
def g19_settings():
    g = load_golden("g19_slow_path.npz")
    for si in range(int(g["n_settings"])):
        for tag, dtype in (("32", np.float32), ("64", np.float64)):
            kind = str(g[f"kind_{si}"])
            if f"slow{tag}_{si}" not in g:         # max-pool (9, 23, 21, 130): the reference tests it in double only
                continue
            if kind == "maxpool":
                tol = dict(rtol=1e-6, atol=1e-6) if tag == "32" else {}
            else:
                tol = dict(rtol=1e-5, atol=1e-5) if tag == "32" else {}
            yield dict(si=si, kind=kind, dtype=dtype, tol=tol, x=g[f"x{tag}_{si}"], chi=g[f"chi{tag}_{si}"], slow=g[f"slow{tag}_{si}"],
                       slowgrad=g[f"slowgrad{tag}_{si}"] if f"slowgrad{tag}_{si}" in g else None, radem=g[f"radem_{si}"],
                       seqlen=g[f"seqlen_{si}"], cw=int(g[f"conv_width_{si}"]), sigma=float(g[f"sigma_{si}"]),
                       scaling=int(g[f"scaling_{si}"]))


def test_g19_oracle_and_dense_reference_against_the_slow_path(orc):
    for s in g19_settings():
        x, chi, n, F = s["x"], s["chi"], s["x"].shape[0], s["chi"].shape[0]
        u_acc = dr.unit_roundoff(s["dtype"])          # the slow path sums its k-mers in the mode's own type
        name = f"g19[{s['si']}] {s['kind']}"
        if s["kind"] == "maxpool":
            out = np.zeros((n, F), dtype=np.float32)
            orc.cpuConv1dMaxpool(x, out, s["radem"], chi, s["seqlen"], s["cw"])
            assert np.allclose(s["slow"], out, **s["tol"]), name
            proj = dr.conv_projections(x, s["seqlen"], s["radem"], chi, s["cw"])
            pmax = float(max(np.abs(p).max() for p in proj))
            ref = dr.conv_maxpool(x, s["seqlen"], s["radem"], chi, s["cw"], proj=proj)[1]
            err, cap = maxerr(s["slow"], ref), dr.cap_conv_maxpool(s["dtype"], x, s["seqlen"], chi, s["cw"], pmax)
        else:
            out, grad = np.zeros((n, 2 * F)), np.zeros((n, 2 * F, 1))
            if s["kind"] == "conv":
                orc.cpuConv1dFGen(x * s["dtype"](s["sigma"]), out, s["radem"], chi, s["seqlen"], s["cw"], s["scaling"])
            else:
                orc.cpuConvGrad(x, out, s["radem"], chi, s["seqlen"], grad, s["sigma"], s["cw"], 0)
                assert np.allclose(s["slowgrad"], grad[:, :, 0], **s["tol"]), name
            assert np.allclose(s["slow"], out, **s["tol"]), name
            proj = dr.conv_projections(x, s["seqlen"], s["radem"], chi, s["cw"])
            pmax = float(max(np.abs(p).max() for p in proj))
            rf, rg = dr.conv_grad(x, s["seqlen"], s["radem"], chi, s["sigma"], s["cw"], s["scaling"], proj=proj)
            capf, capg = dr.cap_conv_grad(s["dtype"], x, s["seqlen"], chi, s["sigma"], s["cw"], s["scaling"], pmax, u_acc=u_acc)
            err, cap = maxerr(s["slow"], rf), capf
            if s["kind"] == "grad":
                report(name + ".g slow", x.shape, s["dtype"], maxerr(s["slowgrad"], rg), capg)
                assert maxerr(s["slowgrad"], rg) <= capg
        report(name + " slow", x.shape, s["dtype"], err, cap)
        assert err <= cap, name
