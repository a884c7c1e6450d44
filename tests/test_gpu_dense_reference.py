"""Every feature operator of xgpr_hip_rfgen_ext against the dense-matrix reference (tests/dense_reference.py): the third,
independent leg next to the CPU oracle and the golden fixtures.  Each case prints HIP against dense, oracle against dense and
the a-priori cap, and asserts

  1. |HIP - dense| <= |oracle - dense| + the parity tolerance the suite already uses for HIP against the oracle on that
     operator (tests/test_gpu_ops.py: 4e-7 c nkmers float32 features, 1e-13 c float64 features, 0 for FHT / SRHT / max-pool,
     1e-6 max|w| for the matvec against an oracle-Z product, 1e-6 / 1e-13 / 1e-12 of the largest entry for the gradients);
  2. |oracle - dense| <= cap.

Shapes, inputs and the oracle calls are those of tests/test_dense_reference_cpu.py (the smallest that cross each dispatch
boundary); the dense projections are computed once per case and shared."""
import numpy as np
import pytest
import torch

import dense_reference as dr
from test_dense_reference_cpu import (g19_settings, FIXED, GRAD_FIXED, GRAD_SCALE, GRAD_SEQ, SCALES, SEQ, SIGMA, TRANSFORM, _signs, fixed_case,
                                      maxerr, oracle_conv, oracle_conv_grad, oracle_maxpool, oracle_rbf, oracle_rbf_grad, report,
                                      seq_case)

pytestmark = pytest.mark.gpu

DEV = "cuda"
BOTH = [np.float32, np.float64]


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def check(what, case, dtype, hip, orc_out, ref, cap, tol):
    e_hip, e_orc = maxerr(hip, ref), maxerr(orc_out, ref)
    report(what, case, dtype, e_orc, cap, hip=e_hip)
    assert e_orc <= cap, f"{what} {case!r}: oracle {e_orc:.3e} above the cap {cap:.3e}"
    assert e_hip <= e_orc + tol, f"{what} {case!r}: HIP {e_hip:.3e} vs oracle {e_orc:.3e} + {tol:.3e}"


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("rows,P", TRANSFORM)
def test_fht_and_srht(ext, oracle, rows, P, dtype):
    rng = np.random.default_rng(P + rows)
    x = rng.standard_normal((rows, P)).astype(np.float32).astype(dtype)
    radem = _signs(rng, P)
    o, h = x.copy(), dev(x)
    oracle.cpuFastHadamardTransform2D(o)
    ext.hipFastHadamardTransform2D(h)
    check("fht2d", (rows, P), dtype, host(h), o, dr.fht(x), dr.cap_fht(dtype, x), 0.0)
    x3 = x.reshape(rows, 2, P // 2).copy() if P > 2 else x.reshape(rows, 1, P).copy()
    o, h = x3.copy(), dev(x3)
    oracle.cpuFastHadamardTransform(o)
    ext.hipFastHadamardTransform(h)
    check("fht3d", x3.shape, dtype, host(h), o, dr.fht(x3), dr.cap_fht(dtype, x3), 0.0)
    o, h = x.copy(), dev(x)
    oracle.cpuSRHT(o, radem)
    ext.hipSRHT(h, dev(radem))
    check("srht", (rows, P), dtype, host(h), o, dr.srht(x, radem), dr.cap_srht(dtype, x), 0.0)


@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("n,d,rffs", FIXED)
def test_rbf_features_cache_and_products(ext, oracle, n, d, rffs, scale, icpt):
    case = fixed_case(n, d, rffs, scale)
    ref = dr.rbf_features(case.x, case.radem, case.chi, icpt, proj=case.proj)
    c = float(dr.rbf_scale(case.F, icpt))
    radem = dev(case.radem)
    orc = {}
    for dtype, tol in ((np.float32, 4e-7 * c), (np.float64, 1e-13 * c)):
        x, chi = case.typed(dtype)
        orc[dtype] = oracle_rbf(oracle, case, dtype, icpt)
        out = torch.full((n, rffs), 7.0, dtype=torch.float64, device=DEV)
        ext.hipRBFFeatureGen(dev(x), out, radem, dev(chi), icpt)
        check(f"rbf icpt={int(icpt)}", case, dtype, host(out), orc[dtype], ref, dr.cap_rbf(dtype, case.x, case.chi, icpt), tol)
    # the float32 rows before scaling: rows * float32(c)
    rows = torch.full((n, rffs), float("nan"), dtype=torch.float32, device=DEV)
    ext.hipRBFFeatureCache(dev(case.x), rows, radem, dev(case.chi))
    cap32 = dr.cap_rbf(np.float32, case.x, case.chi, icpt)
    check(f"cache icpt={int(icpt)}", case, np.float32, host(rows).astype(np.float64) * float(np.float32(c)), orc[np.float32], ref, cap32,
          4e-7 * c)
    if d > 4096:
        return                               # the fused products serve padded widths up to 4096
    assert ext.ztz_matvec_plan(d, case.F) != 0
    rng = np.random.default_rng(rffs)
    v, y = rng.standard_normal(rffs), rng.standard_normal(n)
    z = dr.design_matrix(case.x, case.radem, case.chi, icpt, proj=case.proj)
    zo = orc[np.float32].copy()
    if icpt:
        zo[:, 0] = 1.0
    zmax = max(c, 1.0) if icpt else c
    wref, wo = z.T @ (z @ v.astype(dr.LD)), zo.T @ (zo @ v)
    w = torch.full((rffs,), 7.0, dtype=torch.float64, device=DEV)
    ext.hipZtZMatvec(dev(case.x), radem, dev(case.chi), dev(v), w, icpt)
    check(f"ztz icpt={int(icpt)}", case, np.float32, host(w), wo, wref, dr.cap_matvec(cap32, zmax, n, rffs, v), 1e-6 * float(np.abs(wo).max()))
    yref, yo = z.T @ y.astype(dr.LD), zo.T @ y
    zty = torch.full((rffs,), 7.0, dtype=torch.float64, device=DEV)
    ext.hipZtY(dev(case.x), radem, dev(case.chi), dev(y), zty, icpt)
    check(f"zty icpt={int(icpt)}", case, np.float32, host(zty), yo, yref, dr.cap_zty(cap32, zmax, n, y), 1e-6 * float(np.abs(yo).max()))


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("n,d,rffs", GRAD_FIXED)
def test_rbf_grad(ext, oracle, n, d, rffs, icpt, dtype):
    case = fixed_case(n, d, rffs, GRAD_SCALE)
    rf, rg = dr.rbf_grad(case.x, case.radem, case.chi, SIGMA, icpt, proj=case.proj)
    of, og = oracle_rbf_grad(oracle, case, dtype, icpt)
    capf, capg = dr.cap_rbf_grad(dtype, case.x, case.chi, SIGMA, icpt, case.pmax)
    x, chi = case.typed(dtype)
    o = torch.full((n, rffs), 7.0, dtype=torch.float64, device=DEV)
    g = torch.full((n, rffs, 1), 7.0, dtype=torch.float64, device=DEV)
    ext.hipRBFGrad(dev(x), o, g, dev(case.radem), dev(chi), SIGMA, icpt)
    c = float(dr.rbf_scale(case.F, icpt))
    gmax = float(np.abs(og).max())
    tolf, tolg = (4e-7 * c, 1e-6 * gmax) if dtype == np.float32 else (1e-13 * c, 1e-13 * max(gmax, c))
    check(f"rbfgrad.f i={int(icpt)}", case, dtype, host(o), of, rf, capf, tolf)
    check(f"rbfgrad.g i={int(icpt)}", case, dtype, host(g)[:, :, 0], og, rg, capg, tolg)


def _conv_tol_scale(case, scaling):
    kmax = int(case.seqlen.max()) - case.cw + 1
    return float(np.sqrt(1.0 / case.F)) * {0: kmax, 1: np.sqrt(kmax), 2: 1.0}[scaling]        # c nkmers of the longest row


@pytest.mark.parametrize("n,L,C,cw,rffs", SEQ)
def test_conv_features_rows_and_maxpool(ext, oracle, n, L, C, cw, rffs):
    case = seq_case(n, L, C, cw, rffs)
    radem = dev(case.radem)
    for scaling in (0, 1, 2):
        ref = dr.conv_features(case.x, case.seqlen, case.radem, case.chi, cw, scaling, proj=case.proj)
        scale = _conv_tol_scale(case, scaling)
        orc = {}
        for dtype, tol in ((np.float32, 4e-7 * scale), (np.float64, 1e-13 * scale)):
            x, chi, _ = case.typed(dtype)
            orc[dtype] = oracle_conv(oracle, case, dtype, scaling)
            out = torch.zeros((case.n, rffs), dtype=torch.float64, device=DEV)
            ext.hipConv1dFGen(dev(x), out, radem, dev(chi), case.seqlen, cw, scaling)
            check(f"conv sc={scaling}", case, dtype, host(out), orc[dtype], ref, dr.cap_conv(dtype, case.x, case.seqlen, case.chi, cw, scaling), tol)
        for icpt in (False, True):
            rows = torch.full((case.n, rffs), float("nan"), dtype=torch.float32, device=DEV)
            ext.hipConvFeatureRows(dev(case.x), rows, radem, dev(case.chi), case.seqlen, cw, scaling, icpt)
            want, orows = ref.copy(), orc[np.float32].astype(np.float32)
            if icpt:
                want[:, 0] = 1
                orows[:, 0] = 1.0
            check(f"rows sc={scaling} i={int(icpt)}", case, np.float32, host(rows), orows, want,
                  dr.cap_conv(np.float32, case.x, case.seqlen, case.chi, cw, scaling, u_out=dr.U32), 4e-7 * scale)
    _, ref = dr.conv_maxpool(case.x, case.seqlen, case.radem, case.chi_all, cw, proj=case.proj_all)
    for dtype in BOTH:
        x, _, chi_all = case.typed(dtype)
        out = torch.zeros((case.n, case.M), dtype=torch.float32, device=DEV)
        ext.hipConv1dMaxpool(dev(x), out, radem, dev(chi_all), case.seqlen, cw)
        check("maxpool", case, dtype, host(out), oracle_maxpool(oracle, case, dtype), ref,
              dr.cap_conv_maxpool(dtype, case.x, case.seqlen, case.chi_all, cw, case.pmax), 0.0)


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("n,L,C,cw,rffs", GRAD_SEQ)
def test_conv_grad(ext, oracle, n, L, C, cw, rffs, dtype):
    case = seq_case(n, L, C, cw, rffs)
    x, chi, _ = case.typed(dtype)
    rel = 1e-6 if dtype == np.float32 else 1e-12
    for scaling in (0, 1, 2):
        rf, rg = dr.conv_grad(case.x, case.seqlen, case.radem, case.chi, SIGMA, cw, scaling, proj=case.proj)
        of, og = oracle_conv_grad(oracle, case, dtype, scaling)
        capf, capg = dr.cap_conv_grad(dtype, case.x, case.seqlen, case.chi, SIGMA, cw, scaling, case.pmax)
        o = torch.zeros((case.n, rffs), dtype=torch.float64, device=DEV)
        g = torch.zeros((case.n, rffs, 1), dtype=torch.float64, device=DEV)
        ext.hipConvGrad(dev(x), o, dev(case.radem), dev(chi), case.seqlen, g, SIGMA, cw, scaling)
        check(f"convgrad.f sc={scaling}", case, dtype, host(o), of, rf, capf, rel * float(np.abs(of).max()))
        check(f"convgrad.g sc={scaling}", case, dtype, host(g)[:, :, 0], og, rg, capg, rel * float(np.abs(og).max()))


@pytest.mark.parametrize("n,d,rffs", [(3, 60, 1000), (2, 4000, 8200)])
def test_rbf_grad_float64_into_a_view_8_bytes_into_an_allocation(ext, oracle, n, d, rffs):
    """The wave-tile gradient kernels store a (-sin, cos) pair of grad 16 bytes at a time; into a grad view that is only 8-byte
    aligned they store the two halves separately: same bits as into an aligned buffer, within the dense reference's bound, and the
    8 bytes before and after the view stay untouched."""
    case = fixed_case(n, d, rffs, GRAD_SCALE)
    x, chi = case.typed(np.float64)
    args = (dev(case.radem), dev(chi), SIGMA, True)
    o1 = torch.full((n, rffs), 7.0, dtype=torch.float64, device=DEV)
    g1 = torch.full((n, rffs, 1), 7.0, dtype=torch.float64, device=DEV)
    ext.hipRBFGrad(dev(x), o1, g1, *args)
    guard = -12345.0
    buf = torch.full((n * rffs + 3,), guard, dtype=torch.float64, device=DEV)
    off = 1 if buf.data_ptr() % 16 == 0 else 2
    g2 = buf[off:off + n * rffs].view(n, rffs, 1)
    assert g2.data_ptr() % 16 == 8
    o2 = torch.full((n, rffs), 7.0, dtype=torch.float64, device=DEV)
    ext.hipRBFGrad(dev(x), o2, g2, *args)
    torch.cuda.synchronize()
    flat = host(buf)
    assert np.all(flat[:off] == guard) and np.all(flat[off + n * rffs:] == guard)
    rf, rg = dr.rbf_grad(case.x, case.radem, case.chi, SIGMA, True, proj=case.proj)
    of, og = oracle_rbf_grad(oracle, case, np.float64, True)
    capf, capg = dr.cap_rbf_grad(np.float64, case.x, case.chi, SIGMA, True, case.pmax)
    c = float(dr.rbf_scale(case.F, True))
    check("rbfgrad.g view", case, np.float64, host(g2)[:, :, 0], og, rg, capg, 1e-13 * max(float(np.abs(og).max()), c))
    check("rbfgrad.f view", case, np.float64, host(o2), of, rf, capf, 1e-13 * c)
    same_g = int((g1 != g2).sum())
    print(f"aligned vs 8-byte view: {same_g} of {g1.numel()} gradient entries and {int((o1 != o2).sum())} feature entries differ; "
          f"largest difference {float((g1 - g2).abs().max()):.3e}")
    assert torch.equal(g1, g2) and torch.equal(o1, o2)


def test_g19_hip_operators_against_the_reference_slow_path(ext):
    """hipConv1dFGen, hipConvFeatureRows, hipConvGrad and hipConv1dMaxpool against the outputs of the reference project's own
    slow "ground truth" helpers (tests/golden/g19_slow_path.npz), at the tolerances of the reference's tests."""
    for s in g19_settings():
        x, chi, n, F = s["x"], s["chi"], s["x"].shape[0], s["chi"].shape[0]
        radem, name = dev(s["radem"]), f"g19[{s['si']}] {s['kind']} {np.dtype(s['dtype']).name}"
        if s["kind"] == "maxpool":
            out = torch.zeros((n, F), dtype=torch.float32, device=DEV)
            ext.hipConv1dMaxpool(dev(x), out, radem, dev(chi), s["seqlen"], s["cw"])
            assert np.allclose(s["slow"], host(out), **s["tol"]), name
        elif s["kind"] == "conv":
            xs = dev(x * s["dtype"](s["sigma"]))
            out = torch.zeros((n, 2 * F), dtype=torch.float64, device=DEV)
            ext.hipConv1dFGen(xs, out, radem, dev(chi), s["seqlen"], s["cw"], s["scaling"])
            assert np.allclose(s["slow"], host(out), **s["tol"]), name
            if s["dtype"] == np.float32:
                rows = torch.full((n, 2 * F), float("nan"), dtype=torch.float32, device=DEV)
                ext.hipConvFeatureRows(xs, rows, radem, dev(chi), s["seqlen"], s["cw"], s["scaling"], False)
                assert np.allclose(s["slow"], host(rows), **s["tol"]), name + " rows"
        else:
            out = torch.zeros((n, 2 * F), dtype=torch.float64, device=DEV)
            grad = torch.zeros((n, 2 * F, 1), dtype=torch.float64, device=DEV)
            ext.hipConvGrad(dev(x), out, radem, dev(chi), s["seqlen"], grad, s["sigma"], s["cw"], 0)
            assert np.allclose(s["slow"], host(out), **s["tol"]), name
            assert np.allclose(s["slowgrad"], host(grad)[:, :, 0], **s["tol"]), name + " gradient"
