"""One launch of every arm of the launchers' width dispatch (xgpr_amd/csrc/launchers.inc: dispatch_lg and the plans around it), against
the dense-matrix reference with the caps tests/dense_reference.py derives -- compared the way tests/test_gpu_dense_reference.py does
(its ``check``: the oracle within the cap, HIP within the oracle's error plus the suite's parity tolerance of that operator).

Shapes (tests/test_dense_reference_cpu.py: DISPATCH_FIXED / DISPATCH_SEQ, whose CPU leg shows the reference alone inside the caps):
every padded width 2^lg, lg = 1 .. 13, with rows of 2^lg numbers and of one fewer -- the 16-byte-aligned row fetch and the float by
float one -- three rows, with and without the intercept.  Per shape every operator whose entry point serves that width: the feature and
gradient operators in float32 and float64, the float32 feature cache, the float32 gradient rows, the fused matvec and z^T y (lg <= 12);
for sequences (conv_width 1, lengths 1, 2, 3) features, gradient, max-pool in both types, and the float32 feature / gradient rows.

The float32 rows are, in addition, the float64-output operator's result rounded once to float32, bit for bit (as the row tests of
tests/test_gpu_seq_rows.py / test_gpu_seq_grad_rows.py / test_gpu_nmll_grad_rows.py assert).  The arms only an environment switch
reaches run at lg = 8 in a fresh child process each (the switches are read once per process)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dense_reference as dr
from test_dense_reference_cpu import (DISPATCH_FIXED, DISPATCH_SCALING, DISPATCH_SEQ, DISPATCH_SEQLEN, GRAD_SCALE, SIGMA, fixed_case,
                                      oracle_conv, oracle_conv_grad, oracle_maxpool, oracle_rbf, oracle_rbf_grad, seq_case)
from guarded import Arena, Plain, patched_workspaces
from test_gpu_dense_reference import BOTH, DEV, check, host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SC = DISPATCH_SCALING


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


# ---------------------------------------------------------------------------------------------- what the device computes
def run_fixed(ext, case, icpt, alloc=None):
    """Every fixed-vector operator that serves the case's width -> {name: host array}.  ``alloc`` supplies the arrays (tests/guarded.py:
    separately allocated tensors by default, or a guarded arena)."""
    alloc = alloc or Plain(DEV)
    inp = lambda a, name: alloc.inp(torch.from_numpy(np.ascontiguousarray(a)), name=name)
    n, rffs, radem, out = case.n, case.rffs, inp(case.radem, "radem"), {}
    for dtype in BOTH:
        x, chi = (inp(a, nm) for a, nm in zip(case.typed(dtype), ("x", "chi")))
        tag = np.dtype(dtype).name
        o = alloc.out((n, rffs), torch.float64, fill=7.0, name=f"rbf.{tag}")
        ext.hipRBFFeatureGen(x, o, radem, chi, icpt)
        out[f"rbf.{tag}"] = host(o)
        o = alloc.out((n, rffs), torch.float64, fill=7.0, name=f"gradf.{tag}")
        g = alloc.out((n, rffs, 1), torch.float64, fill=7.0, name=f"gradg.{tag}")
        ext.hipRBFGrad(x, o, g, radem, chi, SIGMA, icpt)
        out[f"gradf.{tag}"], out[f"gradg.{tag}"] = host(o), host(g)[:, :, 0]
    x, chi = inp(case.x, "x"), inp(case.chi, "chi")
    rows = alloc.out((n, rffs), torch.float32, fill=float("nan"), name="cache")
    ext.hipRBFFeatureCache(x, rows, radem, chi)
    out["cache"] = host(rows)
    zr = alloc.out((n, rffs), torch.float32, fill=float("nan"), name="zrows")
    gr = alloc.out((n, rffs), torch.float32, fill=float("nan"), name="grows")
    ext.hipRBFGradRows(x, zr, gr, radem, chi, SIGMA, icpt)
    out["zrows"], out["grows"] = host(zr), host(gr)
    if case.P <= 4096:
        rng = np.random.default_rng(rffs)
        v, y = rng.standard_normal(rffs), rng.standard_normal(n)
        need = ext.ztz_workspace_bytes(rffs, radem.shape[2])
        w = alloc.out((rffs,), torch.float64, fill=7.0, name="ztz")
        ext.hipZtZMatvec(x, radem, chi, inp(v, "v"), w, icpt, alloc.workspace(need, name="ztz workspace"))
        zty = alloc.out((rffs,), torch.float64, fill=7.0, name="zty")
        ext.hipZtY(x, radem, chi, inp(y, "y"), zty, icpt, alloc.workspace(need, name="zty workspace"))
        out["ztz"], out["zty"], out["v"], out["y"] = host(w), host(zty), v, y
    return out


def run_seq(ext, case, icpt, alloc=None, sc=SC):
    alloc = alloc or Plain(DEV)
    inp = lambda a, name: alloc.inp(torch.from_numpy(np.ascontiguousarray(a)), name=name)
    n, rffs, cw, radem, out = case.n, case.rffs, case.cw, inp(case.radem, "radem"), {}
    for dtype in BOTH:
        x, chi, chi_all = (inp(a, nm) for a, nm in zip(case.typed(dtype), ("x", "chi", "chi_all")))
        tag = np.dtype(dtype).name
        o = alloc.out((n, rffs), torch.float64, fill=0.0, name=f"conv.{tag}")
        ext.hipConv1dFGen(x, o, radem, chi, case.seqlen, cw, sc)
        out[f"conv.{tag}"] = host(o)
        o = alloc.out((n, rffs), torch.float64, fill=0.0, name=f"gradf.{tag}")
        g = alloc.out((n, rffs, 1), torch.float64, fill=0.0, name=f"gradg.{tag}")
        ext.hipConvGrad(x, o, radem, chi, case.seqlen, g, SIGMA, cw, sc)
        out[f"gradf.{tag}"], out[f"gradg.{tag}"] = host(o), host(g)[:, :, 0]
        mp = alloc.out((n, case.M), torch.float32, fill=0.0, name=f"maxpool.{tag}")
        ext.hipConv1dMaxpool(x, mp, radem, chi_all, case.seqlen, cw)
        out[f"maxpool.{tag}"] = host(mp)
    x, chi = inp(case.x, "x"), inp(case.chi, "chi")
    rows = alloc.out((n, rffs), torch.float32, fill=float("nan"), name="rows")
    ext.hipConvFeatureRows(x, rows, radem, chi, case.seqlen, cw, sc, icpt)
    out["rows"] = host(rows)
    zr = alloc.out((n, rffs), torch.float32, fill=float("nan"), name="zrows")
    gr = alloc.out((n, rffs), torch.float32, fill=float("nan"), name="grows")
    ext.hipConvGradRows(x, zr, gr, radem, chi, case.seqlen, SIGMA, cw, sc, icpt)
    out["zrows"], out["grows"] = host(zr), host(gr)
    return out


def run_guarded(run, ext, monkeypatch, case, icpt):
    """``run`` with every array inside a guarded arena and exact internal workspaces; the arena verified before the values are used."""
    arena = Arena(DEV)
    with monkeypatch.context() as mp:
        patched_workspaces(mp, ext, arena)
        got = run(ext, case, icpt, arena)
        arena.verify()
    return got


# ---------------------------------------------------------------------------------------------- ... against the dense reference
def _rounded_once(op_out, first_column):
    want = op_out.astype(np.float32)
    if first_column is not None:
        want[:, 0] = first_column
    return want


def check_fixed(oracle, case, icpt, got):
    n, rffs, i = case.n, case.rffs, int(icpt)
    c = float(dr.rbf_scale(case.F, icpt))
    ref = dr.rbf_features(case.x, case.radem, case.chi, icpt, proj=case.proj)
    rf, rg = dr.rbf_grad(case.x, case.radem, case.chi, SIGMA, icpt, proj=case.proj)
    orc = {}
    for dtype in BOTH:
        tag = np.dtype(dtype).name
        orc[dtype] = oracle_rbf(oracle, case, dtype, icpt)
        check(f"rbf icpt={i}", case, dtype, got[f"rbf.{tag}"], orc[dtype], ref, dr.cap_rbf(dtype, case.x, case.chi, icpt),
              4e-7 * c if dtype == np.float32 else 1e-13 * c)
        of, og = oracle_rbf_grad(oracle, case, dtype, icpt)
        capf, capg = dr.cap_rbf_grad(dtype, case.x, case.chi, SIGMA, icpt, case.pmax)
        gmax = float(np.abs(og).max())
        tolf, tolg = (4e-7 * c, 1e-6 * gmax) if dtype == np.float32 else (1e-13 * c, 1e-13 * max(gmax, c))
        check(f"rbfgrad.f i={i}", case, dtype, got[f"gradf.{tag}"], of, rf, capf, tolf)
        check(f"rbfgrad.g i={i}", case, dtype, got[f"gradg.{tag}"], og, rg, capg, tolg)
    cap32 = dr.cap_rbf(np.float32, case.x, case.chi, icpt)
    check(f"cache icpt={i}", case, np.float32, got["cache"].astype(np.float64) * float(np.float32(c)), orc[np.float32], ref, cap32, 4e-7 * c)
    # the gradient rows: what the float32 gradient operator wrote, every entry of which is a float32 value; column 0 is 1 / 0 under the intercept
    assert np.array_equal(got["zrows"], _rounded_once(got["gradf.float32"], 1.0 if icpt else None)), case
    assert np.array_equal(got["grows"], _rounded_once(got["gradg.float32"], 0.0 if icpt else None)), case
    assert np.array_equal(got["zrows"].astype(np.float64)[:, 1:], got["gradf.float32"][:, 1:]), case
    if case.P > 4096:
        assert "ztz" not in got
        return
    v, y = got["v"], got["y"]
    z = dr.design_matrix(case.x, case.radem, case.chi, icpt, proj=case.proj)
    zo = orc[np.float32].copy()
    if icpt:
        zo[:, 0] = 1.0
    zmax = max(c, 1.0) if icpt else c
    wref, wo = z.T @ (z @ v.astype(dr.LD)), zo.T @ (zo @ v)
    check(f"ztz icpt={i}", case, np.float32, got["ztz"], wo, wref, dr.cap_matvec(cap32, zmax, n, rffs, v), 1e-6 * float(np.abs(wo).max()))
    yref, yo = z.T @ y.astype(dr.LD), zo.T @ y
    check(f"zty icpt={i}", case, np.float32, got["zty"], yo, yref, dr.cap_zty(cap32, zmax, n, y), 1e-6 * float(np.abs(yo).max()))


def check_seq(oracle, case, icpt, got):
    cw = case.cw
    kmax = int(case.seqlen.max()) - cw + 1
    scale = float(np.sqrt(1.0 / case.F)) * {0: kmax, 1: np.sqrt(kmax), 2: 1.0}[SC]        # c nkmers of the longest row
    ref = dr.conv_features(case.x, case.seqlen, case.radem, case.chi, cw, SC, proj=case.proj)
    rf, rg = dr.conv_grad(case.x, case.seqlen, case.radem, case.chi, SIGMA, cw, SC, proj=case.proj)
    _, mref = dr.conv_maxpool(case.x, case.seqlen, case.radem, case.chi_all, cw, proj=case.proj_all)
    orc = {}
    for dtype in BOTH:
        tag = np.dtype(dtype).name
        orc[dtype] = oracle_conv(oracle, case, dtype, SC)
        check(f"conv sc={SC}", case, dtype, got[f"conv.{tag}"], orc[dtype], ref, dr.cap_conv(dtype, case.x, case.seqlen, case.chi, cw, SC),
              4e-7 * scale if dtype == np.float32 else 1e-13 * scale)
        of, og = oracle_conv_grad(oracle, case, dtype, SC)
        capf, capg = dr.cap_conv_grad(dtype, case.x, case.seqlen, case.chi, SIGMA, cw, SC, case.pmax)
        rel = 1e-6 if dtype == np.float32 else 1e-12
        check(f"convgrad.f sc={SC}", case, dtype, got[f"gradf.{tag}"], of, rf, capf, rel * float(np.abs(of).max()))
        check(f"convgrad.g sc={SC}", case, dtype, got[f"gradg.{tag}"], og, rg, capg, rel * float(np.abs(og).max()))
        check("maxpool", case, dtype, got[f"maxpool.{tag}"], oracle_maxpool(oracle, case, dtype), mref,
              dr.cap_conv_maxpool(dtype, case.x, case.seqlen, case.chi_all, cw, case.pmax), 0.0)
    want, orows = ref.copy(), orc[np.float32].astype(np.float32)
    if icpt:
        want[:, 0] = 1
        orows[:, 0] = 1.0
    check(f"rows sc={SC} i={int(icpt)}", case, np.float32, got["rows"], orows, want,
          dr.cap_conv(np.float32, case.x, case.seqlen, case.chi, cw, SC, u_out=dr.U32), 4e-7 * scale)
    # the float32 rows: the float64 operator's sums rounded once, bit for bit
    assert np.array_equal(got["rows"], _rounded_once(got["conv.float32"], 1.0 if icpt else None)), case
    assert np.array_equal(got["zrows"], _rounded_once(got["gradf.float32"], 1.0 if icpt else None)), case
    assert np.array_equal(got["grows"], _rounded_once(got["gradg.float32"], 0.0 if icpt else None)), case


@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("n,d,rffs", DISPATCH_FIXED)
def test_fixed_vector_arms(ext, oracle, monkeypatch, n, d, rffs, icpt):
    case = fixed_case(n, d, rffs, GRAD_SCALE)
    check_fixed(oracle, case, icpt, run_guarded(run_fixed, ext, monkeypatch, case, icpt))


@pytest.mark.parametrize("icpt", [False, True])
@pytest.mark.parametrize("n,L,C,cw,rffs", DISPATCH_SEQ)
def test_sequence_arms(ext, oracle, monkeypatch, n, L, C, cw, rffs, icpt):
    case = seq_case(n, L, C, cw, rffs, DISPATCH_SEQLEN)
    check_seq(oracle, case, icpt, run_guarded(run_seq, ext, monkeypatch, case, icpt))


# ---------------------------------------------------------------------------------------------- arms behind an environment switch
FORCED_FIXED, FORCED_SEQ = (3, 256, 4096), (3, 3, 256, 1, 4096)          # lg = 8

CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import test_gpu_dispatch_arms as t
from xgpr_amd import xgpr_hip_rfgen_ext as ext
out = {"fixed." + k: v for k, v in t.run_fixed(ext, t.fixed_case(*t.FORCED_FIXED, t.GRAD_SCALE), True).items()}
out.update({"seq." + k: v for k, v in t.run_seq(ext, t.seq_case(*t.FORCED_SEQ, t.DISPATCH_SEQLEN), True).items()})
np.savez(sys.argv[1], **out)
"""


@pytest.mark.parametrize("switch,value", [("XGPR_FEAT_PLAN", "wave"), ("XGPR_FEAT_PLAN", "z3"), ("XGPR_ZTZ_WAVES", "2"),
                                          ("XGPR_F64_PLAN", "generic")])
def test_arms_behind_an_environment_switch(oracle, tmp_path, switch, value):
    env = dict(os.environ)
    env[switch] = value
    path = str(tmp_path / "forced.npz")
    code = CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    res = subprocess.run([sys.executable, "-c", code, path], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    got = np.load(path)
    check_fixed(oracle, fixed_case(*FORCED_FIXED, GRAD_SCALE), True, {k[6:]: got[k] for k in got.files if k.startswith("fixed.")})
    check_seq(oracle, seq_case(*FORCED_SEQ, DISPATCH_SEQLEN), True, {k[4:]: got[k] for k in got.files if k.startswith("seq.")})
