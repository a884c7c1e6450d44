"""Pins the CPU oracle bit-for-bit against the reference's own compiled arithmetic core
(oracle/_ref/libxgpr_ref.so) on seeded random inputs beyond the committed fixtures.
Every output is checked against the sha256 of the core's output for the same input, recorded in
tests/golden/ref_core_digests.json (tests/golden/make_golden.py ref_core_digests); where
oracle/Makefile could build the core, the two are also compared array for array."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import oracle as orc

DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_core_digests.json")

RBF_CASES = [(5, 16, False), (32, 512, True), (100, 300, False), (513, 4096, True), (1024, 2048, False), (3000, 1024, True)]
CONV_CASES = [(30, 21, 9, 1024, 0), (17, 4, 1, 64, 1), (40, 21, 5, 600, 2), (12, 300, 4, 512, 1)]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def case_id(kind, dtype, params=()):
    return "-".join([kind, np.dtype(dtype).name] + [str(p) for p in params])


def fht_and_srht_outputs(ops, dtype):
    out = {}
    rng = np.random.default_rng(7)
    for P in [2, 8, 64, 128, 2048, 16384]:
        x = rng.standard_normal((5, P)).astype(dtype)
        a = x.copy()
        ops.cpuFastHadamardTransform2D(a)
        out[f"fht2d_{P}"] = a
        radem = rng.choice(np.asarray([-1, 1], np.int8), size=P)
        a = x.copy()
        ops.cpuSRHT(a, radem)
        out[f"srht_{P}"] = a
    x = rng.standard_normal((4, 6, 32)).astype(dtype)
    a = x.copy()
    ops.cpuFastHadamardTransform(a)
    out["fht3d"] = a
    return out


def rbf_outputs(ops, dtype, d, rffs, icpt):
    rng = np.random.default_rng(11)
    radem, chi = orc.draw_sorf_params(rffs, d, 5, double_precision=(dtype == np.float64))
    x = (rng.standard_normal((7, d)) * 3).astype(dtype)
    a = np.zeros((7, rffs))
    ops.cpuRBFFeatureGen(x.copy(), a, radem, chi, icpt)
    b, gb = np.zeros((7, rffs)), np.zeros((7, rffs, 1))
    ops.cpuRBFGrad(x.copy(), b, gb, radem, chi, 1.3, icpt)
    return {"features": a, "grad_features": b, "grad": gb}


def conv_outputs(ops, dtype, L, C, cw, rffs, sc):
    rng = np.random.default_rng(13)
    n = 5
    radem, chi = orc.draw_sorf_params(rffs, cw * C, 9, double_precision=(dtype == np.float64),
                                      conv=True)
    x = rng.standard_normal((n, L, C)).astype(dtype)
    sl = rng.integers(cw, L + 1, size=n).astype(np.int32)
    a = np.zeros((n, rffs))
    ops.cpuConv1dFGen(x, a, radem, chi, sl, cw, sc)
    b, gb = np.zeros((n, rffs)), np.zeros((n, rffs, 1))
    ops.cpuConvGrad(x, b, radem, chi, sl, gb, 0.8, cw, sc)
    # max-pool: F == num_rffs, radem length exactly reps * P
    P = orc.padded_dims(cw * C)
    F = rffs // 2
    reps = -(-F // P)
    radem_m = radem[:, :, :reps * P].copy() if radem.shape[2] >= reps * P else \
        rng.choice(np.asarray([-1, 1], np.int8), size=(3, 1, reps * P))
    chi_m = np.ascontiguousarray(chi[:F])
    mp = np.zeros((n, F), np.float32)
    ops.cpuConv1dMaxpool(x, mp, radem_m, chi_m, sl, cw)
    return {"features": a, "grad_features": b, "grad": gb, "maxpool": mp}


def all_cases():
    """(case id, function of the operator object that returns the case's named outputs)"""
    cases = []
    for dtype in (np.float32, np.float64):
        cases.append((case_id("fht_srht", dtype), lambda ops, dt=dtype: fht_and_srht_outputs(ops, dt)))
        for p in RBF_CASES:
            cases.append((case_id("rbf", dtype, p), lambda ops, dt=dtype, p=p: rbf_outputs(ops, dt, *p)))
        for p in CONV_CASES:
            cases.append((case_id("conv", dtype, p), lambda ops, dt=dtype, p=p: conv_outputs(ops, dt, *p)))
    return cases


def check(oracle, refcore, key, outputs_of):
    with open(DIGESTS) as f:
        recorded = json.load(f)[key]
    got = outputs_of(oracle)
    assert sorted(got) == sorted(recorded), key
    for name, a in got.items():
        assert digest(a) == recorded[name], f"{key} {name}: differs from the reference core's recorded output"
    if refcore is not None:
        ref = outputs_of(refcore)
        for name, a in got.items():
            assert np.array_equal(a, ref[name]), f"{key} {name}"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fht_and_srht(oracle, refcore, dtype):
    check(oracle, refcore, case_id("fht_srht", dtype), lambda ops: fht_and_srht_outputs(ops, dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("d,rffs,icpt", RBF_CASES)
def test_rbf(oracle, refcore, dtype, d, rffs, icpt):
    check(oracle, refcore, case_id("rbf", dtype, (d, rffs, icpt)), lambda ops: rbf_outputs(ops, dtype, d, rffs, icpt))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("L,C,cw,rffs,sc", CONV_CASES)
def test_conv(oracle, refcore, dtype, L, C, cw, rffs, sc):
    check(oracle, refcore, case_id("conv", dtype, (L, C, cw, rffs, sc)),
          lambda ops: conv_outputs(ops, dtype, L, C, cw, rffs, sc))
