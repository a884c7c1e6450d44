"""The memory contract of the entry points of include/xgpr_hip_input_grad.h, as tests/test_gpu_memory_contract.py holds those of
include/xgpr_hip.h to it: the operator runs once the plain way and once with x, w, radem, chi, the output g and the workspace -- exactly
the bytes xgpr_rbf_workspace_bytes advertises, 0xFF-poisoned -- inside the guarded arena of tests/guarded.py.  No guard band may change
(no write outside g), no input may be modified, and both runs must agree bit for bit.  The per-row weights sit in rows with NaN
padding between them (and the arena's NaN guards behind the last row): padding that was read would poison the result."""
import numpy as np
import pytest
import torch

import dense_input_grad as dig
from guarded import Arena, Plain, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64

COVERED = {"xgpr_rbf_input_grad_f32"}
#          n    d     F   intercept  per-row  w_cols
SHAPES = [(5, 3, 37, True, False, 74),             # the register-only transform, one ragged tile, one vector for all rows
          (67, 100, 1324, True, True, 2248),       # the two-layout transform, weights per row ending inside the second tile
          (5, 1024, 2048, False, True, 4096)]      # the full-width load, two whole tiles


def covered_entry_points():
    return set(COVERED)


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def input_grad(ext, A, n, d, F, icpt, per_row, w_cols):
    xs, w, radem, chi, sigma = dig.make_case(n, d, F, per_row, seed=21, stride_pad=5)
    if per_row:
        assert w.shape[1] > w_cols and np.isnan(w[:, 2 * F:]).all()
    out = A.out((n, d), F64, name="g")
    need = int(ext._LIB.xgpr_rbf_workspace_bytes(radem.shape[2]))
    ws = A.workspace(need, name="internal workspace")
    ext.hipRBFInputGrad(A.inp(torch.from_numpy(xs), name="x"), A.inp(torch.from_numpy(w), name="w"), out,
                        A.inp(torch.from_numpy(radem), name="radem"), A.inp(torch.from_numpy(chi), name="chi"), sigma, icpt,
                        w_cols=w_cols, workspace=ws)
    return out, need


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_memory_contract(ext, shape):
    plain, _ = input_grad(ext, Plain(DEV), *shape)
    arena = Arena(DEV)
    guarded, need = input_grad(ext, arena, *shape)
    arena.verify()
    assert {r.name for r in arena.records} == {"g", "internal workspace", "x", "w", "radem", "chi"}
    ws = next(r for r in arena.records if r.name == "internal workspace")
    assert ws.end - ws.start == need > 0                                   # exactly what is advertised
    assert same_bits(plain, guarded), "the guarded run differs from the plain run"
    assert bool(torch.isfinite(plain).all()) and float(plain.abs().max()) > 0


def test_a_workspace_one_byte_short_is_refused(ext):
    xs, w, radem, chi, sigma = dig.make_case(2, 9, 40, False, seed=22)
    need = int(ext._LIB.xgpr_rbf_workspace_bytes(radem.shape[2]))
    out = torch.zeros((2, 9), dtype=F64, device=DEV)
    with pytest.raises(RuntimeError, match="workspace too small"):
        ext.hipRBFInputGrad(torch.from_numpy(xs).to(DEV), torch.from_numpy(w).to(DEV), out, torch.from_numpy(radem).to(DEV),
                            torch.from_numpy(chi).to(DEV), sigma, True, workspace=torch.empty(need - 1, dtype=torch.uint8, device=DEV))
    assert float(out.abs().max()) == 0.0
