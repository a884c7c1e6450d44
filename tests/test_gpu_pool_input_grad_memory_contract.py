"""The memory contract of the entry points of include/xgpr_hip_pool_input_grad.h, in the pattern of
tests/test_gpu_seq_input_grad_memory_contract.py: each writer runs once the plain way and once with every array it sees -- x or
(tokens, table), g, radem, chi, the device copy of the lengths, the outputs ``out`` and ``argmax`` and the workspace, exactly the bytes
xgpr_rbf_workspace_bytes advertises, 0xFF-poisoned -- inside the guarded arena of tests/guarded.py.  No guard band may change (no write
outside out and argmax), no input may be modified, and both runs must agree bit for bit (the workspace's contents do not enter).  The
per-row g sits in rows with NaN padding between them: padding that was read would poison the result."""
import numpy as np
import pytest
import torch

import dense_pool_input_grad as dpg
from guarded import Arena, Plain, patched_workspaces, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64

COVERED = {"xgpr_conv_maxpool_input_grad_f32", "xgpr_conv_token_maxpool_input_grad_f32"}
#          token   n   L   C  cw    F  per-row
SHAPES = [(False, 5, 6, 5, 3, 37, False),              # the register-only transform, one ragged tile, one vector for all
          (False, 5, 12, 21, 9, 1324, True),           # configs[3]'s window, g per row, a second ragged tile
          (False, 3, 10, 128, 8, 2048, True),          # the full-width window, two whole tiles
          (True, 5, 12, 21, 9, 1324, True),            # the same through tokens over a one-hot table
          (True, 4, 7, 5, 3, 37, False)]               # ... and over a random table of 24 rows


def covered_entry_points():
    return set(COVERED)


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def token_case(n, L, C, seed):
    """(tokens uint8 [n, L], table float32 [V, C]): one-hot at C = 21, random with 24 rows otherwise."""
    rng = np.random.default_rng([n, L, C, seed])
    table = np.eye(21, dtype=np.float32) if C == 21 else rng.uniform(-1, 1, size=(24, C)).astype(np.float32)
    return rng.integers(0, table.shape[0], size=(n, L)).astype(np.uint8), table


def pool_input_grad(ext, A, token, n, L, C, cw, F, per_row):
    x, seqlen, g, radem, chi = dpg.make_case(n, L, C, cw, F, per_row, seed=21, stride_pad=5)
    if per_row:
        assert g.shape[1] > F and np.isnan(g[:, F:]).all()
    out = A.out((n, L, C), F64, name="out")
    argmax = A.out((n, F), torch.int32, name="argmax")
    need = int(ext._LIB.xgpr_rbf_workspace_bytes(radem.shape[2]))
    ws = A.workspace(need, name="internal workspace")
    gd, rd, cd = A.inp(torch.from_numpy(g), name="g"), A.inp(torch.from_numpy(radem), name="radem"), A.inp(torch.from_numpy(chi), name="chi")
    if token:
        tokens, table = token_case(n, L, C, 21)
        ext.hipConvTokenMaxpoolInputGrad(A.inp(torch.from_numpy(tokens), name="tokens"), A.inp(torch.from_numpy(table), name="table"), gd,
                                         out, argmax, rd, cd, seqlen, cw, workspace=ws)
    else:
        ext.hipConvMaxpoolInputGrad(A.inp(torch.from_numpy(x), name="x"), gd, out, argmax, rd, cd, seqlen, cw, workspace=ws)
    return out, argmax, need


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_memory_contract(ext, shape, monkeypatch):
    plain, plain_arg, _ = pool_input_grad(ext, Plain(DEV), *shape)
    arena = Arena(DEV)
    patched_workspaces(monkeypatch, ext, arena)              # (the device copy of the lengths becomes a guarded input)
    guarded, guarded_arg, need = pool_input_grad(ext, arena, *shape)
    arena.verify()
    names = {r.name.split("#")[0] for r in arena.records}
    assert names == ({"out", "argmax", "internal workspace", "g", "radem", "chi", "device sequence lengths"}
                     | ({"tokens", "table"} if shape[0] else {"x"}))
    ws = next(r for r in arena.records if r.name == "internal workspace")
    assert ws.end - ws.start == need > 0                                   # exactly what is advertised
    assert same_bits(plain, guarded), "the guarded run differs from the plain run"
    assert same_bits(plain_arg, guarded_arg), "the guarded run's argmax differs from the plain run's"
    assert bool(torch.isfinite(plain).all()) and float(plain.abs().max()) > 0
    nk_max = shape[2] - shape[4] + 1
    assert int(plain_arg.min()) >= -1 and int(plain_arg.max()) < nk_max


@pytest.mark.parametrize("token", [False, True], ids=["dense", "tokens"])
def test_a_workspace_one_byte_short_is_refused(ext, token):
    n, L, C, cw, F = 2, 6, 5, 3, 40
    x, seqlen, g, radem, chi = dpg.make_case(n, L, C, cw, F, False, seed=22)
    need = int(ext._LIB.xgpr_rbf_workspace_bytes(radem.shape[2]))
    out = torch.zeros((n, L, C), dtype=F64, device=DEV)
    argmax = torch.zeros((n, F), dtype=torch.int32, device=DEV)
    short = torch.empty(need - 1, dtype=torch.uint8, device=DEV)
    tail = (torch.from_numpy(g).to(DEV), out, argmax, torch.from_numpy(radem).to(DEV), torch.from_numpy(chi).to(DEV), seqlen, cw)
    with pytest.raises(RuntimeError, match="workspace too small"):
        if token:
            tokens, table = token_case(n, L, C, 22)
            ext.hipConvTokenMaxpoolInputGrad(torch.from_numpy(tokens).to(DEV), torch.from_numpy(table).to(DEV), *tail, workspace=short)
        else:
            ext.hipConvMaxpoolInputGrad(torch.from_numpy(x).to(DEV), *tail, workspace=short)
    assert float(out.abs().max()) == 0.0 and int(argmax.abs().max()) == 0
