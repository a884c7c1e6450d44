"""The memory contract of the entry points of include/xgpr_hip_pool.h, as tests/test_gpu_memory_contract.py holds those of
include/xgpr_hip.h to it: the operator runs once the plain way and once with every input, the output, the internal workspace (exactly
the bytes xgpr_conv_workspace_bytes advertises, 0xFF-poisoned) and the device copy of the sequence lengths inside the guarded arena
of tests/guarded.py.  No guard band may change, no input may be modified, and both runs must agree bit for bit.  The shapes are
borrowed from tests/test_gpu_token_maxpool.py, where the plain numbers are held to the dense operator."""
import pytest
import torch

from guarded import Arena, Plain, patched_workspaces, same_bits
from test_gpu_token_maxpool import N, operands, padded

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32

COVERED = {"xgpr_conv_token_maxpool_f32"}
# a rows-only window with a ragged tile, and configs[3]'s window with two tiles per sequence
SHAPES = [(3, 8, 21, 70), (9, 21, 21, 1100)]


def covered_entry_points():
    return set(COVERED)


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def token_maxpool(ext, A, cw, C_, V, num_features):
    tokens, _, table, radem, chi, lens = (t.cpu() if isinstance(t, torch.Tensor) else t for t in operands(cw, C_, V, num_features))
    assert ext.conv_token_rows_ok(cw * C_, V, C_) == 1
    out = A.out((N, num_features), F32, fill=0.0, name="out")
    ext.hipConvTokenMaxpool(A.inp(tokens, name="tokens"), A.inp(table, name="table"), out, A.inp(radem, name="radem"),
                            A.inp(chi, name="chi"), lens, cw)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_memory_contract(ext, monkeypatch, shape):
    plain = token_maxpool(ext, Plain(DEV), *shape)
    arena = Arena(DEV)
    with monkeypatch.context() as mp:
        patched_workspaces(mp, ext, arena)
        guarded = token_maxpool(ext, arena, *shape)
        arena.verify()
    names = [r.name for r in arena.records]
    assert any(n.startswith("internal workspace") for n in names) and any(n.startswith("device sequence lengths") for n in names)
    ws = next(r for r in arena.records if r.name.startswith("internal workspace"))
    cw, C_, _, num_features = shape
    P = padded(cw * C_)
    assert ws.end - ws.start == ext._LIB.xgpr_conv_workspace_bytes(-(-num_features // P) * P, cw * C_, 4, N)      # exactly what is advertised
    assert same_bits(plain, guarded), "the guarded run differs from the plain run"
    assert bool(torch.isfinite(plain).all()) and float(plain.max()) > 0
