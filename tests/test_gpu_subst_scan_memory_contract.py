"""The memory contract of the entry point of include/xgpr_hip_subst_scan.h, in the pattern of
tests/test_gpu_kmeans_memory_contract.py and tests/test_gpu_seq_input_grad_memory_contract.py: the writer runs once the plain way and
once with every array it sees -- tokens, table, w, radem, chi, the device copy of the lengths, the output and the workspace, exactly
the bytes xgpr_rbf_workspace_bytes advertises, 0xFF-poisoned -- inside the guarded arena of tests/guarded.py.  No guard band may change
(no write outside out), no input may be modified, and both runs must agree bit for bit (the workspace's contents do not enter).  The
tokens past a sequence's length are 255, a row the table does not have: one that was read would gather from beyond the table."""
import numpy as np
import pytest
import torch

import dense_subst_scan as dss
from guarded import Arena, Plain, patched_workspaces, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64

COVERED = {"xgpr_conv_token_subst_scan_f32"}
SHAPES = ["w16_c4_cw3", "w128_c21_cw6", "w1024_c21_cw48", "graph_cw1", "vocab256_c18"]


def covered_entry_points():
    return set(COVERED)


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def subst_scan(ext, A, name):
    c, cw, scaling, icpt = dss.case(name)
    n, L = c["tokens"].shape
    out = A.out((n, L, c["table"].shape[0]), F64, name="out")
    need = int(ext._LIB.xgpr_rbf_workspace_bytes(c["radem"].shape[2]))
    ws = A.workspace(need, name="internal workspace")
    dev = {k: A.inp(torch.from_numpy(c[k]), name=k) for k in ("tokens", "table", "w", "radem", "chi")}
    ext.hipConvTokenSubstScan(dev["tokens"], dev["table"], dev["w"], out, dev["radem"], dev["chi"], c["seqlen"], cw, scaling, icpt,
                              workspace=ws)
    return out, need


@pytest.mark.parametrize("name", SHAPES)
def test_memory_contract(ext, name, monkeypatch):
    plain, _ = subst_scan(ext, Plain(DEV), name)
    arena = Arena(DEV)
    patched_workspaces(monkeypatch, ext, arena)              # (the device copy of the lengths becomes a guarded input)
    guarded, need = subst_scan(ext, arena, name)
    arena.verify()
    names = {r.name.split("#")[0] for r in arena.records}
    assert names == {"out", "internal workspace", "tokens", "table", "w", "radem", "chi", "device sequence lengths"}
    ws = next(r for r in arena.records if r.name == "internal workspace")
    assert ws.end - ws.start == need > 0                                   # exactly what is advertised
    assert same_bits(plain, guarded), "the guarded run differs from the plain run"
    assert bool(torch.isfinite(plain).all()) and float(plain.abs().max()) > 0


def test_a_workspace_one_byte_short_is_refused(ext):
    c, cw, scaling, icpt = dss.case("w16_c4_cw3")
    n, L = c["tokens"].shape
    need = int(ext._LIB.xgpr_rbf_workspace_bytes(c["radem"].shape[2]))
    out = torch.zeros((n, L, c["table"].shape[0]), dtype=F64, device=DEV)
    short = torch.empty(need - 1, dtype=torch.uint8, device=DEV)
    dev = {k: torch.from_numpy(c[k]).to(DEV) for k in ("tokens", "table", "w", "radem", "chi")}
    with pytest.raises(RuntimeError, match="workspace too small"):
        ext.hipConvTokenSubstScan(dev["tokens"], dev["table"], dev["w"], out, dev["radem"], dev["chi"], c["seqlen"], cw, scaling, icpt,
                                  workspace=short)
    assert float(out.abs().max()) == 0.0
