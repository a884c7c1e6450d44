"""The memory contract of the entry point of include/xgpr_hip_pair_scan.h, in the pattern of
tests/test_gpu_subst_scan_memory_contract.py: the writer runs once the plain way and once with every array it sees -- tokens, table,
w, radem, chi, the device copy of the lengths, the output and the workspace, exactly the bytes xgpr_rbf_workspace_bytes advertises,
0xFF-poisoned -- inside the guarded arena of tests/guarded.py.  No guard band may change (no write outside out: the second kernel
works in place on it), no input may be modified, and both runs must agree bit for bit (the workspace's contents do not enter).  The
tokens past a sequence's length are 255, a row the table does not have: one that was read would gather from beyond the table."""
import pytest
import torch

import dense_pair_scan as dp
from guarded import Arena, Plain, patched_workspaces, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64

COVERED = {"xgpr_conv_token_pair_scan_f32"}
SHAPES = ["w16_c4_cw3", "w128_c21_cw6", "w1024_c120_cw8", "cw20_c3", "vocab256_c18", "n65"]


def covered_entry_points():
    return set(COVERED)


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def pair_scan(ext, A, name):
    c, cw, scaling, icpt = dp.case(name)
    n, L = c["tokens"].shape
    V = c["table"].shape[0]
    out = A.out((n, L, cw - 1, V, V), F64, name="out")
    need = int(ext._LIB.xgpr_rbf_workspace_bytes(c["radem"].shape[2]))
    ws = A.workspace(need, name="internal workspace")
    dev = {k: A.inp(torch.from_numpy(c[k]), name=k) for k in ("tokens", "table", "w", "radem", "chi")}
    ext.hipConvTokenPairScan(dev["tokens"], dev["table"], dev["w"], out, dev["radem"], dev["chi"], c["seqlen"], cw, scaling, icpt,
                             workspace=ws)
    return out, need


@pytest.mark.parametrize("name", SHAPES)
def test_memory_contract(ext, name, monkeypatch):
    plain, _ = pair_scan(ext, Plain(DEV), name)
    arena = Arena(DEV)
    patched_workspaces(monkeypatch, ext, arena)              # (the device copy of the lengths becomes a guarded input)
    guarded, need = pair_scan(ext, arena, name)
    arena.verify()
    names = {r.name.split("#")[0] for r in arena.records}
    assert names == {"out", "internal workspace", "tokens", "table", "w", "radem", "chi", "device sequence lengths"}
    ws = next(r for r in arena.records if r.name == "internal workspace")
    assert ws.end - ws.start == need > 0                                   # exactly what is advertised
    assert same_bits(plain, guarded), "the guarded run differs from the plain run"
    assert bool(torch.isfinite(plain).all()) and float(plain.abs().max()) > 0


def test_a_workspace_one_byte_short_is_refused(ext):
    c, cw, scaling, icpt = dp.case("w16_c4_cw3")
    n, L = c["tokens"].shape
    V = c["table"].shape[0]
    need = int(ext._LIB.xgpr_rbf_workspace_bytes(c["radem"].shape[2]))
    out = torch.zeros((n, L, cw - 1, V, V), dtype=F64, device=DEV)
    short = torch.empty(need - 1, dtype=torch.uint8, device=DEV)
    dev = {k: torch.from_numpy(c[k]).to(DEV) for k in ("tokens", "table", "w", "radem", "chi")}
    with pytest.raises(RuntimeError, match="workspace too small"):
        ext.hipConvTokenPairScan(dev["tokens"], dev["table"], dev["w"], out, dev["radem"], dev["chi"], c["seqlen"], cw, scaling, icpt,
                                 workspace=short)
    assert float(out.abs().max()) == 0.0
