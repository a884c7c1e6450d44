"""The memory contract of the writer of include/xgpr_hip_subst_var_scan.h, in the pattern of
tests/test_gpu_subst_scan_memory_contract.py: it runs once the plain way and once with every array it sees -- tokens, table, vm, u, q,
radem, chi, the device copy of the lengths, the output and the workspace, EXACTLY the bytes
xgpr_conv_token_subst_var_scan_workspace_bytes advertises, 0xFF-poisoned -- inside the guarded arena of tests/guarded.py, at the
default slab_rows and at 16 (many slabs; slab edges inside a position's V rows; row tiles that are not full).  No guard band may
change, no input may be modified, and both runs must agree bit for bit: the workspace's contents (NaN rows where a slot past a length
wrote nothing) do not enter.  The tokens past a sequence's length are 255, a row the table does not have."""
import numpy as np
import pytest
import torch

import dense_subst_var_scan as dv
from guarded import Arena, Plain, patched_workspaces, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64

COVERED = {"xgpr_conv_token_subst_var_scan_f32"}
SHAPES = ["w16_c4_cw3", "w128_c21_cw6", "w1024_c21_cw48", "w512_c16_cw20", "graph_cw1", "vocab256_c18"]


def covered_entry_points():
    return set(COVERED)


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def var_scan(ext, A, name, slab_rows):
    k = dv.case(name)
    c, nvar = k["c"], k["nvar"]
    n, L = c["tokens"].shape
    out = A.out((n, L, c["table"].shape[0]), F64, name="out")
    need = ext.conv_token_subst_var_scan_workspace_bytes(c["radem"].shape[2], nvar, slab_rows)
    ws = A.workspace(need, name="internal workspace")
    dev = {key: A.inp(torch.from_numpy(c[key]), name=key) for key in ("tokens", "table", "radem", "chi")}
    full = np.full((nvar, nvar + k["pad"]), np.nan)                  # (the columns behind a strided row are never read)
    full[:, :nvar] = k["vm"]
    vm = A.inp(torch.from_numpy(full), name="vm")[:, :nvar]
    u, q = A.inp(torch.from_numpy(k["u64"]), name="u"), A.inp(torch.from_numpy(k["q64"]), name="q")
    ext.hipConvTokenSubstVarScan(dev["tokens"], dev["table"], vm, u, q, out, dev["radem"], dev["chi"], c["seqlen"], k["cw"], k["scaling"],
                                 k["icpt"], slab_rows=slab_rows, workspace=ws)
    return out, need


@pytest.mark.parametrize("slab_rows", [0, 16])
@pytest.mark.parametrize("name", SHAPES)
def test_memory_contract(ext, name, slab_rows, monkeypatch):
    plain, _ = var_scan(ext, Plain(DEV), name, slab_rows)
    arena = Arena(DEV)
    patched_workspaces(monkeypatch, ext, arena)              # (the device copy of the lengths becomes a guarded input)
    guarded, need = var_scan(ext, arena, name, slab_rows)
    arena.verify()
    names = {r.name.split("#")[0] for r in arena.records}
    assert names == {"out", "internal workspace", "tokens", "table", "vm", "u", "q", "radem", "chi", "device sequence lengths"}
    ws = next(r for r in arena.records if r.name == "internal workspace")
    assert ws.end - ws.start == need > 0                                   # exactly what is advertised
    k = dv.case(name)
    masks = int(ext._LIB.xgpr_rbf_workspace_bytes(k["c"]["radem"].shape[2]))
    if slab_rows:
        assert need == masks + slab_rows * k["nvar"] * 8
    assert same_bits(plain, guarded), "the guarded run differs from the plain run"
    assert bool(torch.isfinite(plain).all()) and float(plain.abs().max()) > 0


@pytest.mark.parametrize("slab_rows", [0, 16])
def test_a_workspace_one_byte_short_is_refused(ext, slab_rows):
    k = dv.case("w16_c4_cw3")
    c, nvar = k["c"], k["nvar"]
    n, L = c["tokens"].shape
    need = ext.conv_token_subst_var_scan_workspace_bytes(c["radem"].shape[2], nvar, slab_rows)
    out = torch.zeros((n, L, c["table"].shape[0]), dtype=F64, device=DEV)
    short = torch.empty(need - 1, dtype=torch.uint8, device=DEV)
    dev = {key: torch.from_numpy(c[key]).to(DEV) for key in ("tokens", "table", "radem", "chi")}
    with pytest.raises(RuntimeError, match="workspace too small"):
        ext.hipConvTokenSubstVarScan(dev["tokens"], dev["table"], torch.from_numpy(k["vm"]).to(DEV), torch.from_numpy(k["u64"]).to(DEV),
                                     torch.from_numpy(k["q64"]).to(DEV), out, dev["radem"], dev["chi"], c["seqlen"], k["cw"], k["scaling"],
                                     k["icpt"], slab_rows=slab_rows, workspace=short)
    assert float(out.abs().max()) == 0.0
