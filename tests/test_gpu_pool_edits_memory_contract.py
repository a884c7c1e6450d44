"""The memory contract of the two writers of include/xgpr_hip/pool_edits.h, in the pattern of
tests/test_gpu_pair_scan_memory_contract.py: each runs once the plain way and once with every array it sees -- tokens, table, radem,
chi, the device copy of the lengths, the two tables, the output and the workspace, exactly the bytes xgpr_rbf_workspace_bytes
advertises, 0xFF-poisoned -- inside the guarded arena of tests/guarded.py.  No guard band may change, no input may be modified (the
edits read the tables: they are inputs there), and both runs must agree bit for bit (the workspace's contents do not enter).  The
tokens past a sequence's length are 255, a row the table does not have: one that was read would gather from beyond the table."""
import pytest
import torch

import test_gpu_pool_edits as pe
from guarded import Arena, Plain, patched_workspaces, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32

COVERED = {"xgpr_conv_token_maxpool_tables_f32", "xgpr_conv_token_maxpool_edits_f32"}
SHAPES = {"w4_c4_cw1": (1, 4, 4, 70), "w24_c8_cw3": (3, 8, 21, 70), "w189_c21_cw9": (9, 21, 21, 1100), "w360_c40_cw9": (9, 40, 100, 70),
          "w630_c21_cw30": (30, 21, 21, 1100), "vocab256_c18": (3, 18, 256, 70)}


def covered_entry_points():
    return set(COVERED)


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def run_tables(ext, A, c):
    d = c["dev"]
    shape = (pe.N, pe.L - c["cw"] + 2, c["F"])
    pm, sm = A.out(shape, F32, name="pm"), A.out(shape, F32, name="sm")
    need = int(ext._LIB.xgpr_rbf_workspace_bytes(d["radem"].shape[2]))
    ws = A.workspace(need, name="internal workspace")
    dev = {k: A.inp(d[k], name=k) for k in ("tokens", "table", "radem", "chi")}
    ext.hipConvTokenMaxpoolTables(dev["tokens"], dev["table"], pm, sm, dev["radem"], dev["chi"], c["lens"], c["cw"], workspace=ws)
    return pm, sm, need


def run_edits(ext, A, c, tables, mode, lo, cnt):
    d = c["dev"]
    _, per = pe.geometry(c["V"], mode)
    out = A.out((cnt, c["F"]) if mode == "deletions" else (cnt, per, c["F"]), F32, name="out")
    need = int(ext._LIB.xgpr_rbf_workspace_bytes(d["radem"].shape[2]))
    ws = A.workspace(need, name="internal workspace")
    dev = {k: A.inp(d[k], name=k) for k in ("tokens", "table", "radem", "chi")}
    pm, sm = A.inp(tables[0], name="pm"), A.inp(tables[1], name="sm")
    ext.hipConvTokenMaxpoolEdits(dev["tokens"], dev["table"], pm, sm, out, dev["radem"], dev["chi"], c["lens"], c["cw"], mode, lo, cnt,
                                 workspace=ws)
    return out, need


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_tables_memory_contract(ext, name, monkeypatch):
    c = pe.operands(*SHAPES[name])
    plain = run_tables(ext, Plain(DEV), c)
    arena = Arena(DEV)
    patched_workspaces(monkeypatch, ext, arena)              # (the device copy of the lengths becomes a guarded input)
    pm, sm, need = run_tables(ext, arena, c)
    arena.verify()
    names = {r.name.split("#")[0] for r in arena.records}
    assert names == {"pm", "sm", "internal workspace", "tokens", "table", "radem", "chi", "device sequence lengths"}
    ws = next(r for r in arena.records if r.name == "internal workspace")
    assert ws.end - ws.start == need > 0                                   # exactly what is advertised
    assert same_bits(plain[0], pm) and same_bits(plain[1], sm), "the guarded run differs from the plain run"
    assert bool(torch.isfinite(pm).all()) and bool(torch.isfinite(sm).all()) and float(pm.max()) > 0    # overwritten as a whole


@pytest.mark.parametrize("mode", pe.MODES)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_edits_memory_contract(ext, name, mode, monkeypatch):
    """A slab that starts and ends inside sequences: the rows in front of and behind it are not the kernel's to write."""
    c = pe.operands(*SHAPES[name])
    tables = pe.tables(ext, c)
    slots, _ = pe.geometry(c["V"], mode)
    lo, cnt = 1, 2 * slots + 5
    plain, _ = run_edits(ext, Plain(DEV), c, tables, mode, lo, cnt)
    arena = Arena(DEV)
    patched_workspaces(monkeypatch, ext, arena)
    guarded, need = run_edits(ext, arena, c, tables, mode, lo, cnt)
    arena.verify()
    names = {r.name.split("#")[0] for r in arena.records}
    assert names == {"out", "pm", "sm", "internal workspace", "tokens", "table", "radem", "chi", "device sequence lengths"}
    ws = next(r for r in arena.records if r.name == "internal workspace")
    assert ws.end - ws.start == need > 0
    assert same_bits(plain, guarded), "the guarded run differs from the plain run"
    assert float(torch.nan_to_num(plain, nan=0.0).max()) > 0
    assert mode == "deletions" or not bool(torch.isnan(plain).any())       # (NaN: the deletions of the one-window sequence)


def test_a_workspace_one_byte_short_is_refused(ext):
    c = pe.operands(3, 8, 21, 70)
    d = c["dev"]
    pm, sm = pe.tables(ext, c)
    need = int(ext._LIB.xgpr_rbf_workspace_bytes(d["radem"].shape[2]))
    short = torch.empty(need - 1, dtype=torch.uint8, device=DEV)
    out = torch.zeros((pe.L, 21, 70), dtype=F32, device=DEV)
    with pytest.raises(RuntimeError, match="workspace too small"):
        ext.hipConvTokenMaxpoolEdits(d["tokens"], d["table"], pm, sm, out, d["radem"], d["chi"], c["lens"], 3, "substitutions", 0, pe.L,
                                     workspace=short)
    keep = pm.clone()
    with pytest.raises(RuntimeError, match="workspace too small"):
        ext.hipConvTokenMaxpoolTables(d["tokens"], d["table"], pm, sm, d["radem"], d["chi"], c["lens"], 3, workspace=short)
    assert float(out.abs().max()) == 0.0 and same_bits(pm, keep)
