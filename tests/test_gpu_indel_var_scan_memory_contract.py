"""The memory contract of the writer of include/xgpr_hip_indel_var_scan.h, in the pattern of
tests/test_gpu_subst_var_scan_memory_contract.py: it runs once the plain way and once with every array it sees -- tokens, table, vm,
the two (u, q) pairs, radem, chi, the device copy of the lengths, both outputs and the workspace, EXACTLY the bytes
xgpr_conv_token_indel_var_scan_workspace_bytes advertises, 0xFF-poisoned -- inside the guarded arena of tests/guarded.py, at the
default slab_rows and at 16 (many slabs; slab edges inside a gap's V rows; row tiles that are not full).  No guard band may change, no
input may be modified, and both runs must agree bit for bit: the workspace's contents (NaN rows where a slot past a length, or a
deletion without a mutant, wrote nothing) do not enter.  The tokens past a sequence's length are 255, a row the table does not have."""
import numpy as np
import pytest
import torch

import dense_indel_var_scan as div
from guarded import Arena, Plain, patched_workspaces, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64

COVERED = {"xgpr_conv_token_indel_var_scan_f32"}
SHAPES = ["w16_c4_cw3", "w128_c21_cw6", "w1024_c21_cw48", "w512_c16_cw20", "graph_cw1", "vocab256_c18"]


def covered_entry_points():
    return set(COVERED)


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def var_scan(ext, A, name, slab_rows, ws=None):
    k = div.case(name)
    c, nvar = k["c"], k["nvar"]
    n, L = c["tokens"].shape
    od = A.out((n, L), F64, name="out_del")
    oi = A.out((n, L + 1, c["table"].shape[0]), F64, name="out_ins")
    need = ext.conv_token_indel_var_scan_workspace_bytes(c["radem"].shape[2], nvar, slab_rows)
    ws = A.workspace(need, name="internal workspace") if ws is None else ws
    dev = {key: A.inp(torch.from_numpy(c[key]), name=key) for key in ("tokens", "table", "radem", "chi")}
    full = np.full((nvar, nvar + k["pad"]), np.nan)                  # (the columns behind a strided row are never read)
    full[:, :nvar] = k["vm"]
    vm = A.inp(torch.from_numpy(full), name="vm")[:, :nvar]
    ops = {key: A.inp(torch.from_numpy(k[key]), name=key) for key in ("u_del", "q_del", "u_ins", "q_ins")}
    ext.hipConvTokenIndelVarScan(dev["tokens"], dev["table"], vm, ops["u_del"], ops["q_del"], ops["u_ins"], ops["q_ins"], od, oi,
                                 dev["radem"], dev["chi"], c["seqlen"], k["cw"], k["scaling"], k["icpt"], slab_rows=slab_rows, workspace=ws)
    return od, oi, need


@pytest.mark.parametrize("slab_rows", [0, 16])
@pytest.mark.parametrize("name", SHAPES)
def test_memory_contract(ext, name, slab_rows, monkeypatch):
    pd, pi, _ = var_scan(ext, Plain(DEV), name, slab_rows)
    arena = Arena(DEV)
    patched_workspaces(monkeypatch, ext, arena)              # (the device copy of the lengths becomes a guarded input)
    gd, gi, need = var_scan(ext, arena, name, slab_rows)
    arena.verify()
    names = {r.name.split("#")[0] for r in arena.records}
    assert names == {"out_del", "out_ins", "internal workspace", "tokens", "table", "vm", "u_del", "q_del", "u_ins", "q_ins", "radem", "chi",
                     "device sequence lengths"}
    ws = next(r for r in arena.records if r.name == "internal workspace")
    assert ws.end - ws.start == need > 0                                   # exactly what is advertised
    k = div.case(name)
    masks = int(ext._LIB.xgpr_rbf_workspace_bytes(k["c"]["radem"].shape[2]))
    if slab_rows:
        assert need == masks + slab_rows * k["nvar"] * 8
    assert same_bits(pd, gd) and same_bits(pi, gi), "the guarded run differs from the plain run"
    assert bool(torch.isfinite(pi).all()) and float(pi.abs().max()) > 0


@pytest.mark.parametrize("slab_rows", [0, 16])
@pytest.mark.parametrize("name", ["w128_c21_cw6", "w16_c4_cw3"])
def test_poison_behind_dead_rows_stays_there(ext, name, slab_rows):
    """A workspace of 0xFF bytes (NaN delta rows) against one of zeros: the rows of positions past a length, of gaps past it and of
    the deletions of the s == conv_width sequence are never written by the delta kernel and never read by the quadratic form, although
    they share 16-row tiles with live rows."""
    k = div.case(name)
    c = k["c"]
    n, L = c["tokens"].shape
    live = (np.arange(L)[None, :] < c["seqlen"][:, None]) & (c["seqlen"][:, None] > k["cw"])
    tiles = np.pad(live.reshape(-1), (0, -live.size % 16)).reshape(-1, 16)
    assert ((tiles.sum(axis=1) > 0) & (tiles.sum(axis=1) < 16)).any()      # a tile with live and dead rows
    need = ext.conv_token_indel_var_scan_workspace_bytes(c["radem"].shape[2], k["nvar"], slab_rows)
    outs = []
    for byte in (0xFF, 0x00):
        ws = torch.full((need,), byte, dtype=torch.uint8, device=DEV)
        od, oi, _ = var_scan(ext, Plain(DEV), name, slab_rows, ws=ws)
        outs.append((od, oi))
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1])
    od = outs[0][0].cpu().numpy()
    assert np.isfinite(od[live]).all() and bool(torch.isfinite(outs[0][1]).all())


@pytest.mark.parametrize("slab_rows", [0, 16])
def test_a_workspace_one_byte_short_is_refused(ext, slab_rows):
    k = div.case("w16_c4_cw3")
    c = k["c"]
    n, L = c["tokens"].shape
    need = ext.conv_token_indel_var_scan_workspace_bytes(c["radem"].shape[2], k["nvar"], slab_rows)
    short = torch.empty(need - 1, dtype=torch.uint8, device=DEV)
    A = Plain(DEV)
    od = torch.zeros((n, L), dtype=F64, device=DEV)
    oi = torch.zeros((n, L + 1, c["table"].shape[0]), dtype=F64, device=DEV)
    dev = {key: torch.from_numpy(c[key]).to(DEV) for key in ("tokens", "table", "radem", "chi")}
    ops = {key: A.inp(torch.from_numpy(k[key])) for key in ("u_del", "q_del", "u_ins", "q_ins")}
    with pytest.raises(RuntimeError, match="workspace too small"):
        ext.hipConvTokenIndelVarScan(dev["tokens"], dev["table"], torch.from_numpy(k["vm"]).to(DEV), ops["u_del"], ops["q_del"], ops["u_ins"],
                                     ops["q_ins"], od, oi, dev["radem"], dev["chi"], c["seqlen"], k["cw"], k["scaling"], k["icpt"],
                                     slab_rows=slab_rows, workspace=short)
    assert float(od.abs().max()) == 0.0 and float(oi.abs().max()) == 0.0
