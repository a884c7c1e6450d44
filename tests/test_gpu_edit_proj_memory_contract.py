"""The memory contract of the two writers of include/xgpr_hip/edit_proj.h, in the pattern of
tests/test_gpu_indel_var_scan_memory_contract.py: each runs once the plain way and once with every array it sees -- tokens, table,
pm (strided where the case says so), the base rows b, radem, chi, the device copy of the lengths, the outputs and the workspace, EXACTLY
the bytes xgpr_conv_token_edit_proj_workspace_bytes advertises, 0xFF-poisoned -- inside the guarded arena of tests/guarded.py, at the
default slab_rows and at 16 (many slabs; slab edges inside a slot's V rows; row tiles that are not full), with K = 65 columns (a second,
ragged column block).  No guard band may change, no input may be modified, and both runs must agree bit for bit: the workspace's
contents do not enter.  The tokens past a sequence's length are 255, a row the table does not have."""
import numpy as np
import pytest
import torch

import dense_indel_var_scan as div
from guarded import Arena, Plain, patched_workspaces, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
K = 65

COVERED = {"xgpr_conv_token_subst_proj_f32", "xgpr_conv_token_indel_proj_f32"}
SHAPES = ["w16_c4_cw3", "w128_c21_cw6", "w1024_c21_cw48", "w512_c16_cw20", "graph_cw1", "vocab256_c18"]


def covered_entry_points():
    return set(COVERED)


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def operands(name):
    """The indel case's operand set (its lengths hold conv_width and conv_width + 1) with a seeded pm [nvar, K] and base rows."""
    k = div.case(name)
    rng = np.random.default_rng([k["nvar"], 65])
    n = k["c"]["tokens"].shape[0]
    return k, rng.normal(size=(k["nvar"], K)), rng.normal(size=(3, n, K))


def run(ext, A, name, slab_rows, ws=None):
    k, pm, b = operands(name)
    c, nvar = k["c"], k["nvar"]
    n, L = c["tokens"].shape
    V = c["table"].shape[0]
    outs = [A.out(shape, F64, name=nm) for nm, shape in (("out", (n, L, V, K)), ("out_del", (n, L, K)), ("out_ins", (n, L + 1, V, K)))]
    need = ext.conv_token_edit_proj_workspace_bytes(c["radem"].shape[2], nvar, slab_rows)
    ws = A.workspace(need, name="internal workspace") if ws is None else ws
    dev = {key: A.inp(torch.from_numpy(c[key]), name=key) for key in ("tokens", "table", "radem", "chi")}
    full = np.full((nvar, K + k["pad"]), np.nan)                     # (the columns behind a strided row are never read)
    full[:, :K] = pm
    pmd = A.inp(torch.from_numpy(full), name="pm")[:, :K]
    bs = [A.inp(torch.from_numpy(np.ascontiguousarray(b[j])), name=nm) for j, nm in enumerate(("b", "b_del", "b_ins"))]
    tail = (dev["radem"], dev["chi"], c["seqlen"], k["cw"], k["scaling"], k["icpt"])
    ext.hipConvTokenSubstProj(dev["tokens"], dev["table"], pmd, bs[0], outs[0], *tail, slab_rows=slab_rows, workspace=ws)
    ext.hipConvTokenIndelProj(dev["tokens"], dev["table"], pmd, bs[1], bs[2], outs[1], outs[2], *tail, slab_rows=slab_rows, workspace=ws)
    return outs, need


@pytest.mark.parametrize("slab_rows", [0, 16])
@pytest.mark.parametrize("name", SHAPES)
def test_memory_contract(ext, name, slab_rows, monkeypatch):
    plain, _ = run(ext, Plain(DEV), name, slab_rows)
    arena = Arena(DEV)
    patched_workspaces(monkeypatch, ext, arena)              # (the device copy of the lengths becomes a guarded input)
    guarded, need = run(ext, arena, name, slab_rows)
    arena.verify()
    names = {r.name.split("#")[0] for r in arena.records}
    assert names == {"out", "out_del", "out_ins", "internal workspace", "tokens", "table", "pm", "b", "b_del", "b_ins", "radem", "chi",
                     "device sequence lengths"}
    ws = next(r for r in arena.records if r.name == "internal workspace")
    assert ws.end - ws.start == need > 0                                   # exactly what is advertised
    k = div.case(name)
    masks = int(ext._LIB.xgpr_rbf_workspace_bytes(k["c"]["radem"].shape[2]))
    if slab_rows:
        assert need == masks + slab_rows * k["nvar"] * 8
    for p, g in zip(plain, guarded):
        assert same_bits(p, g), "the guarded run differs from the plain run"
    assert bool(torch.isfinite(plain[0]).all()) and bool(torch.isfinite(plain[2]).all()) and float(plain[2].abs().max()) > 0


@pytest.mark.parametrize("slab_rows", [0, 16])
@pytest.mark.parametrize("name", ["w128_c21_cw6", "w16_c4_cw3"])
def test_poison_behind_dead_rows_stays_there(ext, name, slab_rows):
    """A workspace of 0xFF bytes (NaN delta rows) against one of zeros: the rows of positions past a length, of gaps past it and of
    the deletions of the s == conv_width sequence are never written by the delta kernels and never read by the projection, although
    they share 16-row tiles with live rows."""
    k = div.case(name)
    c = k["c"]
    n, L = c["tokens"].shape
    live = (np.arange(L)[None, :] < c["seqlen"][:, None]) & (c["seqlen"][:, None] > k["cw"])
    tiles = np.pad(live.reshape(-1), (0, -live.size % 16)).reshape(-1, 16)
    assert ((tiles.sum(axis=1) > 0) & (tiles.sum(axis=1) < 16)).any()      # a tile with live and dead rows
    need = ext.conv_token_edit_proj_workspace_bytes(c["radem"].shape[2], k["nvar"], slab_rows)
    runs = []
    for byte in (0xFF, 0x00):
        ws = torch.full((need,), byte, dtype=torch.uint8, device=DEV)
        runs.append(run(ext, Plain(DEV), name, slab_rows, ws=ws)[0])
    for a, b in zip(*runs):
        assert same_bits(a, b)
    od = runs[0][1].cpu().numpy()
    assert np.isfinite(od[live]).all() and bool(torch.isfinite(runs[0][0]).all()) and bool(torch.isfinite(runs[0][2]).all())
    past = np.arange(L)[None, :] >= c["seqlen"][:, None]
    assert not od[past].view(np.uint64).any() and np.isnan(od[~past & ~live]).all()


@pytest.mark.parametrize("slab_rows", [0, 16])
def test_a_workspace_one_byte_short_is_refused(ext, slab_rows):
    k, pm, b = operands("w16_c4_cw3")
    c = k["c"]
    n, L = c["tokens"].shape
    V = c["table"].shape[0]
    need = ext.conv_token_edit_proj_workspace_bytes(c["radem"].shape[2], k["nvar"], slab_rows)
    short = torch.empty(need - 1, dtype=torch.uint8, device=DEV)
    outs = [torch.zeros(shape, dtype=F64, device=DEV) for shape in ((n, L, V, K), (n, L, K), (n, L + 1, V, K))]
    dev = {key: torch.from_numpy(c[key]).to(DEV) for key in ("tokens", "table", "radem", "chi")}
    pmd = torch.from_numpy(pm).to(DEV)
    bs = [torch.from_numpy(np.ascontiguousarray(b[j])).to(DEV) for j in range(3)]
    tail = (dev["radem"], dev["chi"], c["seqlen"], k["cw"], k["scaling"], k["icpt"])
    with pytest.raises(RuntimeError, match="workspace too small"):
        ext.hipConvTokenSubstProj(dev["tokens"], dev["table"], pmd, bs[0], outs[0], *tail, slab_rows=slab_rows, workspace=short)
    with pytest.raises(RuntimeError, match="workspace too small"):
        ext.hipConvTokenIndelProj(dev["tokens"], dev["table"], pmd, bs[1], bs[2], outs[1], outs[2], *tail, slab_rows=slab_rows, workspace=short)
    assert all(float(o.abs().max()) == 0.0 for o in outs)
