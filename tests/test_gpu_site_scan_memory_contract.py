"""The memory contract of the writer of include/xgpr_hip/site_scan.h, in the pattern of tests/test_gpu_pair_scan_memory_contract.py:
it runs once the plain way and once with every array it sees -- tokens, table, w, radem, chi, the device copy of the lengths, the
output and the workspace, exactly the bytes xgpr_conv_token_site_scan_workspace_bytes advertises (the packed sign masks and one
double per sequence and possible run), 0xFF-poisoned -- inside the guarded arena of tests/guarded.py.  No guard band may change (no
write outside out and the workspace: the third kernel works in place on out), no input may be modified, and both runs must agree
bit for bit (the workspace's contents do not enter: the saved parent sums are written before they are read).  The tokens past a
sequence's length are 255, a row the table does not have: one that was read would gather from beyond the table."""
import pytest
import torch

import dense_site_scan as ds
from guarded import Arena, Plain, patched_workspaces, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64

COVERED = {"xgpr_conv_token_site_scan_f32"}
SHAPES = ["w16_c4_cw3", "w128_c21_cw6", "w1024_c120_cw8", "g4_cw9", "two_components", "vocab256_c5", "n65"]


def covered_entry_points():
    return set(COVERED)


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext as e
    return e


def site_scan(ext, A, name):
    c, sites, cw, scaling, icpt = ds.case(name)
    n, L = c["tokens"].shape
    V = c["table"].shape[0]
    out = A.out((n, ds.run_offsets(ds.site_runs(sites, L, cw), V)[1]), F64, name="out")
    need = int(ext._LIB.xgpr_conv_token_site_scan_workspace_bytes(c["radem"].shape[2], n, len(sites)))
    ws = A.workspace(need, name="internal workspace")
    dev = {k: A.inp(torch.from_numpy(c[k]), name=k) for k in ("tokens", "table", "w", "radem", "chi")}
    ext.hipConvTokenSiteScan(dev["tokens"], dev["table"], dev["w"], out, dev["radem"], dev["chi"], c["seqlen"], sites, cw, scaling, icpt,
                             workspace=ws)
    return out, need


@pytest.mark.parametrize("name", SHAPES)
def test_memory_contract(ext, name, monkeypatch):
    plain, _ = site_scan(ext, Plain(DEV), name)
    arena = Arena(DEV)
    patched_workspaces(monkeypatch, ext, arena)              # (the device copy of the lengths becomes a guarded input)
    guarded, need = site_scan(ext, arena, name)
    arena.verify()
    names = {r.name.split("#")[0] for r in arena.records}
    assert names == {"out", "internal workspace", "tokens", "table", "w", "radem", "chi", "device sequence lengths"}
    ws = next(r for r in arena.records if r.name == "internal workspace")
    assert ws.end - ws.start == need > int(ext._LIB.xgpr_rbf_workspace_bytes(ds.case(name)[0]["radem"].shape[2]))   # exactly what is advertised
    assert same_bits(plain, guarded), "the guarded run differs from the plain run"
    assert bool(torch.isfinite(plain).all()) and float(plain.abs().max()) > 0


def test_a_workspace_one_byte_short_is_refused(ext):
    c, sites, cw, scaling, icpt = ds.case("w16_c4_cw3")
    n, L = c["tokens"].shape
    V = c["table"].shape[0]
    need = int(ext._LIB.xgpr_conv_token_site_scan_workspace_bytes(c["radem"].shape[2], n, len(sites)))
    out = torch.zeros((n, ds.run_offsets(ds.site_runs(sites, L, cw), V)[1]), dtype=F64, device=DEV)
    short = torch.empty(need - 1, dtype=torch.uint8, device=DEV)
    dev = {k: torch.from_numpy(c[k]).to(DEV) for k in ("tokens", "table", "w", "radem", "chi")}
    with pytest.raises(RuntimeError, match="workspace too small"):
        ext.hipConvTokenSiteScan(dev["tokens"], dev["table"], dev["w"], out, dev["radem"], dev["chi"], c["seqlen"], sites, cw, scaling, icpt,
                                 workspace=short)
    assert float(out.abs().max()) == 0.0
