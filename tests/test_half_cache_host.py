"""CPU-only checks of the binary16 feature cache (cache_features="half"): the three C entry points are declared, exported and
bound; their launchers' validation (code, message, order) without a device, as tests/test_launcher_validation_host.py does it;
the mode's resolution on stub kernel / dataset objects; the refusal of the mode by the paths that do not serve it; and the
compiler's resource figures of the new kernels."""
import os
import re
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("xgpr_rows_pack_f16", "xgpr_zcache_matvec_f16", "xgpr_zcache_matvec_scaled_f16")
A = 0x100000                     # a dummy 4096-byte-aligned address, never dereferenced before validation fails
BIG = 1 << 30
NO_DATAPOINTS, ODD_OUTPUT, ARRAY_DIMS, UNSUPPORTED, WORKSPACE = -1, -2, -8, -20, -21


def test_symbols_are_declared_exported_and_bound():
    from xgpr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "xgpr_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert name in doc
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    for fn in ("RowsToHalf", "ZCacheMatvecHalf", "ZCacheMatvecHalfScaled"):
        assert getattr(ext, "cuda" + fn) is getattr(ext, "hip" + fn)
    assert ext.half_cache_ok(8192) and ext.half_cache_ok(1) and not ext.half_cache_ok(8193)


def zmv(zc=A, v=A, w=A, n=4, m=128, icpt=0, ws=A, wb=BIG):
    return "xgpr_zcache_matvec_f16", (zc, v, w, n, m, icpt, ws, wb, None)


def zmvs(zc=A, v=A, w=A, n=4, m=128, scale=0.1, ws=A, wb=BIG):
    return "xgpr_zcache_matvec_scaled_f16", (zc, v, w, n, m, scale, ws, wb, None)


def pack(rows=A, out=A, count=64):
    return "xgpr_rows_pack_f16", (rows, out, count, None)


WIDTH = "cached matvec over binary16 rows supports num_freqs <= 8192"
ALIGN = "vector pointers must be 16-byte aligned, the binary16 cache 4-byte aligned"
WS = "workspace too small (see xgpr_ztz_matvec_workspace_bytes)"
PACK_ALIGN = "float32 rows must be 16-byte aligned and binary16 rows 8-byte aligned"

# the order of zcache_matvec_impl: no datapoints, odd output, unsupported width, alignment, workspace
CASES = {
    "n == 0": (zmv(n=0), (NO_DATAPOINTS, "no datapoints")),
    "odd num_rffs": (zmv(m=127), (ODD_OUTPUT, "last dim of output must be even number")),
    "num_rffs < 2": (zmv(m=0), (ODD_OUTPUT, "last dim of output must be even number")),
    "num_freqs 8193": (zmv(m=2 * 8193), (UNSUPPORTED, WIDTH)),
    "num_freqs 8192 passes the width check": (zmv(m=2 * 8192, v=A + 8), (WORKSPACE, ALIGN)),
    "misaligned v": (zmv(v=A + 8), (WORKSPACE, ALIGN)),
    "misaligned w": (zmv(w=A + 8), (WORKSPACE, ALIGN)),
    "cache 2 bytes off": (zmv(zc=A + 2), (WORKSPACE, ALIGN)),
    "cache 4 bytes off passes, no workspace": (zmv(zc=A + 4, ws=None, wb=0), (WORKSPACE, WS)),
    "no workspace": (zmv(ws=None, wb=0), (WORKSPACE, WS)),
    "short workspace": (zmv(wb=4096), (WORKSPACE, WS)),
    "workspace 8 bytes off": (zmv(ws=A + 8), (WORKSPACE, WS)),
    "n == 0 and odd num_rffs": (zmv(n=0, m=127), (NO_DATAPOINTS, "no datapoints")),
    "odd num_rffs and misaligned v": (zmv(m=127, v=A + 8), (ODD_OUTPUT, "last dim of output must be even number")),
    "num_freqs 8193 and misaligned w": (zmv(m=2 * 8193, w=A + 8), (UNSUPPORTED, WIDTH)),
    "misaligned cache and no workspace": (zmv(zc=A + 2, ws=None, wb=0), (WORKSPACE, ALIGN)),
    "scaled: scale 0": (zmvs(scale=0.0), (ARRAY_DIMS, "scale must be positive")),
    "scaled: scale 0 and n == 0": (zmvs(scale=0.0, n=0), (ARRAY_DIMS, "scale must be positive")),
    "scaled: n == 0": (zmvs(n=0), (NO_DATAPOINTS, "no datapoints")),
    "scaled: num_freqs 8193": (zmvs(m=2 * 8193), (UNSUPPORTED, WIDTH)),
    "scaled: short workspace": (zmvs(wb=4096), (WORKSPACE, WS)),
    "pack: count 0": (pack(count=0), (NO_DATAPOINTS, "no datapoints")),
    "pack: rows 8 bytes off": (pack(rows=A + 8), (WORKSPACE, PACK_ALIGN)),
    "pack: out 4 bytes off": (pack(out=A + 4), (WORKSPACE, PACK_ALIGN)),
    "pack: count 0 and misaligned": (pack(count=0, out=A + 4), (NO_DATAPOINTS, "no datapoints")),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_launcher_validation(name):
    from xgpr_amd import _lib
    (fn, args), expected = CASES[name]
    rc = getattr(_lib.load(), fn)(*args)
    assert (int(rc), _lib.last_error()) == expected


class _Kernel:
    device = "cpu"

    def __init__(self, half):
        if half is not None:
            self.half_cache_ok = lambda: half


class _Dataset:
    def feature_cache_f16(self, kernel):
        raise AssertionError("resolving the mode builds nothing")


def test_resolve_cache_mode_half():
    from xgpr_amd.cg import _resolve_cache_mode, ConjugateGrad
    assert _resolve_cache_mode("half", _Kernel(True), _Dataset()) == "half"
    as_true = _resolve_cache_mode(True, _Kernel(True), _Dataset())
    assert as_true is True
    # the unsupported request is answered exactly as True is: a kernel that says no, a kernel class without the method, a
    # dataset class without the binary16 cache
    for kernel, dataset in ((_Kernel(False), _Dataset()), (_Kernel(None), _Dataset()), (_Kernel(True), object())):
        got = _resolve_cache_mode("half", kernel, dataset)
        assert got is as_true
    # the answers for the other requests are what they were
    assert _resolve_cache_mode(False, _Kernel(True), _Dataset()) is False
    assert _resolve_cache_mode("auto", _Kernel(True), _Dataset()) is False      # no cache_ok on the stub
    half, full, off = ConjugateGrad(cache_features="half"), ConjugateGrad(cache_features=True), ConjugateGrad()
    assert half._half and not half._wants_f32_cache
    assert not full._half and full._wants_f32_cache
    assert not off._half and not off._wants_f32_cache

    class _Cached:
        def cache_ok(self):
            return True
    # half mode never asks for the float32 cache; True still does
    assert not half._use_cache(_Cached(), None) and full._use_cache(_Cached(), None) and not off._use_cache(_Cached(), None)


def test_paths_that_do_not_serve_half_say_so():
    from xgpr_amd.cg import _resolve_cache_mode
    from xgpr_amd.models import xGPClassification
    from xgpr_amd import nmll
    with pytest.raises(ValueError, match="half"):
        xGPClassification(num_rffs=64, device="cpu", verbose=False).fit(None, cache_features="half")
    with pytest.raises(ValueError, match="half"):
        nmll.approximate_nmll(_Kernel(True), _Dataset(), cache_features="half")
    with pytest.raises(ValueError, match="half"):
        _resolve_cache_mode("half", _Kernel(True), _Dataset(), block=True)


def test_new_kernels_use_no_scratch_and_keep_their_occupancy():
    """rows_pack_f16_kernel and every instantiation of zcache16_ztz_kernel: no scratch, no spilled VGPR, and a register-limited
    occupancy of at least the two waves per SIMD of __launch_bounds__(512, 2) -- the launcher puts one 8-wave workgroup on a
    CU."""
    import resource_usage
    rows = [r for r in resource_usage.collect() if r["name"].startswith(("zcache16_ztz_kernel", "rows_pack_f16_kernel"))]
    names = {r["name"].split("<")[0] for r in rows}
    assert names == {"zcache16_ztz_kernel", "rows_pack_f16_kernel"}
    assert len(rows) >= 4                                    # the packer and the three load widths
    for r in rows:
        assert r.get("ScratchSize", 0) == 0, r
        assert r.get("VGPRs Spill", 0) == 0, r
        bound = 2 if r["name"].startswith("zcache16") else 1
        assert r["Occupancy"] >= bound, r
