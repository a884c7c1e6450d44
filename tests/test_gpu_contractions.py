"""Every arm of the float64 matrix-core contractions over float32 feature rows -- the block kernels (zblock.inc), the three
sketch_gemm kernels, gram.inc and cross_gram.inc -- through the Python surface, against tests/dense_contractions.py:

  * the EXACT leg on every case: inputs whose products and partial sums are all representable, so the result must equal the
    numpy float64 product bit for bit -- payload, padding columns and the guard elements around the output; the same for an
    accumulating call from exact start values, and a repeat of the call must give the same bits;
  * the ROUNDED leg on the listed subsets: uniform rows, the default scale, against a longdouble product entry by entry
    under the derived cap (the largest error / cap per kernel family goes to profiles/contraction_errors.txt: a record, the
    bar is the cap);
  * the arm model of the helper against the workspace sizes the library reports, for every case, with the device's CU count,
    and the set of arms the tables launch on this device against every arm the model knows.

Outputs start from a sentinel, workspaces are exactly the advertised bytes, poisoned with 0xFF, with 4 KiB of 0xFF behind them
that must stay.  The row-tile counts 2 and 4 of the block T kernel are forced with XGPR_ZB_RT, which the library reads once
per process: one fresh child process per value, one after the other."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dense_contractions as dc

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("matvec", "project", "backproject")
WS_GUARD = 4096
RATIOS = {}                      # kernel family -> largest measured error / cap of the rounded leg
LAUNCHED = set()                 # arms of the cases this session ran (device CU count)
FAMILIES = ("block_matvec", "block_project", "block_backproject", "block_matvec_forced_rt", "block_project_forced_rt",
            "block_backproject_forced_rt", "sketch_direct", "sketch_lds", "sketch_lds_bt", "gram", "cross_gram")


@pytest.fixture(scope="module")
def ext():
    from xgpr_amd import xgpr_hip_rfgen_ext
    return xgpr_hip_rfgen_ext


def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ------------------------------------------------------------------------------------------------ device arrays
def dev_out(rows, ld, init=None):
    """-> (flat buffer, [rows, ld] view): SENTINEL everywhere, dc.GUARD elements around the view (16-byte aligned)."""
    buf = torch.full((2 * dc.GUARD + rows * ld,), dc.SENTINEL, dtype=torch.float64, device=DEV)
    view = buf[dc.GUARD:dc.GUARD + rows * ld].view(rows, ld)
    if init is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(init)))
    return buf, view


def split_guards(flat, rows, ld):
    """The host copy of a dev_out buffer -> its [rows, ld] array, after checking the guards."""
    flat = np.asarray(flat)
    assert flat.shape == (2 * dc.GUARD + rows * ld,)
    assert np.all(flat[:dc.GUARD] == dc.SENTINEL) and np.all(flat[dc.GUARD + rows * ld:] == dc.SENTINEL), "a guard element changed"
    return flat[dc.GUARD:dc.GUARD + rows * ld].reshape(rows, ld)


class Workspace:
    """Exactly ``need`` bytes of 0xFF with WS_GUARD more behind them."""

    def __init__(self, need):
        self.need = int(need)
        self.buf = torch.full((self.need + WS_GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        self.view = self.buf[:self.need]

    def intact(self):
        return bool((self.buf[self.need:] == 0xFF).all())


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def record(family, ratio):
    RATIOS[family] = max(RATIOS.get(family, 0.0), float(ratio))
    print(f"CONTRACTION {family:<28} error / cap {ratio:.4f}")
    if all(f in RATIOS for f in FAMILIES):
        lines = ["# tests/test_gpu_contractions.py: the rounded leg against the long-double reference, largest measured error / derived cap\n"]
        lines += [f"{f:<28} ratio {RATIOS[f]:.4f}\n" for f in FAMILIES]
        try:
            with open(os.path.join(ROOT, "profiles", "contraction_errors.txt"), "w") as f:
                f.writelines(lines)
        except OSError:                                    # a read-only checkout: the CONTRACTION lines above say the same
            pass


# ------------------------------------------------------------------------------------------------ block kernels
def run_block(ext, case, exact=True):
    """Launches the three modes of one case -> host arrays (whole guarded buffers) and what the library reports."""
    from xgpr_amd import _lib
    n, M, k = case.n, case.M, case.k
    got = {"ws_bytes": np.int64(ext.zcache_block_workspace_bytes(n, M, k)),
           "proj_ws_bytes": np.int64(ext.zcache_block_project_workspace_bytes(n, M, k))}
    ws_ok = True
    for mode in MODES:
        zc, op, scale, c0 = dc.make_block(case, mode, exact)
        zc_d, op_d = up(zc), up(op)
        rows = n if mode == "project" else M
        sc = scale if exact else 0.0                       # the rounded leg runs the library's default scale

        def call(view, accumulate=False, workspace="need"):
            nonlocal ws_ok
            if mode == "project":
                if workspace is None:                      # the unsplit kernel: no workspace at the C ABI
                    _lib.check(_lib.load().xgpr_zcache_block_project_f32(
                        C.c_void_p(zc_d.data_ptr()), C.c_void_p(op_d.data_ptr()), C.c_void_p(view.data_ptr()), n, M, k,
                        int(case.icpt), float(sc), None, C.c_size_t(0), None))
                    return
                ws = Workspace(int(got["proj_ws_bytes"]))
                ext.hipZCacheBlockProject(zc_d, op_d, view, case.icpt, sc, ws.view if ws.need else None)
            else:
                ws = Workspace(int(got["ws_bytes"]))
                fn = ext.hipZCacheBlockMatvec if mode == "matvec" else ext.hipZCacheBlockBackproject
                fn(zc_d, op_d, view, case.icpt, ws.view, sc, accumulate)
            torch.cuda.synchronize()
            ws_ok = ws_ok and ws.intact()

        buf, view = dev_out(rows, k)
        call(view)
        got[mode] = buf.cpu().numpy()
        buf2, view2 = dev_out(rows, k)
        call(view2)
        got[mode + "_same"] = np.bool_(torch.equal(buf, buf2))
        if not exact:
            continue
        if mode != "project":
            buf3, view3 = dev_out(rows, k, c0)
            call(view3, accumulate=True)
            got[mode + "_acc"] = buf3.cpu().numpy()
        elif int(got["proj_ws_bytes"]):
            buf3, view3 = dev_out(rows, k)
            call(view3, workspace=None)
            got["project_unsplit"] = buf3.cpu().numpy()
    got["ws_ok"] = np.bool_(ws_ok)
    return got


def check_block(case, got, ncus, exact=True, family_suffix=""):
    n, M, k = case.n, case.M, case.k
    g = dc.zb_model(n, M, k, ncus, case.rt)
    assert int(got["proj_ws_bytes"]) == g["project_ws_bytes"], (case, "model: msplit / kp", g)
    assert int(got["ws_bytes"]) == g["block_ws_bytes"], (case, "model: nrb / kp / msplit", g)
    assert bool(got["ws_ok"]), (case, "bytes behind a workspace changed")
    LAUNCHED.update(dc.zb_arms(case, ncus))
    for mode in MODES:
        zc, op, scale, c0 = dc.make_block(case, mode, exact)
        rows = n if mode == "project" else M
        assert bool(got[mode + "_same"]), (case, mode, "a second call gave other bits")
        out = split_guards(got[mode], rows, k)
        if not exact:
            ref = dc.ref_block(mode, zc, op, case, scale, dtype=dc.LD, cus=ncus)
            ratio = dc.worst_ratio(ref, out, dc.cap_block(mode, zc, op, case, scale))
            record(f"block_{mode}{family_suffix}", ratio)
            assert ratio <= 1.0, (case, mode, ratio)
            continue
        assert np.array_equal(out, dc.ref_block(mode, zc, op, case, scale, cus=ncus)), (case, mode)
        if mode != "project":
            acc = split_guards(got[mode + "_acc"], rows, k)
            assert np.array_equal(acc, dc.ref_block(mode, zc, op, case, scale, c0=c0, accumulate=True, cus=ncus)), (case, mode, "accumulate")
        elif g["msplit"] > 1:
            assert np.array_equal(split_guards(got["project_unsplit"], rows, k), out), (case, "unsplit projection")


def column_cases(col):
    return [c for c in dc.block_cases(1) if dc.column_arm(c.k) == col and c.n < 40000]


@pytest.mark.parametrize("col", dc.COLUMN_ARMS)
def test_block_kernels_exact_one_row_tile(ext, col):
    """RT = 1 (every n below the size thresholds): both ends of the column arm x every n x every M, three modes."""
    for case in column_cases(col):
        check_block(case, run_block(ext, case), cus())


@pytest.mark.parametrize("n,M,k", dc.BLOCK_LONG + (dc.BLOCK_BY_SIZE,))
def test_block_kernels_exact_long_ranges_and_row_tiles_by_size(ext, n, M, k):
    """W ranges of three and seven chunks; 131072 + 129 rows: two row tiles per wave by size, the last tile ragged, k = 22."""
    case = next(c for c in dc.block_cases(1) if (c.n, c.M, c.k) == (n, M, k))
    check_block(case, run_block(ext, case), cus())


def test_block_kernels_rounded(ext):
    for case in dc.BLOCK_ROUNDED:
        check_block(case, run_block(ext, case, exact=False), cus(), exact=False)


def run_block_table(ext, rt):
    """What a forced-RT child computes: its whole table, exact leg + the rounded subset, as one flat dict."""
    out = {}
    for i, case in enumerate(dc.block_cases(rt)):
        out.update({f"e{i}.{key}": v for key, v in run_block(ext, case).items()})
    for i, case in enumerate(c for c in dc.BLOCK_ROUNDED_FORCED if c.rt == rt):
        out.update({f"r{i}.{key}": v for key, v in run_block(ext, case, exact=False).items()})
    return out


CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import test_gpu_contractions as t
from xgpr_amd import xgpr_hip_rfgen_ext as ext
np.savez(sys.argv[1], **t.run_block_table(ext, int(sys.argv[2])))
"""


def test_block_kernels_forced_row_tiles(tmp_path):
    """RT = 2 and RT = 4 of zblock_t_kernel at every column arm, n around one and three row tiles: one child process per
    value (the switch is read once per process), one at a time; a child that fails ends the test."""
    ncus = cus()
    code = CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    for rt in (2, 4):
        env = dict(os.environ)
        env["XGPR_ZB_RT"] = str(rt)
        path = str(tmp_path / f"rt{rt}.npz")
        res = subprocess.run([sys.executable, "-c", code, path, str(rt)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr[-3000:]
        data = np.load(path)
        keys = {}
        for name in data.files:
            keys.setdefault(name.split(".", 1)[0], []).append(name)
        for i, case in enumerate(dc.block_cases(rt)):
            assert dc.zb_model(case.n, case.M, case.k, ncus, case.rt)["rt"] == rt
            check_block(case, {name.split(".", 1)[1]: data[name] for name in keys[f"e{i}"]}, ncus)
        for i, case in enumerate(c for c in dc.BLOCK_ROUNDED_FORCED if c.rt == rt):
            check_block(case, {name.split(".", 1)[1]: data[name] for name in keys[f"r{i}"]}, ncus, exact=False,
                        family_suffix="_forced_rt")
        data.close()
        os.remove(path)


# ------------------------------------------------------------------------------------------------ sketch gemm
def run_sketch(ext, case, exact=True):
    zc, a, scale = dc.make_sketch(case, exact)
    zc_d, a_d = up(zc), up(a)
    sc = scale if exact else 0.0
    j = case.n if case.bt else case.m
    kdim = case.m if case.bt else case.n
    got = {}
    for trans in (False, True):
        ldc = dc.sketch_ldc(case, trans)
        rows = j if trans else case.r
        need = ext.sketch_gemm_workspace_bytes(case.r, j, kdim, ldc, trans)
        got[f"ws_bytes_{int(trans)}"] = need
        ok = True

        def call(view, accumulate=False):
            nonlocal ok
            ws = Workspace(need)
            ext.hipSketchGemm(a_d, zc_d, view, case.r, case.bt, trans, case.icpt, sc, accumulate, ws.view)
            torch.cuda.synchronize()
            ok = ok and ws.intact()

        buf, view = dev_out(rows, ldc)
        call(view)
        got[f"out_{int(trans)}"] = buf.cpu().numpy()
        buf2, view2 = dev_out(rows, ldc)
        call(view2)
        got[f"same_{int(trans)}"] = torch.equal(buf, buf2)
        if exact:
            buf3, view3 = dev_out(rows, ldc, dc.sketch_start(case, trans))
            call(view3, accumulate=True)
            got[f"acc_{int(trans)}"] = buf3.cpu().numpy()
        got[f"ws_ok_{int(trans)}"] = ok
    return zc, a, scale, got


def check_sketch(case, zc, a, scale, got, ncus, exact=True):
    j = case.n if case.bt else case.m
    for trans in (False, True):
        t = int(trans)
        ldc = dc.sketch_ldc(case, trans)
        rows = j if trans else case.r
        g = dc.sk_model(case.n, case.m, case.r, case.pad, case.bt, trans, ldc, ncus)
        assert got[f"ws_bytes_{t}"] == g["ws_bytes"], (case, trans, "model: nsplit", g)
        assert got[f"ws_ok_{t}"], (case, trans, "bytes behind the workspace changed")
        assert got[f"same_{t}"], (case, trans, "a second call gave other bits")
        LAUNCHED.update(dc.sk_arms(case, trans, ncus))
        out = split_guards(got[f"out_{t}"], rows, ldc)
        if not exact:
            ref = dc.ref_sketch(a, zc, case, trans, scale, dtype=dc.LD, cus=ncus)
            ratio = dc.worst_ratio(ref, out, dc.cap_sketch(a, zc, case, trans, scale))
            record(f"sketch_{g['kernel']}", ratio)
            assert ratio <= 1.0, (case, trans, ratio)
            continue
        assert np.array_equal(out, dc.ref_sketch(a, zc, case, trans, scale, cus=ncus)), (case, trans)
        acc = split_guards(got[f"acc_{t}"], rows, ldc)
        want = dc.ref_sketch(a, zc, case, trans, scale, c0=dc.sketch_start(case, trans), accumulate=True, cus=ncus)
        assert np.array_equal(acc, want), (case, trans, "accumulate")


@pytest.mark.parametrize("name", [c.name for c in dc.SKETCH_CASES])
def test_sketch_gemm_exact(ext, name):
    """Both stores, with and without accumulate: the named edges, tile maps of several blocks, the K % 16 recursion, a last
    range below 16 contraction indices."""
    case = next(c for c in dc.SKETCH_CASES if c.name == name)
    zc, a, scale, got = run_sketch(ext, case)
    check_sketch(case, zc, a, scale, got, cus())


def test_sketch_gemm_rounded(ext):
    for name in dc.SKETCH_ROUNDED:
        case = next(c for c in dc.SKETCH_CASES if c.name == name)
        zc, a, scale, got = run_sketch(ext, case, exact=False)
        check_sketch(case, zc, a, scale, got, cus(), exact=False)


# ------------------------------------------------------------------------------------------------ gram and cross gram
def run_gram(ext, case, exact=True):
    """One case of hipZtZGram (GramCase) or hipCrossGram (CrossCase) -> inputs and host copies."""
    cross = isinstance(case, dc.CrossCase)
    msub = case.M if cross else case.msub
    ld = msub + case.ldpad
    if cross:
        a, b = dc.make_cross(case, exact)
        ins, dev = (a, b), (up(a), up(b))
        need = int(ext._LIB.xgpr_cross_gram_workspace_bytes(case.M, case.n))
    else:
        zc, scale = dc.make_gram(case, exact)
        ins, dev = (zc, scale), (up(zc),)
        need = int(ext._LIB.xgpr_ztz_gram_workspace_bytes(case.msub, case.n))
    got = {"ws_bytes": need, "ws_ok": True}

    def call(view, accumulate=False):
        ws = Workspace(need)
        if cross:
            ext.hipCrossGram(dev[0], dev[1], view, accumulate, ws.view)
        else:
            ext.hipZtZGram(dev[0], view, case.icpt, ins[1] if exact else 0.0, accumulate, ws.view)
        torch.cuda.synchronize()
        got["ws_ok"] = got["ws_ok"] and ws.intact()

    buf, view = dev_out(msub, ld)
    call(view)
    got["out"] = buf.cpu().numpy()
    buf2, view2 = dev_out(msub, ld)
    call(view2)
    got["same"] = torch.equal(buf, buf2)
    if exact:
        buf3, view3 = dev_out(msub, ld, dc.gram_start(msub, case.ldpad, case.n))
        call(view3, accumulate=True)
        got["acc"] = buf3.cpu().numpy()
    return ins, got


def check_gram(case, ins, got, ncus, exact=True):
    cross = isinstance(case, dc.CrossCase)
    msub = case.M if cross else case.msub
    ld = msub + case.ldpad
    g = dc.gram_model(msub, case.n, ncus, cross)
    assert got["ws_bytes"] == g["ws_bytes"], (case, "model: workgroups", g)
    assert got["ws_ok"] and got["same"], case
    LAUNCHED.update(dc.gram_arms(case, ncus))
    out = split_guards(got["out"], msub, ld)
    assert np.array_equal(out[:, :msub], out[:, :msub].T), (case, "not symmetric bit for bit")
    ref_fn = (lambda **kw: dc.ref_cross(ins[0], ins[1], case, cus=ncus, **kw)) if cross else \
             (lambda **kw: dc.ref_gram(ins[0], case, ins[1], cus=ncus, **kw))
    if not exact:
        cap = dc.cap_cross(ins[0], ins[1], case) if cross else dc.cap_gram(ins[0], case, ins[1])
        ratio = dc.worst_ratio(ref_fn(dtype=dc.LD), out, cap)
        record("cross_gram" if cross else "gram", ratio)
        assert ratio <= 1.0, (case, ratio)
        return
    assert np.array_equal(out, ref_fn()), case
    acc = split_guards(got["acc"], msub, ld)
    assert np.array_equal(acc, ref_fn(c0=dc.gram_start(msub, case.ldpad, case.n), accumulate=True)), (case, "accumulate")


@pytest.mark.parametrize("case", dc.GRAM_CASES, ids=lambda c: f"n{c.n}_m{c.m}_msub{c.msub}_pad{c.ldpad}_i{int(c.icpt)}")
def test_gram_exact(ext, case):
    ins, got = run_gram(ext, case)
    check_gram(case, ins, got, cus())


@pytest.mark.parametrize("case", dc.CROSS_CASES, ids=lambda c: f"n{c.n}_M{c.M}_pad{c.ldpad}")
def test_cross_gram_exact(ext, case):
    """Two different row arrays: A^T B alone is not symmetric, the sum is -- bit for bit."""
    ins, got = run_gram(ext, case)
    check_gram(case, ins, got, cus())


def test_gram_and_cross_gram_rounded(ext):
    for case in dc.GRAM_ROUNDED + dc.CROSS_ROUNDED:
        ins, got = run_gram(ext, case, exact=False)
        check_gram(case, ins, got, cus(), exact=False)


# ------------------------------------------------------------------------------------------------ coverage
def test_the_tables_cover_every_arm_on_this_device():
    """With the device's CU count (the thresholds, the tile map and the range counts depend on it): every arm the model knows
    is launched by a case of the tables above -- each test runs its whole table, none skips --, and what this session
    launched is part of it.  On a part where a shape lands in another arm, this fails and names the arm."""
    ncus = cus()
    covered, want = dc.covered_arms(ncus), dc.all_arms()
    missing, unlisted = want - covered, covered - dc.ARMS_ELSEWHERE - want
    assert not missing and not unlisted, (f"{ncus} CUs: arms never launched: {sorted(map(str, missing))}; "
                                          f"arms the model does not list: {sorted(map(str, unlisted))}")
    assert LAUNCHED <= covered, sorted(map(str, LAUNCHED - covered))
