#!/usr/bin/env python3
"""Solver passes on float32 feature rows beyond padded width 4096 (no fused kernel there): 131 072 rows, 8192 RFFs,
d = 5000 / 9000 (padded width 8192 on wave tiles, 16384 on the any-width path).  Per shape: the cache build, one CG matvec
from the resident cache, from regenerated windows and on the float64 route (SORFKernel.rows_ok switched off: float64 Z
materialised chunk by chunk + library GEMMs), z^T y, the k = 26 matvec, the rank-512 preconditioner build and a checksum.
Timing as bench.py's wide_probe (events around repeated calls after one warm-up call; the preconditioner build: the second
of two, host clock).

    python tools/bench_wide_rows.py [out.json]          (default profiles/wide_rows.json)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ev_ms(fn, reps=5):
    import torch
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    import numpy as np
    import torch
    from xgpr_amd.kernels import make_kernel, padded_dims, SORFKernel
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.cg import ConjugateGrad, calc_zty
    from xgpr_amd.preconditioner import RandNysPreconditioner
    out_file = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "wide_rows.json")
    device = torch.device("cuda", 0)
    rows, m = 131072, 8192
    res = {"rows": rows, "num_rffs": m, "device": torch.cuda.get_device_name(device), "shapes": []}
    g = torch.Generator(device=device).manual_seed(7)
    for d in (5000, 9000):
        x = torch.randn(rows, d, device=device, generator=g) / d ** 0.5
        y = torch.randn(rows, dtype=torch.float64, device=device, generator=g)
        kern = make_kernel("RBF", (rows, d), m, 123, device, {})
        kern.set_hyperparams(np.array([0.1, 1.0]), logspace=False)
        assert kern.rows_ok() and kern.cache_ok() and kern.block_ok() and not kern.fused_ok()
        ds = build_regression_dataset(x, y, chunk_size=16384, device=device)
        xs = ds.scaled_x(kern.hyperparams[1])
        zc = torch.empty((rows, m), dtype=torch.float32, device=device)
        build = ev_ms(lambda: kern.fill_feature_cache(xs, zc), reps=3)
        del zc
        vec = torch.randn(m, 1, dtype=torch.float64, device=device, generator=g)
        v1 = vec[:, 0].contiguous()
        vec26 = torch.randn(m, 26, dtype=torch.float64, device=device, generator=g)
        w1 = torch.zeros(m, dtype=torch.float64, device=device)
        w26 = torch.zeros((m, 26), dtype=torch.float64, device=device)
        # regenerated windows first (the dataset holds no cache yet)
        cgw = ConjugateGrad(cache_features=False)
        mv_win = ev_ms(lambda: cgw._ztz(ds, kern, v1, w1))
        chk_win = float(w1.sum())
        zty_win = ev_ms(lambda: calc_zty(ds, kern), reps=3)
        k26_win = ev_ms(lambda: cgw._matvec(ds, kern, vec26, w26, add_ridge=False), reps=3)
        RandNysPreconditioner(kern, ds, 512, False, 123, "srht")      # warm-up: library set-up and workspaces are not the build
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pre = RandNysPreconditioner(kern, ds, 512, False, 123, "srht")
        torch.cuda.synchronize()
        t_pre = time.perf_counter() - t0
        cgc = ConjugateGrad(cache_features=True)
        ds.feature_cache(kern)
        mv_res = ev_ms(lambda: cgc._ztz(ds, kern, v1, w1))
        chk_res = float(w1.sum())
        zty_res = ev_ms(lambda: calc_zty(ds, kern), reps=3)
        k26_res = ev_ms(lambda: cgc._matvec(ds, kern, vec26, w26, add_ridge=False), reps=3)
        chk_k26 = float(w26.sum())
        ds._zcache = None
        ds._zcache_key = None
        # the float64 route: Z materialised chunk by chunk (what the reference does, and this tree did before)
        rows_ok = SORFKernel.rows_ok
        SORFKernel.rows_ok = lambda self: False
        try:
            assert not kern.cache_ok() and not kern.block_ok()
            wf = torch.zeros((m, 1), dtype=torch.float64, device=device)
            mv_f64 = ev_ms(lambda: ConjugateGrad(cache_features=False)._matvec(ds, kern, vec, wf, add_ridge=False), reps=2)
            chk_f64 = float(wf.sum())
            zty_f64 = ev_ms(lambda: calc_zty(ds, kern), reps=2)
        finally:
            SORFKernel.rows_ok = rows_ok
        zty_res_v = calc_zty(ds, kern)[0]
        P = padded_dims(d)
        res["shapes"].append({
            "d": d, "padded_width": P, "cache_plan": "wave tiles" if P == 8192 else "any-width path",
            "cache_build_ms": build, "cache_build_GBs": (4.0 * d + 4.0 * m) * rows / (build * 1e-3) / 1e9,
            "matvec_resident_ms": mv_res, "matvec_resident_GBs": 4.0 * m * rows / (mv_res * 1e-3) / 1e9,
            "matvec_windows_ms": mv_win, "matvec_float64_route_ms": mv_f64,
            "zty_windows_ms": zty_win, "zty_resident_ms": zty_res, "zty_float64_route_ms": zty_f64,
            "k26_matvec_resident_ms": k26_res, "k26_matvec_windows_ms": k26_win,
            "precond_rank512_build_s": t_pre, "precond_achieved_ratio": float(pre.achieved_ratio),
            "checksum": {"matvec_resident": chk_res, "matvec_windows": chk_win, "matvec_float64_route": chk_f64,
                         "k26_matvec": chk_k26, "zty": float(zty_res_v.sum())},
        })
        print(json.dumps(res["shapes"][-1]), flush=True)
        del x, xs, ds, pre
        torch.cuda.empty_cache()
    with open(out_file, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_file)


if __name__ == "__main__":
    main()
