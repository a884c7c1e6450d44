#!/usr/bin/env python3
"""The streaming CG matvec over the resident feature cache, float32 rows (hipZCacheMatvec, the yardstick) against IEEE binary16
rows (hipZCacheMatvecHalf, cache_features="half"), at the shapes the mode is for:

    cfg3        RBF, d = 1024, M = 8192, 1 000 000 rows      (BASELINE configs[2], one GPU)
    cfg3_shard  RBF, d = 1024, M = 8192,   125 000 rows      (its share of 8 GPUs)
    wide        RBF, d = 1024, M = 16384,  250 000 rows      (num_freqs = 8192: the widest row the binary16 stream serves)

    python tools/bench_half_cache.py [--shapes cfg3,cfg3_shard,wide] [--rounds 7] [--inner 10] [--solve]
                                     [--out profiles/half_cache.json]

Needs a GPU (no fallback).  One process per run, both caches resident; per shape: the binary16 cache is built first with no
float32 cache present (regenerated windows, timed, peak memory recorded), then the float32 cache (timed), then the binary16 cache
once more packed from the resident float32 rows (timed) and compared bit for bit with torch's rounding of them.  Both matvecs are
warmed up, then `rounds` rounds alternate (float32, binary16), each round `inner` launches between two device events.  The margin
a difference is read against is the float32 kernel's own min .. max over the rounds; both are recorded.  Bytes per second are the
cache bytes (rows x M x 4 or 2) over the time of one matvec.
--solve: at cfg3_shard, one CG fit with cache_features=True and one with "half" (same preconditioner, tol 1e-6) and the distance
between their predictions on held-out points -- the effect of rounding the features, reported, not asserted anywhere."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"cfg3": (1_000_000, 1024, 8192), "cfg3_shard": (125_000, 1024, 8192), "wide": (250_000, 1024, 16384)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def stats(ms):
    return {"ms": ms, "median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms)}


def problem(n, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, d, generator=g, device="cuda", dtype=torch.float32) / np.sqrt(d)
    wvec = 3.0 * torch.randn(d, generator=g, device="cuda")
    y = torch.sin(x @ wvec).double() + 0.1 * torch.randn(n, generator=g, device="cuda", dtype=torch.float64)
    return x, y


def run_shape(name, n, d, m, args):
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.kernels import make_kernel
    x, y = problem(n, d, 11)
    ds = build_regression_dataset(x, y, chunk_size=8192, device="cuda")
    del x
    k = make_kernel("RBF", (n, d), m, 123, "cuda", {})
    k.set_hyperparams(np.array([0.1, 1.0]), logspace=False)
    ds.scaled_x(k.hyperparams[1])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    z16, build16_windows_ms = timed(lambda: ds.feature_cache_f16(k))
    peak16 = torch.cuda.max_memory_allocated() - base
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    z32, build32_ms = timed(lambda: ds.feature_cache(k))
    peak32 = torch.cuda.max_memory_allocated() - base
    ds._zcache16_key = None
    del z16
    z16, pack_ms = timed(lambda: ds.feature_cache_f16(k))
    step = 65536
    identical = all(torch.equal(z16[lo:lo + step].view(torch.int16), z32[lo:lo + step].half().view(torch.int16)) for lo in range(0, n, step))
    v = torch.randn(m, generator=torch.Generator(device="cuda").manual_seed(5), device="cuda", dtype=torch.float64)
    w32, w16 = torch.empty_like(v), torch.empty_like(v)
    ws = torch.empty(k.workspace_bytes(), dtype=torch.uint8, device="cuda")
    f32 = lambda: ext.hipZCacheMatvec(z32, v, w32, k.fit_intercept, ws)
    f16 = lambda: ext.hipZCacheMatvecHalf(z16, v, w16, k.fit_intercept, ws)

    def window(fn):
        def many():
            for _ in range(args.inner):
                fn()
        return timed(many)[1] / args.inner

    for fn in (f32, f16):
        for _ in range(3):
            fn()
    t32, t16 = [], []
    for _ in range(args.rounds):
        t32.append(window(f32))
        t16.append(window(f16))
    rel = float((w16 - w32).abs().max() / w32.abs().max())
    s32, s16 = stats(t32), stats(t16)
    out = {
        "rows": n, "d": d, "num_rffs": m,
        "float32": dict(s32, cache_bytes=n * m * 4, bytes_per_s=n * m * 4 / (s32["median_ms"] * 1e-3), build_ms=build32_ms,
                        peak_bytes_during_build=int(peak32)),
        "binary16": dict(s16, cache_bytes=n * m * 2, bytes_per_s=n * m * 2 / (s16["median_ms"] * 1e-3),
                         build_from_windows_ms=build16_windows_ms, pack_from_resident_float32_ms=pack_ms,
                         peak_bytes_during_build_from_windows=int(peak16), equals_torch_half_of_float32_cache=bool(identical)),
        "binary16_over_float32": s16["median_ms"] / s32["median_ms"],
        "float32_spread_rel": (s32["max_ms"] - s32["min_ms"]) / s32["median_ms"],
        "faster_beyond_float32_spread": bool(s16["max_ms"] < s32["min_ms"]),
        "matvec_rel_diff_binary16_vs_float32": rel,
        "peak_bytes_both_resident": int(torch.cuda.max_memory_allocated()),
    }
    if args.solve and name == "cfg3_shard":
        out["solve"] = solve(ds, k, d)
    return out


def solve(ds, k, d):
    from xgpr_amd.cg import cg_fit_lib_internal
    from xgpr_amd.preconditioner import RandNysPreconditioner
    pre = RandNysPreconditioner(k, ds, 256, False, 123, "srht")
    res = {}
    for mode in (True, "half"):
        (w, niter, _), ms = timed(lambda: cg_fit_lib_internal(k, ds, 1e-6, 500, pre, False, cache_features=mode))
        res[mode] = (w, niter, ms)
    xt, _ = problem(20_000, d, 99)
    zt = k.transform_x(xt)
    p32, p16 = zt @ res[True][0], zt @ res["half"][0]
    return {"what": "CG fit, rank-256 preconditioner, tol 1e-6, lambda 0.1; predictions (standardised y) on 20 000 held-out points",
            "iterations": {"float32": res[True][1], "binary16": res["half"][1]},
            "fit_ms": {"float32": res[True][2], "binary16": res["half"][2]},
            "prediction_rms": float(p32.pow(2).mean().sqrt()),
            "prediction_rms_diff": float((p16 - p32).pow(2).mean().sqrt()),
            "prediction_max_diff": float((p16 - p32).abs().max()),
            "weights_rel_diff": float(torch.linalg.norm(res["half"][0] - res[True][0]) / torch.linalg.norm(res[True][0]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg3,cfg3_shard,wide")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--solve", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "half_cache.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_half_cache.py needs a GPU")
    out = {"workload": "streaming CG matvec over the resident feature cache: float32 rows (hipZCacheMatvec) against IEEE binary16 rows "
                       "(hipZCacheMatvecHalf)",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "launches_per_round": args.inner,
           "timing": "device events around `launches_per_round` launches; float32 and binary16 alternate "
                     "round by round in one process after a warm-up of each; both caches resident",
           "shapes": {}}
    for name in args.shapes.split(","):
        n, d, m = SHAPES[name]
        out["shapes"][name] = run_shape(name, n, d, m, args)
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:            # after every shape: a later shape's failure keeps the earlier figures
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
