#!/usr/bin/env python3
"""One Lloyd iteration over resident float32 rows -- hipKMeansAssign + hipKMeansUpdate (include/xgpr_hip_cluster.h) -- against the
route the library offered before them, composed of existing operators: hipZCacheBlockProject in blocks of 32 centres into an
[n, K] float64 table, ``torch.argmin``, then ``index_add_`` of the rows widened to float64 (in slices of 65536 rows).

    python tools/bench_kmeans.py [--rows 1000000] [--rffs 512,2048] [--clusters 8,32,256] [--rounds 5] [--inner 3]
                                 [--out profiles/kmeans.json]

Needs a GPU (no fallback).  One process; per shape both routes are warmed up, then ``rounds`` rounds alternate (operators, composed),
each round ``inner`` iterations between two device events.  Beside every time stands the floor of reading the rows twice,
2 * 4 n M bytes over the rate the float32 cache matvec (hipZCacheMatvecScaled) reaches on the same rows in the same process
(4 n M bytes per matvec: the convention of tools/bench_half_cache.py).  The two routes' labels and sums are compared once per shape."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCK = 32          # columns per hipZCacheBlockProject call (include/xgpr_hip.h)
SLICE = 65536       # rows per index_add_ slice of the composed route (the float64 copy of a slice: 65536 x M x 8 bytes)


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def stats(ms):
    return {"ms": ms, "median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms)}


def run_shape(rows, k, args, matvec_rate):
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    n, m = rows.shape
    g = torch.Generator(device="cuda").manual_seed(1000 * m + k)
    centers = rows[torch.randint(0, n, (k,), generator=g, device="cuda")].to(torch.float64).contiguous()
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    dist2 = torch.empty(n, dtype=torch.float64, device="cuda")
    sums = torch.empty((k, m), dtype=torch.float64, device="cuda")
    counts = torch.empty(k, dtype=torch.int64, device="cuda")
    aws = torch.empty(max(int(ext._LIB.xgpr_kmeans_assign_workspace_bytes(n, m, k)), 256), dtype=torch.uint8, device="cuda")
    uws = torch.empty(max(int(ext._LIB.xgpr_kmeans_update_workspace_bytes(n, m, k)), 256), dtype=torch.uint8, device="cuda")

    def assign():
        ext.hipKMeansAssign(rows, centers, labels, dist2, workspace=aws)

    def update():
        ext.hipKMeansUpdate(rows, labels, sums, counts, workspace=uws)

    def pair():
        assign()
        update()

    table = torch.empty((n, k), dtype=torch.float64, device="cuda")
    blocks = [(lo, min(k, lo + BLOCK)) for lo in range(0, k, BLOCK)]
    tmp = {hi - lo: torch.empty((n, hi - lo), dtype=torch.float64, device="cuda") for lo, hi in blocks}
    vt = [centers[lo:hi].T.contiguous() for lo, hi in blocks]
    pws = torch.empty(max(ext.zcache_block_project_workspace_bytes(n, m, min(k, BLOCK)), 256), dtype=torch.uint8, device="cuda")
    csums = torch.empty((k, m), dtype=torch.float64, device="cuda")
    clabels = [None]

    def composed():
        cn = (centers * centers).sum(dim=1)
        for (lo, hi), v in zip(blocks, vt):
            t = tmp[hi - lo]
            ext.hipZCacheBlockProject(rows, v, t, False, scale=1.0, workspace=pws)
            table[:, lo:hi] = t
        table.mul_(-2.0).add_(cn[None, :])
        lab = torch.argmin(table, dim=1)
        csums.zero_()
        for lo in range(0, n, SLICE):
            csums.index_add_(0, lab[lo:lo + SLICE], rows[lo:lo + SLICE].to(torch.float64))
        clabels[0] = lab

    for fn in (pair, composed, assign, update):
        for _ in range(2):
            fn()
    agree = float((clabels[0] == labels.long()).double().mean())
    sums_rel = float((csums - sums).abs().max() / csums.abs().max())
    t_pair, t_comp, t_assign, t_update = [], [], [], []
    for _ in range(args.rounds):
        t_pair.append(timed(pair, args.inner))
        t_comp.append(timed(composed, 1))
        t_assign.append(timed(assign, args.inner))
        t_update.append(timed(update, args.inner))
    sp, sc = stats(t_pair), stats(t_comp)
    floor_ms = 2 * 4 * n * m / matvec_rate * 1e3
    return {"rows": n, "num_rffs": m, "clusters": k,
            "operators": dict(sp, assign=stats(t_assign), update=stats(t_update)),
            "composed": dict(sc, row_passes=len(blocks) + 1, table_bytes=n * k * 8),
            "two_row_reads_floor_ms": floor_ms,
            "operators_over_floor": sp["median_ms"] / floor_ms,
            "composed_over_operators": sc["median_ms"] / sp["median_ms"],
            "operators_faster_beyond_spread": bool(sp["max_ms"] < sc["min_ms"]),
            "labels_agreeing_share": agree, "sums_rel_diff": sums_rel,
            "assign_float64_flops_per_s": 2.0 * n * m * k / (float(np.median(t_assign)) * 1e-3),
            "update_bytes_per_s": 4.0 * n * m / (float(np.median(t_update)) * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rffs", default="512,2048")
    ap.add_argument("--clusters", default="8,32,256")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kmeans.py needs a GPU")
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    out = {"workload": "one Lloyd iteration over resident float32 rows: hipKMeansAssign + hipKMeansUpdate against hipZCacheBlockProject in "
                       "blocks of 32 centres + torch.argmin + index_add_",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iterations_per_round": args.inner,
           "timing": "device events; the two routes alternate round by round in one process after two warm-up runs of each",
           "shapes": {}}
    n = args.rows
    for m in (int(s) for s in args.rffs.split(",")):
        g = torch.Generator(device="cuda").manual_seed(m)
        rows = torch.randn((n, m), generator=g, device="cuda", dtype=torch.float32)
        rows += 3.0 * torch.randn((64, m), generator=g, device="cuda")[torch.randint(0, 64, (n,), generator=g, device="cuda")]
        v = torch.randn(m, generator=g, device="cuda", dtype=torch.float64)
        w = torch.empty_like(v)
        ws = torch.empty(ext.ztz_workspace_bytes(m, 2), dtype=torch.uint8, device="cuda")
        mv = lambda: ext.hipZCacheMatvecScaled(rows, v, w, 1.0, ws)
        for _ in range(3):
            mv()
        tm = [timed(mv, 10) for _ in range(args.rounds)]
        rate = 4.0 * n * m / (float(np.median(tm)) * 1e-3)
        out["cache_matvec_" + str(m)] = dict(stats(tm), bytes_per_s=rate)
        for k in (int(s) for s in args.clusters.split(",")):
            out["shapes"][f"M{m}_K{k}"] = run_shape(rows, k, args, rate)
            torch.cuda.empty_cache()
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:            # after every shape: a later shape's failure keeps the earlier figures
                json.dump(out, f, indent=1)
        del rows
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
