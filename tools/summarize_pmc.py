#!/usr/bin/env python3
"""Turns the rocprofv3 outputs of tools/collect_profiles.sh (under $XGPR_PROF_OUT, default prof_out/) into the committed
summaries under profiles/: kernel stats of the bench command, the FETCH_SIZE / WRITE_SIZE rows of the bench's
dominant kernels, and the per-launch HBM traffic JSONs bench.py reads.  gfx950 correction (MI355X_MICROARCH.md,
HBM section): FETCH_SIZE tallies 64 B per 128-B request for wide streaming reads, so it is doubled; WRITE_SIZE is
taken as reported.  Counter units are KiB."""
import csv, glob, json, os, shutil, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.environ.get("XGPR_PROF_OUT", os.path.join(ROOT, "prof_out"))
P = os.path.join(ROOT, "profiles")
ROUND = os.environ.get("XGPR_ROUND", "r3")


def one(pattern):
    f = glob.glob(os.path.join(G, pattern))
    if not f:
        sys.exit(f"missing {pattern}")
    return max(f, key=os.path.getmtime)      # files of several collections may sit side by side: take the latest


shutil.copy(one("prof_stats/*/*kernel_stats.csv"), os.path.join(P, f"{ROUND}_bench_n1_kernel_stats.csv"))
KERNELS = {"ztz3_kernel<10, 0": "fused", "ztz3_kernel<10, 5": "cache_rows_z3", "sketch_gemm_lds_kernel<": "sketch_gemm", "srht_sample_rows": "srht_rows", "zcache_ztz_kernel": "cached", "zblock_t_kernel": "block_t", "zblock_w_kernel": "block_w",
           "reduce_slabs_kernel": "reduce", "wave_rbf_kernel": "featgen"}
per = {}
for tag, counter in (("fetch", "FETCH_SIZE"), ("write", "WRITE_SIZE")):
    rows = [r for r in csv.DictReader(open(one(f"prof_{tag}/*/*counter_collection.csv")))
            if any(k in r["Kernel_Name"] for k in KERNELS) and r["Counter_Name"] == counter]
    keep = ["Dispatch_Id", "Kernel_Name", "Grid_Size", "Workgroup_Size", "LDS_Block_Size", "Scratch_Size", "VGPR_Count",
            "Counter_Name", "Counter_Value", "Start_Timestamp", "End_Timestamp"]
    with open(os.path.join(P, f"{ROUND}_bench_n1_pmc_{tag}_size.csv"), "w", newline="") as fo:
        w = csv.DictWriter(fo, keep)
        w.writeheader()
        for r in rows:
            d = {k: r[k] for k in keep}
            d["Kernel_Name"] = d["Kernel_Name"][:90]
            w.writerow(d)
    for r in rows:
        for k, short in KERNELS.items():
            if k in r["Kernel_Name"]:
                per.setdefault(short, {}).setdefault(counter, []).append(float(r["Counter_Value"]))
bench = json.loads(open(os.path.join(G, "prof_fetch.json")).read().strip().splitlines()[-1])
n_local, d, m = bench["config"]["rows_per_gpu"], 1024, 8192


def mean_main(vals):
    """mean over the launches of the full-size problem (the largest values; short probe launches are dropped)"""
    top = max(vals)
    sel = [v for v in vals if v > 0.5 * top]
    return sum(sel) / len(sel)


note = ("gfx950: FETCH_SIZE counts 64 B per 128-B request -> x2 (MI355X_MICROARCH.md, HBM); WRITE_SIZE as reported; "
        "separate --pmc passes with --kernel-trace only (tools/collect_profiles.sh)")
for short, kname, alg in (("fused", "ztz3_kernel<10, Z3_MATVEC>", 4.0 * d * n_local),
                          ("cached", "zcache_ztz_kernel<true, 2>", 4.0 * m * n_local)):
    if short not in per:
        continue
    fk, wk = mean_main(per[short]["FETCH_SIZE"]), mean_main(per[short]["WRITE_SIZE"])
    hbm = (2.0 * fk + wk) * 1024.0
    out = {"round": int(ROUND[1:]), "build_id": bench.get("build_id"), "command": "rocprofv3 --pmc FETCH_SIZE|WRITE_SIZE --kernel-trace --output-format csv -- python bench.py "
           "--full --steps 3 --warmup 1 --no-cpu-baseline", "kernel": kname,
           "config": {"rows_per_gpu": n_local, "dim": d, "rffs": m, "n_gpus": 1},
           "FETCH_SIZE_KiB_per_launch": fk, "WRITE_SIZE_KiB_per_launch": wk, "correction": note,
           "hbm_bytes_per_launch": hbm, "algorithmic_bytes_per_launch": alg, "traffic_over_algorithmic": hbm / alg}
    name = f"{ROUND}_pmc_traffic.json" if short == "fused" else f"{ROUND}_pmc_traffic_cached.json"
    json.dump(out, open(os.path.join(P, name), "w"), indent=1)
    print(short, f"traffic/algorithmic = {hbm / alg:.4f}")
for short in ("block_t", "block_w"):
    if short in per:
        fk, wk = mean_main(per[short]["FETCH_SIZE"]), mean_main(per[short]["WRITE_SIZE"])
        print(short, f"HBM bytes per launch {(2 * fk + wk) * 1024 / 1e9:.2f} GB (cache read algorithmic {4.0 * m * n_local / 1e9:.2f} GB)")

# the preconditioner pass over float32 feature rows (windows of ROW_WINDOW_BYTES / (4 M) rows, rank 512): the largest
# launches are the full windows
win = min(n_local, max(8192, (4 << 30) // (4 * m)))
rank = 512
pre = {}
for short, kname, alg in (("sketch_gemm", "sketch_gemm_lds_kernel<false>", win * (rank * 8.0 + m * 4.0) + 2 * rank * m * 8.0),
                          ("srht_rows", "srht_sample_rows16_kernel<13>", win * (m * 4.0 + rank * 8.0))):
    if short in per:
        fk, wk = max(per[short]["FETCH_SIZE"]), max(per[short]["WRITE_SIZE"])      # the largest = a full window
        hbm = (2.0 * fk + wk) * 1024.0
        pre[short] = {"kernel": kname, "rows_per_launch": win, "FETCH_SIZE_KiB": fk, "WRITE_SIZE_KiB": wk,
                      "FETCH_SIZE_KiB_all_launches": sorted(per[short]["FETCH_SIZE"]),
                      "hbm_bytes_per_launch": hbm, "algorithmic_bytes_per_launch": alg, "traffic_over_algorithmic": hbm / alg}
        print(short, f"traffic/algorithmic = {hbm / alg:.4f}")
if pre:
    pre["correction"] = note
    pre["build_id"] = bench.get("build_id")
    json.dump(pre, open(os.path.join(P, f"{ROUND}_pmc_traffic_precond.json"), "w"), indent=1)
