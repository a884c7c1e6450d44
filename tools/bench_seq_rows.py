#!/usr/bin/env python3
"""Times the sequence kernels' feature cache build and the uncached k = 1 CG matvec in THIS tree against another checkout
(the parent commit, with its own built library), alternating the two in one call; writes profiles/seq_rows.json.

    python tools/bench_seq_rows.py --parent /path/to/parent/checkout [--rounds 5] [--out profiles/seq_rows.json]
    python tools/bench_seq_rows.py --worker SHAPE          (one tree, one shape: prints a JSON line; what the driver starts)

Shapes: "conv" = BASELINE configs[3]'s share of one GPU (62 500 one-hot sequences, L 64..512 drawn as bench.py draws them,
21 channels, conv_width 9, 16384 RFFs, 'sqrt' averaging); "graph" = GraphRBF, 500 000 graphs of 8..24 nodes, 32 features per
node, 4096 RFFs.  Every worker is a fresh process (its tree's package and library), warmed up once, timed with device events
around synchronised work; the driver alternates parent / this tree `rounds` times and reports median and spread (max - min).

What is inside the timed region.  "cache_build_new_sigma": the whole of kernel.build_feature_cache(dataset) as it runs at a
sigma the dataset has not seen -- what tuning pays once per NMLL evaluation: the dataset's memoised sigma-scaled copy is
dropped before every repetition (outside the timed region), so a tree that reads dataset.scaled_x pays the scaling inside it,
as a tree that scales per slice inside transform_x always does.  "cache_build_scaled_sigma": the same call with the scaled
copy left in place (a rebuild at a sigma whose scaled copy exists, e.g. after the cache alone was dropped); identical to the
first for a tree that does not read scaled_x.  "matvec_k1_uncached": one k = 1 pass of ConjugateGrad._matvec without a
cache at a FIXED sigma, as in a CG solve: the scaled copy is reused across passes where the tree keeps one."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12        # bytes/s, MI355X HBM3E

SHAPES = {"conv": dict(kernel="Conv1dRBF", n=62500, L=512, C=21, m=16384, lo=64, onehot=True, parms={"conv_width": 9, "averaging": "sqrt"}),
          "graph": dict(kernel="GraphRBF", n=500000, L=24, C=32, m=4096, lo=8, onehot=False, parms={"averaging": "sqrt"})}


def worker(shape, repo, reps):
    sys.path.insert(0, repo)
    import numpy as np
    import torch
    from xgpr_amd.kernels import make_kernel
    from xgpr_amd.dataset import DeviceDataset
    from xgpr_amd.cg import ConjugateGrad
    s = SHAPES[shape]
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    if s["onehot"]:
        x = torch.nn.functional.one_hot(torch.randint(0, s["C"], (s["n"], s["L"]), device=dev, generator=g), s["C"]).to(torch.float32)
    else:
        x = torch.randn((s["n"], s["L"], s["C"]), device=dev, generator=g)
    sl = torch.randint(s["lo"], s["L"] + 1, (s["n"],), generator=torch.Generator().manual_seed(5)).numpy().astype(np.int32)
    y = torch.randn(s["n"], device=dev, generator=g, dtype=torch.float64)
    ds = DeviceDataset(x, y, sl, chunk_size=2000, device=dev)
    kern = make_kernel(s["kernel"], (s["n"], s["L"], s["C"]), s["m"], 123, dev, s["parms"])
    kern.set_hyperparams(np.array([1.0, 0.8]), logspace=False)

    def timed(fn, reps, before=None):
        fn()                                             # warm-up (allocator, kernel load)
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            if before is not None:
                before()                                 # (outside the timed region)
                torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    res = {"shape": shape, "repo": repo, "cache_bytes": s["n"] * s["m"] * 4}
    def drop_scaled():
        ds._scaled = {}                                  # the memoised sigma-scaled shard: as at a sigma not seen before

    res["build_new_sigma_ms"] = timed(lambda: kern.build_feature_cache(ds), reps, drop_scaled)
    res["build_ms"] = timed(lambda: kern.build_feature_cache(ds), reps)
    vec = torch.randn((s["m"], 1), device=dev, generator=g, dtype=torch.float64)
    mv = torch.zeros_like(vec)
    cg = ConjugateGrad(cache_features=False)
    res["matvec_ms"] = timed(lambda: cg._matvec(ds, kern, vec, mv, add_ridge=False), max(1, reps // 2))
    print("RESULT " + json.dumps(res), flush=True)


def run_worker(repo, shape, reps):
    env = dict(os.environ)
    env.pop("XGPR_HIP_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", shape, "--repo", repo, "--reps", str(reps)]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, check=True).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])


def git_id(repo):
    try:
        return subprocess.run(["git", "-C", repo, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return None


def summary(runs, key):
    vals = [statistics.median(r[key]) for r in runs]
    return {"median_ms": statistics.median(vals), "spread_ms": max(vals) - min(vals), "per_process_median_ms": vals}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker")
    ap.add_argument("--repo", default=ROOT)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--parent")
    ap.add_argument("--parent-id")
    ap.add_argument("--this-id")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="conv,graph")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_rows.json"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.repo, a.reps)
    doc = {"tool": "tools/bench_seq_rows.py", "rounds": a.rounds, "reps_per_process": a.reps,
           "parent_commit": a.parent_id or git_id(a.parent), "commit": a.this_id or git_id(ROOT),
           "timing": "device events around synchronised work, one warm-up per process, parent and this tree alternated; "
                     "median over processes of the per-process median, spread = max - min over processes",
           "timed_region": {"cache_build_new_sigma": "kernel.build_feature_cache(dataset) with the dataset's memoised sigma-scaled copy "
                                                     "dropped before every repetition: scaling + build, the cost of a rebuild at a new sigma",
                            "cache_build_scaled_sigma": "the same call with the scaled copy in place (the parent scales inside "
                                                        "transform_x either way, so its two figures are the same measurement)",
                            "matvec_k1_uncached": "one k = 1 pass without a cache at a fixed sigma; this tree reuses the scaled copy "
                                                  "across passes, the parent rescales every chunk on every pass"},
           "shapes": {}}
    for shape in a.shapes.split(","):
        old, new = [], []
        for _ in range(a.rounds):                        # alternated: parent, this tree, parent, ...
            old.append(run_worker(os.path.abspath(a.parent), shape, a.reps))
            new.append(run_worker(ROOT, shape, a.reps))
        s = SHAPES[shape]
        entry = {"kernel": s["kernel"], "sequences": s["n"], "L": [s["lo"], s["L"]], "channels": s["C"], "num_rffs": s["m"]}
        for key, label in (("build_new_sigma_ms", "cache_build_new_sigma"), ("build_ms", "cache_build_scaled_sigma"),
                           ("matvec_ms", "matvec_k1_uncached")):
            o, n = summary(old, key), summary(new, key)
            entry[label] = {"parent": o, "this": n, "ratio_parent_over_this": o["median_ms"] / n["median_ms"]}
        bw = new[0]["cache_bytes"] / (entry["cache_build_scaled_sigma"]["this"]["median_ms"] * 1e-3)     # the operator alone
        entry["cache_build_scaled_sigma"]["this"]["bytes_written_per_s"] = bw
        entry["cache_build_scaled_sigma"]["this"]["share_of_hbm_peak"] = bw / HBM_PEAK
        doc["shapes"][shape] = entry
        print(json.dumps({shape: entry}), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
