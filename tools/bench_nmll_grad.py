#!/usr/bin/env python3
"""Times one exact_nmll_gradient evaluation (what every L-BFGS-B cost evaluation of tune_hyperparams is) in THIS tree against
another checkout (the parent commit, with its own built library), and the two Gram kernels of the float32-rows route on their
own; writes profiles/nmll_grad_rows.json.

    python tools/bench_nmll_grad.py --parent /path/to/parent/checkout [--rounds 1] [--out profiles/nmll_grad_rows.json]
    python tools/bench_nmll_grad.py --worker SHAPE          (one tree, one shape: prints a JSON line; what the driver starts)
    python tools/bench_nmll_grad.py --worker kernels        (this tree: xgpr_cross_gram_f64 and xgpr_ztz_gram_f64 alone)

Shapes: "tabular" = the README's usage example, 36 584 x 9 at 8192 RFFs; "wide" = 131 072 x 1024 at 8192 RFFs; RBF with an
intercept, chunk_size 2000.  Every worker is a fresh process, warmed up once, timed with device events around the whole call
(feature generation, accumulations, the M x M factorisation and solves: the evaluation as the tuner pays it), median of
`reps` >= 5 runs.  "kernels": 65 536 x 8192 float32 rows, the cross Gram (2 x the flops of Z^T Z) and Z^T Z in the same process,
share of the FP64 matrix peak = useful flops (upper-triangle tiles only) / time / 78.6 TFLOP/s."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP64_MATRIX_PEAK = 78.6e12      # flop/s, MI355X at 2.4 GHz

SHAPES = {"tabular": dict(n=36584, d=9, m=8192), "wide": dict(n=131072, d=1024, m=8192)}


def _timed(torch, fn, reps):
    fn()                                             # warm-up (allocator, kernel load)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def worker(shape, repo, reps):
    sys.path.insert(0, repo)
    import numpy as np
    import torch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    if shape == "kernels":
        from xgpr_amd import xgpr_hip_rfgen_ext as ext
        n, m = 65536, 8192
        a = torch.randn((n, m), device=dev, generator=g, dtype=torch.float32)
        b = torch.randn((n, m), device=dev, generator=g, dtype=torch.float32)
        c = torch.zeros((m, m), device=dev, dtype=torch.float64)
        ws = {}
        tiles = (m // 128) * (m // 128 + 1) // 2
        flops = 2.0 * tiles * 128 * 128 * n           # Z^T Z over the tiles on or above the diagonal
        t_cross = _timed(torch, lambda: ws.__setitem__("c", ext.hipCrossGram(a, b, c, accumulate=True, workspace=ws.get("c"))), reps)
        t_gram = _timed(torch, lambda: ws.__setitem__("g", ext.hipZtZGram(a, c, False, 1.0, accumulate=True, workspace=ws.get("g"))), reps)
        mc, mg = statistics.median(t_cross), statistics.median(t_gram)
        res = {"shape": shape, "rows": n, "num_rffs": m, "box": box(torch), "cross_gram_ms": t_cross, "ztz_gram_ms": t_gram,
               "cross_gram_share_of_fp64_matrix_peak": 2 * flops / (mc * 1e-3) / FP64_MATRIX_PEAK,
               "ztz_gram_share_of_fp64_matrix_peak": flops / (mg * 1e-3) / FP64_MATRIX_PEAK}
        print("RESULT " + json.dumps(res), flush=True)
        return
    from xgpr_amd.kernels import make_kernel
    from xgpr_amd.dataset import DeviceDataset
    from xgpr_amd import nmll
    s = SHAPES[shape]
    x = torch.randn((s["n"], s["d"]), device=dev, generator=g, dtype=torch.float32)
    w = torch.randn(s["d"], device=dev, generator=g, dtype=torch.float32)
    y = (torch.sin(x @ w) + 0.1 * torch.randn(s["n"], device=dev, generator=g)).to(torch.float64)
    ds = DeviceDataset(x, y, None, chunk_size=2000, trainy_mean=float(y.mean()), trainy_std=float(y.std()), device=dev)
    kern = make_kernel("RBF", (s["n"], s["d"]), s["m"], 123, dev, {"intercept": True})
    kern.set_hyperparams(np.array([1.0, 0.5 / np.sqrt(s["d"])]), logspace=False)
    last = {}

    def evaluate():
        last["score"], last["grad"] = nmll.exact_nmll_gradient(kern, ds)
    ms = _timed(torch, evaluate, reps)
    route = bool(getattr(kern, "grad_rows_ok", lambda: False)())
    res = {"shape": shape, "repo": repo, "eval_ms": ms, "rows_route": route, "score": last["score"],
           "grad": [float(v) for v in last["grad"]], "peak_alloc_gib": torch.cuda.max_memory_allocated() / 2 ** 30}
    print("RESULT " + json.dumps(res), flush=True)


def run_worker(repo, shape, reps):
    env = dict(os.environ)
    env.pop("XGPR_HIP_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", shape, "--repo", repo, "--reps", str(reps)]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900, check=True).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])


def git_id(repo):
    try:
        return subprocess.run(["git", "-C", repo, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return None


def box(torch):
    """(asked in a worker: the driver never opens the device, it only starts children)"""
    p = torch.cuda.get_device_properties(0)
    return {"device": p.name, "compute_units": p.multi_processor_count, "hip": torch.version.hip, "torch": torch.__version__}


def summary(runs):
    vals = [statistics.median(r["eval_ms"]) for r in runs]
    return {"median_ms": statistics.median(vals), "spread_ms": max(vals) - min(vals), "per_process_median_ms": vals,
            "rows_route": runs[0]["rows_route"], "score": runs[0]["score"], "grad": runs[0]["grad"],
            "peak_alloc_gib": runs[0]["peak_alloc_gib"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker")
    ap.add_argument("--repo", default=ROOT)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", help="checkout of the parent commit with its own built library (required unless --worker)")
    ap.add_argument("--parent-id")
    ap.add_argument("--this-id")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--shapes", default="tabular,wide")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nmll_grad_rows.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: the median of at least five runs")
    if a.worker:
        return worker(a.worker, a.repo, a.reps)
    if not a.parent or not os.path.isdir(a.parent):
        ap.error("--parent: a checkout of the parent commit is required")
    doc = {"tool": "tools/bench_nmll_grad.py", "rounds": a.rounds, "reps_per_process": a.reps,
           "parent_commit": a.parent_id or git_id(a.parent), "commit": a.this_id or git_id(ROOT),
           "timing": "device events around the whole exact_nmll_gradient call, one warm-up per process, a fresh process per tree, "
                     "shape and round (parent first); per process the median of reps_per_process runs, then the median over "
                     "the `rounds` processes of a tree (with rounds = 1 that is the one process's median and the spread is 0)",
           "shapes": {}}
    for shape in a.shapes.split(","):
        old, new = [], []
        for _ in range(a.rounds):
            old.append(run_worker(os.path.abspath(a.parent), shape, a.reps))
            new.append(run_worker(ROOT, shape, a.reps))
        o, n = summary(old), summary(new)
        entry = dict(SHAPES[shape], parent=o, this=n, ratio_parent_over_this=o["median_ms"] / n["median_ms"])
        doc["shapes"][shape] = entry
        print(json.dumps({shape: entry}), flush=True)
        with open(a.out, "w") as f:                      # (kept up to date shape by shape)
            json.dump(doc, f, indent=1)
            f.write("\n")
    doc["kernels"] = run_worker(ROOT, "kernels", a.reps)
    doc["box"] = doc["kernels"].pop("box")
    print(json.dumps({"kernels": doc["kernels"]}), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
