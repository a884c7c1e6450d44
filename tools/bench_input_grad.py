#!/usr/bin/env python3
"""Times the input-gradient operator (xgpr_rbf_input_grad_f32) on the device and writes profiles/input_grad.json.

    python tools/bench_input_grad.py [--out profiles/input_grad.json] [--rounds 7] [--reps 200]

Shapes: n = 2000 rows, M = 8192 features (4096 frequencies), d in {9, 128, 1024}; one weight vector for all rows over all columns,
and one weight row per datapoint with w_cols = 1024 (the variance gradient's form: tiles past w_cols are skipped).  Compared, on
the same tree and the same operands, with
  * the composed fallback (SORFKernel.input_gradient_composed: the float64 feature operator, three float64 transforms, torch glue), and
  * hipRBFFeatureCache on the same shape: the forward half alone (transform, chi, cos / sin, float32 rows stored).
The three arms alternate inside every round (one process, one device); each timing is a device-event window around ``reps``
back-to-back calls after a warm-up of every arm; the median and the minimum over the rounds are recorded, in microseconds per call.
Needs a HIP device: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, M = 2000, 8192
WIDTHS = (9, 128, 1024)
VAR_COLS = 1024


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps          # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_grad.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_input_grad.py needs a HIP device")
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    from xgpr_amd.kernels import SORFKernel
    dev = "cuda"
    rows = []
    for d in WIDTHS:
        rng = np.random.default_rng(d)
        k = SORFKernel("RBF", (N, d), M, 123, dev, {"intercept": True})
        k.set_hyperparams(np.asarray([1.0, 2.1 / np.sqrt(d)]), logspace=False)
        xs = k.scaled_f32(rng.uniform(-1, 1, size=(N, d)))
        zc = torch.empty((N, M), dtype=torch.float32, device=dev)
        out = torch.empty((N, d), dtype=torch.float64, device=dev)
        sigma = float(k.hyperparams[1])
        for mode, w, w_cols in (("shared", torch.from_numpy(rng.standard_normal(M)).to(dev), M),
                                ("per-row", torch.from_numpy(rng.standard_normal((N, VAR_COLS))).to(dev), VAR_COLS)):
            arms = {
                "operator": lambda: ext.hipRBFInputGrad(xs, w, out, k.radem_diag, k.chi_arr, sigma, True, w_cols=w_cols),
                "fallback": lambda: k.input_gradient_composed(xs, w, w_cols),
                "feature_cache": lambda: ext.hipRBFFeatureCache(xs, zc, k.radem_diag, k.chi_arr),
            }
            for fn in arms.values():                     # warm-up: code objects, allocator
                fn()
                fn()
            torch.cuda.synchronize()
            diff = float((out - arms["fallback"]()).abs().max())
            times = {name: [] for name in arms}
            for _ in range(args.rounds):
                for name, fn in arms.items():
                    times[name].append(timed(fn, args.reps))
            med = {name: float(np.median(t)) for name, t in times.items()}
            row = {"n": N, "num_rffs": M, "d": d, "weights": mode, "w_cols": w_cols,
                   "us_median": med, "us_min": {name: float(np.min(t)) for name, t in times.items()},
                   "fallback_over_operator": med["fallback"] / med["operator"],
                   "operator_over_feature_cache": med["operator"] / med["feature_cache"],
                   "max_abs_diff_operator_fallback": diff}
            rows.append(row)
            print(json.dumps(row), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps_per_window": args.reps,
              "unit": "microseconds per call (device events)", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
