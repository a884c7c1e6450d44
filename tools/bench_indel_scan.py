#!/usr/bin/env python3
"""Times the single-deletion / single-insertion scan (xgpr_conv_token_window_scores_f32 + xgpr_conv_token_indel_scan_f32) against the
composed route that materialises every mutant, and writes profiles/indel_scan.json.

    python tools/bench_indel_scan.py [--out profiles/indel_scan.json] [--rounds 3] [--reps 5] [--composed-reps 1]

Workloads, at BASELINE configs[3]'s sequence shape -- an array of L = 512 positions, one-hot tokens over V = 21 rows (C = 21 channels),
conv_width 9, averaging "sqrt", M = 16384 features (8192 frequencies), one weight vector:
  * one      1 sequence of 300 residues (one protein: the common call);
  * batch64  64 sequences with lengths uniform in 64 .. 512.
Arms, on the same tree and the same operands:
  * operator  ConvSORFKernel.indel_scan's kernels, ext.hipConvTokenWindowScores then ext.hipConvTokenIndelScan (deletions and
              insertions), into preallocated outputs;
  * composed  ConvSORFKernel.indel_scan_composed: mutant token rows of L + 1 positions, fill_feature_rows, hipZCacheBlockProject,
              subtraction -- existing operators, the baseline.
The arms alternate inside every round (one process, one device); each timing is a device-event window around ``reps`` back-to-back
calls (``composed-reps`` for the composed route) after a warm-up of every arm; the median and the minimum over the rounds are recorded,
in milliseconds per call.  Peak device memory is torch's max_memory_allocated over one call, less what was allocated before it.  Beside
the measured ratio of times stands the ratio of k-mer window transforms (one window through all tiles) the two routes perform.
Needs a HIP device: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, V, CONV_WIDTH, M = 512, 21, 9, 16384
MIN_LEN = 64


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps                # milliseconds per call


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def window_transforms(lengths):
    """(operator, composed): the operator transforms the nk windows of a sequence once, the junction windows of every deletion and
    the V variants of the windows that hold the new token of every insertion; the composed route transforms every window of the
    L + (L + 1) V mutant rows it writes (those past a length are the sequence itself) and of the sequence."""
    op = comp = 0
    for s in lengths:
        s = int(s)
        nk = s - CONV_WIDTH + 1
        junction = sum(max(0, min(p - 1, nk - 2) - max(0, p - CONV_WIDTH + 1) + 1) for p in range(s)) if nk > 1 else 0
        holding = sum(min(g, nk) - max(0, g - CONV_WIDTH + 1) + 1 for g in range(s + 1))
        op += nk + junction + V * holding
        comp += nk + (s * (nk - 1) if nk > 1 else s * nk) + (L - s) * nk + (s + 1) * V * (nk + 1) + (L - s) * V * nk
    return op, comp


def run(name, lengths, k, ext, args, rng):
    from xgpr_amd.dataset import TokenBatch
    dev = "cuda"
    n = lengths.shape[0]
    tokens = torch.from_numpy(rng.integers(0, V, size=(n, L)).astype(np.uint8)).to(dev)
    raw = TokenBatch(tokens, torch.eye(V, dtype=torch.float32, device=dev))
    batch = k.scaled_f32(raw)
    w = torch.from_numpy(rng.standard_normal(M)).to(dev)
    scores = torch.empty((n, L), dtype=torch.float64, device=dev)
    dele = torch.empty((n, L), dtype=torch.float64, device=dev)
    out = torch.empty((n, L + 1, V), dtype=torch.float64, device=dev)
    composed_out = []

    def operator():
        ext.hipConvTokenWindowScores(batch.tokens, batch.table, w, scores, k.radem_diag, k.chi_arr, lengths, CONV_WIDTH, True)
        ext.hipConvTokenIndelScan(batch.tokens, batch.table, w, scores, dele, out, k.radem_diag, k.chi_arr, lengths, CONV_WIDTH,
                                  k.scaling_type, True)

    arms = {
        "operator": operator,
        "scores_only": lambda: ext.hipConvTokenWindowScores(batch.tokens, batch.table, w, scores, k.radem_diag, k.chi_arr, lengths,
                                                            CONV_WIDTH, True),
        "composed": lambda: composed_out.__setitem__(slice(None), k.indel_scan_composed(raw, lengths, w)),
    }
    reps = {"operator": args.reps, "scores_only": args.reps, "composed": args.composed_reps}
    for fn in arms.values():                             # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    diff = max(float((out - composed_out[1]).abs().max()), float((dele - composed_out[0]).abs().max()))
    big = max(float(out.abs().max()), float(dele.abs().max()))
    composed_out.clear()
    torch.cuda.empty_cache()
    peaks = {nm: peak_bytes(fn) for nm, fn in arms.items()}
    composed_out.clear()
    times = {nm: [] for nm in arms}
    for _ in range(args.rounds):
        for nm, fn in arms.items():
            times[nm].append(timed(fn, reps[nm]))
    composed_out.clear()
    med = {nm: float(np.median(t)) for nm, t in times.items()}
    op, comp = window_transforms(lengths)
    return {"workload": {"name": name, "n": int(n), "L": L, "lengths": [int(lengths.min()), int(lengths.max())],
                         "positions_inside_sequences": int(lengths.sum()), "V": V, "C": V, "conv_width": CONV_WIDTH,
                         "averaging": "sqrt", "num_rffs": M},
            "reps_per_window": reps, "ms_median": med, "ms_min": {nm: float(np.min(t)) for nm, t in times.items()},
            "operator_ms_per_sequence": med["operator"] / n,
            "composed_over_operator_time": med["composed"] / med["operator"],
            "window_transforms": {"operator": op, "composed": comp}, "composed_over_operator_window_transforms": comp / op,
            "peak_device_bytes_over_the_operands": peaks, "output_bytes": int((out.numel() + dele.numel() + scores.numel()) * 8),
            "max_abs_diff_operator_composed": diff, "max_abs_output": big}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "indel_scan.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--composed-reps", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_indel_scan.py needs a HIP device")
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    from xgpr_amd.kernels import ConvSORFKernel
    rng = np.random.default_rng(5)
    k = ConvSORFKernel("Conv1dRBF", (64, L, V), M, 123, "cuda", {"intercept": True, "conv_width": CONV_WIDTH, "averaging": "sqrt"})
    k.set_hyperparams(np.asarray([1.0, 2.1 / np.sqrt(CONV_WIDTH)]), logspace=False)
    shapes = [("one", np.asarray([300], dtype=np.int32)), ("batch64", rng.integers(MIN_LEN, L + 1, size=64).astype(np.int32))]
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "unit": "milliseconds per call (device events)",
              "note": "the composed arm's windows hold composed-reps calls each: short windows",
              "peak_note": "the operator writes into preallocated outputs (scores and del n L, ins n (L + 1) V float64, not counted); the "
                           "composed route allocates its own, counted",
              "shapes": [run(name, lengths, k, ext, args, rng) for name, lengths in shapes]}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
