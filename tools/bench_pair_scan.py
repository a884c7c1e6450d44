#!/usr/bin/env python3
"""Times the pairwise substitution scan (xgpr_conv_token_pair_scan_f32) against the composed route that writes every double mutant out,
and writes profiles/pair_scan.json.

    python tools/bench_pair_scan.py [--out profiles/pair_scan.json] [--rounds 3] [--reps 3] [--composed-reps 1]

Workloads and protocol are those of tools/bench_subst_scan.py: an array of L = 512 positions, one-hot tokens over V = 21 rows
(C = 21 channels), conv_width 9, averaging "sqrt", M = 16384 features (8192 frequencies), one weight vector:
  * one     1 sequence of 300 residues (one protein: the common call);
  * batch4  4 sequences with lengths uniform in 64 .. 512 (the output is 14.5 MB per sequence).
Arms, on the same tree and the same operands:
  * operator  ConvSORFKernel.pair_substitution_scan's kernels, ext.hipConvTokenPairScan, into a preallocated output;
  * composed  ConvSORFKernel.pair_substitution_scan_composed: single and double mutants' token rows, fill_feature_rows,
              hipZCacheBlockProject, the double difference.
The arms alternate inside every round (one process, one device); each timing is a device-event window around ``reps`` back-to-back
calls (``composed-reps``, one by default, for the composed route) after a warm-up of every arm; the median and the minimum over the
rounds are recorded, in milliseconds per call.  Peak device memory is torch's max_memory_allocated over one call, less what was
allocated before it.  Beside the measured ratio of times stands the ratio of k-mer window transforms (one window through all tiles)
the two routes perform.  Needs a HIP device: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_subst_scan import CONV_WIDTH, L, M, MIN_LEN, V, peak_bytes, timed     # noqa: E402


def window_transforms(lengths):
    """(operator, composed): the operator transforms V V variants of every window shared by two positions inside a sequence less
    than conv_width apart; the composed route transforms every window of every such pair's V V double mutants, of every position's V
    single mutants and of the sequence itself."""
    op = comp = 0
    for s in lengths:
        s = int(s)
        nk = s - CONV_WIDTH + 1
        shared = pairs = 0
        for l1 in range(s):
            for d in range(1, CONV_WIDTH):
                if l1 + d < s:
                    pairs += 1
                    shared += min(l1, nk - 1) - max(0, l1 + d - CONV_WIDTH + 1) + 1
        op += V * V * shared
        comp += (pairs * V * V + s * V + 1) * nk
    return op, comp


def run(name, lengths, k, ext, args, rng):
    from xgpr_amd.dataset import TokenBatch
    dev = "cuda"
    n = lengths.shape[0]
    tokens = torch.from_numpy(rng.integers(0, V, size=(n, L)).astype(np.uint8)).to(dev)
    raw = TokenBatch(tokens, torch.eye(V, dtype=torch.float32, device=dev))
    batch = k.scaled_f32(raw)
    w = torch.from_numpy(rng.standard_normal(M)).to(dev)
    out = torch.empty((n, L, CONV_WIDTH - 1, V, V), dtype=torch.float64, device=dev)
    composed_out = []
    arms = {
        "operator": lambda: ext.hipConvTokenPairScan(batch.tokens, batch.table, w, out, k.radem_diag, k.chi_arr, lengths, CONV_WIDTH,
                                                     k.scaling_type, True),
        "composed": lambda: composed_out.__setitem__(slice(None), [k.pair_substitution_scan_composed(raw, lengths, w)]),
    }
    reps = {"operator": args.reps, "composed": args.composed_reps}
    for fn in arms.values():                             # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    diff = float((out - composed_out[0]).abs().max())
    big = float(out.abs().max())
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
    time_ratio, count_ratio = med["composed"] / med["operator"], comp / op
    return {"workload": {"name": name, "n": int(n), "L": L, "lengths": [int(lengths.min()), int(lengths.max())],
                         "positions_inside_sequences": int(lengths.sum()), "V": V, "C": V, "conv_width": CONV_WIDTH,
                         "averaging": "sqrt", "num_rffs": M},
            "reps_per_window": reps, "ms_median": med, "ms_min": {nm: float(np.min(t)) for nm, t in times.items()},
            "operator_ms_per_sequence": med["operator"] / n,
            "composed_over_operator_time": time_ratio,
            "window_transforms": {"operator": op, "composed": comp}, "composed_over_operator_window_transforms": count_ratio,
            "time_ratio_over_count_ratio": time_ratio / count_ratio,
            "operator_is_faster": bool(med["operator"] < med["composed"]),
            "peak_device_bytes_over_the_operands": peaks, "output_bytes": int(out.numel() * 8),
            "max_abs_diff_operator_composed": diff, "max_abs_output": big}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_scan.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--composed-reps", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pair_scan.py needs a HIP device")
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    from xgpr_amd.kernels import ConvSORFKernel
    rng = np.random.default_rng(5)
    k = ConvSORFKernel("Conv1dRBF", (4, L, V), M, 123, "cuda", {"intercept": True, "conv_width": CONV_WIDTH, "averaging": "sqrt"})
    k.set_hyperparams(np.asarray([1.0, 2.1 / np.sqrt(CONV_WIDTH)]), logspace=False)
    shapes = [("one", np.asarray([300], dtype=np.int32)), ("batch4", rng.integers(MIN_LEN, L + 1, size=4).astype(np.int32))]
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "unit": "milliseconds per call (device events)",
              "note": "the composed arm's windows hold composed-reps calls each: short windows",
              "peak_note": "the operator writes into a preallocated output (n L (conv_width - 1) V V float64, not counted); the "
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
