#!/usr/bin/env python3
"""Times the substitution variance scan (xgpr_conv_token_subst_var_scan_f32) against the composed route that writes every mutant out,
and writes profiles/subst_var_scan.json.

    python tools/bench_subst_var_scan.py [--out profiles/subst_var_scan.json] [--rounds 3] [--reps 3] [--composed-reps 1] [--no-split]

Workloads, at BASELINE configs[3]'s sequence shape -- an array of L = 512 positions, one-hot tokens over V = 21 rows (C = 21 channels),
conv_width 9, averaging "sqrt", M = 16384 features -- for nvar = 512 and 1024 variance columns and a seeded symmetric Vm:
  * one      1 sequence of 300 residues (one protein: the common call);
  * batch64  64 sequences with lengths uniform in 64 .. 512.
Arms, on the same tree and the same operands:
  * operator  ext.hipConvTokenSubstVarScan into a preallocated output, with u and q precomputed (the C-ABI call alone);
  * kernel    ConvSORFKernel.substitution_variance_scan: the float32 rows of the sequences, u and q with torch, then the operator;
  * composed  ConvSORFKernel.substitution_variance_scan_composed: mutant token rows, fill_feature_rows, xv @ Vm with torch.
The arms alternate inside every round (one process, one device); each timing is a device-event window around ``reps`` back-to-back
calls (``composed-reps`` for the composed route) after a warm-up of every arm; the median and the minimum over the rounds are recorded,
in milliseconds per call.  Peak device memory is torch's max_memory_allocated over one call, less what was allocated before it (the
operator's workspace is allocated inside the call and counted).  The operator's time is split into its two kernels from the device
durations torch.profiler reports for one call (sums over the slabs).  Beside the measured times stand the two routes' tile-transform
counts (one window through ONE 1024-frequency tile: the operator transforms tile 0 alone, the composed route all M / 2048 tiles) and an
ARITHMETIC FLOOR for the operator: its tile transforms at the mean scan's measured rate (profiles/subst_scan.json, batch64: window
transforms x 8 tiles per millisecond) plus 2 rows nvar^2 flop at the FP64 matrix rate gram.inc reaches (73.6 TFLOP/s).
Needs a HIP device: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_subst_scan import CONV_WIDTH, L, M, MIN_LEN, V, peak_bytes, timed      # noqa: E402  (the mean scan's shapes and timers)

GRAM_TFLOPS = 73.6
NVARS = (512, 1024)


def seeded_vm(nvar, rng):
    a = rng.uniform(-1, 1, size=(nvar, nvar))
    a = (a + a.T) / (2 * 0.67 * (nvar - 1))
    a[np.arange(nvar), np.arange(nvar)] = rng.uniform(0.75, 1.25, size=nvar)
    return a


def tile_transforms(lengths):
    """(operator, composed) in transforms of one window through one 1024-frequency tile.  The operator: per position inside a sequence
    and covering window, V variants split over four waves, each of which also forms the own token's sums once -- (V + 4) per window.
    The composed route: every window of L V mutants through M / 2048 tiles."""
    op = comp = 0
    for s in lengths:
        nk = int(s) - CONV_WIDTH + 1
        cover = sum(min(l, nk - 1) - max(0, l - CONV_WIDTH + 1) + 1 for l in range(int(s)))
        op += (V + 4) * cover
        comp += L * V * nk * (M // 2048)
    return op, comp


def mean_scan_rate():
    """tile transforms per millisecond of the mean scan on batch64 (profiles/subst_scan.json), or None."""
    try:
        shape = json.load(open(os.path.join(ROOT, "profiles", "subst_scan.json")))["shapes"][1]
        return shape["window_transforms"]["operator"] * (M // 2048) / shape["ms_median"]["operator"]
    except (OSError, KeyError, IndexError, ValueError):
        return None


def kernel_split(fn):
    """{kernel name prefix: device milliseconds} over one call, from torch.profiler; None where the profiler reports no device time."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        split = {}
        for ev in prof.key_averages():
            dur = getattr(ev, "device_time_total", None)
            if dur is None:
                dur = getattr(ev, "cuda_time_total", 0.0)
            for key in ("subst_var_delta_kernel", "var_quad_kernel", "pack_masks"):
                if key in ev.key and dur:
                    split[key] = split.get(key, 0.0) + dur / 1000.0
        return split or None
    except Exception as exc:                              # the profiler is an aid: the timings above do not depend on it
        return {"error": repr(exc)}


def run(name, lengths, nvar, k, ext, args, rng):
    from xgpr_amd.dataset import TokenBatch
    dev = "cuda"
    n = lengths.shape[0]
    tokens = torch.from_numpy(rng.integers(0, V, size=(n, L)).astype(np.uint8)).to(dev)
    raw = TokenBatch(tokens, torch.eye(V, dtype=torch.float32, device=dev))
    batch = k.scaled_f32(raw)
    vm = torch.from_numpy(seeded_vm(nvar, rng)).to(dev)
    rows = torch.empty((n, M), dtype=torch.float32, device=dev)
    k.fill_feature_rows(batch, lengths, rows)
    z = rows[:, :nvar].to(torch.float64)
    u = (z @ vm).contiguous()
    q = (z * u).sum(dim=1).contiguous()
    out = torch.empty((n, L, V), dtype=torch.float64, device=dev)
    held = []
    arms = {
        "operator": lambda: ext.hipConvTokenSubstVarScan(batch.tokens, batch.table, vm, u, q, out, k.radem_diag, k.chi_arr, lengths,
                                                         CONV_WIDTH, k.scaling_type, True),
        "kernel": lambda: held.__setitem__(slice(None), [k.substitution_variance_scan(raw, lengths, vm)]),
        "composed": lambda: held.__setitem__(slice(None), [k.substitution_variance_scan_composed(raw, lengths, vm)]),
    }
    reps = {"operator": args.reps, "kernel": args.reps, "composed": args.composed_reps}
    for fn in arms.values():                             # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    diff = float((out - held[0]).abs().max())             # (held: the composed route's result)
    spread = float((out - q[:, None, None]).abs()[out != 0].max())
    held.clear()
    torch.cuda.empty_cache()
    peaks = {nm: peak_bytes(fn) for nm, fn in arms.items()}
    held.clear()
    times = {nm: [] for nm in arms}
    for _ in range(args.rounds):
        for nm, fn in arms.items():
            times[nm].append(timed(fn, reps[nm]))
    held.clear()
    split = None if args.no_split else kernel_split(arms["operator"])
    med = {nm: float(np.median(t)) for nm, t in times.items()}
    op, comp = tile_transforms(lengths)
    live_rows = int(lengths.sum()) * V
    rate = mean_scan_rate()
    floor = {"tile_transforms_ms": op / rate if rate else None, "quadratic_form_ms": 2.0 * live_rows * nvar * nvar / (GRAM_TFLOPS * 1e9),
             "mean_scan_tile_transforms_per_ms": rate, "fp64_matrix_tflops": GRAM_TFLOPS, "rows_inside_sequences": live_rows}
    floor["total_ms"] = (floor["tile_transforms_ms"] or 0.0) + floor["quadratic_form_ms"]
    return {"workload": {"name": name, "n": int(n), "L": L, "lengths": [int(lengths.min()), int(lengths.max())],
                         "positions_inside_sequences": int(lengths.sum()), "V": V, "C": V, "conv_width": CONV_WIDTH,
                         "averaging": "sqrt", "num_rffs": M, "nvar": nvar},
            "reps_per_window": reps, "ms_median": med, "ms_min": {nm: float(np.min(t)) for nm, t in times.items()},
            "operator_ms_per_sequence": med["operator"] / n,
            "composed_over_operator_time": med["composed"] / med["operator"], "composed_over_kernel_time": med["composed"] / med["kernel"],
            "operator_kernel_ms_one_call": split, "arithmetic_floor": floor, "operator_over_floor": med["operator"] / floor["total_ms"],
            "tile_transforms": {"operator": op, "composed": comp}, "composed_over_operator_tile_transforms": comp / op,
            "peak_device_bytes_over_the_operands": peaks, "output_bytes": int(out.numel() * 8),
            "workspace_bytes": ext.conv_token_subst_var_scan_workspace_bytes(k.radem_diag.shape[2], nvar, 0),
            "max_abs_diff_operator_composed": diff, "max_abs_Q_minus_q": spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subst_var_scan.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--composed-reps", type=int, default=1)
    ap.add_argument("--no-split", action="store_true", help="skip the torch.profiler pass that splits the operator into its kernels")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_subst_var_scan.py needs a HIP device")
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    from xgpr_amd.kernels import ConvSORFKernel
    rng = np.random.default_rng(6)
    k = ConvSORFKernel("Conv1dRBF", (64, L, V), M, 123, "cuda", {"intercept": True, "conv_width": CONV_WIDTH, "averaging": "sqrt"})
    k.set_hyperparams(np.asarray([1.0, 2.1 / np.sqrt(CONV_WIDTH)]), logspace=False)
    shapes = [("one", np.asarray([300], dtype=np.int32)), ("batch64", rng.integers(MIN_LEN, L + 1, size=64).astype(np.int32))]
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "unit": "milliseconds per call (device events)",
              "note": "the composed arm's windows hold composed-reps calls each: short windows",
              "peak_note": "the operator arm writes into a preallocated output (n L V float64, not counted) and allocates its workspace "
                           "inside the call (counted); the kernel and composed arms allocate their outputs, counted",
              "shapes": [run(name, lengths, nvar, k, ext, args, rng) for nvar in NVARS for name, lengths in shapes]}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
