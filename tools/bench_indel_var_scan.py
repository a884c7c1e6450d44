#!/usr/bin/env python3
"""Times the indel variance scan (xgpr_conv_token_indel_var_scan_f32) against the composed route that writes every mutant out, and
writes profiles/indel_var_scan.json.

    python tools/bench_indel_var_scan.py [--out profiles/indel_var_scan.json] [--rounds 3] [--reps 3] [--composed-reps 1] [--no-split]

Workloads and protocol are those of tools/bench_subst_var_scan.py: an array of L = 512 positions, one-hot tokens over V = 21 rows,
conv_width 9, averaging "sqrt", M = 16384 features, nvar = 512 and 1024 variance columns, a seeded symmetric Vm; one sequence of 300
residues, and 64 sequences with lengths uniform in 64 .. 512.  Arms, on the same tree and the same operands:
  * operator  ext.hipConvTokenIndelVarScan into preallocated outputs, with the two (u~, q~) pairs precomputed (the C-ABI call alone);
  * kernel    ConvSORFKernel.indel_variance_scan: the float32 rows of the sequences, b, u~ and q~ with torch, then the operator;
  * composed  ConvSORFKernel.indel_variance_scan_composed: mutant token rows, fill_feature_rows, xv @ Vm with torch -- code made of
              existing operators: the baseline.
The arms alternate inside every round (one process, one device); each timing is a device-event window around ``reps`` back-to-back
calls after a warm-up of every arm; median and minimum over the rounds, in milliseconds per call.  Peak device memory, the split of
the operator into its delta kernels and its quadratic forms (torch.profiler, one call, sums over the slabs), the two routes'
tile-transform counts and the arithmetic floor are formed as in tools/bench_subst_var_scan.py.  Needs a HIP device: there is no
fallback."""
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
from bench_subst_var_scan import GRAM_TFLOPS, NVARS, mean_scan_rate, seeded_vm     # noqa: E402

KERNELS = ("var_delta_kernel", "var_quad_kernel", "pack_masks")


def tile_transforms(lengths):
    """(operator, composed) in transforms of one window through one 1024-frequency tile.  The operator: a deletion transforms its
    junction windows and the covering windows once (one wave); a gap transforms its straddling windows in each of the four waves and
    its V times |A| mutant windows.  The composed route: every window of L + (L + 1) V written-out rows through M / 2048 tiles (a row
    past the length is the sequence itself)."""
    cw = CONV_WIDTH
    op = comp = 0
    for s in (int(v) for v in lengths):
        nk = s - cw + 1
        for p in range(s):
            lo = max(0, p - cw + 1)
            op += max(0, min(p - 1, nk - 2) - lo + 1) + (min(p, nk - 1) - lo + 1)
        for g in range(s + 1):
            lo = max(0, g - cw + 1)
            op += 4 * max(0, min(g - 1, nk - 1) - lo + 1) + V * (min(g, nk) - lo + 1)
        rows = s * (nk - 1) + (L - s) * nk + V * ((s + 1) * (nk + 1) + (L - s) * nk)
        comp += rows * (M // 2048)
    return op, comp


def kernel_split(fn):
    """{kernel name: device milliseconds} over one call, from torch.profiler (the two row sets of either kernel told apart by their
    template argument -- the mode, the row map -- where the profiler prints it); None where the profiler reports no device time."""
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
            for key in KERNELS:
                if key in ev.key and dur:
                    name = key
                    if key == "var_delta_kernel":
                        name += " (deletions)" if ", 1>" in ev.key else " (insertions)" if ", 2>" in ev.key else ""
                    elif key == "var_quad_kernel":
                        name += " (deletions)" if "DelRowMap" in ev.key else " (insertions)" if "InsRowMap" in ev.key else ""
                    split[name] = split.get(name, 0.0) + dur / 1000.0
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
    nk = lengths.astype(np.float64) - CONV_WIDTH + 1
    pairs = []
    for nkm in (nk - 1, nk + 1):                          # averaging "sqrt": rho = sqrt(nk / nk'); column 0 stays 1 under the intercept
        b = z * torch.from_numpy(np.sqrt(nk / nkm)).to(dev)[:, None]
        b[:, 0] = 1.0
        u = (b @ vm).contiguous()
        pairs += [u, (b * u).sum(dim=1).contiguous()]
    od = torch.empty((n, L), dtype=torch.float64, device=dev)
    oi = torch.empty((n, L + 1, V), dtype=torch.float64, device=dev)
    held = []
    arms = {
        "operator": lambda: ext.hipConvTokenIndelVarScan(batch.tokens, batch.table, vm, pairs[0], pairs[1], pairs[2], pairs[3], od, oi,
                                                         k.radem_diag, k.chi_arr, lengths, CONV_WIDTH, k.scaling_type, True),
        "kernel": lambda: held.__setitem__(slice(None), [k.indel_variance_scan(raw, lengths, vm)]),
        "composed": lambda: held.__setitem__(slice(None), [k.indel_variance_scan_composed(raw, lengths, vm)]),
    }
    reps = {"operator": args.reps, "kernel": args.reps, "composed": args.composed_reps}
    for fn in arms.values():                             # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    diff = max(float((od - held[0][0]).abs().max()), float((oi - held[0][1]).abs().max()))      # (held: the composed route's result)
    spread = max(float((od - pairs[1][:, None]).abs()[od != 0].max()), float((oi - pairs[3][:, None, None]).abs()[oi != 0].max()))
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
    live_rows = int(lengths.sum()) + int((lengths + 1).sum()) * V
    rate = mean_scan_rate()
    floor = {"tile_transforms_ms": op / rate if rate else None, "quadratic_form_ms": 2.0 * live_rows * nvar * nvar / (GRAM_TFLOPS * 1e9),
             "mean_scan_tile_transforms_per_ms": rate, "fp64_matrix_tflops": GRAM_TFLOPS, "rows_inside_sequences": live_rows}
    floor["total_ms"] = (floor["tile_transforms_ms"] or 0.0) + floor["quadratic_form_ms"]
    return {"workload": {"name": name, "n": int(n), "L": L, "lengths": [int(lengths.min()), int(lengths.max())],
                         "positions_inside_sequences": int(lengths.sum()), "V": V, "C": V, "conv_width": CONV_WIDTH,
                         "averaging": "sqrt", "num_rffs": M, "nvar": nvar, "rows": {"deletions": int(n * L), "insertions": int(n * (L + 1) * V)}},
            "reps_per_window": reps, "ms_median": med, "ms_min": {nm: float(np.min(t)) for nm, t in times.items()},
            "operator_ms_per_sequence": med["operator"] / n,
            "composed_over_operator_time": med["composed"] / med["operator"], "composed_over_kernel_time": med["composed"] / med["kernel"],
            "operator_kernel_ms_one_call": split, "arithmetic_floor": floor, "operator_over_floor": med["operator"] / floor["total_ms"],
            "tile_transforms": {"operator": op, "composed": comp}, "composed_over_operator_tile_transforms": comp / op,
            "peak_device_bytes_over_the_operands": peaks, "output_bytes": int((od.numel() + oi.numel()) * 8),
            "workspace_bytes": ext.conv_token_indel_var_scan_workspace_bytes(k.radem_diag.shape[2], nvar, 0),
            "max_abs_diff_operator_composed": diff, "max_abs_Q_minus_q": spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "indel_var_scan.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--composed-reps", type=int, default=1)
    ap.add_argument("--no-split", action="store_true", help="skip the torch.profiler pass that splits the operator into its kernels")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_indel_var_scan.py needs a HIP device")
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    from xgpr_amd.kernels import ConvSORFKernel
    rng = np.random.default_rng(6)
    k = ConvSORFKernel("Conv1dRBF", (64, L, V), M, 123, "cuda", {"intercept": True, "conv_width": CONV_WIDTH, "averaging": "sqrt"})
    k.set_hyperparams(np.asarray([1.0, 2.1 / np.sqrt(CONV_WIDTH)]), logspace=False)
    shapes = [("one", np.asarray([300], dtype=np.int32)), ("batch64", rng.integers(MIN_LEN, L + 1, size=64).astype(np.int32))]
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "unit": "milliseconds per call (device events)",
              "note": "the composed arm's windows hold composed-reps calls each: short windows",
              "peak_note": "the operator arm writes into preallocated outputs (not counted) and allocates its workspace inside the call "
                           "(counted); the kernel and composed arms allocate their outputs, counted",
              "shapes": [run(name, lengths, nvar, k, ext, args, rng) for nvar in NVARS for name, lengths in shapes]}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
