#!/usr/bin/env python3
"""Times the single-edit projection (xgpr_conv_token_subst_proj_f32 + xgpr_conv_token_indel_proj_f32) against the composed route that
writes every mutant out, and writes profiles/edit_proj.json.

    python tools/bench_edit_proj.py [--out profiles/edit_proj.json] [--rounds 3] [--reps 3] [--composed-reps 1] [--no-split]

Workloads: the shapes of tools/bench_subst_var_scan.py -- an array of L = 512 positions, one-hot tokens over V = 21 rows, conv_width 9,
averaging "sqrt", M = 16384 features, nvar = 512 and 1024 variance columns; 1 sequence of 300 residues (``one``) and 64 sequences with
lengths uniform in 64 .. 512 (``batch64``) -- each for K = 16 columns (draws) and K = nvar (a factor of the neighbourhood's covariance).
Arms, on the same tree and the same operands, ALL THREE row sets (substitutions, deletions, insertions) per call:
  * operator  ext.hipConvTokenSubstProj + ext.hipConvTokenIndelProj into preallocated outputs, with the base rows precomputed;
  * kernel    ConvSORFKernel.substitution_projection_scan + indel_projection_scan: the sequences' float32 rows, the base rows with torch,
              then the operators;
  * composed  the two ``*_projection_scan_composed``: mutant token rows, fill_feature_rows, rows[:, :nvar] @ proj with torch;
  * variance  ext.hipConvTokenSubstVarScan + ext.hipConvTokenIndelVarScan at the same shape: the delta kernels are the same code, so
              operator - variance is var_proj_kernel against var_quad_kernel.
The arms alternate inside every round (one process, one device); each timing is a device-event window around ``reps`` back-to-back
calls (``composed-reps`` for the composed route) after a warm-up of every arm; the median and the minimum over the rounds are recorded,
in milliseconds per call.  Peak device memory is torch's max_memory_allocated over one call, less what was allocated before it.  The
operator's time is split into its kernels from the device durations torch.profiler reports for one call (sums over the slabs and the
row sets).  Beside them: ``xGPRegression.select_single_edit_batch(batch_size=96)`` end to end for the one sequence (a plate), on a model
whose weights and var are SEEDED, not fitted -- the time does not depend on their values.
Needs a HIP device: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_subst_scan import CONV_WIDTH, L, M, MIN_LEN, V, peak_bytes, timed      # noqa: E402  (the mean scan's shapes and timers)
from bench_subst_var_scan import NVARS, seeded_vm                                 # noqa: E402

KERNELS = ("subst_var_delta_kernel", "var_delta_kernel", "var_proj_kernel", "var_quad_kernel", "pack_masks")


def window_transforms(lengths):
    """(operator, composed) in transforms of one window through one 1024-frequency tile, the three row sets together: the counts of
    tools/bench_subst_var_scan.py and tools/bench_indel_var_scan.py (operator: tile 0 of the windows at the edit; composed: every
    window of every written-out mutant through M / 2048 tiles)."""
    op = comp = 0
    cw = CONV_WIDTH
    for s in (int(v) for v in lengths):
        nk = s - cw + 1
        cover = sum(min(l, nk - 1) - max(0, l - cw + 1) + 1 for l in range(s))
        op += (V + 4) * cover                                                                    # substitutions
        op += sum((min(p - 1, nk - 2) - max(0, p - cw + 1) + 1) + (min(p, nk - 1) - max(0, p - cw + 1) + 1) for p in range(s))
        op += sum(V * (min(g, nk) - max(0, g - cw + 1) + 1) + 4 * max(0, min(g - 1, nk - 1) - max(0, g - cw + 1) + 1) for g in range(s + 1))
        comp += (L * V * nk + L * (nk - 1) + (L + 1) * V * (nk + 1)) * (M // 2048)
    return op, comp


def kernel_split(fn):
    """{kernel name: device milliseconds} over one call, from torch.profiler; None where the profiler reports no device time."""
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
                if key in ev.key and dur and not (key == "var_delta_kernel" and "subst_var_delta_kernel" in ev.key):
                    split[key] = split.get(key, 0.0) + dur / 1000.0
        return split or None
    except Exception as exc:                              # the profiler is an aid: the timings above do not depend on it
        return {"error": repr(exc)}


def run(name, lengths, nvar, K, k, ext, args, rng):
    from xgpr_amd.dataset import TokenBatch
    dev = "cuda"
    n = lengths.shape[0]
    tokens = torch.from_numpy(rng.integers(0, V, size=(n, L)).astype(np.uint8)).to(dev)
    raw = TokenBatch(tokens, torch.eye(V, dtype=torch.float32, device=dev))
    batch = k.scaled_f32(raw)
    vm = torch.from_numpy(seeded_vm(nvar, rng)).to(dev)
    pm = torch.linalg.cholesky(vm)[:, :K].contiguous()
    rows = torch.empty((n, M), dtype=torch.float32, device=dev)
    k.fill_feature_rows(batch, lengths, rows)
    z = rows[:, :nvar].to(torch.float64)
    b = (z @ pm).contiguous()                             # (the indel base rows differ by rho alone: the same cost)
    u = (z @ vm).contiguous()
    q = (z * u).sum(dim=1).contiguous()
    f64 = dict(dtype=torch.float64, device=dev)
    outs = [torch.empty((n, L, V, K), **f64), torch.empty((n, L, K), **f64), torch.empty((n, L + 1, V, K), **f64)]
    quads = [torch.empty((n, L, V), **f64), torch.empty((n, L), **f64), torch.empty((n, L + 1, V), **f64)]
    tail = (k.radem_diag, k.chi_arr, lengths, CONV_WIDTH, k.scaling_type, True)
    held = []

    def operator():
        ext.hipConvTokenSubstProj(batch.tokens, batch.table, pm, b, outs[0], *tail)
        ext.hipConvTokenIndelProj(batch.tokens, batch.table, pm, b, b, outs[1], outs[2], *tail)

    def variance():
        ext.hipConvTokenSubstVarScan(batch.tokens, batch.table, vm, u, q, quads[0], *tail)
        ext.hipConvTokenIndelVarScan(batch.tokens, batch.table, vm, u, q, u, q, quads[1], quads[2], *tail)

    arms = {
        "operator": operator,
        "kernel": lambda: held.__setitem__(slice(None), [k.substitution_projection_scan(raw, lengths, pm), k.indel_projection_scan(raw, lengths, pm)]),
        "composed": lambda: held.__setitem__(slice(None), [k.substitution_projection_scan_composed(raw, lengths, pm),
                                                           k.indel_projection_scan_composed(raw, lengths, pm)]),
        "variance": variance,
    }
    reps = {"operator": args.reps, "kernel": args.reps, "composed": args.composed_reps, "variance": args.reps}
    arms["kernel"]()                                      # warm-up: code objects, allocator -- and the two routes' agreement
    kern = held[0].clone()
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    diff = float((kern - held[0]).abs().max())            # (held: the composed route's substitutions)
    signal = float((kern - (z @ pm)[:, None, None, :]).abs().max())
    del kern
    held.clear()
    torch.cuda.empty_cache()
    peaks = {nm: peak_bytes(fn) for nm, fn in arms.items()}
    held.clear()
    times = {nm: [] for nm in arms}
    for _ in range(args.rounds):
        for nm, fn in arms.items():
            times[nm].append(timed(fn, reps[nm]))
        held.clear()
    split = None if args.no_split else {"operator": kernel_split(operator), "variance": kernel_split(variance)}
    med = {nm: float(np.median(t)) for nm, t in times.items()}
    op, comp = window_transforms(lengths)
    return {"workload": {"name": name, "n": int(n), "L": L, "lengths": [int(lengths.min()), int(lengths.max())],
                         "positions_inside_sequences": int(lengths.sum()), "V": V, "C": V, "conv_width": CONV_WIDTH, "averaging": "sqrt",
                         "num_rffs": M, "nvar": nvar, "K": K},
            "reps_per_window": reps, "ms_median": med, "ms_min": {nm: float(np.min(t)) for nm, t in times.items()},
            "composed_over_operator_time": med["composed"] / med["operator"], "composed_over_kernel_time": med["composed"] / med["kernel"],
            "operator_over_variance_time": med["operator"] / med["variance"], "kernel_ms_one_call": split,
            "tile_transforms": {"operator": op, "composed": comp}, "composed_over_operator_tile_transforms": comp / op,
            "peak_device_bytes_over_the_operands": peaks, "output_bytes": int(sum(o.numel() for o in outs) * 8),
            "workspace_bytes": ext.conv_token_edit_proj_workspace_bytes(k.radem_diag.shape[2], nvar, 0),
            "max_abs_diff_kernel_composed_substitutions": diff, "max_abs_out_minus_b_substitutions": signal}


def plate(k, nvar, rng, batch_size=96):
    """select_single_edit_batch(batch_size) end to end for the one sequence of 300 residues, wall-clock milliseconds (median of 3)."""
    from xgpr_amd.models import xGPRegression
    model = xGPRegression(num_rffs=M, variance_rffs=nvar, kernel_choice="Conv1dRBF", device="cuda", verbose=False,
                          kernel_settings={"intercept": True, "conv_width": CONV_WIDTH, "averaging": "sqrt"})
    model.kernel = k
    model.weights = torch.from_numpy(rng.normal(size=M) / np.sqrt(M)).to("cuda")
    model.var = torch.from_numpy(seeded_vm(nvar, rng)).to("cuda")
    tokens = rng.integers(0, V, size=(1, L)).astype(np.int64)
    lens, table = np.asarray([300], dtype=np.int32), np.eye(V, dtype=np.float32)
    model.select_single_edit_batch(tokens, lens, token_table=table, batch_size=4)          # warm-up, the factor of var cached
    times = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        picks = model.select_single_edit_batch(tokens, lens, token_table=table, batch_size=batch_size)[0]
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return {"nvar": nvar, "batch_size": batch_size, "edits": L * V + L + (L + 1) * V, "ms_median": float(np.median(times)),
            "ms_min": float(np.min(times)), "picks": len(picks), "distinct_sites_in_the_plate": len({(p["kind"], p["position"]) for p in picks})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_proj.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--composed-reps", type=int, default=1)
    ap.add_argument("--no-split", action="store_true", help="skip the torch.profiler passes that split the calls into their kernels")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_edit_proj.py needs a HIP device")
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    from xgpr_amd.kernels import ConvSORFKernel
    rng = np.random.default_rng(6)
    k = ConvSORFKernel("Conv1dRBF", (64, L, V), M, 123, "cuda", {"intercept": True, "conv_width": CONV_WIDTH, "averaging": "sqrt"})
    k.set_hyperparams(np.asarray([1.0, 2.1 / np.sqrt(CONV_WIDTH)]), logspace=False)
    shapes = [("one", np.asarray([300], dtype=np.int32)), ("batch64", rng.integers(MIN_LEN, L + 1, size=64).astype(np.int32))]
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "unit": "milliseconds per call (device events)",
              "note": "every arm computes the three row sets; the composed arm's windows hold composed-reps calls each: short windows",
              "peak_note": "the operator and variance arms write into preallocated outputs (not counted) and allocate their workspace inside "
                           "the call (counted); the kernel and composed arms allocate their outputs, counted",
              "shapes": [run(name, lengths, nvar, K, k, ext, args, rng) for nvar in NVARS for name, lengths in shapes for K in (16, nvar)],
              "select_single_edit_batch": [plate(k, nvar, rng) for nvar in NVARS]}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
