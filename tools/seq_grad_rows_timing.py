#!/usr/bin/env python3
"""One exact_nmll_gradient evaluation of the sequence kernels on the float32-rows route against the chunked float64
formulation (the parent commit's route, taken by forcing ``grad_rows_ok`` false), and what the rounding of the rows costs;
writes profiles/seq_grad_rows.json.

    python tools/seq_grad_rows_timing.py [--reps 5] [--conv-n 16384] [--graph-n 131072] [--out profiles/seq_grad_rows.json]
    python tools/seq_grad_rows_timing.py --rounding-only      (the second part alone: seconds)

Timing.  Shapes: "conv" = BASELINE configs[3]'s window (Conv1dRBF, one-hot sequences of L 64..512 over 21 channels, conv_width
9: 9 x 21 = 189 -> padded 256, 'sqrt' averaging), "graph" = GraphRBF (8..24 nodes, 32 features per node), both at M = 8192.
One process, one warm-up evaluation per route, then the two routes ALTERNATED ``reps`` times; every evaluation sits between
two events on the launch stream (the evaluation ends in host reads of device scalars, so the second event closes finished
work); median and spread (max - min) are reported.  "writer" / "operator": the feature-and-gradient generation alone over the
same shard -- ``fill_grad_rows`` per window of the rows route against ``kernel_specific_gradient`` (zero fill + hipConvGrad)
per chunk of the float64 formulation.

Rounding.  The rows route differs from the float64 formulation by the one rounding to float32 of the float64 k-mer sums.  What
that alone costs is measured on neither route: ``exact_nmll_reg_grad`` is fed the five terms accumulated in float64 torch from
``gradient_x`` outputs, once as they are and once cast to float32 and back, at the shapes and the two hyperparameter settings
of tests/test_gpu_seq_grad_rows.py (``route_problem``, ``HPARAMS``).  The test measures the same cost for each of its cases and
sets its bars to ten times that; this tool records the values."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {"conv": dict(kernel="Conv1dRBF", L=512, C=21, lo=64, onehot=True, parms={"conv_width": 9, "averaging": "sqrt"}),
          "graph": dict(kernel="GraphRBF", L=24, C=32, lo=8, onehot=False, parms={"averaging": "sqrt"})}
M_TIMED = 8192

# ---- the route tests' problems (tests/test_gpu_seq_grad_rows.py imports these)
HPARAMS = [(0.7, 0.45), (0.2, 1.2)]                     # (lambda, sigma)
ROUTE_KERNELS = {"Conv1dRBF": dict(L=20, C=8, parms={"conv_width": 5, "averaging": "sqrt"}),
                 "GraphMatern": dict(L=14, C=10, parms={"averaging": "sqrt", "matern_nu": 2.5})}


def route_problem(name, device="cuda", n=2051, m=256, chunk=500):
    """(dataset, kernel): n seeded sequences in chunks of ``chunk``, M = m; lengths drawn in [conv_width, L]."""
    import numpy as np
    from xgpr_amd.dataset import build_regression_dataset
    from xgpr_amd.kernels import make_kernel
    s = ROUTE_KERNELS[name]
    rng = np.random.default_rng(len(name) + s["L"])
    x = rng.standard_normal((n, s["L"], s["C"])).astype(np.float32)
    cw = s["parms"].get("conv_width", 1)
    sl = rng.integers(cw, s["L"] + 1, size=n).astype(np.int32)
    w = rng.standard_normal(s["C"])
    mean = np.array([x[i, :sl[i]].mean(axis=0) @ w for i in range(n)])
    y = np.sin(2.0 * mean) + 0.05 * rng.standard_normal(n)
    ds = build_regression_dataset(x, y, sl, chunk_size=chunk, device=device)
    kern = make_kernel(name, x.shape, m, 123, device, dict(s["parms"], intercept=True))
    return ds, kern


def terms_from_gradient_x(ds, kern, rounded):
    """The five terms of calc_gradient_terms in float64 torch from ``gradient_x`` outputs, chunk by chunk; ``rounded``: the
    outputs cast to float32 and back first (the values the rows route contracts)."""
    import torch
    m = kern.get_num_rffs()
    f64 = dict(dtype=torch.float64, device=kern.device)
    ztz, zty, dzty, inner = torch.zeros((m, m), **f64), torch.zeros(m, **f64), torch.zeros((m, 1), **f64), torch.zeros((m, m), **f64)
    yty = torch.zeros(1, **f64)
    for xin, yin, ldata in ds.get_chunked_data():
        z, dz, y = kern.gradient_x_y(xin, yin, ldata)
        g = dz[:, :, 0]
        if rounded:
            z, g = z.float().double(), g.float().double()
        ztz += z.T @ z
        zty += z.T @ y
        yty += y @ y
        dzty[:, 0] += g.T @ y
        inner += g.T @ z
    inner = inner + inner.T
    return ztz, zty, float(yty.item()), dzty, inner[:, :, None].contiguous()


def rounding_cost(ds, kern):
    """(relative score difference, max |gradient difference| / max |gradient|) between the terms of unrounded and rounded
    ``gradient_x`` outputs at the kernel's current hyperparameters."""
    import numpy as np
    from xgpr_amd import nmll
    hp = kern.get_hyperparams(logspace=False)
    n = ds.get_ndatapoints()
    res = []
    for rounded in (False, True):
        t = terms_from_gradient_x(ds, kern, rounded)
        score, grad, _ = nmll.exact_nmll_reg_grad(t[0], t[1], t[2], hp, n, t[3], t[4])
        res.append((float(score), np.asarray(grad)))
    (s0, g0), (s1, g1) = res
    return abs(s1 - s0) / abs(s0), float(np.abs(g1 - g0).max() / np.abs(g0).max())


def measure_rounding():
    import numpy as np
    out = {"cases": [], "metric": "score: |rounded - unrounded| / |unrounded|; gradient: max |rounded - unrounded| / max |unrounded|"}
    for name in ROUTE_KERNELS:
        ds, kern = route_problem(name)
        for lam, sigma in HPARAMS:
            kern.set_hyperparams(np.array([lam, sigma]), logspace=False)
            s, g = rounding_cost(ds, kern)
            out["cases"].append({"kernel": name, "lambda": lam, "sigma": sigma, "score_rel": s, "grad_rel": g})
            print(json.dumps(out["cases"][-1]), flush=True)
    out["score_rel_max"] = max(c["score_rel"] for c in out["cases"])
    out["grad_rel_max"] = max(c["grad_rel"] for c in out["cases"])
    for c in out["cases"]:                               # the bars of the test's case: ten times its own rounding cost
        c["score_bar"], c["grad_bar"] = 10 * c["score_rel"], 10 * c["grad_rel"]
    return out


def _events(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _stats(vals):
    return {"median_ms": statistics.median(vals), "spread_ms": max(vals) - min(vals), "ms": vals}


def time_shape(shape, n, reps):
    import numpy as np
    import torch
    from xgpr_amd import nmll
    from xgpr_amd.cg import window_ranges
    from xgpr_amd.dataset import DeviceDataset
    from xgpr_amd.kernels import make_kernel
    s = SHAPES[shape]
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    if s["onehot"]:
        x = torch.nn.functional.one_hot(torch.randint(0, s["C"], (n, s["L"]), device=dev, generator=g), s["C"]).to(torch.float32)
    else:
        x = torch.randn((n, s["L"], s["C"]), device=dev, generator=g)
    sl = torch.randint(s["lo"], s["L"] + 1, (n,), generator=torch.Generator().manual_seed(5)).numpy().astype(np.int32)
    y = torch.randn(n, device=dev, generator=g, dtype=torch.float64)
    ds = DeviceDataset(x, y, sl, chunk_size=2000, device=dev)
    kern = make_kernel(s["kernel"], (n, s["L"], s["C"]), M_TIMED, 123, dev, s["parms"])
    kern.set_hyperparams(np.array([1.0, 0.8]), logspace=False)
    if not nmll._grad_rows_route(ds, kern):
        raise RuntimeError("the rows route is not taken for this shape")
    cls = type(kern)
    rows_ok = cls.grad_rows_ok

    def evaluate(rows):
        cls.grad_rows_ok = rows_ok if rows else (lambda self: False)
        try:
            return nmll.exact_nmll_gradient(kern, ds)
        finally:
            cls.grad_rows_ok = rows_ok

    step = min(nmll._grad_window_rows(M_TIMED), n)
    zwin = torch.empty((step, M_TIMED), dtype=torch.float32, device=dev)
    gwin = torch.empty((step, M_TIMED), dtype=torch.float32, device=dev)

    def writer():
        for lo, hi, wl in window_ranges(n, step, sl):
            kern.fill_grad_rows(x[lo:hi], zwin[:hi - lo], gwin[:hi - lo], wl)

    def operator():
        for xin, _, ldata in ds.get_chunked_data():
            kern.kernel_specific_gradient(xin, ldata)

    results = {k: [] for k in ("rows", "float64", "writer", "operator")}
    vals = {True: evaluate(True), False: evaluate(False)}            # warm-up of both routes; their results are compared below
    writer()
    operator()
    torch.cuda.synchronize()
    for _ in range(reps):                                            # alternated
        results["float64"].append(_events(lambda: evaluate(False)))
        results["rows"].append(_events(lambda: evaluate(True)))
        results["operator"].append(_events(operator))
        results["writer"].append(_events(writer))
    (sr, gr), (sf, gf) = vals[True], vals[False]
    entry = {"kernel": s["kernel"], "sequences": n, "L": [s["lo"], s["L"]], "channels": s["C"], "num_rffs": M_TIMED,
             "window_rows": step, "chunk_rows": 2000,
             "evaluation_float64_route": _stats(results["float64"]), "evaluation_rows_route": _stats(results["rows"]),
             "generation_float64_operator": _stats(results["operator"]), "generation_rows_writer": _stats(results["writer"]),
             "score_rel_diff_between_routes": abs(sr - sf) / abs(sf),
             "grad_rel_diff_between_routes": float(np.abs(gr - gf).max() / np.abs(gf).max())}
    entry["evaluation_ratio_float64_over_rows"] = entry["evaluation_float64_route"]["median_ms"] / entry["evaluation_rows_route"]["median_ms"]
    entry["generation_ratio_operator_over_writer"] = entry["generation_float64_operator"]["median_ms"] / entry["generation_rows_writer"]["median_ms"]
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--conv-n", type=int, default=16384)
    ap.add_argument("--graph-n", type=int, default=131072)
    ap.add_argument("--rounding-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_grad_rows.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("this measurement needs a HIP device")
    doc = {"tool": "tools/seq_grad_rows_timing.py", "device": torch.cuda.get_device_name(0),
           "timing": "one process; one warm-up evaluation per route, then float64 route / rows route / float64 operator / rows writer "
                     "alternated `reps` times; each between two events on the launch stream; median and spread (max - min)",
           "reps": a.reps}
    if os.path.exists(a.out) and a.rounding_only:
        with open(a.out) as f:
            doc = json.load(f)
    doc["rounding"] = measure_rounding()
    if not a.rounding_only:
        doc["shapes"] = {}
        for shape, n in (("conv", a.conv_n), ("graph", a.graph_n)):
            doc["shapes"][shape] = time_shape(shape, n, a.reps)
            print(json.dumps({shape: doc["shapes"][shape]}), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
