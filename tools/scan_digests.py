#!/usr/bin/env python3
"""sha256 digests of what the three edit-scan operators write -- the bitwise contract of DESIGN.md 3.20 / 3.21, pinned.

    python tools/scan_digests.py [--out FILE] [--commit HASH]     record (needs a HIP device)
    python tools/scan_digests.py --check FILE                     compare with a recorded file; exit status 1 on the first difference

For every case of tests/dense_subst_scan.py (and the case of the same name of tests/dense_indel_scan.py) the operators run through
the public ``ext`` calls only -- hipConvTokenSubstScan on the former's operands, hipConvTokenWindowScores and hipConvTokenIndelScan
(both outputs) on the latter's -- so the same file runs on any tree that has them.  Recorded per case: the sha256 of the raw bytes of
each output (NaN payloads included) and of every input array.  ``--check`` reports a mismatch of input digests as "operands differ"
(numpy / scipy built other operands: nothing is said about the kernels), and otherwise names the first case and output that differ.
tests/test_gpu_edit_scan_bits.py holds the tree to tests/golden/edit_scan_digests.json."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dense_indel_scan as dis      # noqa: E402
import dense_subst_scan as dss      # noqa: E402

NAMES = [c[0] for c in dss.CASES]
OUTPUTS = ("subst", "scores", "del", "ins")
ARRAYS = ("tokens", "table", "seqlen", "w", "radem", "chi")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def input_digests(name):
    """{"subst": {array: sha256}, "indel": {...}}: the operands of the substitution scan and of the two indel calls; no device."""
    return {which: {k: sha(mod.case(name)[0][k]) for k in ARRAYS} for which, mod in (("subst", dss), ("indel", dis))}


def output_digests(ext, name):
    """{"subst", "scores", "del", "ins": sha256} of what the operators write for the case, on the current HIP device."""
    import torch
    nan = float("nan")
    out = {}
    for which, mod in (("subst", dss), ("indel", dis)):
        c, cw, scaling, icpt = mod.case(name)
        tokens, table, w, radem, chi = (torch.from_numpy(c[k]).to("cuda") for k in ("tokens", "table", "w", "radem", "chi"))
        n, L = c["tokens"].shape
        V = c["table"].shape[0]
        if which == "subst":
            sub = torch.full((n, L, V), nan, dtype=torch.float64, device="cuda")
            ext.hipConvTokenSubstScan(tokens, table, w, sub, radem, chi, c["seqlen"], cw, scaling, icpt)
            out["subst"] = sha(sub.cpu().numpy())
        else:
            scores, dele = (torch.full((n, L), nan, dtype=torch.float64, device="cuda") for _ in range(2))
            ins = torch.full((n, L + 1, V), nan, dtype=torch.float64, device="cuda")
            ext.hipConvTokenWindowScores(tokens, table, w, scores, radem, chi, c["seqlen"], cw, icpt)
            ext.hipConvTokenIndelScan(tokens, table, w, scores, dele, ins, radem, chi, c["seqlen"], cw, scaling, icpt)
            out.update(scores=sha(scores.cpu().numpy()), ins=sha(ins.cpu().numpy()))
            out["del"] = sha(dele.cpu().numpy())
    return out


def first_difference(recorded, name, outputs=None):
    """None, or one line that says how the case differs from ``recorded`` (the loaded file): its operands first, then ``outputs``
    (what output_digests returned) in the order of OUTPUTS."""
    want = recorded["cases"][name]
    mine = input_digests(name)
    for which in ("subst", "indel"):
        for k in ARRAYS:
            if mine[which][k] != want["inputs"][which][k]:
                return f"{name}: operands differ ({which} case, {k}): the recorded digests say nothing about this run"
    for o in OUTPUTS if outputs is not None else ():
        if outputs[o] != want["outputs"][o]:
            return f"{name}: output {o} differs from the recorded bits"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the digests here (default: print them)")
    ap.add_argument("--commit", default=None, help="the commit the digests are recorded from, noted in the file")
    ap.add_argument("--check", default=None, metavar="FILE")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("scan_digests.py needs a HIP device")
    from xgpr_amd import xgpr_hip_rfgen_ext as ext
    if args.check:
        with open(args.check) as f:
            recorded = json.load(f)
        for name in NAMES:
            diff = first_difference(recorded, name, output_digests(ext, name))
            if diff:
                print(diff)
                return 1
        print(f"{len(NAMES)} cases x {len(OUTPUTS)} outputs equal {args.check}")
        return 0
    result = {"commit": args.commit, "device": torch.cuda.get_device_name(0),
              "cases": {name: {"inputs": input_digests(name), "outputs": output_digests(ext, name)} for name in NAMES}}
    text = json.dumps(result, indent=1) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        print("wrote", args.out)
    else:
        print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
