#!/usr/bin/env python
"""Errors of the approxmatch EMD kernels (csrc/approxmatch.hip) against the float64 model, next to the error the same formulation in
float32 torch ops with dense [B,n,m] tensors makes on the same GPU: runs tests/test_approxmatch_gpu.py in this process and writes every
comparison its `near` made (case, tensor, err_hip, e_ref, scale, bound = max(4 e_ref, 8 * 2^-24 * scale), ratio = err_hip / bound) to
profiles/approxmatch_accuracy.json, with the worst ratio per tensor.

    python tools/approxmatch_accuracy.py [--out profiles/approxmatch_accuracy.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sp-gan_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "approxmatch_accuracy.json"))
    args = ap.parse_args()
    import pytest
    import torch
    rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_approxmatch_gpu.py")])
    log = sys.modules["test_approxmatch_gpu"].LOG
    worst = max(log, key=lambda e: e["ratio"]) if log else None
    per_tensor = {}
    for e in log:
        if e["ratio"] > per_tensor.get(e["tensor"], {"ratio": -1.0})["ratio"]:
            per_tensor[e["tensor"]] = {"ratio": e["ratio"], "case": e["case"]}
    doc = {"device": torch.cuda.get_device_name(0), "pytest_exit": int(rc), "comparisons": len(log),
           "outside_bound": [e for e in log if e["err_hip"] > e["bound"]],
           "hip_worse_than_torch": sum(1 for e in log if e["err_hip"] > e["e_ref"]),
           "worst_err_over_bound": worst, "worst_ratio_per_tensor": per_tensor, "entries": log}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("%d comparisons, %d outside their bound, worst ratio %s, pytest exit %d -> %s"
          % (len(log), len(doc["outside_bound"]), worst and "%.3f (%s %s)" % (worst["ratio"], worst["case"], worst["tensor"]), rc, args.out))
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
