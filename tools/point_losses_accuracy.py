#!/usr/bin/env python
"""Errors of the point-distribution losses' kernels (csrc/point_losses.hip) against the float64 model, next to the error the same
formulation in float32 torch ops makes on the same GPU: runs tests/test_point_losses_gpu.py in this process and writes every comparison
its `near` made (case, tensor, err_hip, e_ref, scale, bound = max(4 e_ref, 8 * 2^-24 * scale), active_share = the share of tail terms
with a non-zero derivative) to profiles/point_losses_accuracy.json.

    python tools/point_losses_accuracy.py [--out profiles/point_losses_accuracy.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_losses_accuracy.json"))
    args = ap.parse_args()
    import pytest
    import torch
    rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_point_losses_gpu.py")])
    log = sys.modules["test_point_losses_gpu"].LOG
    worst = max(log, key=lambda e: e["err_hip"] / e["bound"]) if log else None
    doc = {"device": torch.cuda.get_device_name(0), "pytest_exit": int(rc), "comparisons": len(log),
           "outside_bound": [e for e in log if e["err_hip"] > e["bound"]],
           "hip_worse_than_torch": sum(1 for e in log if e["err_hip"] > e["e_ref"]),
           "least_active_share": min((e["active_share"] for e in log if e["active_share"] is not None), default=None),
           "worst_err_over_bound": worst, "entries": log}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("%d comparisons, %d outside their bound, pytest exit %d -> %s" % (len(log), len(doc["outside_bound"]), rc, args.out))
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
