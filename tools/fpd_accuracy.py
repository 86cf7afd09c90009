#!/usr/bin/env python3
"""The accuracy record of the FPD kernels: every case of tests/fpd_model.py on one GPU against tests/golden/fpd.npz ->
|ours - exact| / scale, its bound, the reference's own gap and the iterations per stage, as one JSON document.

    python tools/fpd_accuracy.py [--out profiles/fpd_accuracy.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sp-gan_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fpd_model as fm      # noqa: E402
from spgan import fpd       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gold = np.load(os.path.join(ROOT, "tests", "golden", "fpd.npz"))
    rec = {"device": torch.cuda.get_device_name(0), "stages": ["sqrt(S1)", "sqrt(S2)", "polar"], "cases": {}}
    for name, (d, n1, n2, _) in fm.CASES.items():
        a, b = fm.case_inputs(name)
        m1, s1 = fpd.activation_statistics(torch.from_numpy(a).cuda())
        m2, s2 = fpd.activation_statistics(torch.from_numpy(b).cuda())
        info = fpd.frechet_distance_info(m1, s1, m2, s2)
        exact, scale, ref = float(gold[name + "|exact"]), float(gold[name + "|scale"]), float(gold[name + "|ref"])
        model, mits = fm.fpd(a, b)
        rec["cases"][name] = {"d": d, "n1": n1, "n2": n2, "value": info["distance"], "exact": exact, "scale": scale,
                              "err_over_scale": abs(info["distance"] - exact) / scale, "bound": fm.bound(name),
                              "reference_err_over_scale": abs(ref - exact) / scale, "iterations": list(info["iterations"]),
                              "numpy_model_err_over_scale": abs(model - exact) / scale, "numpy_model_iterations": list(mits)}
    text = json.dumps(rec, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
