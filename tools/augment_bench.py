#!/usr/bin/env python
"""Microbenchmark of the device-side batch augmentation (csrc/augment.hip, spgan.augment): DeviceDataset.get_batch at [32,2048,3] from a
4096-cloud resident set, device-event timing inside a warmed loop, eager issue, one JSON document.  GPU only.

  pair   the reference pair (point shuffle, rotation about y, one scale in [0.8, 1.25]): DeviceDataset(transform=reference_transform("ref"))
         against DeviceDataset(augment=True), the eager torch path that `transform=None` keeps.
  full   every stage on (reference_transform("full")) against the same stages written as torch ops.

Every time is a median with its min and max over 21 repeats of 20 back-to-back calls after warm-up; the routes take turns.  "below"
compares min-max ranges.  Launches per call are counted by torch.profiler in a pass of its own after the timing, which also gives the
device time of the apply launch; its rate is stated against the batch's own bytes (B * N * C * 4, once) and against everything it reads
and writes.

    python tools/augment_bench.py [--out FILE] [--quick]          (default: profiles/augment_bench.json)
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sp-gan_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from deform_bench import timed_pair          # noqa: E402
from gan_layers_bench import launches        # noqa: E402


def torch_full(data, index, gen):
    """The stages of reference_transform("full") as float32 torch ops on the device (the draws come from torch's generator)."""
    B, P = index.numel(), data.shape[1]
    dev = data.device
    r = lambda *s: torch.rand(s, generator=gen, device=dev)                   # noqa: E731
    n = lambda *s: torch.randn(s, generator=gen, device=dev)                  # noqa: E731
    out = data[index]
    out = out[torch.arange(B, device=dev)[:, None], r(B, P).argsort(dim=1)]
    a = r(B) * (2 * math.pi)
    c, s = torch.cos(a), torch.sin(a)
    R = torch.zeros((B, 3, 3), device=dev)
    R[:, 0, 0] = c; R[:, 0, 2] = s; R[:, 1, 1] = 1.0; R[:, 2, 0] = -s; R[:, 2, 2] = c
    g = (0.06 * n(B, 3)).clamp(-0.18, 0.18)
    cx, sx, cy, sy, cz, sz = torch.cos(g[:, 0]), torch.sin(g[:, 0]), torch.cos(g[:, 1]), torch.sin(g[:, 1]), torch.cos(g[:, 2]), torch.sin(g[:, 2])
    one, zero = torch.ones_like(cx), torch.zeros_like(cx)
    Rx = torch.stack([one, zero, zero, zero, cx, -sx, zero, sx, cx], dim=1).view(B, 3, 3)
    Ry = torch.stack([cy, zero, sy, zero, one, zero, -sy, zero, cy], dim=1).view(B, 3, 3)
    Rz = torch.stack([cz, -sz, zero, sz, cz, zero, zero, zero, one], dim=1).view(B, 3, 3)
    A = torch.bmm(R.transpose(1, 2), torch.bmm(Rz, torch.bmm(Ry, Rx)).transpose(1, 2)) * (0.8 + 0.45 * r(B)).view(B, 1, 1)
    out = torch.bmm(out, A) + ((2 * r(B) - 1) * 0.1).view(B, 1, 1)
    out = out + (0.01 * n(B, P, 3)).clamp(-0.05, 0.05)
    drop = r(B, P) <= (r(B) * 0.875).view(B, 1)
    return torch.where(drop[:, :, None], out[:, :1], out)


def kernel_times(fn, match, calls=5):
    """Device time (us) of the kernels whose name contains `match`, one entry per launch, from torch.profiler."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        t = [float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0)) for e in prof.events()
             if str(getattr(e, "device_type", "")).endswith("CUDA") and match in e.name]
        return t if t and min(t) > 0 else None
    except Exception as e:                                   # noqa: BLE001
        return "not measured: %s" % e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    ap.add_argument("--quick", action="store_true", help="a small set and few repeats (a rehearsal, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench.py needs a GPU")
    from spgan.augment import reference_transform
    from spgan.dataset import DeviceDataset
    dev = torch.device("cuda", 0)
    S, B, N = (256, 32, 2048) if a.quick else (4096, 32, 2048)
    repeats, iters = (3, 5) if a.quick else (21, 20)
    g = np.random.default_rng(0)
    src = torch.tensor(g.standard_normal((S, N, 3)), dtype=torch.float32)
    parent = DeviceDataset(src, num_points=N, batch_size=B, augment=True, device=dev, seed=0)
    pair = DeviceDataset(src, num_points=N, batch_size=B, device=dev, transform=reference_transform("ref", seed=0, device=dev))
    full = DeviceDataset(src, num_points=N, batch_size=B, device=dev, transform=reference_transform("full", seed=0, device=dev))
    index = torch.tensor(g.permutation(S)[:B], dtype=torch.int64, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    routes = {"parent_pair": lambda: parent.get_batch(index), "fused_pair": lambda: pair.get_batch(index),
              "torch_full": lambda: torch_full(parent.data, index, gen), "fused_full": lambda: full.get_batch(index)}
    names = list(routes)
    t = dict(zip(names, timed_pair([routes[k] for k in names], warmup=5, iters=iters, repeats=repeats)))
    res = {"device": torch.cuda.get_device_name(0), "quick": bool(a.quick), "set": [S, N, 3], "batch": [B, N, 3],
           "timing": "device events; median / min / max of %d repeats of %d back-to-back calls after warm-up; the routes take turns; eager issue"
                     % (repeats, iters),
           "ms_per_batch": t,
           "ratio_parent_over_fused_pair": t["parent_pair"]["median"] / t["fused_pair"]["median"],
           "ratio_torch_over_fused_full": t["torch_full"]["median"] / t["fused_full"]["median"],
           "fused_pair_below_parent": t["fused_pair"]["max"] < t["parent_pair"]["min"],
           "fused_full_below_torch": t["fused_full"]["max"] < t["torch_full"]["min"]}
    print(json.dumps(res), flush=True)
    res["launches_per_batch"] = {k: launches(routes[k]) for k in names}
    batch_bytes = B * N * 3 * 4
    moved = 2 * batch_bytes + B * N * 4 + B * 16 * 4 + B * 8                    # rows in, rows out, the permutation, the records, the indices
    rates = {}
    for k in ("fused_pair", "fused_full"):
        kt = kernel_times(routes[k], "augment_apply_kernel")
        pt = kernel_times(routes[k], "augment_prepare_kernel")
        if isinstance(kt, list) and isinstance(pt, list):
            us = statistics.median(kt)
            rates[k] = {"apply_us": {"median": us, "min": min(kt), "max": max(kt)},
                        "prepare_us": {"median": statistics.median(pt), "min": min(pt), "max": max(pt)},
                        "batch_bytes": batch_bytes, "bytes_read_and_written": moved,
                        "batch_gb_per_s": batch_bytes / us * 1e-3, "traffic_gb_per_s": moved / us * 1e-3}
        else:
            rates[k] = {"apply_us": kt, "prepare_us": pt}
    res["apply_launch"] = rates
    print(json.dumps({"launches_per_batch": res["launches_per_batch"], "apply_launch": rates}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
