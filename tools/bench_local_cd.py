#!/usr/bin/env python3
"""Time the local-shape Chamfer on one GPU and print one JSON line:

  get_local_pair forward + backward at B = 32, N = M = 2048 (K = 20), and
  pairwise_local_cd at S = R = 128, N = 2048 (K = 8; 16384 pairs).

    python tools/bench_local_cd.py [--reps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sp-gan_amd"))

from spgan import losses, metrics  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    B, N = 32, 2048
    p1 = (torch.randn((B, 3, N), generator=g) * 0.3).cuda().requires_grad_(True)
    p2 = (p1.detach() + 0.01 * torch.randn((B, 3, N), generator=g).cuda()).requires_grad_(True)

    def glp():
        m, v = losses.get_local_pair(p1, p2)
        torch.autograd.grad(m + v, (p1, p2))

    def glp_fwd():
        with torch.no_grad():
            losses.get_local_pair(p1, p2)

    S = 128
    s = (torch.randn((1, N, 3), generator=g) * 0.3 + 0.01 * torch.randn((S, N, 3), generator=g)).cuda()
    r = (torch.randn((1, N, 3), generator=g) * 0.3 + 0.01 * torch.randn((S, N, 3), generator=g)).cuda()
    fb_med, fb_min = timed(glp, a.reps, a.warmup)
    f_med, f_min = timed(glp_fwd, a.reps, a.warmup)
    pw_med, pw_min = timed(lambda: metrics.pairwise_local_cd(s, r), a.reps, 1)
    print(json.dumps({
        "device": torch.cuda.get_device_name(0),
        "get_local_pair_B32_N2048_fwd_bwd_ms": round(fb_med, 3), "get_local_pair_fwd_bwd_min_ms": round(fb_min, 3),
        "get_local_pair_B32_N2048_fwd_ms": round(f_med, 3), "get_local_pair_fwd_min_ms": round(f_min, 3),
        "pairwise_local_cd_S128_R128_N2048_ms": round(pw_med, 3), "pairwise_local_cd_min_ms": round(pw_min, 3),
        "pairwise_us_per_entry": round(1e3 * pw_med / (S * S), 3), "reps": a.reps}))


if __name__ == "__main__":
    main()
