#!/usr/bin/env python
"""Microbenchmark of the MST expansion penalty and minimum-density sampling (csrc/expansion.hip): device-event timing inside a warmed
loop, one JSON document.  GPU only.

  expansion penalty   [32, 2048, 3] with primitive_size 512 and 128, and MSN's [20, 8192, 3] with 512: forward, forward + backward and the
                      peak memory of one forward + backward, next to the 2 * B * n * 512 * 4 bytes of adjacency workspace the reference
                      allocates and this design does not;
  sampling            minimum_density_sample at [32, 2048] -> 512 and [20, 13192] -> 8192 (mean_mst_length from the penalty at 512 / 8
                      primitives of the first 8192 points);
  torch baselines     what a user could write without the kernels: Prim's algorithm as p-1 batched torch steps over all primitives at once
                      (the tree only: no owner assignment, no backward), and the density loop as npoint-1 batched steps.
Kernel and baseline take turns in the same process; every figure is a median with its min and max over the stated repeats of one call
after 3 warm-up rounds (the baselines: 1-2 warm-up rounds, fewer repeats -- a call is thousands of launches).  No ratio is asserted.

    python tools/expansion_bench.py [--out FILE] [--quick]          (default: profiles/expansion_bench.json)
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sp-gan_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from deform_bench import peak_bytes, timed_pair          # noqa: E402


def torch_prim(xyz, p):
    """Prim's algorithm over all primitives at once, one batched step per tree edge -> (parent, edge length) [P, p]."""
    pts = xyz.reshape(-1, p, 3)
    P = pts.shape[0]
    rows = torch.arange(P, device=pts.device)
    cur = torch.full((P, p), float("inf"), device=pts.device)
    par = torch.zeros((P, p), dtype=torch.long, device=pts.device)
    vis = torch.zeros((P, p), dtype=torch.bool, device=pts.device)
    vis[:, 0] = True
    cur[:, 0] = 0.0
    last = torch.zeros(P, dtype=torch.long, device=pts.device)
    for _ in range(p - 1):
        d = (pts - pts[rows, last][:, None, :]).norm(dim=2)
        upd = ~vis & (d < cur)
        cur = torch.where(upd, d, cur)
        par = torch.where(upd, last[:, None], par)
        last = cur.masked_fill(vis, float("inf")).argmin(dim=1)
        vis[rows, last] = True
    return par, cur


def torch_mds(xyz, npoint, L, split=8192):
    B, n, _ = xyz.shape
    rows = torch.arange(B, device=xyz.device)
    t = (5.0 * L * L)[:, None]
    w = torch.where(torch.arange(n, device=xyz.device) < split, 1.0, 2.0)[None]
    T = torch.zeros((B, n), device=xyz.device)
    T[:, 0] = 1e9
    out = torch.zeros((B, npoint), dtype=torch.long, device=xyz.device)
    last = torch.zeros(B, dtype=torch.long, device=xyz.device)
    for j in range(1, npoint):
        d = (xyz - xyz[rows, last][:, None, :]).square().sum(2)
        T = T + w * torch.exp(-d / t)
        last = T.argmin(dim=1)
        out[:, j] = last
        T[rows, last] = 1e9
    return out


def bench_penalty(spgan, B, n, p, quick):
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, n, 3, generator=g).cuda().requires_grad_(True)
    cot = torch.randn(B, n, generator=g).cuda()
    mod = spgan.expansionPenaltyModule()

    def fwd():
        with torch.no_grad():
            return mod(x, p, 1.5)

    def step():
        x.grad = None
        (mod(x, p, 1.5)[0] * cot).sum().backward()

    def base():
        with torch.no_grad():
            return torch_prim(x, p)
    t = timed_pair([fwd, step], warmup=3, iters=1, repeats=5 if quick else 21)
    tb = timed_pair([base], warmup=1 if quick else 2, iters=1, repeats=2 if quick else 5)
    par, w = base()
    mean_t = (w.sum(1) / (p - 1)).view(B, n // p).mean(1)
    diff = float(((fwd()[2] - mean_t).abs() / mean_t).max())
    return {"op": "expansion_penalty", "shape": dict(B=B, n=n, primitive_size=p, alpha=1.5),
            "forward_ms": t[0], "forward_backward_ms": t[1], "torch_prim_only_ms": tb[0],
            "measured_ratio_torch_prim_over_forward": tb[0]["median"] / t[0]["median"],
            "max_rel_difference_mean_mst_length_vs_torch": diff,
            "peak_bytes_forward_backward": peak_bytes(step), "reference_adjacency_workspace_bytes": 2 * B * n * 512 * 4}


def bench_sampling(spgan, B, n, npoint, quick):
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, n, 3, generator=g).cuda()
    with torch.no_grad():
        L = spgan.expansionPenaltyModule()(x[:, :(n // 512) * 512].contiguous(), 512, 1.5)[2]

    def kern():
        return spgan.minimum_density_sample(x, npoint, L)

    def base():
        return torch_mds(x, npoint, L)
    t = timed_pair([kern], warmup=3, iters=1, repeats=5 if quick else 21)
    tb = timed_pair([base], warmup=1, iters=1, repeats=2 if quick else 3)
    a, b = kern().long(), base()
    return {"op": "minimum_density_sample", "shape": dict(B=B, n=n, npoint=npoint, split=8192), "kernel_ms": t[0], "torch_loop_ms": tb[0],
            "measured_ratio_torch_over_kernel": tb[0]["median"] / t[0]["median"],
            "share_of_picks_equal_to_torch_loop": float((a == b).float().mean()), "peak_bytes_kernel": peak_bytes(kern)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expansion_bench.json"))
    ap.add_argument("--quick", action="store_true", help="fewer repeats")
    ap.add_argument("--note", default="", help="recorded verbatim (e.g. the kernel shape this build uses)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("expansion_bench.py needs a GPU")
    import spgan
    res = {"device": torch.cuda.get_device_name(0), "note": a.note,
           "timing": "device events; median / min / max of %d repeats of 1 call after 3 warm-up rounds; torch baselines: %s repeats" %
                     ((5, "2") if a.quick else (21, "5 (Prim) / 3 (density loop)")), "configs": []}
    jobs = [lambda: bench_penalty(spgan, 32, 2048, 512, a.quick), lambda: bench_penalty(spgan, 32, 2048, 128, a.quick),
            lambda: bench_penalty(spgan, 20, 8192, 512, a.quick), lambda: bench_sampling(spgan, 32, 2048, 512, a.quick),
            lambda: bench_sampling(spgan, 20, 13192, 8192, a.quick)]
    for job in jobs:
        res["configs"].append(job())
        print(json.dumps(res["configs"][-1]), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
