#!/usr/bin/env python
"""Microbenchmark of the PointConv path (spgan.pointconv_util): device-event timing inside a warmed loop, one JSON document.

  * compute_density forward and forward + backward (spgan_kde_density: no [B,N,N] matrix) beside the route the library offered before it:
    pointnet_util.square_distance -> torch.exp -> mean, which stores [B,N,N]; with the bytes each route moves;
  * spgan_pointconv_aggregate forward and backward beside torch.matmul on the same stored rows (the reference's expression), each with
    the bytes moved and the fraction of the achievable HBM rate that implies;
  * one PointConvDensitySetAbstraction forward + backward with its device kernel count.

The two routes of a pair are timed alternately in the same process.

    python tools/pointconv_bench.py [--out profiles/pointconv_bench.json] [--B 32 --N 2048 --S 512 --K 32 --D 64 --mlp 64 64 128]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sp-gan_amd"))
HBM_ACHIEVABLE = 6.3e12          # bytes/s: the float4-copy rate of an MI355X


def timed_pair(fns, warmup=5, iters=10, repeats=7):
    """Per function: (median, min, max) over `repeats` of the mean device time (ms) of `iters` back-to-back calls; the functions take
    turns inside every repeat."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            out[i].append(e0.elapsed_time(e1) / iters)
    return [{"median": statistics.median(o), "min": min(o), "max": max(o)} for o in out]


def kernel_count(fn):
    """Device kernels of one call, counted by the profiler (None where it is not available)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn(); torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "Memcpy" not in e.name and "Memset" not in e.name)
    except Exception:          # the profiler is optional equipment: the timings above do not depend on it
        return None


def rate(nbytes, ms):
    return {"bytes": nbytes, "TB_per_s": nbytes / (ms * 1e-3) / 1e12, "fraction_of_achievable_hbm": nbytes / (ms * 1e-3) / HBM_ACHIEVABLE}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32); ap.add_argument("--N", type=int, default=2048); ap.add_argument("--S", type=int, default=512)
    ap.add_argument("--K", type=int, default=32); ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--mlp", type=int, nargs="+", default=[64, 64, 128])
    ap.add_argument("--bandwidth", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from spgan import pointconv_util as pc, pointnet_util as pu
    B, N, S, K, D, h = a.B, a.N, a.S, a.K, a.D, a.bandwidth
    C = a.mlp[-1]
    g = torch.Generator().manual_seed(0)
    xyz = torch.rand(B, N, 3, generator=g).cuda()
    res = {"device": torch.cuda.get_device_name(0), "shape": dict(B=B, N=N, S=S, K=K, D=D, mlp=a.mlp, bandwidth=h)}

    # ---- kernel density
    gd = torch.randn(B, N, generator=g).cuda()
    xg = xyz.clone().requires_grad_(True)

    def kde_fwd():
        with torch.no_grad():
            return pc.compute_density(xyz, h)

    def composed_fwd():
        with torch.no_grad():
            return (torch.exp(-pu.square_distance(xyz, xyz) / (2.0 * h * h)) / (2.5 * h)).mean(dim=-1)

    def kde_step():
        xg.grad = None
        pc.compute_density(xg, h).backward(gd)

    def composed_step():
        # square_distance carries no gradient in the library: the differentiable composed route is the reference's own expression
        xg.grad = None
        d = -2 * torch.matmul(xg, xg.permute(0, 2, 1)) + (xg ** 2).sum(-1).view(B, N, 1) + (xg ** 2).sum(-1).view(B, 1, N)
        (torch.exp(-d / (2.0 * h * h)) / (2.5 * h)).mean(dim=-1).backward(gd)

    err = float((kde_fwd() - composed_fwd()).abs().max() / composed_fwd().abs().max())
    t = timed_pair([kde_fwd, composed_fwd, kde_step, composed_step])
    mat = 4 * B * N * N
    res["compute_density"] = {
        "max_rel_difference_forward": err,
        "kernel_forward_ms": t[0], "composed_forward_ms": t[1], "kernel_forward_backward_ms": t[2], "composed_forward_backward_ms": t[3],
        "forward_speedup": t[1]["median"] / t[0]["median"], "forward_backward_speedup": t[3]["median"] / t[2]["median"],
        "kernel_bytes": {"forward": 4 * B * N * (3 + 2), "forward_backward": 4 * B * N * (3 + 2) + 4 * B * N * (3 + 1 + 3)},
        "composed_bytes_at_least": {"forward": 4 * B * N * 3 * 2 + mat * (1 + 2 + 2 + 2 + 1),
                                    "note": "square_distance writes [B,N,N]; the negate/divide, exp and divide passes each read and write it; the mean reads it"},
    }

    # ---- the PointConv product
    Q = B * S
    F = torch.randn(Q * K, C, generator=g).cuda().requires_grad_(True)
    Wt = torch.randn(Q * K, 16, generator=g).cuda().requires_grad_(True)
    dens = torch.rand(Q * K, 1, generator=g).cuda().requires_grad_(True)
    dE = torch.randn(Q, 16 * C, generator=g).cuda()

    def leaves_reset():
        F.grad = None; Wt.grad = None; dens.grad = None

    def agg_fwd():
        with torch.no_grad():
            return pc.pointconv_aggregate(F, Wt, dens, K)

    def matmul_expr(f, w, dn):
        return torch.matmul((f * dn).view(Q, K, C).permute(0, 2, 1), w.view(Q, K, 16)).view(Q, -1)

    def matmul_fwd():
        with torch.no_grad():
            return matmul_expr(F, Wt, dens)

    def agg_step():
        leaves_reset()
        pc.pointconv_aggregate(F, Wt, dens, K).backward(dE)

    def matmul_step():
        leaves_reset()
        matmul_expr(F, Wt, dens).backward(dE)

    err = float((agg_fwd() - matmul_fwd()).abs().max() / matmul_fwd().abs().max())
    t = timed_pair([agg_fwd, matmul_fwd, agg_step, matmul_step])
    fwd_bytes = 4 * Q * (K * (C + 17) + 16 * C)
    bwd_bytes = 4 * Q * (16 * C + K * (C + 17) + K * (C + 17))
    bwd_ms = max(t[2]["median"] - t[0]["median"], 1e-6)
    res["pointconv_aggregate"] = {
        "max_rel_difference_forward": err,
        "kernel_forward_ms": t[0], "matmul_forward_ms": t[1], "kernel_forward_backward_ms": t[2], "matmul_forward_backward_ms": t[3],
        "forward_speedup": t[1]["median"] / t[0]["median"], "forward_backward_speedup": t[3]["median"] / t[2]["median"],
        "kernel_forward": rate(fwd_bytes, t[0]["median"]),
        "kernel_backward_by_difference": rate(bwd_bytes, bwd_ms),
        "matmul_forward": rate(fwd_bytes + 2 * 4 * Q * K * C, t[1]["median"]),
        "note": "the matmul route also writes and reads the density-scaled copy of F; its backward stores further copies (not counted)",
    }

    # ---- one module step
    torch.manual_seed(0)
    m = pc.PointConvDensitySetAbstraction(S, K, 3 + D, a.mlp, h, False).cuda().train()
    xyz_cm = xyz.transpose(1, 2).contiguous()
    pts_cm = torch.randn(B, D, N, generator=g).cuda().requires_grad_(True)

    def step():
        for p in m.parameters():
            p.grad = None
        pts_cm.grad = None
        _, f = m(xyz_cm, pts_cm)
        f.backward(f)

    def fwd():
        with torch.no_grad():
            m(xyz_cm, pts_cm)

    t = timed_pair([step, fwd], 3, 5, 5)
    res["density_set_abstraction"] = {
        "forward_backward_ms": t[0], "forward_only_ms": t[1], "device_kernels_forward_backward": kernel_count(step),
        "stored_bytes": {"feature_rows_F": 4 * Q * K * C, "aggregate_E": 4 * Q * 16 * C},
    }
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
