#!/usr/bin/env python
"""Microbenchmark of the PointNet++ path (spgan.pointnet_util): device-event timing inside a warmed loop, one JSON document.

  * three_nn + three_interpolate (fused pair, no [B,N,S] matrix) against the route the library offered before them:
    square_distance -> torch.sort -> index_points -> weighted sum, with the bytes each route moves;
  * one PointNetSetAbstraction forward + backward (stored-tensor route: the grouped [B,S,K,3+D] rows are written by
    spgan_group_concat and read by the first GEMM).

    python tools/pointnet2_bench.py [--out profiles/pointnet2_bench.json] [--B 32 --N 2048 --S 512 --K 32 --D 64]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sp-gan_amd"))


def timed(fn, warmup=10, iters=30, repeats=5):
    """Median over `repeats` of the mean device time (ms) of `iters` back-to-back calls, after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32); ap.add_argument("--N", type=int, default=2048); ap.add_argument("--S", type=int, default=512)
    ap.add_argument("--K", type=int, default=32); ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--mlp", type=int, nargs="+", default=[64, 64, 128])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from spgan import pointnet_util as pu
    B, N, S, K, D = a.B, a.N, a.S, a.K, a.D
    g = torch.Generator().manual_seed(0)
    xyz1 = torch.rand(B, N, 3, generator=g).cuda()
    xyz2 = xyz1[:, :S].contiguous()
    p2 = torch.randn(B, S, D, generator=g).cuda()

    def fused():
        idx, w = pu.three_nn(xyz1, xyz2)
        return pu.three_interpolate(p2, idx, w)

    def unfused():
        dist, idx = pu.square_distance(xyz1, xyz2).sort(dim=-1)
        dist, idx = dist[:, :, :3], idx[:, :, :3].contiguous()
        r = 1.0 / (dist + 1e-8)
        w = r / r.sum(dim=2, keepdim=True)
        return (pu.index_points(p2, idx) * w.unsqueeze(-1)).sum(dim=2)

    err = float((fused() - unfused()).abs().max())
    tf, tu = timed(fused), timed(unfused)
    coords = 4 * 3 * B * (N + S)
    feats = 4 * B * D * (S + N)
    res = {
        "device": torch.cuda.get_device_name(0), "shape": dict(B=B, N=N, S=S, K=K, D=D, mlp=a.mlp),
        "three_nn_interpolate": {
            "fused_ms": {"median": tf[0], "min": tf[1], "max": tf[2]},
            "square_distance_sort_route_ms": {"median": tu[0], "min": tu[1], "max": tu[2]},
            "speedup": tu[0] / tf[0], "max_abs_difference": err,
            "fused_bytes": {"coordinates": coords, "idx_weight_write_read": 2 * B * N * 3 * 12, "features_read_write": feats},
            "sort_route_bytes": {"coordinates": coords, "distance_matrix_write": 4 * B * N * S,
                                 "sort_read_write_at_least": 2 * 4 * B * N * S + 2 * 8 * B * N * S, "features_read_write": feats + 4 * B * N * 3 * D * 2},
        },
    }
    torch.manual_seed(0)
    sa = pu.PointNetSetAbstraction(S, 0.2, K, 3 + D, a.mlp, False).cuda().train()
    xyz_cm = xyz1.transpose(1, 2).contiguous()
    pts_cm = torch.randn(B, D, N, generator=g).cuda().requires_grad_(True)
    start = torch.zeros(B, dtype=torch.long).cuda()

    def sa_step():
        for p in sa.parameters():
            p.grad = None
        pts_cm.grad = None
        _, f = sa(xyz_cm, pts_cm, start=start)
        f.backward(f)

    def sa_fwd():
        with torch.no_grad():
            sa(xyz_cm, pts_cm, start=start)

    def sampling():
        pu.sample_and_group(S, 0.2, K, xyz1, None, start=start)

    ts, tfw, tsm = timed(sa_step, 5, 10), timed(sa_fwd, 5, 10), timed(sampling, 5, 10)
    res["set_abstraction"] = {
        "route": "stored grouped rows (spgan_group_concat); the gather-and-centre GEMM prologue is not built",
        "forward_backward_ms": {"median": ts[0], "min": ts[1], "max": ts[2]},
        "forward_only_ms": {"median": tfw[0], "min": tfw[1], "max": tfw[2]},
        "of_which_fps_ball_query_group_ms": {"median": tsm[0], "min": tsm[1], "max": tsm[2]},
        "grouped_rows_bytes_written_and_read_back": 2 * 4 * B * S * K * (3 + D),
    }
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
