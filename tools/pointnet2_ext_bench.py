#!/usr/bin/env python
"""Microbenchmark of the pointnet2 extension's set abstraction (spgan.pointnet2_modules, csrc/sa_group.hip): device-event timing inside a
warmed loop, one JSON document.  GPU only.

At B 32, N 2048, 64 input features (random clouds in the unit cube, train mode):

  msg      PointnetSAModuleMSG(npoint=512, radii=[0.1, 0.2, 0.4], nsamples=[16, 32, 64], mlps=[[64, 64, 64, 128]] * 3)
  single   PointnetSAModule(npoint=512, radius=0.2, nsample=32, mlp=[64, 64, 128])
           each forward and forward + backward, with the peak memory of one call, on three routes:
             fused      the hoisted first layer (fused=True),
             unfused    the reference's forward over the ops (fused=False),
             previous   spgan.pointnet_util.PointNetSetAbstractionMsg / PointNetSetAbstraction at the same shape, the route that existed
                        before (its farthest point sampling starts at point 0 here as well);
  query    pointnet2_utils.ball_query_multi of the three radii against three ball_query calls.
The routes take turns in the same process; every figure is a median with its min and max over 21 repeats of one call after 3 warm-up
rounds.  "faster" compares non-overlapping min-max ranges: a route is faster only when its slowest repeat beats the other's fastest.
No ratio is asserted.

    python tools/pointnet2_ext_bench.py [--out FILE] [--quick]          (default: profiles/pointnet2_ext_bench.json)
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

B, N, C, NPOINT = 32, 2048, 64, 512


def faster(a, b):
    """a is faster than b only when a's whole range lies below b's."""
    return a["max"] < b["min"]


def bench_module(spgan, name, radii, nsamples, mlp, quick):
    pm, pu = spgan.pointnet2_modules, spgan.pointnet_util
    g = torch.Generator().manual_seed(len(radii))
    xyz = torch.rand(B, N, 3, generator=g).cuda().requires_grad_(True)
    feat = torch.randn(B, C, N, generator=g).cuda().requires_grad_(True)
    xyz_cm = xyz.detach().transpose(1, 2).contiguous().requires_grad_(True)
    start = torch.zeros(B, dtype=torch.long, device="cuda")
    torch.manual_seed(0)
    if len(radii) > 1:
        new = pm.PointnetSAModuleMSG(npoint=NPOINT, radii=list(radii), nsamples=list(nsamples), mlps=[list(mlp) for _ in radii]).cuda().train()
        old = pu.PointNetSetAbstractionMsg(NPOINT, list(radii), list(nsamples), C, [list(mlp[1:]) for _ in radii]).cuda().train()
    else:
        new = pm.PointnetSAModule(npoint=NPOINT, radius=radii[0], nsample=nsamples[0], mlp=list(mlp)).cuda().train()
        old = pu.PointNetSetAbstraction(NPOINT, radii[0], nsamples[0], C + 3, list(mlp[1:]), False).cuda().train()
    Cout = len(radii) * mlp[-1]
    cot = torch.randn(B, Cout, NPOINT, generator=g).cuda()

    def call(route):
        if route == "previous":
            return old(xyz_cm, feat, start=start)[1]
        new.fused = route == "fused"
        return new(xyz, feat)[1]

    def fwd(route):
        def run():
            with torch.no_grad():
                return call(route)
        return run

    def step(route):
        def run():
            xyz.grad = feat.grad = xyz_cm.grad = None
            for p in list(new.parameters()) + list(old.parameters()):
                p.grad = None
            call(route).backward(cot)
        return run
    routes = ["fused", "unfused", "previous"]
    with torch.no_grad():
        a, b = call("fused"), call("unfused")
    rec = {"op": name, "shape": dict(B=B, N=N, C=C, npoint=NPOINT, radii=list(radii), nsamples=list(nsamples), mlp=list(mlp)),
           "fused_vs_unfused_rel_l2": float((a - b).norm() / b.norm())}
    reps = 5 if quick else 21
    tf = timed_pair([fwd(r) for r in routes], warmup=3, iters=1, repeats=reps)
    ts = timed_pair([step(r) for r in routes], warmup=3, iters=1, repeats=reps)
    for i, r in enumerate(routes):
        rec[r] = {"forward_ms": tf[i], "forward_backward_ms": ts[i], "peak_bytes_forward": peak_bytes(fwd(r)),
                  "peak_bytes_forward_backward": peak_bytes(step(r))}
    rec["grouped_tensor_bytes"] = sum(B * NPOINT * k * (3 + C) * 4 for k in nsamples)
    rec["fused_faster_than_unfused_forward"] = faster(tf[0], tf[1])
    rec["fused_faster_than_unfused_forward_backward"] = faster(ts[0], ts[1])
    rec["unfused_faster_than_fused_forward_backward"] = faster(ts[1], ts[0])
    rec["fused_faster_than_previous_forward_backward"] = faster(ts[0], ts[2])
    return rec


def bench_query(spgan, quick):
    p2 = spgan.pointnet2_utils
    g = torch.Generator().manual_seed(9)
    xyz = torch.rand(B, N, 3, generator=g).cuda()
    new_xyz = xyz[:, :NPOINT].contiguous()
    radii, nsamples = [0.1, 0.2, 0.4], [16, 32, 64]
    multi = p2.ball_query_multi(radii, nsamples, xyz, new_xyz)
    assert all(torch.equal(t, p2.ball_query(r, k, xyz, new_xyz)) for r, k, t in zip(radii, nsamples, multi))
    t = timed_pair([lambda: p2.ball_query_multi(radii, nsamples, xyz, new_xyz),
                    lambda: [p2.ball_query(r, k, xyz, new_xyz) for r, k in zip(radii, nsamples)]], warmup=3, iters=1, repeats=5 if quick else 21)
    return {"op": "ball_query", "shape": dict(B=B, N=N, npoint=NPOINT, radii=radii, nsamples=nsamples), "multi_radius_ms": t[0],
            "three_single_queries_ms": t[1], "multi_faster_than_single": faster(t[0], t[1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointnet2_ext_bench.json"))
    ap.add_argument("--quick", action="store_true", help="fewer repeats")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointnet2_ext_bench.py needs a GPU")
    import spgan
    reps = 5 if a.quick else 21
    res = {"device": torch.cuda.get_device_name(0),
           "timing": "device events; median / min / max of %d repeats of 1 call after 3 warm-up rounds; the routes take turns" % reps, "configs": []}
    jobs = [lambda: bench_module(spgan, "msg", (0.1, 0.2, 0.4), (16, 32, 64), (C, 64, 64, 128), a.quick),
            lambda: bench_module(spgan, "single", (0.2,), (32,), (C, 64, 128), a.quick), lambda: bench_query(spgan, a.quick)]
    for job in jobs:
        rec = job()
        res["configs"].append(rec)
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
