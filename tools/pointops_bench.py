#!/usr/bin/env python
"""Microbenchmark of the pointops family (csrc/pointops.hip): device-event timing inside a warmed loop, one JSON document.  GPU only.

Shapes: B 32, n = m = 2048 and B 16, n = m = 4096 (random clouds in the unit cube).

  knnquery        nsample 20, 64 and 200 next to spgan_knn_point (one thread per query, nsample <= 32 only) and torch.cdist + topk;
  QueryAndGroup   nsample 20, C = 128 features, a kNN graph computed once and injected: forward and forward + backward of
                    fused      spgan_pointops_group_cm, one launch per slice into one buffer (the modules' path),
                    composed   the launchers that existed before: spgan_gather_points_cm per slice on a transposed copy, the
                               subtraction, torch.cat,
                    torch      the reference's formulation in plain torch (transpose, gather, in-place subtraction, cat),
                  with the peak memory of one call and the achieved fraction of the 8 TB/s HBM peak on the (3 + C) * m * K * 4 written bytes.
The routes take turns in the same process; every figure is a median with its min and max over 21 repeats of one call after 3 warm-up
rounds.  "not_slower" compares non-overlapping min-max ranges: a route is slower only when its fastest repeat is slower than the other's
slowest.  No ratio is asserted.

    python tools/pointops_bench.py [--out FILE] [--quick]          (default: profiles/pointops_bench.json)
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

HBM_PEAK = 8.0e12


def not_slower(a, b):
    """a is not slower than b unless a's whole range lies above b's."""
    return not a["min"] > b["max"]


def torch_group(xyz, new_xyz, feat, idx64):
    B, C, n = feat.shape
    _, m, K = idx64.shape
    flat = idx64.reshape(B, 1, m * K)
    gx = torch.gather(xyz.transpose(1, 2).contiguous(), 2, flat.expand(B, 3, m * K)).reshape(B, 3, m, K)
    gx -= new_xyz.transpose(1, 2).unsqueeze(-1)
    gf = torch.gather(feat, 2, flat.expand(B, C, m * K)).reshape(B, C, m, K)
    return torch.cat([gx, gf], dim=1)


def bench_knn(spgan, B, n, quick):
    po, pu = spgan.pointops, spgan.pointnet_util
    g = torch.Generator().manual_seed(n)
    xyz = torch.rand(B, n, 3, generator=g).cuda()
    out = []
    for nsample in (20, 64, 200):
        fns = [lambda: po.knnquery(nsample, xyz, xyz), lambda: torch.cdist(xyz, xyz).topk(nsample, dim=2, largest=False)[1]]
        names = ["pointops_knnquery_ms", "torch_cdist_topk_ms"]
        if nsample <= 32:
            fns.append(lambda: pu.knn_point(nsample, xyz, xyz))
            names.append("spgan_knn_point_ms")
        t = timed_pair(fns, warmup=3, iters=1, repeats=5 if quick else 21)
        rec = {"op": "knnquery", "shape": dict(B=B, n=n, m=n, nsample=nsample)}
        rec.update(dict(zip(names, t)))
        if nsample <= 32:
            rec["knnquery_not_slower_than_knn_point"] = not_slower(t[0], t[2])
            rec["share_of_indices_equal_to_knn_point"] = float((po.knnquery(nsample, xyz, xyz).long() == pu.knn_point(nsample, xyz, xyz)).float().mean())
        out.append(rec)
    return out


def bench_group(spgan, B, n, quick):
    po = spgan.pointops
    C, K = 128, 20
    g = torch.Generator().manual_seed(n + 1)
    xyz = torch.rand(B, n, 3, generator=g).cuda().requires_grad_(True)
    feat = torch.randn(B, C, n, generator=g).cuda().requires_grad_(True)
    cot = torch.randn(B, 3 + C, n, K, generator=g).cuda()
    idx = po.knnquery(K, xyz, xyz)
    idx64 = idx.long()
    mod = po.QueryAndGroup(None, K)

    def fused(a, b, c):
        return po._GroupSlices.apply(a, b, c, idx)

    def composed(a, b, c):
        return po._group_composed(a, b, c, idx)

    def plain(a, b, c):
        return torch_group(a, b, c, idx64)
    routes = {"fused": fused, "composed": composed, "torch": plain}

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn(xyz, xyz, feat)
        return run

    def step(fn):
        def run():
            xyz.grad = feat.grad = None
            fn(xyz, xyz, feat).backward(cot)
        return run
    assert torch.equal(mod(xyz, xyz, feat, idx), fused(xyz, xyz, feat))
    assert torch.equal(fused(xyz, xyz, feat), composed(xyz, xyz, feat)) and torch.equal(fused(xyz, xyz, feat), plain(xyz, xyz, feat))
    names = list(routes)
    tf = timed_pair([fwd(routes[r]) for r in names], warmup=3, iters=1, repeats=5 if quick else 21)
    ts = timed_pair([step(routes[r]) for r in names], warmup=3, iters=1, repeats=5 if quick else 21)
    written = (3 + C) * B * n * K * 4
    rec = {"op": "QueryAndGroup", "shape": dict(B=B, n=n, m=n, nsample=K, C=C), "written_bytes": written}
    for i, r in enumerate(names):
        rec[r] = {"forward_ms": tf[i], "forward_backward_ms": ts[i], "peak_bytes_forward": peak_bytes(fwd(routes[r])),
                  "peak_bytes_forward_backward": peak_bytes(step(routes[r])),
                  "forward_fraction_of_hbm_peak_on_written_bytes": written / (tf[i]["median"] * 1e-3) / HBM_PEAK}
    rec["fused_not_slower_than_composed_forward"] = not_slower(tf[0], tf[1])
    rec["fused_not_slower_than_composed_forward_backward"] = not_slower(ts[0], ts[1])
    return [rec]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointops_bench.json"))
    ap.add_argument("--quick", action="store_true", help="fewer repeats")
    ap.add_argument("--note", default="", help="recorded verbatim (e.g. the kernel shape this build uses)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointops_bench.py needs a GPU")
    import spgan
    res = {"device": torch.cuda.get_device_name(0), "note": a.note,
           "timing": "device events; median / min / max of %d repeats of 1 call after 3 warm-up rounds; the routes take turns" % (5 if a.quick else 21),
           "hbm_peak_bytes_per_s": HBM_PEAK, "configs": []}
    for B, n in ((32, 2048), (16, 4096)):
        for job in (bench_knn, bench_group):
            for rec in job(spgan, B, n, a.quick):
                res["configs"].append(rec)
                print(json.dumps(rec), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
