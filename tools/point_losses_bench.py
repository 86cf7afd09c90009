#!/usr/bin/env python
"""Microbenchmark of get_repulsion_loss (csrc/point_losses.hip): device-event timing inside a warmed loop, one JSON document.  GPU only.

Shapes: [32,2048,3], nsample 20, radius 0.07, h 0.001 on
  sphere   the unit-sphere cloud of spgan/data/balls.npz under 32 seeded rotations (two or three points per ball: every scan runs to the
           end of the cloud and most slots are padding),
  dense    the same clouds scaled by 0.15 (about a hundred points per ball: most balls overflow nsample and the scan stops early).
Routes, forward and forward + backward, with the peak memory of one call:
  fused        spgan.model_utils.get_repulsion_loss, the backward through spgan_gather_csr's slot lists (the default),
  fused_table  the same forward, the backward by the walk over the cloud's index table,
  composed    (a) the launchers that existed before: pointops.ballquery, pointops.grouping, the subtraction, the reduction, torch.topk
              and the tail,
  torch       (b) the plain torch formulation: a [B,N,N] distance matrix, a masked sort for the first-nsample rule, a gather, topk.
The routes take turns in the same process; every figure is a median with its min and max over 21 repeats of 10 back-to-back calls after
3 warm-up rounds.  "below" compares min-max ranges: fused lies below composed only when its slowest repeat is faster than the other's
fastest.  The scan's own bound: the candidates the forward scan evaluates (counted from the data: 64 per step until the nsample-th hit)
over the forward time, against 256 CUs * 4 SIMDs * 16 lanes * 2.4 GHz / 9 separately rounded operations per candidate (3 subtractions,
3 products, 2 sums, 1 comparison; the kernel forbids contraction, so no FMA).

    python tools/point_losses_bench.py [--out FILE] [--quick]          (default: profiles/point_losses_bench.json)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sp-gan_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from deform_bench import peak_bytes, timed_pair          # noqa: E402

B, N, NSAMPLE, RADIUS, H = 32, 2048, 20, 0.07, 0.001
VALU_LANE_OPS = 256 * 4 * 16 * 2.4e9
OPS_PER_CANDIDATE = 9


def clouds(scale):
    ball = torch.tensor(np.load(os.path.join(ROOT, "sp-gan_amd", "spgan", "data", "balls.npz"))["ball_%d" % N], dtype=torch.float64)
    g = torch.Generator().manual_seed(17)
    q, _ = torch.linalg.qr(torch.randn(B, 3, 3, generator=g, dtype=torch.float64))
    return (torch.matmul(ball[None], q) * scale).float().cuda()


def composed(po):
    def fn(x):
        idx = po.ballquery(RADIUS, NSAMPLE, x, x)
        xt = x.transpose(1, 2).contiguous()
        g = po.grouping(xt, idx) - xt.unsqueeze(-1)                     # [B,3,N,K]
        d = (g * g).sum(1)
        val = torch.topk(-d, 5, dim=2)[0][:, :, 1:]
        return torch.relu(H + val).mean()
    return fn


def plain_groups(x):
    """-> (idx [B,N,nsample] of the first-nsample rule, cnt [B,N], the sorted hit lists)."""
    d2 = ((x[:, :, None, :] - x[:, None, :, :]) ** 2).sum(-1)
    ar = torch.arange(N, device=x.device)
    mask = d2 < RADIUS * RADIUS
    order = torch.sort(torch.where(mask, ar, N + ar), dim=2).indices[:, :, :NSAMPLE]
    cnt = mask.sum(2).clamp(max=NSAMPLE)
    slot = torch.arange(NSAMPLE, device=x.device)
    return torch.gather(order, 2, torch.where(slot < cnt[..., None], slot, torch.zeros_like(slot)).expand(B, N, NSAMPLE)), mask.sum(2), order


def plain(x):
    with torch.no_grad():
        idx, _, _ = plain_groups(x)
    g = x[torch.arange(B, device=x.device)[:, None, None], idx] - x[:, :, None, :]
    d = (g * g).sum(-1)
    val = torch.topk(-d, 5, dim=2)[0][:, :, 1:]
    return torch.relu(H + val).mean()


def scanned_candidates(x):
    """What the forward scan evaluates: 64 candidates per step up to the step that holds the nsample-th hit, else the whole cloud."""
    with torch.no_grad():
        _, hits, order = plain_groups(x)
    last = order[:, :, NSAMPLE - 1]
    steps = torch.where(hits >= NSAMPLE, last // 64 + 1, torch.full_like(last, (N + 63) // 64))
    return int((steps * 64).clamp(max=N).sum()), float((hits > NSAMPLE).float().mean()), float(hits.float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_losses_bench.json"))
    ap.add_argument("--quick", action="store_true", help="fewer repeats")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("point_losses_bench.py needs a GPU")
    import spgan
    from spgan import model_utils as mu
    repeats, iters = (5, 3) if a.quick else (21, 10)
    res = {"device": torch.cuda.get_device_name(0), "shape": dict(B=B, N=N, nsample=NSAMPLE, radius=RADIUS, h=H),
           "timing": "device events; median / min / max of %d repeats of %d back-to-back calls after 3 warm-up rounds; the routes take turns"
                     % (repeats, iters),
           "scan_bound": "%d separately rounded VALU operations per candidate at %.3g lane-operations/s" % (OPS_PER_CANDIDATE, VALU_LANE_OPS),
           "configs": []}

    fused = lambda x: mu.get_repulsion_loss(x, NSAMPLE, RADIUS, h=H)          # noqa: E731
    routes = {"fused": fused, "fused_table": fused, "composed": composed(spgan.pointops), "torch": plain}
    for name, scale in (("sphere", 1.0), ("dense", 0.15)):
        x = clouds(scale).requires_grad_(True)

        def fwd(fn):
            def run():
                with torch.no_grad():
                    return fn(x)
            return run

        def step(r):
            def run():
                x.grad = None
                mu.BACKWARD_ROUTE = "table" if r == "fused_table" else "csr"      # read when the backward runs: set around the whole step
                try:
                    routes[r](x).backward()
                finally:
                    mu.BACKWARD_ROUTE = "csr"
            return run
        names = list(routes)
        losses = {r: float(routes[r](x.detach())) for r in names}
        step("fused")()
        g_csr = x.grad.clone()
        step("fused_table")()
        g_table = x.grad.clone()
        step("torch")()
        g_torch = x.grad.clone()
        tf = timed_pair([fwd(routes[r]) for r in names if r != "fused_table"], warmup=3, iters=iters, repeats=repeats)
        ts = timed_pair([step(r) for r in names], warmup=3, iters=iters, repeats=repeats)
        fnames = [r for r in names if r != "fused_table"]
        cand, overflow, mean_hits = scanned_candidates(x)
        rec = {"cloud": name, "mean_points_per_ball": mean_hits, "share_of_balls_over_nsample": overflow, "losses": losses,
               "max_abs_grad_table_minus_csr": float((g_table - g_csr).abs().max()),
               "max_abs_grad_table_minus_torch": float((g_table - g_torch).abs().max()), "max_abs_grad": float(g_torch.abs().max()),
               "scanned_candidates": cand, "all_pairs": B * N * N}
        for i, r in enumerate(fnames):
            rec.setdefault(r, {})["forward_ms"] = tf[i]
            rec[r]["peak_bytes_forward"] = peak_bytes(fwd(routes[r]))
        for i, r in enumerate(names):
            rec.setdefault(r, {})["forward_backward_ms"] = ts[i]
            rec[r]["peak_bytes_forward_backward"] = peak_bytes(step(r))
        rate = cand / (rec["fused"]["forward_ms"]["median"] * 1e-3)
        rec["fused_candidates_per_s"] = rate
        rec["fused_fraction_of_scan_bound"] = rate / (VALU_LANE_OPS / OPS_PER_CANDIDATE)
        rec["fused_below_composed_forward"] = rec["fused"]["forward_ms"]["max"] < rec["composed"]["forward_ms"]["min"]
        rec["fused_below_composed_forward_backward"] = rec["fused"]["forward_backward_ms"]["max"] < rec["composed"]["forward_backward_ms"]["min"]
        rec["csr_below_table_forward_backward"] = rec["fused"]["forward_backward_ms"]["max"] < rec["fused_table"]["forward_backward_ms"]["min"]
        rec["table_below_csr_forward_backward"] = rec["fused_table"]["forward_backward_ms"]["max"] < rec["fused"]["forward_backward_ms"]["min"]
        res["configs"].append(rec)
        print(json.dumps(rec), flush=True)
        del x
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
