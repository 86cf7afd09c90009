#!/usr/bin/env python
"""Microbenchmark of the approxmatch EMD (csrc/approxmatch.hip): device-event timing inside a warmed loop, one JSON document.  GPU only.

  loss       spgan.model_utils.get_emd_loss at [32,2048,3] (unit-cube clouds), forward and forward + backward, with the peak memory of
             one call, against `torch` -- the same formulation in float32 torch ops over dense [B,n,m] tensors (its backward is the
             definition's: the plan held constant, the two gradient sums written out).  The routes take turns in one process.
             Also the fused forward with one wave per block (`fused_1wave`, spgan.approxmatch.SWEEP_WAVES = 1): the placement that lost.
  pairwise   spgan.metrics.pairwise_emd of 64 x 64 clouds of 2048, emd="match_cost", against the torch formulation (one sample cloud
             against the 64 references per dense evaluation, as the fused driver chunks it) and, for orientation only, the auction route,
             which computes a different quantity.
  sweep      exp evaluations per second of the fused forward (30 per point pair: ten levels of sweep 1, 2 and 3) against the register-only
             expf loop of tools/exp/exp_peak.hip.

Every figure is a median with its min and max over 21 repeats after warm-up, eager issue.  "below" compares min-max ranges: a route lies
below another only when its slowest repeat is faster than the other's fastest.

    python tools/approxmatch_bench.py [--out FILE] [--quick]          (default: profiles/approxmatch_bench.json)
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
sys.path.insert(0, os.path.join(ROOT, "tools", "exp"))

from deform_bench import peak_bytes, timed_pair          # noqa: E402

LEVELS = [-(4.0 ** j) for j in range(7, -2, -1)] + [0.0]
EXP_PER_PAIR = 30


def clouds(B, n, seed):
    g = np.random.default_rng(seed)
    return torch.tensor(g.random((B, n, 3)), dtype=torch.float32).cuda()


def torch_plan(a, b):
    """-> (match [B,n,m], diff, dist): the definition in float32 torch ops over dense tensors."""
    B, n, m = a.shape[0], a.shape[1], b.shape[1]
    diff = a[:, :, None, :] - b[:, None, :, :]
    d2 = (diff * diff).sum(-1)
    big = float(max(n, m))
    remain_l = torch.full((B, n), big / n, device=a.device)
    remain_r = torch.full((B, m), big / m, device=a.device)
    match = torch.zeros((B, n, m), device=a.device)
    for level in LEVELS:
        e = torch.exp(level * d2)
        ratio_l = remain_l / (1e-9 + (e * remain_r[:, None, :]).sum(2))
        sumr = remain_r * (e * ratio_l[:, :, None]).sum(1)
        ratio_r = torch.minimum(remain_r / (sumr + 1e-9), torch.ones_like(sumr)) * remain_r
        remain_r = (remain_r - sumr).clamp_min(0)
        w = e * ratio_l[:, :, None] * ratio_r[:, None, :]
        match += w
        remain_l = (remain_l - w.sum(2)).clamp_min(0)
    return match, diff, d2.sqrt()


def torch_cost(a, b):
    match, _, dist = torch_plan(a, b)
    return (match * dist).sum((1, 2))


def torch_loss_and_grads(a, b, radius):
    match, diff, dist = torch_plan(a, b)
    n = a.shape[1]
    loss = ((match * dist).sum((1, 2)) / radius / n).mean()
    t = match / dist.clamp_min(1e-20) / (radius * n * a.shape[0])
    return loss, (t[..., None] * diff).sum(2), -(t[..., None] * diff).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "approxmatch_bench.json"))
    ap.add_argument("--quick", action="store_true", help="small shapes and few repeats (a rehearsal, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("approxmatch_bench.py needs a GPU")
    import spgan
    from spgan import approxmatch as am
    from spgan import metrics, model_utils as mu
    repeats = 3 if a.quick else 21
    B, N = (4, 256) if a.quick else (32, 2048)
    S = 4 if a.quick else 64
    res = {"device": torch.cuda.get_device_name(0), "quick": bool(a.quick),
           "timing": "device events; median / min / max of %d repeats after warm-up; the routes take turns; eager issue" % repeats}

    # ------------------------------------------------------------------------------------------------ loss
    x, y = clouds(B, N, 1).requires_grad_(True), clouds(B, N, 2).requires_grad_(True)
    radius = 0.5

    def fused_fwd():
        with torch.no_grad():
            return mu.get_emd_loss(x, y, radius)

    def fused_1wave():
        am.SWEEP_WAVES = 1
        try:
            return fused_fwd()
        finally:
            am.SWEEP_WAVES = 4

    def torch_fwd():
        with torch.no_grad():
            return (torch_cost(x, y) / radius / N).mean()

    def fused_step():
        x.grad = y.grad = None
        mu.get_emd_loss(x, y, radius).backward()

    def torch_step():
        with torch.no_grad():
            return torch_loss_and_grads(x, y, radius)
    fused_step()
    gx, gy = x.grad.clone(), y.grad.clone()
    tl, tgx, tgy = torch_step()
    loss = {"shape": [B, N, 3], "radius": radius, "loss_fused": float(fused_fwd()), "loss_fused_1wave": float(fused_1wave()),
            "loss_torch": float(tl), "max_abs_grad_fused_minus_torch": float(max((gx - tgx).abs().max(), (gy - tgy).abs().max())),
            "max_abs_grad": float(tgx.abs().max()), "torch_chunked": False}
    del tl, tgx, tgy
    iters = 2 if a.quick else 5
    tf = timed_pair([fused_fwd, fused_1wave, torch_fwd], warmup=2, iters=iters, repeats=repeats)
    ts = timed_pair([fused_step, torch_step], warmup=2, iters=iters, repeats=repeats)
    loss["forward_ms"] = {"fused": tf[0], "fused_1wave": tf[1], "torch": tf[2]}
    loss["forward_backward_ms"] = {"fused": ts[0], "torch": ts[1]}
    loss["peak_bytes_forward"] = {"fused": peak_bytes(fused_fwd), "torch": peak_bytes(torch_fwd)}
    loss["peak_bytes_forward_backward"] = {"fused": peak_bytes(fused_step), "torch": peak_bytes(torch_step)}
    loss["one_plan_bytes"] = B * N * N * 4
    loss["fused_below_torch_forward"] = tf[0]["max"] < tf[2]["min"]
    loss["fused_below_torch_forward_backward"] = ts[0]["max"] < ts[1]["min"]
    loss["four_waves_below_one_wave_forward"] = tf[0]["max"] < tf[1]["min"]
    loss["one_wave_below_four_waves_forward"] = tf[1]["max"] < tf[0]["min"]
    res["loss"] = loss
    print(json.dumps(loss), flush=True)

    # ------------------------------------------------------------------------------------------------ sweep rate
    def cost_only():
        with torch.no_grad():
            return am.match_cost(x, y)
    tc = timed_pair([cost_only], warmup=2, iters=iters, repeats=repeats)[0]
    n_exp = float(B) * N * N * EXP_PER_PAIR
    sweep = {"exp_per_forward": n_exp, "forward_ms": tc, "gexp_per_s": n_exp / (tc["median"] * 1e-3) / 1e9}
    try:
        from run_exp_peak import measure
        probe = measure()
        sweep["probe"] = probe
        sweep["fraction_of_expf_loop"] = sweep["gexp_per_s"] / probe["ceiling_expf_gexp_per_s"]
    except Exception as e:                                   # noqa: BLE001  (the probe is a separate build)
        sweep["probe_error"] = repr(e)
    res["sweep"] = sweep
    print(json.dumps(sweep), flush=True)
    del x, y
    torch.cuda.empty_cache()

    # ------------------------------------------------------------------------------------------------ pairwise
    s, r = clouds(S, N, 3), clouds(S, N, 4)

    def pw_fused():
        return metrics.pairwise_emd(s, r, emd="match_cost")

    def pw_torch():
        with torch.no_grad():
            return torch.stack([torch_cost(s[i:i + 1].expand(S, -1, -1), r) / N for i in range(S)])

    def pw_auction():
        with torch.no_grad():
            return metrics.pairwise_emd(s, r)
    mf, mt = pw_fused(), pw_torch()
    pw = {"shape": [S, S, N], "max_abs_fused_minus_torch": float((mf - mt).abs().max()), "mean_emd_match_cost": float(mf.mean()),
          "mean_emd_auction": float(pw_auction().mean())}
    tp = timed_pair([pw_fused, pw_torch, pw_auction], warmup=1, iters=1, repeats=repeats)
    pw["ms"] = {"fused": tp[0], "torch": tp[1], "auction": tp[2]}
    pw["peak_bytes"] = {"fused": peak_bytes(pw_fused), "torch": peak_bytes(pw_torch), "auction": peak_bytes(pw_auction)}
    pw["fused_below_torch"] = tp[0]["max"] < tp[1]["min"]
    pw["pairs_per_s_fused"] = S * S / (tp[0]["median"] * 1e-3)
    res["pairwise"] = pw
    print(json.dumps(pw), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
