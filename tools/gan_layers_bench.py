#!/usr/bin/env python
"""Times the GAN-stabiliser layers of spgan.gan_layers against the reference's formulation in torch on the same GPU and writes
profiles/gan_layers_bench.json.

  * spectral norm: the critic's eight weights as ONE group (spgan.gan_layers.sn_group, torch.nn.utils.spectral_norm's rule, one power
    iteration) against eight torch.nn.utils.spectral_norm layers whose hooks are called one after the other; kernel launches of both
    counted with torch.profiler;
  * MinibatchStdDev at [32,256,2048], LayerEpilogue (noise, LeakyReLU, pixel norm, instance norm) at [32,128,2048], AdaptiveInstanceNorm at
    [32,128,2048,1] against the reference's chains of torch ops; peak memory of one forward + backward above the resident inputs, and
    the bytes the algorithm has to move (computed from the shapes, below) per second against the 6.3 TB/s the README takes as sustained.

Every figure: median of 21 samples with min and max; a sample is the device-event time of `reps` back-to-back calls (reps chosen so
that a sample lasts about 20 ms) divided by reps; the two routes alternate sample by sample.  forward = forward alone under no_grad;
fwdbwd = forward + backward with a fixed cotangent g.

    python tools/gan_layers_bench.py [--out profiles/gan_layers_bench.json] [--samples 21]
"""
import argparse
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sp-gan_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch                      # noqa: E402
import torch.nn as nn             # noqa: E402
import torch.nn.functional as F   # noqa: E402

import spgan                      # noqa: E402
from spgan import gan_layers as gl   # noqa: E402

SUSTAINED = 6.3e12
CRITIC = [(64, 3), (128, 64), (256, 128), (1024, 256), (512, 1024), (256, 512), (64, 256), (1, 64)]
DEV = "cuda"


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def compare(routes, samples):
    """routes: {name: fn}; -> {name: {median_us, min_us, max_us, reps}}; the routes alternate sample by sample"""
    reps = {}
    for name, fn in routes.items():
        for _ in range(3):
            fn()                                       # warm-up: code objects, library algorithm choices, allocator
        torch.cuda.synchronize()
        t = timed(fn, 5)
        reps[name] = max(5, min(2000, int(0.02 / max(t, 1e-7))))
    got = {name: [] for name in routes}
    for _ in range(samples):
        for name, fn in routes.items():
            got[name].append(timed(fn, reps[name]))
    return {name: {"median_us": statistics.median(v) * 1e6, "min_us": min(v) * 1e6, "max_us": max(v) * 1e6, "reps": reps[name]}
            for name, v in got.items()}


def launches(fn):
    """kernel launches of one call, counted by torch.profiler (None with the reason when the profiler reports no device activity)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n if n > 0 else None
    except Exception as e:                                   # noqa: BLE001
        return "not measured: %s" % e


def peak_bytes(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def rate(entry, nbytes):
    entry["bytes_moved"] = nbytes
    entry["TB_per_s"] = nbytes / (entry["median_us"] * 1e-6) / 1e12
    entry["share_of_6.3TB_per_s"] = nbytes / (entry["median_us"] * 1e-6) / SUSTAINED
    return entry


def bench_layer(name, ours, theirs, inputs, params, fwd_bytes, fwdbwd_bytes, samples, hip_launches):
    """ours / theirs: callables over `inputs`; the backward takes the gradients of the inputs that require grad and of `params`"""
    out = {}
    g = torch.randn_like(ours(*inputs))

    def fwd(f):
        def run():
            with torch.no_grad():
                f(*inputs)
        return run

    def fwdbwd(f):
        def run():
            torch.autograd.grad(f(*inputs), [t for t in inputs if t.requires_grad] + list(params), g)
        return run
    for mode, wrap, nbytes in (("forward", fwd, fwd_bytes), ("fwdbwd", fwdbwd, fwdbwd_bytes)):
        r = compare({"hip": wrap(ours), "torch": wrap(theirs)}, samples)
        for k in r:
            rate(r[k], nbytes)
            r[k]["peak_bytes"] = peak_bytes(wrap(ours if k == "hip" else theirs))
            r[k]["launches"] = launches(wrap(ours if k == "hip" else theirs))
        r["hip"]["launches_by_design"] = hip_launches[mode]
        r["speedup_hip_over_torch"] = r["torch"]["median_us"] / r["hip"]["median_us"]
        out[mode] = r
        print("%s %s: hip %.1f us (%.2f TB/s), torch %.1f us, x%.2f" % (name, mode, r["hip"]["median_us"], r["hip"]["TB_per_s"],
                                                                       r["torch"]["median_us"], r["speedup_hip_over_torch"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gan_layers_bench.json"))
    ap.add_argument("--samples", type=int, default=21)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gan_layers_bench needs a GPU: nothing is measured without one")
    torch.manual_seed(0)
    doc = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "sustained_bytes_per_s": SUSTAINED}

    # ---------------------------------------------------------------- spectral norm: eight weights, one group
    Ws = [torch.randn(s, device=DEV, requires_grad=True) for s in CRITIC]
    us = [F.normalize(torch.randn(s[0], device=DEV), dim=0) for s in CRITIC]
    vs = [F.normalize(torch.randn(s[1], device=DEV), dim=0) for s in CRITIC]
    Gs = [torch.randn(s, device=DEV) for s in CRITIC]
    layers = []
    for s, W in zip(CRITIC, Ws):
        m = nn.Linear(s[1], s[0]).to(DEV)
        m.weight.data.copy_(W.data)
        layers.append(torch.nn.utils.spectral_norm(m).train())
    hooks = [next(h for h in m._forward_pre_hooks.values()) for m in layers]

    def hip_fwd():
        return gl.sn_group(Ws, us, vs, 1, gl.RULE_F_NORMALIZE, 1e-12)

    def torch_fwd():
        return [h.compute_weight(m, True) for h, m in zip(hooks, layers)]

    def nograd(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def hip_fb():
        torch.autograd.grad(hip_fwd(), Ws, Gs)

    def torch_fb():
        torch.autograd.grad(torch_fwd(), [m.weight_orig for m in layers], Gs)
    sn = {}
    nW = sum(s[0] * s[1] for s in CRITIC)
    for mode, a, b, passes in (("forward", nograd(hip_fwd), nograd(torch_fwd), 4), ("fwdbwd", hip_fb, torch_fb, 4 + 4)):
        r = compare({"hip": a, "torch": b}, args.samples)
        r["hip"]["launches"], r["torch"]["launches"] = launches(a), launches(b)
        r["speedup_hip_over_torch"] = r["torch"]["median_us"] / r["hip"]["median_us"]
        # forward: W read by W^T u, by W v and by the quotient, written once; backward: G and W read by the reduction, G read and dW written
        rate(r["hip"], 4 * nW * passes)
        sn[mode] = r
        print("spectral norm %s: hip %.1f us (%s launches), torch %.1f us (%s launches)" % (
            mode, r["hip"]["median_us"], r["hip"]["launches"], r["torch"]["median_us"], r["torch"]["launches"]), flush=True)
    sn["hip_launches_by_design"] = {"forward": 5, "backward": 2, "note": "4 per power iteration + 1, whatever the number of weights"}
    sn["weights"] = CRITIC
    doc["spectral_norm_critic_group"] = sn

    # ---------------------------------------------------------------- minibatch stddev
    B, C, N = 32, 256, 2048
    x = torch.randn(B, C, N, device=DEV, requires_grad=True)
    ref_mb = MinibatchStdDevTorch(4)
    e = 4 * B * C * N
    e1 = 4 * B * (C + 1) * N
    doc["MinibatchStdDev_32x256x2048"] = bench_layer("MinibatchStdDev", spgan.MinibatchStdDev(4), ref_mb, [x], [], e + e1, (e + e1) + (e + e1 + e),
                                                     args.samples, {"forward": 2, "fwdbwd": 4})

    # ---------------------------------------------------------------- layer epilogue, all stages
    B, C, N = 32, 128, 2048
    x = torch.randn(B, C, N, device=DEV, requires_grad=True)
    nz = torch.randn(B, 1, N, device=DEV)
    ours = spgan.LayerEpilogue(C, 0, False, True, True, True, False, nn.LeakyReLU(0.2)).to(DEV)
    ours.top_epi.noise.weight.data.normal_()
    ours.top_epi.noise.noise = nz
    w = ours.top_epi.noise.weight

    def theirs(x_):
        t = F.leaky_relu(x_ + w.view(1, -1, 1) * nz, 0.2)
        t = t * torch.rsqrt(torch.mean(t ** 2, dim=1, keepdim=True) + 1e-8)
        return F.instance_norm(t.unsqueeze(0), eps=1e-5).squeeze(0)           # nn.InstanceNorm2d on the 3-D tensor
    e = 4 * B * C * N
    doc["LayerEpilogue_32x128x2048"] = bench_layer("LayerEpilogue", ours, theirs, [x], [w], 3 * e, 3 * e + 5 * e, args.samples,
                                                   {"forward": 3, "fwdbwd": 3 + 4})

    # ---------------------------------------------------------------- AdaIN
    x = torch.randn(B, C, N, 1, device=DEV, requires_grad=True)
    style = torch.randn(B, 128, device=DEV, requires_grad=True)
    ours = spgan.AdaptiveInstanceNorm(C, 128).to(DEV)

    def theirs_adain(x_, s_):
        gb = F.linear(s_, ours.style.weight, ours.style.bias).unsqueeze(2).unsqueeze(3)
        gamma, beta = gb.chunk(2, 1)
        return gamma * F.instance_norm(x_, eps=1e-5) + beta
    doc["AdaptiveInstanceNorm_32x128x2048x1"] = bench_layer("AdaptiveInstanceNorm", ours, theirs_adain, [x, style],
                                                            [ours.style.linear.weight_orig, ours.style.linear.bias], 3 * e, 3 * e + 5 * e,
                                                            args.samples, {"forward": 3, "fwdbwd": 3 + 3})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


class MinibatchStdDevTorch(nn.Module):
    """the reference's formulation (Generation/modules.py:97-135) in torch ops"""

    def __init__(self, group_size=4):
        super().__init__()
        self.group_size = group_size

    def forward(self, x, alpha=1e-8):
        B, C, N = x.shape
        G = self.group_size if B > self.group_size else B
        y = torch.reshape(x, [G, -1, C, N])
        y = y - y.mean(dim=0, keepdim=True)
        y = torch.sqrt(y.pow(2).mean(dim=0, keepdim=False) + alpha)
        y = y.mean(dim=[1, 2], keepdim=True)
        y = y.repeat(G, 1, N)
        return torch.cat([x, y], 1)


if __name__ == "__main__":
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        main()
