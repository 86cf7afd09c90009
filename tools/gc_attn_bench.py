#!/usr/bin/env python
"""Microbenchmark of spgan.GC_attn (csrc/gc_attn.hip), Self_Attn2 and Dense_Attn_2D: device-event timing inside a warmed loop, one JSON
document.

Per configuration, on the same GPU in the same process:
  layer       the spgan module: forward, forward + backward, peak memory of one forward + backward;
  reference   the reference's formulation written in torch on the module's own parameter containers (conv -> softmax -> bmm -> the two
              branches -> x * mul + add; conv / batch norm / leaky relu / bmm / softmax; conv / batch norm / leaky relu / cat): the same.
Configurations: GC_attn(128) at [32,128,2048] and [32,128,2048,20], Self_Attn2(128) at [32,128,2048], Dense_Attn_2D(64, mlps=[64,64,128],
atten='gc') at [32,64,2048,20].  `launchers`: the four streaming launchers of spgan.gc_attn alone, in both layouts, as algorithmic bytes
(|x|, 2|x|, 2|x|, 3|x|) over the launcher's device time against the 6.3 TB/s the chip sustains -- pool_fwd includes its combine launch;
kernel-only durations: tools/gc_attn_trace.sh.  The routes are timed alternately; every figure is a median with its min and max over the
repeats.  No ratio is asserted: the file records what was measured.

    python tools/gc_attn_bench.py [--out profiles/gc_attn_bench.json] [--small]
    python tools/gc_attn_bench.py --trace-pass          (the launches tools/gc_attn_trace.sh profiles; no timing)
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sp-gan_amd"))
HBM_TBS = 6.3


def timed(fns, warmup=2, iters=3, repeats=7):
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


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


# ----------------------------------------------------------------------------- the reference's formulations, in torch
def gc_reference(m, x):
    f = x.flatten(2)
    if m.pool == "att":
        ctx = torch.bmm(f, torch.softmax(m.conv_mask(f), dim=2).transpose(1, 2))
    else:
        ctx = f.mean(dim=2, keepdim=True)
    out = f * m.channel_mul_conv(ctx) if m.channel_mul_conv is not None else f
    if m.channel_add_conv is not None:
        out = out + m.channel_add_conv(ctx)
    return out.view(x.shape)


def sa2_reference(m, x):
    f = x.flatten(2)
    attn = torch.softmax(torch.bmm(m.query(f).transpose(1, 2), m.key(f)), dim=1)
    return m.gamma * torch.bmm(m.value(f), attn).view(x.shape) + x


def dense2d_reference(m, x):
    y = None
    for layer in m.dense_modules:
        y = layer(x)
        x = torch.cat([x, y], dim=1)
    return y


def da2d_reference(m, x):
    return gc_reference(m.atten, dense2d_reference(m.dense, x))


def bench_module(name, m, reference, shape, seed):
    g = torch.Generator().manual_seed(seed)
    m = m.cuda().train()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("gamma"):                # the attention units start at gamma = 0 (out == x): compare and time them switched on
                p.fill_(0.5)
    x = torch.randn(shape, generator=g).cuda().requires_grad_(True)
    with torch.no_grad():
        out_shape = m(x).shape
    cot = torch.randn(tuple(out_shape), generator=g).cuda()

    def reset():
        x.grad = None
        for p in m.parameters():
            p.grad = None

    def layer_fwd():
        with torch.no_grad():
            return m(x)

    def reference_fwd():
        with torch.no_grad():
            return reference(m, x)

    def layer_step():
        reset()
        m(x).backward(cot)

    def reference_step():
        reset()
        reference(m, x).backward(cot)

    ref = reference_fwd()
    diff = float((layer_fwd() - ref).abs().max() / ref.abs().max())
    del ref
    t = timed([layer_fwd, reference_fwd, layer_step, reference_step])
    size = x.numel() * 4
    res = {"layer": name, "shape": list(shape), "x_bytes": size, "max_rel_difference_forward": diff,
           "layer_forward_ms": t[0], "reference_forward_ms": t[1], "layer_forward_backward_ms": t[2], "reference_forward_backward_ms": t[3],
           "measured_ratio_forward": t[1]["median"] / t[0]["median"], "measured_ratio_forward_backward": t[3]["median"] / t[2]["median"],
           "peak_bytes_forward_backward": {"layer": peak_bytes(layer_step), "reference": peak_bytes(reference_step)}}
    res["peak_over_x"] = {k: v / size for k, v in res["peak_bytes_forward_backward"].items()}
    return res


def launcher_args(B, C, L, layout, seed=0):
    g = torch.Generator().manual_seed(seed)
    shape = (B, C, L) if layout == "cm" else (B * L, C)
    x, cot = torch.randn(shape, generator=g).cuda(), torch.randn(shape, generator=g).cuda()
    w = (torch.randn(C, generator=g) / C ** 0.5).cuda()
    bias = torch.zeros(1).cuda()
    mul, add, dctx = torch.rand(B, C, generator=g).cuda(), torch.randn(B, C, generator=g).cuda(), (torch.randn(B, C, generator=g) / L).cuda()
    return x, cot, w, bias, mul, add, dctx


def bench_launchers(B, C, L, layout):
    from spgan import gc_attn
    x, cot, w, bias, mul, add, dctx = launcher_args(B, C, L, layout)
    ctx, lse, stat, m = gc_attn.pool_fwd(x, layout, B, L, w, bias)
    fns = [lambda: gc_attn.pool_fwd(x, layout, B, L, w, bias), lambda: gc_attn.apply_fwd(x, layout, B, L, mul, add),
           lambda: gc_attn.bwd_reduce(x, cot, layout, B, L), lambda: gc_attn.bwd_apply(x, cot, layout, B, L, mul, dctx, ctx, w, m, stat)]
    t = timed(fns, iters=5)
    size = x.numel() * 4
    res = {"layout": layout, "shape": [B, C, L], "x_bytes": size, "hbm_sustained_tb_per_s": HBM_TBS}
    for name, passes, tt in zip(("pool_fwd", "apply_fwd", "bwd_reduce", "bwd_apply"), (1, 2, 2, 3), t):
        tbs = passes * size / tt["median"] * 1e-9
        res[name] = {"ms": tt, "algorithmic_bytes": passes * size, "tb_per_s": tbs, "fraction_of_sustained": tbs / HBM_TBS}
    return res


def trace_pass(B=32, C=128, L=40960, reps=5):
    """what tools/gc_attn_trace.sh profiles: GC_attn(128) forward + backward in both layouts"""
    import spgan
    torch.manual_seed(0)
    m = spgan.GC_attn(C).cuda()
    for layout in ("cm", "pm"):
        x = torch.randn((B, C, L) if layout == "cm" else (B * L, C), device="cuda").requires_grad_(True)
        cot = torch.randn_like(x)
        for _ in range(reps):
            x.grad = None
            (m(x) if layout == "cm" else m.forward_pm(x, B, L)).backward(cot)
        torch.cuda.synchronize()
        del x, cot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a 16th of the positions: a quick functional pass")
    ap.add_argument("--trace-pass", action="store_true")
    a = ap.parse_args()
    if a.trace_pass:
        trace_pass()
        return
    import spgan
    N, k = (128, 20) if a.small else (2048, 20)
    torch.manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "timing": "device events; median / min / max of 7 repeats of 3 calls (launchers: 5) after 2 warm-up rounds",
           "configs": [bench_module("GC_attn(128)", spgan.GC_attn(128), gc_reference, (32, 128, N), 0),
                       bench_module("GC_attn(128)", spgan.GC_attn(128), gc_reference, (32, 128, N, k), 1),
                       bench_module("Self_Attn2(128)", spgan.Self_Attn2(128), sa2_reference, (32, 128, N), 2),
                       bench_module("Dense_Attn_2D(64, mlps=[64,64,128], atten='gc')", spgan.Dense_Attn_2D(64, mlps=[64, 64, 128]), da2d_reference,
                                    (32, 64, N, k), 3)],
           "launchers": [bench_launchers(32, 128, L, layout) for L in (N, N * k) for layout in ("cm", "pm")]}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
