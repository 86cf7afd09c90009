#!/usr/bin/env python
"""Microbenchmark of the upsampling edge convolution (spgan.upsample_edgeConv, csrc/edge_window.hip): device-event timing inside a
warmed loop, one JSON document.

Per configuration (default upsample_edgeConv(128,256,10) and (3,64,10) at B = 32, N = 2048, train mode): forward and forward +
backward of the layer beside the composed route, on the same GPU and the same kNN graph: spgan.get_edge_features (the [B,2Fin,N,k]
tensor) -> torch.nn.functional.conv2d / batch_norm / leaky_relu -> the transpose / view chain and the concatenation of the reference
-> conv2d / batch_norm / relu -> the final views; peak memory of one forward + backward of either route; the largest difference of
the two outputs.  The two routes are timed alternately in the same process; every figure is a median with its min and max over the
repeats.  No ratio is asserted: the file records what was measured.

    python tools/upsample_bench.py [--out profiles/upsample_bench.json] [--B 32 --N 2048]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sp-gan_amd"))


def timed_pair(fns, warmup=3, iters=5, repeats=7):
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


def bench(spgan, B, N, Fin, Fout, k, seed):
    g = torch.Generator().manual_seed(seed)
    m = spgan.upsample_edgeConv(Fin, Fout, k, -1).cuda().train()
    conv1, bn1, conv2, bn2 = m.inte_conv_hk[0], m.inte_conv_hk[1], m.conv2.conv, m.conv2.bn
    x = (torch.rand(B, Fin, N, generator=g) * 2 - 1 if Fin <= 4 else torch.randn(B, Fin, N, generator=g) * 0.7).cuda().requires_grad_(True)
    cot = torch.randn(B, Fout, 2 * N, generator=g).cuda()
    with torch.no_grad():
        _, idx = spgan.get_edge_features(x.detach(), k, return_idx=True)          # one graph for both routes
    idx32 = spgan.ops.idx_from_local64(idx, B, N, k)      # the layer's own format: an int64 graph is range-checked with a host synchronisation per call

    def composed(xx):
        ee = spgan.get_edge_features(xx, k, idx=idx)                               # [B,2Fin,N,k]
        h = F_.conv2d(ee, conv1.weight, conv1.bias)
        h = F_.leaky_relu(F_.batch_norm(h, None, None, bn1.weight, bn1.bias, True, 0.1, 1e-5), 0.01, inplace=True)
        h = h.transpose(2, 1).contiguous().view(B, N, 2 * Fin, 2, k // 2).contiguous().view(B, N, 2 * Fin, k).permute(0, 2, 1, 3)
        y = F_.conv2d(torch.cat((ee, h), 3), conv2.weight, conv2.bias)
        y = torch.relu(F_.batch_norm(y, None, None, bn2.weight, bn2.bias, True, 0.1, 1e-5))
        return y.contiguous().view(B, Fout, 2, N).contiguous().view(B, Fout, 2 * N)

    def reset():
        x.grad = None
        for p in m.parameters():
            p.grad = None

    def layer_fwd():
        with torch.no_grad():
            return m(x, idx=idx32)

    def composed_fwd():
        with torch.no_grad():
            return composed(x)

    def layer_step():
        reset()
        (m(x, idx=idx32) * cot).sum().backward()

    def composed_step():
        reset()
        (composed(x) * cot).sum().backward()

    ref = composed_fwd()
    diff = float((layer_fwd() - ref).abs().max() / ref.abs().max())
    del ref
    t = timed_pair([layer_fwd, composed_fwd, layer_step, composed_step])
    edge = 4 * B * 2 * Fin * N * k
    w = k // 2 + 1
    return {
        "layer": "upsample_edgeConv(%d,%d,%d)" % (Fin, Fout, k), "shape": dict(B=B, N=N),
        "max_rel_difference_forward": diff,
        "layer_forward_ms": t[0], "composed_forward_ms": t[1], "layer_forward_backward_ms": t[2], "composed_forward_backward_ms": t[3],
        "measured_ratio_forward": t[1]["median"] / t[0]["median"], "measured_ratio_forward_backward": t[3]["median"] / t[2]["median"],
        "peak_bytes_forward_backward": {"layer": peak_bytes(layer_step), "composed": peak_bytes(composed_step), "one_edge_tensor": edge},
        "forward_flops": {"layer": 2 * B * N * (Fin * 4 * Fin + (k // 2) * w * Fin * 4 * Fin + Fin * 2 * Fout + k * Fin * 2 * Fout
                                                + 2 * Fin * k * 2 * Fout),
                          "composed": 2 * B * N * ((k // 2) * w * 2 * Fin * 4 * Fin + 2 * k * 2 * Fin * 2 * Fout)},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32); ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import spgan
    res = {"device": torch.cuda.get_device_name(0), "timing": "device events; median / min / max of 7 repeats of 5 calls after 3 warm-up rounds",
           "configs": [bench(spgan, a.B, a.N, 128, 256, 10, 0), bench(spgan, a.B, a.N, 3, 64, 10, 1)]}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
