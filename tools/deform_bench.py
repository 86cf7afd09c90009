#!/usr/bin/env python
"""Microbenchmark of the full-rank edge convolutions (spgan.deform_edgeConv_simple / deform_edgeConv_first, csrc/edge_rank.hip):
device-event timing inside a warmed loop, one JSON document.

Per configuration (default deform_edgeConv_first(128,256,20), deform_edgeConv_simple(128,256,20) and deform_edgeConv_simple(3,64,10) at
B = 32, N = 2048, train mode), on the same GPU and the same kNN graph:
  layer     the module: forward, forward + backward, peak memory of one forward + backward;
  (a)       the reference's formulation in torch: spgan.get_edge_features (the [B,2Fin,N,k] tensor) -> torch.nn.functional.conv2d /
            batch_norm / leaky_relu -> conv2d with the [1,k] kernel / batch_norm / relu: forward, forward + backward, peak memory;
  (b)       the composition of the launchers that existed before edge_rank.hip, which stores the activated [M*k,F1] tensor:
            edge_window_gemm with w = 1 (the 1x1 convolution over the differences, with its statistics), BatchNorm + LeakyReLU applied
            by ops.affine_act, ops.gemm_nt over the [M, k*F1] view (with conv2's statistics); forward, and forward plus the two products
            of conv2's backward over the stored tensor (gemm_tn for the weight, gemm_nt for the activation gradient) -- not a full backward;
  kernel    spgan_edge_rank_gemm alone and its achieved TFLOP/s (2*M*k*F1*Fout FLOP).
The routes are timed alternately in the same process; every figure is a median with its min and max over the repeats.  No ratio is
asserted: the file records what was measured.

    python tools/deform_bench.py [--out profiles/deform_bench.json] [--B 32 --N 2048]
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

PEAK_FP32_MFMA_TFLOPS = 157.3


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


def bench(spgan, cls, B, N, Fin, Fout, k, seed):
    ops, ew, em, er = spgan.ops, spgan.edge_window, spgan.edge_max, spgan.edge_rank
    g = torch.Generator().manual_seed(seed)
    simple = cls == "simple"
    m = (spgan.deform_edgeConv_simple if simple else spgan.deform_edgeConv_first)(Fin, Fout, k).cuda().train()
    conv1, bn1, conv2, bn2 = m.inte_conv_hk[0], m.inte_conv_hk[1], m.conv2.conv, m.conv2.bn
    F1, M = conv1.weight.shape[0], B * N
    x = (torch.rand(B, Fin, N, generator=g) * 2 - 1 if Fin <= 4 else torch.randn(B, Fin, N, generator=g) * 0.7).cuda().requires_grad_(True)
    cot = torch.randn(B, Fout, N, generator=g).cuda()
    with torch.no_grad():
        _, idx = spgan.get_edge_features(x.detach(), k, return_idx=True)          # one graph for every route
    idx32 = ops.idx_from_local64(idx, B, N, k)      # the layer's own format: an int64 graph is range-checked with a host synchronisation per call

    def layer(xx):
        return (m(xx, None, idx=idx32) if simple else m(xx, idx=idx32)).view(B, Fout, N)

    def composed(xx):                                                              # (a)
        ee = spgan.get_edge_features(xx, k, idx=idx)                               # [B,2Fin,N,k]
        h = F_.conv2d(ee, conv1.weight, conv1.bias)
        h = F_.leaky_relu(F_.batch_norm(h, None, None, bn1.weight, bn1.bias, True, 0.1, 1e-5), 0.01, inplace=True)
        y = F_.conv2d(h, conv2.weight, conv2.bias)
        return torch.relu(F_.batch_norm(y, None, None, bn2.weight, bn2.bias, True, 0.1, 1e-5)).squeeze(3)

    with torch.no_grad():
        W1 = conv1.weight.detach().view(F1, 2 * Fin)
        Wc, Wd = W1[:, :Fin].contiguous(), W1[:, Fin:].contiguous()
        W2i = conv2.weight.detach()[:, :, 0, :].permute(0, 2, 1).reshape(Fout, k * F1).contiguous()
        W2t = W2i.t().contiguous()
        zeros_m, ones_v = torch.zeros(F1, device="cuda"), torch.ones(F1, device="cuda")
        dy = torch.randn(M, Fout, generator=g).cuda()

    def stored(backward_products):                                                 # (b): train-mode statistics on scratch running buffers
        with torch.no_grad():
            x_pm = ops.cm_to_pm(x.detach())
            Q = ops.gemm_nt(x_pm, Wc, conv1.bias.detach())
            U, part, rows = ew.edge_window_gemm(x_pm, idx32, Wd, rowadd=Q, stats=True)          # [M*k, F1]
            st1 = em.edge_max_bn(part, rows, M * k, bn1.weight.detach(), bn1.bias.detach(), zeros_m.clone(), ones_v.clone())
            H = ops.affine_act(U, st1[0], st1[1], 0.01)                            # the stored activated tensor
            del U
            Y = ops.gemm_nt(H.view(M, k * F1), W2i, conv2.bias.detach(), stats=True)
            if backward_products:
                return ops.gemm_tn(dy, H.view(M, k * F1)), ops.gemm_nt(dy, W2t)
            return Y

    def reset():
        x.grad = None
        for p in m.parameters():
            p.grad = None

    def layer_fwd():
        with torch.no_grad():
            return layer(x)

    def composed_fwd():
        with torch.no_grad():
            return composed(x)

    def layer_step():
        reset()
        (layer(x) * cot).sum().backward()

    def composed_step():
        reset()
        (composed(x) * cot).sum().backward()

    ref = composed_fwd()
    diff = float((layer_fwd() - ref).abs().max() / ref.abs().max())
    del ref
    with torch.no_grad():
        Wst = torch.cat([Wd, Wc - Wd], dim=0)
        PQ = ops.gemm_nt(ops.cm_to_pm(x.detach()), Wst, torch.cat([torch.zeros_like(conv1.bias), conv1.bias.detach()]))
        sc = (torch.rand(F1, generator=g) + 0.5).cuda()
        sh = (torch.randn(F1, generator=g) * 0.2).cuda()

    def kernel_only():
        return er.edge_rank_gemm(PQ, idx32, sc, sh, W2i, conv2.bias.detach(), stats=True)

    t = timed_pair([layer_fwd, composed_fwd, lambda: stored(False), layer_step, composed_step, lambda: stored(True), kernel_only])
    flop = 2.0 * M * k * F1 * Fout
    tf = flop / (t[6]["median"] * 1e-3) / 1e12
    return {
        "layer": "deform_edgeConv_%s(%d,%d,%d)" % (cls, Fin, Fout, k), "shape": dict(B=B, N=N, F1=F1),
        "max_rel_difference_forward": diff,
        "layer_forward_ms": t[0], "torch_forward_ms": t[1], "stored_launchers_forward_ms": t[2],
        "layer_forward_backward_ms": t[3], "torch_forward_backward_ms": t[4], "stored_launchers_forward_plus_conv2_backward_products_ms": t[5],
        "measured_ratio_forward_torch_over_layer": t[1]["median"] / t[0]["median"],
        "measured_ratio_forward_stored_over_layer": t[2]["median"] / t[0]["median"],
        "measured_ratio_forward_backward_torch_over_layer": t[4]["median"] / t[3]["median"],
        "peak_bytes": {"layer_forward_backward": peak_bytes(layer_step), "torch_forward_backward": peak_bytes(composed_step),
                       "layer_forward": peak_bytes(layer_fwd), "stored_launchers_forward": peak_bytes(lambda: stored(False)),
                       "one_activated_edge_tensor": 4 * M * k * F1},
        "edge_rank_gemm_kernel": {"ms": t[6], "flop": flop, "tflops": tf, "fraction_of_fp32_mfma_peak": tf / PEAK_FP32_MFMA_TFLOPS},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32); ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import spgan
    res = {"device": torch.cuda.get_device_name(0), "timing": "device events; median / min / max of 7 repeats of 5 calls after 3 warm-up rounds",
           "fp32_mfma_peak_tflops": PEAK_FP32_MFMA_TFLOPS,
           "configs": [bench(spgan, "first", a.B, a.N, 128, 256, 20, 0), bench(spgan, "simple", a.B, a.N, 128, 256, 20, 1),
                       bench(spgan, "simple", a.B, a.N, 3, 64, 10, 2)]}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
