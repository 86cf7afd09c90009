#!/usr/bin/env python
"""Microbenchmark of the dense edge layer (spgan.DenseEdgeModule, csrc/edge_dense.hip): device-event timing inside a warmed loop, one
JSON document.

Per configuration (default DenseEdgeModule(64,4,64,20) and DenseEdgeModule(6,3,32,20) at B = 32, N = 2048), on the same GPU and the same
graph:
  layer       the module: forward, forward + backward, peak memory of one forward + backward;
  reference   (a) the reference's formulation written in torch: the materialised [B,2C,N,k] tensor (spgan.get_graph_feature), per level
              matmul -> batch norm -> leaky relu -> torch.cat, then the max: forward, forward + backward, peak memory;
  composed    (b) the layer's forward with each level composed from the launchers that existed before the level kernel:
              ops.gemm_nt(pro=..., out=slice) for the product, then a gather pass for Q_i + P_j, an in-place add and a statistics pass
              (edge_weight.edge_weight_gather, ops.colstats, ops.bn_prepare): forward only -- the backward is the layer's own;
  level       the level kernel alone at the last level's shape (M = B*N*k, N = G, K = (L-1) G, addend and records on) in TFLOP/s against
              the 157.3 TFLOP/s fp32-MFMA peak, beside gemm_nt(pro=...) at the same shape.
The routes are timed alternately in the same process; every figure is a median with its min and max over the repeats.  No ratio is
asserted: the file records what was measured.

    python tools/dense_edge_bench.py [--out profiles/dense_edge_bench.json] [--B 32 --N 2048]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sp-gan_amd"))
PEAK_TFLOPS = 157.3
SLOPE = 0.2


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


def bench(spgan, B, N, C, L, G, k, seed):
    from spgan import edge_conv, edge_dense, edge_weight, ops
    g = torch.Generator().manual_seed(seed)
    m = spgan.DenseEdgeModule(2 * C, L, G, k).cuda().train()
    x = (torch.rand(B, C, N, generator=g) * 2 - 1 if C <= 4 else torch.randn(B, C, N, generator=g)).cuda().requires_grad_(True)
    cot = torch.randn(B, G, N, generator=g).cuda()
    M, E, LG = B * N, B * N * k, L * G
    with torch.no_grad():
        idx32 = edge_conv.dense_graph(ops.cm_to_pm(x.detach()), B, N, k, 1 if C <= 4 else 0)      # one graph for every route
        idx64 = ops.idx_to_local64(idx32, B, N)
    Ws = [s[0].weight for s in m.dense_modules]
    bs = [s[0].bias for s in m.dense_modules]
    bns = [s[1] for s in m.dense_modules]

    def reference(xx):
        f = spgan.get_graph_feature(xx, k, idx=idx64)                             # [B,2C,N,k]
        y = None
        for l in range(L):
            cin = f.shape[1]
            y = torch.matmul(Ws[l].view(G, cin), f.reshape(B, cin, N * k)).view(B, G, N, k) + bs[l].view(1, G, 1, 1)
            y = torch.nn.functional.leaky_relu(bns[l](y), SLOPE)
            f = torch.cat([f, y], dim=1)
        return y.max(dim=-1)[0]

    def composed_fwd():
        """the layer's forward, every level from the launchers of the parent commit (no autograd: forward only)"""
        with torch.no_grad():
            x_pm = ops.cm_to_pm(x)
            Wst, _, Wy, _ = edge_conv.dense_edge_images(Ws, C)
            PQ = ops.gemm_nt(x_pm, Wst, torch.cat([torch.zeros_like(b) for b in bs] + list(bs)), exact=True)
            Z = torch.empty((E, LG), dtype=torch.float32, device=x.device)
            SC = torch.empty((2, LG), dtype=torch.float32, device=x.device)
            st = None
            for l in range(L):
                lo, hi = l * G, (l + 1) * G
                add = edge_weight.edge_weight_gather(torch.cat([PQ[:, lo:hi], PQ[:, LG + lo:LG + hi]], dim=1), idx32)
                if l:
                    ops.gemm_nt(Z[:, :lo], Wy[l - 1], pro=(SC[0, :lo], SC[1, :lo], SLOPE), out=Z[:, lo:hi], exact=True)
                    Z[:, lo:hi] += add
                else:
                    Z[:, lo:hi] = add
                del add
                mean, var = ops.colstats(Z[:, lo:hi], E)
                st = ops._bn_prepare4(mean[0].contiguous(), var[0].contiguous(), bns[l].weight, bns[l].bias, E, True, None, None)
                SC[:, lo:hi] = st[:2]
            from spgan import pointnet_util
            return ops.pm_to_cm(pointnet_util._group_max(Z[:, LG - G:], M, k, st[0], st[1], SLOPE)[0], B, N)

    def reset():
        x.grad = None
        for p in m.parameters():
            p.grad = None

    def layer_fwd():
        with torch.no_grad():
            return m(x, idx=idx32)

    def reference_fwd():
        with torch.no_grad():
            return reference(x)

    def layer_step():
        reset()
        (m(x, idx=idx32) * cot).sum().backward()

    def reference_step():
        reset()
        (reference(x) * cot).sum().backward()

    def layer_step_own_graph():
        reset()
        (m(x) * cot).sum().backward()

    ref = reference_fwd()
    diff = float((layer_fwd() - ref).abs().max() / ref.abs().max())
    diff_c = float((composed_fwd() - ref).abs().max() / ref.abs().max())
    t = timed_pair([layer_fwd, reference_fwd, composed_fwd, layer_step, reference_step, layer_step_own_graph])
    res = {
        "layer": "DenseEdgeModule(%d,%d,%d,%d)" % (2 * C, L, G, k), "shape": dict(B=B, N=N, edges=E),
        "max_rel_difference_forward": {"layer_vs_reference": diff, "composed_vs_reference": diff_c},
        "layer_forward_ms": t[0], "reference_forward_ms": t[1], "composed_forward_ms": t[2],
        "layer_forward_backward_ms": t[3], "reference_forward_backward_ms": t[4], "layer_forward_backward_with_knn_ms": t[5],
        "measured_ratio_forward": {"reference_over_layer": t[1]["median"] / t[0]["median"], "composed_over_layer": t[2]["median"] / t[0]["median"]},
        "measured_ratio_forward_backward": t[4]["median"] / t[3]["median"],
        "peak_bytes_forward_backward": {"layer": peak_bytes(layer_step), "reference": peak_bytes(reference_step),
                                        "one_level_edge_tensor": 4 * E * G, "contract_bound": (2 * L + 3) * E * G * 4 + 32 * 2 ** 20},
        "peak_bytes_forward": {"layer": peak_bytes(layer_fwd), "reference": peak_bytes(reference_fwd), "composed": peak_bytes(composed_fwd)},
    }
    if L > 1:                                                                      # the level kernel alone, at the last level's shape
        K = (L - 1) * G
        Z = torch.randn(E, LG, generator=torch.Generator().manual_seed(seed + 1)).cuda()
        W = (torch.randn(G, K, generator=g) / K ** 0.5).cuda()
        sc, sh = torch.rand(K, generator=g).cuda() + 0.5, (torch.randn(K, generator=g) * 0.1).cuda()
        PQ = torch.randn(M, 2 * G, generator=g).cuda()
        ad = (PQ[:, :G], PQ[:, G:], idx32)

        def level():
            edge_dense.edge_dense_level(Z[:, :K], W, Z[:, K:], raw_cols=0, scale=sc, shift=sh, slope=SLOPE, addend=ad, stats=True)

        def level_plain():
            edge_dense.edge_dense_level(Z[:, :K], W, Z[:, K:], raw_cols=0, scale=sc, shift=sh, slope=SLOPE)

        def nt():
            ops.gemm_nt(Z[:, :K], W, pro=(sc, sh, SLOPE), out=Z[:, K:], exact=True)

        tl = timed_pair([level, level_plain, nt])
        flops = 2.0 * E * G * K
        res["level_kernel"] = {
            "shape": dict(M=E, N=G, K=K), "flops": flops, "fp32_mfma_peak_tflops": PEAK_TFLOPS,
            "with_addend_and_records_ms": tl[0], "product_only_ms": tl[1], "gemm_nt_pro_product_only_ms": tl[2],
            "with_addend_and_records_tflops": flops / tl[0]["median"] * 1e-9, "product_only_tflops": flops / tl[1]["median"] * 1e-9,
            "gemm_nt_pro_product_only_tflops": flops / tl[2]["median"] * 1e-9,
            "bytes_moved_at_least": 4.0 * E * (K + G), "with_addend_and_records_tb_per_s": 4.0 * E * (K + G) / tl[0]["median"] * 1e-9,
        }
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32); ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import spgan
    res = {"device": torch.cuda.get_device_name(0), "timing": "device events; median / min / max of 7 repeats of 5 calls after 3 warm-up rounds",
           "configs": [bench(spgan, a.B, a.N, 32, 4, 64, 20, 0), bench(spgan, a.B, a.N, 3, 3, 32, 20, 1)]}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
