#!/usr/bin/env python
"""Microbenchmark of the weighted full-rank edge convolution (spgan.deform_edgeConv_feat, csrc/edge_rank.hip's spgan_edge_weight_*
launchers): device-event timing inside a warmed loop, one JSON document.  It follows tools/deform_bench.py.

Per configuration (default deform_edgeConv_feat(128,256,20) and deform_edgeConv_feat(3,64,10) at B = 32, N = 2048, train mode), on the
same GPU and the same kNN graph:
  layer     the module: forward, forward + backward, peak memory of one forward + backward;
  composed  the reference's formulation in torch: spgan.get_edge_features (the [B,2Fin,N,k] tensor) -> torch.nn.functional.conv2d /
            batch_norm / leaky_relu / softmax, the product, conv2d with the [1,k] kernel / batch_norm / relu;
  kernel    spgan_edge_weight_gemm beside spgan_edge_rank_gemm on the same (M, k, F1, O): the gap is the cost of the modulation;
            likewise the dgrad and wgrad launchers (with their finalize / reduce launches) beside the unweighted ones.
The routes are timed alternately in the same process; every figure is a median with its min and max over the repeats.  No ratio is
asserted: the file records what was measured.

    python tools/deform_feat_bench.py [--out profiles/deform_feat_bench.json] [--B 32 --N 2048]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sp-gan_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from deform_bench import PEAK_FP32_MFMA_TFLOPS, peak_bytes, timed_pair          # noqa: E402


def bench(spgan, B, N, Fin, Fout, k, seed):
    ops, er, ew = spgan.ops, spgan.edge_rank, spgan.edge_weight
    g = torch.Generator().manual_seed(seed)
    m = spgan.deform_edgeConv_feat(Fin, Fout, k).cuda().train()
    M = B * N
    x = (torch.rand(B, Fin, N, generator=g) * 2 - 1 if Fin <= 4 else torch.randn(B, Fin, N, generator=g) * 0.7).cuda().requires_grad_(True)
    cot = torch.randn(B, Fout, N, generator=g).cuda()
    with torch.no_grad():
        _, idx = spgan.get_edge_features(x.detach(), k, return_idx=True)          # one graph for both routes
    idx32 = ops.idx_from_local64(idx, B, N, k)      # the layer's own format: an int64 graph is range-checked with a host synchronisation per call

    def block(t, conv, bn):
        return F_.leaky_relu(F_.batch_norm(F_.conv2d(t, conv.weight, conv.bias), None, None, bn.weight, bn.bias, True, 0.1, 1e-5), 0.01)

    def composed(xx):
        e = spgan.get_edge_features(xx, k, idx=idx)                                # [B,2Fin,N,k]
        w = e
        for i in (0, 3, 6):
            w = block(w, m.conv_fea[i], m.conv_fea[i + 1])
        hs = block(e, m.inte_conv_hk[0], m.inte_conv_hk[1]) * F_.softmax(w, dim=-1)
        y = F_.conv2d(hs, m.conv2.conv.weight, m.conv2.conv.bias)
        return torch.relu(F_.batch_norm(y, None, None, m.conv2.bn.weight, m.conv2.bn.bias, True, 0.1, 1e-5)).squeeze(3)

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
    with torch.no_grad():
        PQ = (torch.randn(M, 2 * Fin, generator=g) * 0.7).cuda()
        z3 = torch.randn(M * k, Fin, generator=g).cuda()
        sc, sc3 = (torch.rand(Fin, generator=g) + 0.5).cuda(), (torch.rand(Fin, generator=g) + 0.5).cuda()
        sh, sh3 = (torch.randn(Fin, generator=g) * 0.2).cuda(), (torch.randn(Fin, generator=g) * 0.2).cuda()
        W2i = m.conv2.conv.weight.detach()[:, :, 0, :].permute(0, 2, 1).reshape(Fout, k * Fin).contiguous()
        b2 = m.conv2.conv.bias.detach()
        nrm = ew.edge_weight_norm(z3, k, sc3, sh3)

    def weighted_kernel():
        return ew.edge_weight_gemm(PQ, idx32, sc, sh, z3, sc3, sh3, nrm, W2i, b2, stats=True)

    def plain_kernel():
        return er.edge_rank_gemm(PQ, idx32, sc, sh, W2i, b2, stats=True)

    with torch.no_grad():
        W2t = W2i.t().contiguous()
        dy = torch.randn(M, Fout, generator=g).cuda()
        mu, iv = (torch.randn(Fin, generator=g) * 0.1).cuda(), (torch.rand(Fin, generator=g) + 0.5).cuda()

    def weighted_dgrad():                                                          # dm, du, g3 and both column records: two passes over the ranks
        return ew.edge_weight_dgrad(dy, W2t, PQ, idx32, sc, sh, mu, iv, z3, sc3, sh3, mu, iv, nrm)

    def plain_dgrad():
        return er.edge_rank_dgrad(dy, W2t, PQ, idx32, sc, sh, mu, iv)

    def weighted_wgrad():
        return ew.edge_weight_wgrad(PQ, idx32, sc, sh, z3, sc3, sh3, nrm, dy)

    def plain_wgrad():
        return er.edge_rank_wgrad(PQ, idx32, sc, sh, dy)

    t = timed_pair([layer_fwd, composed_fwd, layer_step, composed_step, weighted_kernel, plain_kernel, weighted_dgrad, plain_dgrad,
                    weighted_wgrad, plain_wgrad])
    flop = 2.0 * M * k * Fin * Fout
    tf = [flop / (t[i]["median"] * 1e-3) / 1e12 for i in (4, 5)]
    return {
        "layer": "deform_edgeConv_feat(%d,%d,%d)" % (Fin, Fout, k), "shape": dict(B=B, N=N),
        "max_rel_difference_forward": diff,
        "layer_forward_ms": t[0], "torch_forward_ms": t[1], "layer_forward_backward_ms": t[2], "torch_forward_backward_ms": t[3],
        "measured_ratio_forward_torch_over_layer": t[1]["median"] / t[0]["median"],
        "measured_ratio_forward_backward_torch_over_layer": t[3]["median"] / t[2]["median"],
        "peak_bytes": {"layer_forward_backward": peak_bytes(layer_step), "torch_forward_backward": peak_bytes(composed_step),
                       "layer_forward": peak_bytes(layer_fwd), "one_edge_tensor_E1": 4 * M * k * Fin},
        "edge_weight_gemm_kernel": {"ms": t[4], "flop": flop, "tflops": tf[0], "fraction_of_fp32_mfma_peak": tf[0] / PEAK_FP32_MFMA_TFLOPS},
        "edge_rank_gemm_kernel_same_shape": {"ms": t[5], "tflops": tf[1], "fraction_of_fp32_mfma_peak": tf[1] / PEAK_FP32_MFMA_TFLOPS},
        "modulation_cost_ms": t[4]["median"] - t[5]["median"],
        "edge_weight_dgrad_ms": t[6], "edge_rank_dgrad_same_shape_ms": t[7],
        "edge_weight_wgrad_ms": t[8], "edge_rank_wgrad_same_shape_ms": t[9],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32); ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import spgan
    res = {"device": torch.cuda.get_device_name(0), "timing": "device events; median / min / max of 7 repeats of 5 calls after 3 warm-up rounds",
           "fp32_mfma_peak_tflops": PEAK_FP32_MFMA_TFLOPS,
           "configs": [bench(spgan, a.B, a.N, 128, 256, 20, 0), bench(spgan, a.B, a.N, 3, 64, 10, 1)]}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
