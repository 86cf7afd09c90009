#!/usr/bin/env python
"""Microbenchmark of the bilateral upsampling edge convolution (spgan.bilateral_upsample_edgeConv, csrc/edge_rank.hip's spgan_edge_stored_gemm /
_wgrad / _dgrad beside the rank-window and weighted-layer launchers): device-event timing inside a warmed loop, one JSON document.  It
follows tools/deform_xyz_bench.py.

Per configuration (default bilateral_upsample_edgeConv(128,256,10) and (3,64,10) at B = 32, N = 2048, train mode), on the same GPU and the
same int32 kNN graph:
  layer     the module: forward, forward + backward, peak memory of one forward + backward;
  composed  the reference's formulation in torch: spgan.get_edge_features for x and pc on one graph -> torch.nn.functional.conv2d /
            batch_norm / leaky_relu / softmax, the reference's transpose / view chain, the product, the concatenation, conv2d with the
            [1,2k] kernel;
  upsample  spgan.upsample_edgeConv of the same sizes in the same process: the difference is what the weight costs;
  kernel    the new product launch against the gemm_nt-with-prologue launch it replaces on the same (M, K, O), and the new input gradient
            against gemm_nt_bnbwd, likewise.
The routes are timed alternately in the same process; every figure is a median with its min and max over the repeats.  No ratio is
asserted: the file records what was measured.

    python tools/bilateral_bench.py [--out profiles/bilateral_bench.json] [--B 32 --N 2048]
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

from deform_bench import peak_bytes, timed_pair          # noqa: E402


def bench(spgan, B, N, C, F, k, seed):
    ops, ew = spgan.ops, spgan.edge_weight
    g = torch.Generator().manual_seed(seed)
    m = spgan.bilateral_upsample_edgeConv(C, F, k, -1).cuda().train()
    up = spgan.upsample_edgeConv(C, F, k, -1).cuda().train()
    M, T, F1, F2 = B * N, k // 2, 2 * C, 2 * F
    x = (torch.rand(B, C, N, generator=g) * 2 - 1 if C <= 4 else torch.randn(B, C, N, generator=g) * 0.7).cuda().requires_grad_(True)
    pc = (torch.rand(B, 3, N, generator=g) * 2 - 1).cuda().requires_grad_(True)
    cot = torch.randn(B, F, 2 * N, generator=g).cuda()
    with torch.no_grad():
        _, idx = spgan.get_edge_features(x.detach(), k, return_idx=True)          # one graph for every route
    idx32 = ops.idx_from_local64(idx, B, N, k)      # the layers' own format: an int64 graph is range-checked with a host synchronisation per call

    def block(t, conv, bn, slope=0.01):
        return F_.leaky_relu(F_.batch_norm(F_.conv2d(t, conv.weight, conv.bias), None, None, bn.weight, bn.bias, True, 0.1, 1e-5), slope)

    def composed(xx, pp):
        e, y = spgan.get_edge_features(xx, k, idx=idx), spgan.get_edge_features(pp, k, idx=idx)
        w = block(e, m.conv_fea[0], m.conv_fea[1]) * block(y, m.conv_xyz[0], m.conv_xyz[1])
        for i in (0, 3):
            w = block(w, m.conv_all[i], m.conv_all[i + 1])
        w = F_.softmax(w, dim=-1)
        inte = block(e, m.inte_conv_hk[0], m.inte_conv_hk[1])
        inte = inte.transpose(2, 1).contiguous().view(B, N, F1, 2, T).contiguous().view(B, N, F1, k).permute(0, 2, 1, 3)
        out = block(torch.cat((e, inte * w), 3), m.conv2.conv, m.conv2.bn, 0.0)
        return out.unsqueeze(3).contiguous().view(B, F, 2, N).contiguous().view(B, F, 2 * N)

    def reset():
        x.grad = pc.grad = None
        for p in list(m.parameters()) + list(up.parameters()):
            p.grad = None

    def layer_fwd():
        with torch.no_grad():
            return m(x, pc, idx=idx32)

    def composed_fwd():
        with torch.no_grad():
            return composed(x, pc)

    def up_fwd():
        with torch.no_grad():
            return up(x, idx=idx32)

    def layer_step():
        reset()
        (m(x, pc, idx=idx32) * cot).sum().backward()

    def composed_step():
        reset()
        (composed(x, pc) * cot).sum().backward()

    def up_step():
        reset()
        (up(x, idx=idx32) * cot).sum().backward()

    ref = composed_fwd()
    diff = float((layer_fwd() - ref).abs().max() / ref.abs().max())
    del ref
    # the launches on their own: the same (M, K = k*2C, O = 2Fout) for the product with prologue and the stored-operand product
    with torch.no_grad():
        U = (torch.randn(M * T, 2 * F1, generator=g) * 0.7).cuda()
        z3 = (torch.randn(M * k, F1, generator=g) * 0.7).cuda()
        W = (torch.randn(F2, k * F1, generator=g) / (k * F1) ** 0.5).cuda()
        Wt = W.t().contiguous()
        dy = torch.randn(M, F2, generator=g).cuda()
        v1 = [(torch.rand(2 * F1, generator=g) + 0.5).cuda() if i % 2 == 0 else (torch.randn(2 * F1, generator=g) * 0.2).cuda() for i in range(4)]
        v3 = [(torch.rand(F1, generator=g) + 0.5).cuda() if i % 2 == 0 else (torch.randn(F1, generator=g) * 0.2).cuda() for i in range(4)]
        sc1, sh1, inv1, mu1 = v1
        sc3, sh3, inv3, mu3 = v3
        r1 = [t.repeat(T) for t in v1]
        Uf = U.view(M, T * 2 * F1)

    def norm_kernel():
        return ew.edge_weight_norm(z3, k, sc3, sh3)
    norm = norm_kernel()

    def gemm_old():
        return ops.gemm_nt(Uf, W, pro=(r1[0], r1[1], 0.01), exact=True)

    def gemm_new():
        return ew.edge_stored_gemm(U, k, sc1, sh1, z3, sc3, sh3, norm, W)

    def dgrad_old():
        return ops.gemm_nt_bnbwd(dy, Wt, Uf, r1[0], r1[1], r1[3], r1[2], 0.01, exact=True)

    def dgrad_new():                                                               # with the two finalize launches of its records
        return ew.edge_stored_dgrad(dy, Wt, U, k, sc1, sh1, mu1, inv1, z3, sc3, sh3, mu3, inv3, norm)

    def wgrad_old():
        return ops.gemm_tn(dy, Uf, pro=(r1[0], r1[1], 0.01), exact=True)

    def wgrad_new():
        return ew.edge_stored_wgrad(U, k, sc1, sh1, z3, sc3, sh3, norm, dy)

    t = timed_pair([layer_fwd, composed_fwd, up_fwd, layer_step, composed_step, up_step, gemm_old, gemm_new, dgrad_old, dgrad_new, wgrad_old,
                    wgrad_new, norm_kernel])
    flop = 2.0 * M * k * F1 * F2
    kern = {}
    for name, i in (("gemm_nt_prologue", 6), ("edge_stored_gemm", 7), ("gemm_nt_bnbwd", 8), ("edge_stored_dgrad", 9), ("gemm_tn_prologue", 10),
                    ("edge_stored_wgrad", 11)):
        kern[name] = {"ms": t[i], "M": M, "K": k * F1, "O": F2, "tflops": flop / (t[i]["median"] * 1e-3) / 1e12}
    kern["edge_weight_norm"] = {"ms": t[12]}
    E = 4 * M * k * F1
    res = {
        "layer": "bilateral_upsample_edgeConv(%d,%d,%d)" % (C, F, k), "shape": dict(B=B, N=N),
        "max_rel_difference_forward": diff,
        "layer_forward_ms": t[0], "torch_forward_ms": t[1], "upsample_forward_ms": t[2],
        "layer_forward_backward_ms": t[3], "torch_forward_backward_ms": t[4], "upsample_forward_backward_ms": t[5],
        "measured_ratio_forward_torch_over_layer": t[1]["median"] / t[0]["median"],
        "measured_ratio_forward_backward_torch_over_layer": t[4]["median"] / t[3]["median"],
        "weight_cost_ms": {"forward": t[0]["median"] - t[2]["median"], "forward_backward": t[3]["median"] - t[5]["median"]},
        "peak_bytes": {"layer_forward_backward": peak_bytes(layer_step), "torch_forward_backward": peak_bytes(composed_step),
                       "upsample_forward_backward": peak_bytes(up_step), "layer_forward": peak_bytes(layer_fwd), "one_edge_tensor_E": E},
        "launches": kern,
    }
    return res


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
