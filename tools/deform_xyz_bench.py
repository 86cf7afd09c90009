#!/usr/bin/env python
"""Microbenchmark of the coordinate-guided full-rank edge convolution (spgan.deform_edgeConv, csrc/edge_rank.hip's spgan_edge_weight_gather2 /
spgan_edge_weight_split beside the weighted layer's launchers): device-event timing inside a warmed loop, one JSON document.  It follows
tools/deform_feat_bench.py.

Per configuration (default deform_edgeConv(128,128,20) and deform_edgeConv(3,3,10) at B = 32, N = 2048, train mode), on the same GPU and
the same kNN graph:
  layer     the module: forward, forward + backward, peak memory of one forward + backward;
  composed  the reference's formulation in torch: spgan.get_edge_features for x and pc on one graph (the [B,2Fin,N,k] and [B,6,N,k]
            tensors) -> torch.nn.functional.conv2d / batch_norm / leaky_relu / softmax, the products, conv2d with the [1,k] kernel;
  feat      spgan.deform_edgeConv_feat of the same sizes in the same process: the difference is the cost of the coordinate branch;
  kernel    the two new launches on their own, with the bytes they move over the time against the HBM bandwidth.
The routes are timed alternately in the same process; every figure is a median with its min and max over the repeats.  No ratio is
asserted: the file records what was measured.

    python tools/deform_xyz_bench.py [--out profiles/deform_xyz_bench.json] [--B 32 --N 2048]
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

HBM_PEAK_TBS, HBM_COPY_TBS = 8.0, 6.3                    # the specified rate and what a float4 copy reaches


def bench(spgan, B, N, F, k, seed):
    ops, ew = spgan.ops, spgan.edge_weight
    g = torch.Generator().manual_seed(seed)
    m = spgan.deform_edgeConv(F, F, k).cuda().train()
    feat = spgan.deform_edgeConv_feat(F, F, k).cuda().train()
    M = B * N
    x = (torch.rand(B, F, N, generator=g) * 2 - 1 if F <= 4 else torch.randn(B, F, N, generator=g) * 0.7).cuda().requires_grad_(True)
    pc = (torch.rand(B, 3, N, generator=g) * 2 - 1).cuda().requires_grad_(True)
    cot = torch.randn(B, F, N, generator=g).cuda()
    with torch.no_grad():
        _, idx = spgan.get_edge_features(x.detach(), k, return_idx=True)          # one graph for every route
    idx32 = ops.idx_from_local64(idx, B, N, k)      # the layers' own format: an int64 graph is range-checked with a host synchronisation per call

    def block(t, conv, bn):
        return F_.leaky_relu(F_.batch_norm(F_.conv2d(t, conv.weight, conv.bias), None, None, bn.weight, bn.bias, True, 0.1, 1e-5), 0.01)

    def composed(xx, pp):
        e, y = spgan.get_edge_features(xx, k, idx=idx), spgan.get_edge_features(pp, k, idx=idx)
        w = block(e, m.conv_fea[0], m.conv_fea[1]) * block(y, m.conv_xyz[0], m.conv_xyz[1])
        for i in (0, 3):
            w = block(w, m.conv_all[i], m.conv_all[i + 1])
        hs = block(e, m.inte_conv_hk[0], m.inte_conv_hk[1]) * F_.softmax(w, dim=-1)
        return block(hs, m.conv2[0], m.conv2[1]).squeeze(3)

    def reset():
        x.grad = pc.grad = None
        for p in list(m.parameters()) + list(feat.parameters()):
            p.grad = None

    def layer_fwd():
        with torch.no_grad():
            return m(x, pc, idx=idx32)

    def composed_fwd():
        with torch.no_grad():
            return composed(x, pc)

    def feat_fwd():
        with torch.no_grad():
            return feat(x, idx=idx32)

    def layer_step():
        reset()
        (m(x, pc, idx=idx32) * cot).sum().backward()

    def composed_step():
        reset()
        (composed(x, pc) * cot).sum().backward()

    def feat_step():
        reset()
        (feat(x, idx=idx32) * cot).sum().backward()

    ref = composed_fwd()
    diff = float((layer_fwd() - ref).abs().max() / ref.abs().max())
    del ref
    Fb = 16
    with torch.no_grad():
        PQa, PQb = (torch.randn(M, 2 * Fb, generator=g) * 0.7).cuda(), (torch.randn(M, 2 * Fb, generator=g) * 0.7).cuda()
        dw0 = torch.randn(M * k, Fb, generator=g).cuda()
        v = [(torch.rand(Fb, generator=g) + 0.5).cuda() if i % 2 == 0 else (torch.randn(Fb, generator=g) * 0.2).cuda() for i in range(8)]
        sa, ta, ia, ma, sb, tb, ib, mb = v

    def gather2_kernel():
        return ew.edge_weight_gather2(PQa, PQb, idx32, sa, ta, sb, tb)

    def split_kernel():                                                            # with the two finalize launches of its records
        return ew.edge_weight_split(dw0, PQa, PQb, idx32, sa, ta, ma, ia, sb, tb, mb, ib)

    t = timed_pair([layer_fwd, composed_fwd, feat_fwd, layer_step, composed_step, feat_step, gather2_kernel, split_kernel])
    row = 4 * Fb
    # per edge: the graph entry and one row written (two for split, which also reads the incoming row); the per-point rows ([P | Q] of both
    # branches) are read from HBM once and gathered out of the caches
    moved = {"gather2": M * k * (4 + row) + 2 * M * 2 * row, "split": M * k * (4 + 3 * row) + 2 * M * 2 * row}
    gathered = M * k * 2 * row                                                     # the neighbour rows as the lanes request them
    kern = {}
    for name, i in (("gather2", 6), ("split", 7)):
        tbs = moved[name] / (t[i]["median"] * 1e-3) / 1e12
        kern["edge_weight_%s_kernel" % name] = {"ms": t[i], "hbm_bytes": moved[name], "gathered_row_bytes_from_cache": gathered, "hbm_tb_per_s": tbs,
                                                "fraction_of_hbm_peak": tbs / HBM_PEAK_TBS, "fraction_of_copy_rate": tbs / HBM_COPY_TBS}
    res = {
        "layer": "deform_edgeConv(%d,%d,%d)" % (F, F, k), "shape": dict(B=B, N=N),
        "max_rel_difference_forward": diff,
        "layer_forward_ms": t[0], "torch_forward_ms": t[1], "feat_forward_ms": t[2],
        "layer_forward_backward_ms": t[3], "torch_forward_backward_ms": t[4], "feat_forward_backward_ms": t[5],
        "measured_ratio_forward_torch_over_layer": t[1]["median"] / t[0]["median"],
        "measured_ratio_forward_backward_torch_over_layer": t[4]["median"] / t[3]["median"],
        "coordinate_branch_cost_ms": {"forward": t[0]["median"] - t[2]["median"], "forward_backward": t[3]["median"] - t[5]["median"]},
        "peak_bytes": {"layer_forward_backward": peak_bytes(layer_step), "torch_forward_backward": peak_bytes(composed_step),
                       "feat_forward_backward": peak_bytes(feat_step), "layer_forward": peak_bytes(layer_fwd), "one_edge_tensor_E1": 4 * M * k * F},
    }
    res.update(kern)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32); ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import spgan
    res = {"device": torch.cuda.get_device_name(0), "timing": "device events; median / min / max of 7 repeats of 5 calls after 3 warm-up rounds",
           "hbm_peak_tb_per_s": HBM_PEAK_TBS, "hbm_copy_tb_per_s": HBM_COPY_TBS,
           "configs": [bench(spgan, a.B, a.N, 128, 20, 0), bench(spgan, a.B, a.N, 3, 10, 1)]}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
