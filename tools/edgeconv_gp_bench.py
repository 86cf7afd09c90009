#!/usr/bin/env python
"""Microbenchmark of one gradient-penalty evaluation through the max-aggregation edge convolution with its opt-in double backward
(spgan.edgeConv(double_backward=True), csrc/edge_max.hip's dbl passes): device-event timing inside a warmed loop, one JSON document.

Per configuration (default edgeConv(64,128,10) and edgeConv(3,64,20) at B = 32, N = 2048) one evaluation is: forward, disc = mean of the
output per shape, autograd.grad(disc, x, create_graph=True), penalty = 10 * mean((||g_b|| - 1)^2), penalty.backward() -- the same torch
glue around either route.  The layer (inside functions.input_grad_only(), as spgan.GradientPenalty runs it) stands beside the only route
a user had before it, on the same GPU and the same kNN graph: the materialised composition in torch, edge features [B,2Fin,N,k] (a torch
gather: differentiable twice) -> matmul -> batch norm -> relu -> max.  The two routes are timed alternately in the same process; every
figure is a median with its min and max over the repeats; peak memory is that of one evaluation of either route; the gradients
of the two routes are compared with each other and with one float64 evaluation of the composition, and the entries whose selected
neighbour differs between any two of the three are counted (a near-tie in the max resolves by rounding: a discrete difference, which
moves a gradient far more than float32 arithmetic does).  No ratio is asserted: the file records what was measured, a shape where
the layer loses included.

    python tools/edgeconv_gp_bench.py [--out profiles/edgeconv_gp_bench.json] [--B 32 --N 2048]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sp-gan_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from edgeconv_bench import peak_bytes, timed_pair  # noqa: E402


def penalty(out, x):
    B = x.shape[0]
    disc = out.mean(dim=(1, 2))
    (g,) = torch.autograd.grad(disc, x, torch.ones_like(disc), create_graph=True)
    return 10.0 * ((g.reshape(B, -1).norm(2, dim=1) - 1.0) ** 2).mean()


def bench(spgan, B, N, Fin, F, k, seed):
    from spgan.functions import input_grad_only
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)                               # the layer's initial weights
    m = spgan.edgeConv(Fin, F, k, double_backward=True).cuda().train()
    bn = torch.nn.BatchNorm2d(F).cuda().train()
    x = (torch.rand(B, Fin, N, generator=g) * 2 - 1 if Fin <= 4 else torch.randn(B, Fin, N, generator=g) * 0.7).cuda().requires_grad_(True)
    with torch.no_grad():
        _, idx = spgan.get_edge_features(x.detach(), k, return_idx=True)          # one graph for both routes
        m.conv.bn.weight.copy_(torch.rand(F, generator=g) + 0.5)
        bn.weight.copy_(m.conv.bn.weight)
    idx32 = spgan.ops.idx_from_local64(idx, B, N, k)      # the layer's own format: an int64 graph is range-checked with a host synchronisation per call
    W, b = m.conv.conv.weight, m.conv.conv.bias
    nb = idx.view(B, 1, N * k).expand(B, Fin, N * k)

    def pre_norm(xx, Wm, bias):
        cen = xx.unsqueeze(3).expand(B, Fin, N, k)
        ee = torch.cat([cen, torch.gather(xx, 2, nb).view(B, Fin, N, k) - cen], dim=1)                  # [B,2Fin,N,k]
        return torch.matmul(Wm.view(F, 2 * Fin), ee.reshape(B, 2 * Fin, N * k)).view(B, F, N, k) + bias.view(1, F, 1, 1)

    def composed(xx):
        return torch.relu(bn(pre_norm(xx, W, b))).max(dim=3)[0]

    def composed_float64():
        """the same composition in float64, once: the arbiter between the two float32 routes -> (gradients of (conv weight, bn weight, x),
        the selected neighbours [B,F,N])"""
        x64 = x.detach().double().requires_grad_(True)
        W64, b64, g64, be64 = (t.detach().double().requires_grad_(True) for t in (W, b, bn.weight, bn.bias))
        y = torch.nn.functional.batch_norm(pre_norm(x64, W64, b64), None, None, g64, be64, True, 0.0, bn.eps)
        out, ind = torch.relu(y).max(dim=3)
        return torch.autograd.grad(penalty(out, x64), (W64, g64, x64)), ind

    def selection_differences(ind64):
        """entries whose selected neighbour differs between two routes, among those the layer's ReLU does not clip"""
        with torch.no_grad():
            m(x, idx=idx32)
            ind = torch.relu(bn(pre_norm(x, W, b))).max(dim=3)[1]                                        # [B,F,N]
        sel = m.last_sel.view(B, N, F).permute(0, 2, 1)
        active = (sel & 0x80) == 0
        rank = (sel & 0x7f).long()

        def count(u, w):
            return int(((u != w) & active).sum())
        return {"layer_vs_composed": count(rank, ind), "layer_vs_float64": count(rank, ind64), "composed_vs_float64": count(ind, ind64),
                "of": int(active.sum())}

    def reset():
        x.grad = None
        for p in list(m.parameters()) + list(bn.parameters()):
            p.grad = None

    def layer_gp():
        reset()
        with input_grad_only():
            pen = penalty(m(x, idx=idx32), x)
        pen.backward()
        return pen

    def composed_gp():
        reset()
        pen = penalty(composed(x), x)
        pen.backward()
        return pen

    def rel(a, c):
        return float((a.double() - c.double()).norm() / c.double().norm())

    def rel3(a, c):
        return dict(zip(("conv_weight", "bn_weight", "x"), [rel(u, w) for u, w in zip(a, c)]))

    p_l = float(layer_gp())
    got = [W.grad.clone(), m.conv.bn.weight.grad.clone(), x.grad.clone()]
    p_c = float(composed_gp())
    want = [W.grad.clone(), bn.weight.grad.clone(), x.grad.clone()]
    f64, ind64 = composed_float64()
    sel_diff = selection_differences(ind64)
    del ind64
    t = timed_pair([layer_gp, composed_gp])
    return {
        "layer": "edgeConv(%d,%d,%d, double_backward=True)" % (Fin, F, k), "shape": dict(B=B, N=N),
        "penalty": {"layer": p_l, "composed": p_c},
        "rel_l2_difference_of_gradients": rel3(got, want),
        "rel_l2_vs_float64_composition": {"layer": rel3(got, f64), "composed": rel3(want, f64)},
        "selected_neighbour_differs": sel_diff,
        "layer_penalty_ms": t[0], "composed_penalty_ms": t[1], "measured_ratio": t[1]["median"] / t[0]["median"],
        "peak_bytes": {"layer": peak_bytes(layer_gp), "composed": peak_bytes(composed_gp), "one_pre_norm_edge_tensor": 4 * B * F * N * k,
                       "kept_between_the_backwards_r_and_dPQ": 4 * B * N * 3 * F},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32); ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import spgan
    res = {"device": torch.cuda.get_device_name(0), "timing": "device events; median / min / max of 7 repeats of 5 calls after 3 warm-up rounds",
           "evaluation": "forward, autograd.grad(create_graph=True), penalty, backward",
           "configs": [bench(spgan, a.B, a.N, 64, 128, 10, 0), bench(spgan, a.B, a.N, 3, 64, 20, 1)]}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
