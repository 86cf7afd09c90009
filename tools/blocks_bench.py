#!/usr/bin/env python
"""Microbenchmark of the bilateral / deform blocks (spgan.bilateral_block_l1, bilateral_block_l2, deform_block_feat; edge_conv.BlockTailFn over
csrc/block_tail.hip): device-event timing inside a warmed loop, one JSON document.  It follows tools/bilateral_bench.py.

Per configuration (default bilateral_block_l2(128,256,N,num_k=20), bilateral_block_l1(128,256,N,20) and deform_block_feat(128,128,20) at
B = 32, N = 2048, and one small shape; train mode), on the same GPU and the same int32 kNN graph:
  block     the module: forward + backward, peak memory of one forward + backward (peak_bytes: the bytes the code requested;
            peak_allocated_bytes: the allocator's blocks, see peak_bytes());
  baseline  what a user wrote before the blocks existed: the same spgan layer (the same module object) with the reference's tail in torch --
            torch.max, the fc / g_fc Sequentials, batch_norm, leaky_relu, repeat, cat, and the add_cov Sequential (Conv1d) where the block has one,
            in the reference's order (the global branch, then the layer).  Autograd runs a graph's nodes latest first, so in that order the
            dense [B,Fin,N] cotangent of the max appears after the layer's backward, where the memory peaks; `baseline_layer_first` is the
            peak of the same code with the layer called first, where that tensor waits through the layer's backward (recorded, not compared);
  tail      the tail's launches alone, with the arguments the block hands them (cm_stats + finalize + block_tail_fwd; block_tail_bwd_reduce +
            finalize + block_tail_bwd_apply), against the same part of the torch tail alone on the same Y, xs, g, with the GB/s each launch
            achieves on the bytes it has to move (Y read once per pass, every output written once).  "concatenating" form (the plain
            blocks): both outputs, torch = batch_norm, leaky_relu, two repeats, two cats and their autograd backward.  "middle" form (the
            blocks with add_cov): g_out alone in forward, g_out's cotangent and the product's cotangent of the activated tensor (`extra`)
            in backward, torch = batch_norm, leaky_relu, one repeat, one cat; the add_cov product itself is outside this figure.
The routes are timed alternately in the same process; every figure is a median with its min and max over the repeats.  `verdict` compares
the spreads: "faster" / "slower" only where the [min, max] ranges of block and baseline do not overlap, "tie" otherwise.  No ratio is
asserted: the file records what was measured.

    python tools/blocks_bench.py [--out profiles/blocks_bench.json] [--B 32 --N 2048]
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

from deform_bench import timed_pair          # noqa: E402


def peak_bytes(fn):
    """-> (requested, allocated): the peak of one call above what was live before it.  `requested` sums the sizes the code asked the
    caching allocator for; `allocated` (max_memory_allocated, the sibling tools' figure) sums the sizes of the blocks it handed out, and a
    block above 1 MiB is handed out whole when what a split would leave is 1 MiB or less: that figure moves by up to 1 MiB per live large
    tensor with the order of earlier allocations and frees, which is more than the two routes differ by."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    st = torch.cuda.memory_stats()
    base = st["requested_bytes.all.current"], st["allocated_bytes.all.current"]
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    st = torch.cuda.memory_stats()
    return st["requested_bytes.all.peak"] - base[0], st["allocated_bytes.all.peak"] - base[1]


def torch_tail(y, xs, g, bn, middle=False):
    """the reference's tail behind the layer, as written there (middle: x_ec goes on to add_cov, only g_out is concatenated here)"""
    B, _, L = y.shape
    x_ec = F_.leaky_relu(F_.batch_norm(y, None, None, bn.weight, bn.bias, True, 0.1, 1e-5), 0.01)
    x_out = x_ec if middle else torch.cat((xs.view(B, -1, 1).repeat(1, 1, L), x_ec), 1)
    g_out = None if g is None else torch.cat((g.view(B, -1, 1).repeat(1, 1, L), x_ec), dim=1)
    return x_out, g_out


def bench(spgan, name, args, B, N, seed, takes_pc):
    ops, bt, em = spgan.ops, spgan.block_tail, spgan.edge_max
    g = torch.Generator().manual_seed(seed)
    m = getattr(spgan, name)(*args).cuda().train()
    layer, bn, _ = m._parts()
    k, Fin = layer.k, layer.Fin
    g_fc, add_cov = getattr(m, "g_fc", None), getattr(m, "add_cov", None)
    x = (torch.randn(B, Fin, N, generator=g) * 0.7).cuda().requires_grad_(True)
    pc = (torch.rand(B, 3, N, generator=g) * 2 - 1).cuda().requires_grad_(True) if takes_pc else None
    with torch.no_grad():
        _, idx = spgan.get_edge_features(x.detach(), k, return_idx=True)          # one graph for both routes
    idx32 = ops.idx_from_local64(idx, B, N, k)      # the layers' own format: an int64 graph is range-checked with a host synchronisation per call

    def run_layer():
        return layer(x, pc, idx=idx32) if takes_pc else layer(x, idx=idx32)

    def block():
        out = m(x, pc, idx=idx32) if takes_pc else m(x, idx=idx32)
        return out if isinstance(out, tuple) else (out, None)

    def baseline(layer_first=False):
        y = run_layer() if layer_first else None
        xs = m.fc(torch.max(x, 2)[0])                   # the reference's order: the global branch, then the layer
        gv = None if g_fc is None else g_fc(xs)
        if y is None:
            y = run_layer()
        x_out, g_out = torch_tail(y, xs, gv, bn)
        return (x_out if add_cov is None else add_cov(x_out)), g_out
    with torch.no_grad():
        o_b, o_t = block(), baseline()
        diff = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(o_b, o_t) if a is not None)
        cots = [None if o is None else torch.randn(o.shape, generator=g).cuda() for o in o_b]
        Y = run_layer().contiguous()
        del o_b, o_t

    def reset():
        x.grad = None
        if pc is not None:
            pc.grad = None
        for p in m.parameters():
            p.grad = None

    def step(fn):
        def run():
            reset()
            outs = fn()
            sum((o * c).sum() for o, c in zip(outs, cots) if o is not None).backward()
        return run
    block_step, base_step = step(block), step(baseline)
    # the tail alone, with the arguments the block hands its launches
    middle = add_cov is not None
    C, L = Y.shape[1], Y.shape[2]
    Cs, Cg = (0 if middle else m.fc[3].weight.shape[0]), (512 if g_fc is not None else 0)
    xs = torch.randn(B, m.fc[3].weight.shape[0], generator=g).cuda()
    gv = torch.randn(B, Cg, generator=g).cuda() if Cg else None
    dx, dg = torch.randn(B, Cs + C, L, generator=g).cuda(), (torch.randn(B, Cg + C, L, generator=g).cuda() if Cg else None)
    kx, kex = (None, dx) if middle else (dx, None)              # middle: the product's cotangent of the activated tensor arrives as `extra`
    gamma, beta = bn.weight.detach(), bn.bias.detach()
    st = {}

    def k_stats():
        part, rows = bt.cm_stats(Y)
        st["v"] = em.edge_max_bn(part, rows, B * L, gamma, beta, None, None)

    def k_fwd():
        return bt.block_tail_fwd(Y, None if middle else xs, gv, st["v"][0], st["v"][1], want_x=not middle, want_g=Cg > 0)

    def k_reduce():
        st["sums"] = bt.block_tail_bwd_reduce(Y, kx, dg, kex, Cs, Cg, st["v"][0], st["v"][1], st["v"][3], st["v"][2])[0]

    def k_apply():
        return bt.block_tail_bwd_apply(Y, kx, dg, kex, Cs, Cg, st["v"][0], st["v"][1], st["v"][3], st["v"][2], gamma, st["sums"])

    def fused_tail():
        k_stats(); k_fwd(); k_reduce(); k_apply()
    Yr, xsr = Y.clone().requires_grad_(True), xs.clone().requires_grad_(True)
    gvr = None if gv is None else gv.clone().requires_grad_(True)

    def torch_tail_step():
        Yr.grad = xsr.grad = None
        if gvr is not None:
            gvr.grad = None
        x_out, g_out = torch_tail(Yr, xsr, gvr, bn, middle)
        x_out.backward(dx) if g_out is None else torch.autograd.backward([x_out, g_out], [dx, dg])
    k_stats(); k_reduce()
    t = timed_pair([block_step, base_step, fused_tail, torch_tail_step, k_stats, k_fwd, k_reduce, k_apply])
    n = 4.0 * B * L
    wide = ((Cg + C) if Cg else 0) + (C if middle else Cs + C)       # the channels of the outputs written / the cotangents read
    moved = {"cm_stats": n * C, "block_tail_fwd": n * (C + wide - (C if middle else 0)),
             "block_tail_bwd_reduce": n * (C + wide), "block_tail_bwd_apply": n * C * (3 + (1 if Cg else 0))}
    launches = {q: {"ms": t[i], "bytes": moved[q], "GBps": moved[q] / (t[i]["median"] * 1e-3) / 1e9}
                for q, i in (("cm_stats", 4), ("block_tail_fwd", 5), ("block_tail_bwd_reduce", 6), ("block_tail_bwd_apply", 7))}
    routes = {"block_forward_backward": block_step, "baseline_forward_backward": base_step,
              "baseline_layer_first_forward_backward": step(lambda: baseline(True)), "fused_tail": fused_tail, "torch_tail": torch_tail_step}
    both = {q: peak_bytes(fn) for q, fn in routes.items()}
    pk, pka = {q: v[0] for q, v in both.items()}, {q: v[1] for q, v in both.items()}
    return {
        "block": "%s%s" % (name, tuple(args)), "shape": dict(B=B, N=N, C=C, L=L, Cs=Cs, Cg=Cg),
        "tail_form": "middle" if middle else "concatenating",
        "max_rel_difference_forward": diff,
        "block_forward_backward_ms": t[0], "baseline_forward_backward_ms": t[1],
        "measured_ratio_baseline_over_block": t[1]["median"] / t[0]["median"],
        "verdict": "faster" if t[0]["max"] < t[1]["min"] else ("slower" if t[0]["min"] > t[1]["max"] else "tie"),
        "tail_alone": {"fused_ms": t[2], "torch_ms": t[3], "measured_ratio_torch_over_fused": t[3]["median"] / t[2]["median"], "launches": launches},
        "peak_bytes": pk, "peak_allocated_bytes": pka,
        "block_peak_minus_baseline_bytes": pk["block_forward_backward"] - pk["baseline_forward_backward"],
        "block_peak_lower": pk["block_forward_backward"] < pk["baseline_forward_backward"],
        "block_peak_allocated_minus_baseline_bytes": pka["block_forward_backward"] - pka["baseline_forward_backward"],
        "block_peak_allocated_lower": pka["block_forward_backward"] < pka["baseline_forward_backward"],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32); ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import spgan
    res = {"device": torch.cuda.get_device_name(0), "timing": "device events; median / min / max of 7 repeats of 5 calls after 3 warm-up rounds",
           "configs": [bench(spgan, "bilateral_block_l2", (128, 256, a.N, 1, 20), a.B, a.N, 0, True),
                       bench(spgan, "bilateral_block_l1", (128, 256, a.N, 1, 20), a.B, a.N, 1, False),
                       bench(spgan, "deform_block_feat", (128, 128, 1, 20), a.B, a.N, 2, False),
                       bench(spgan, "deform_block_feat", (32, 32, 1, 8), 8, 256, 3, False)]}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
