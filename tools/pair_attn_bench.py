#!/usr/bin/env python
"""Microbenchmark of spgan.PointTransformerLayer (csrc/pair_attn.hip): device-event timing inside a warmed loop, one JSON document.  It
follows tools/deform_xyz_bench.py.

Per shape (dim 128, pos_mlp_hidden_dim 64, attn_mlp_hidden_mult 4), on the same GPU:
  layer   the module: forward, forward + backward, peak memory of one forward + backward;
  torch   the reference's formulation written in torch (the [b,n,n,3], [b,n,n,dim] and [b,n,n,dim*mult] tensors), where it fits:
          b 4 n 512 and b 1 n 1024; at n = 2048 its hidden tensor alone is 8.6 GB per cloud and only the layer runs;
  kernel  the forward pair launch on its own: the FLOPs it issues (the K = H product, 2 b n^2 Mp Hp) over its time against the
          157.3 TFLOP/s fp32-MFMA peak.
The routes are timed alternately in the same process; every figure is a median with its min and max over 21 repeats of one call after
3 warm-up rounds.  No ratio is asserted: the file records what was measured.

    python tools/pair_attn_bench.py [--out FILE]          (default: profiles/pair_attn_bench.json)
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sp-gan_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from deform_bench import peak_bytes, timed_pair          # noqa: E402

MFMA_F32_PEAK_TFLOPS = 157.3
SHAPES = [(4, 512, True), (1, 1024, True), (1, 2048, False), (32, 2048, False)]      # (b, n, the torch formulation fits)


def bench(spgan, b, n, with_torch, dim=128, H=64, mult=4, seed=0):
    from spgan import pair_attn
    g = torch.Generator().manual_seed(seed)
    m = spgan.PointTransformerLayer(dim, H, mult).cuda()
    x = torch.randn(b, n, dim, generator=g).cuda().requires_grad_(True)
    pos = torch.randn(b, n, 3, generator=g).cuda().requires_grad_(True)
    cot = torch.randn(b, n, dim, generator=g).cuda()

    def composed(xx, pp):
        q, k, v = m.to_qkv(xx).chunk(3, dim=-1)
        e = m.pos_mlp(pp[:, :, None] - pp[:, None, :])
        a = m.attn_mlp(q[:, :, None] - k[:, None, :] + e).squeeze(-1).softmax(dim=-1)
        return torch.einsum("bij,bijd->bid", a, v[:, None] + e)

    def reset():
        x.grad = pos.grad = None
        for p in m.parameters():
            p.grad = None

    def layer_fwd():
        with torch.no_grad():
            return m(x, pos)

    def torch_fwd():
        with torch.no_grad():
            return composed(x, pos)

    def layer_step():
        reset()
        (m(x, pos) * cot).sum().backward()

    def torch_step():
        reset()
        (composed(x, pos) * cot).sum().backward()

    # the forward pair launch on its own, on the operands the module hands it
    with torch.no_grad():
        p0, p2, a0, a2 = m.pos_mlp[0], m.pos_mlp[2], m.attn_mlp[0], m.attn_mlp[2]
        Wp1p, Wa1p, _, _, _, Wc, _, cvec, wa2, _, _ = pair_attn.images(p0.weight, p0.bias, p2.weight, p2.bias, a0.weight, a0.bias, a2.weight, m.to_qkv.weight)
        qkv = spgan.ops.gemm_nt(x.detach().view(b * n, dim), m.to_qkv.weight.detach(), exact=True)
        QaC = spgan.ops.gemm_nt(qkv[:, :dim], Wa1p, cvec, exact=True)
        Ka = spgan.ops.gemm_nt(qkv[:, dim:2 * dim], Wa1p, exact=True)
        posc = pos.detach().contiguous()

    def pair_kernel():
        return pair_attn.pair_attn_fwd(posc, Wp1p, QaC, Ka, Wc, wa2, qkv[:, 2 * dim:])

    fns = [layer_fwd, layer_step, pair_kernel] + ([torch_fwd, torch_step] if with_torch else [])
    t = timed_pair(fns, warmup=3, iters=1, repeats=21)
    flops = 2.0 * b * n * n * Wc.shape[0] * Wc.shape[1]
    tf = flops / (t[2]["median"] * 1e-3) / 1e12
    res = {"shape": dict(b=b, n=n, dim=dim, pos_mlp_hidden_dim=H, attn_mlp_hidden_mult=mult),
           "layer_forward_ms": t[0], "layer_forward_backward_ms": t[1],
           "pair_forward_kernel": {"ms": t[2], "flops_issued": flops, "tflops": tf, "fraction_of_fp32_mfma_peak": tf / MFMA_F32_PEAK_TFLOPS},
           "peak_bytes": {"layer_forward_backward": peak_bytes(layer_step), "layer_forward": peak_bytes(layer_fwd),
                          "one_pair_tensor_b_n_n_dim": 4 * b * n * n * dim}}
    if with_torch:
        ref = torch_fwd()
        res["max_rel_difference_forward"] = float((layer_fwd() - ref).abs().max() / ref.abs().max())
        del ref
        res.update({"torch_forward_ms": t[3], "torch_forward_backward_ms": t[4],
                    "measured_ratio_forward_torch_over_layer": t[3]["median"] / t[0]["median"],
                    "measured_ratio_forward_backward_torch_over_layer": t[4]["median"] / t[1]["median"]})
        res["peak_bytes"]["torch_forward_backward"] = peak_bytes(torch_step)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_attn_bench.json"))
    a = ap.parse_args()
    import spgan
    res = {"device": torch.cuda.get_device_name(0), "timing": "device events; median / min / max of 21 repeats of 1 call after 3 warm-up rounds",
           "fp32_mfma_peak_tflops": MFMA_F32_PEAK_TFLOPS, "configs": []}
    for b, n, fits in SHAPES:
        res["configs"].append(bench(spgan, b, n, fits))
        print(json.dumps(res["configs"][-1]), flush=True)
        torch.cuda.empty_cache()
    txt = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
