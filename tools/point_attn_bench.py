#!/usr/bin/env python
"""Microbenchmark of dot-product point attention without a [B,N,N] map (csrc/point_attn.hip): device-event timing inside a warmed loop,
one JSON document.  It follows tools/pair_attn_bench.py.

  Attention(640)   B 32, N 2048 (the generator's call) and B 4, N 8192: forward, forward + backward and the peak memory of one forward +
                   backward, materialize=True against materialize=False;
  Self_Attn(128)   B 32, N 2048: the module against the reference's formulation written in torch (bmm, softmax over dim 1, bmm);
  kernel           the forward launch on its own at Attention(640)'s widths (dk 80, dv 320): 2 B N^2 (dk + dv) FLOPs over its time, as a
                   share of the 157.3 TFLOP/s fp32-MFMA peak (the comparable figure of pair_attn's forward kernel is 0.52).  The time is
                   taken with device events around the launch; a kernel-trace figure is recorded as "not measured" unless --kernel-ms
                   hands one in from a separate profiler run.
The routes are timed alternately in the same process; every figure is a median with its min and max over 21 repeats of one call after
3 warm-up rounds.  No ratio is asserted: the file records what was measured.

    python tools/point_attn_bench.py [--out FILE] [--kernel-ms MS]          (default: profiles/point_attn_bench.json)
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


def _inputs(B, ch, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (0.5 * torch.randn(B, ch, N, generator=g)).cuda().requires_grad_(True)
    return x, torch.randn(B, ch, N, generator=g).cuda()


def _steps(m, x, cot, fn=None):
    fn = fn or m

    def fwd():
        with torch.no_grad():
            return fn(x)

    def step():
        x.grad = None
        for p in m.parameters():
            p.grad = None
        (fn(x) * cot).sum().backward()
    return fwd, step


def bench_attention(spgan, B, N, ch=640):
    torch.manual_seed(0)
    m = spgan.Attention(ch).cuda()
    with torch.no_grad():
        m.gamma.fill_(0.5)
    x, cot = _inputs(B, ch, N)

    def route(flag):
        def fn(xx):
            m.materialize = flag
            return m(xx)
        return _steps(m, x, cot, fn)
    mat_f, mat_s = route(True)
    fus_f, fus_s = route(False)
    t = timed_pair([mat_f, fus_f, mat_s, fus_s], warmup=3, iters=1, repeats=21)
    ref = mat_f()
    diff = float((fus_f() - ref).abs().max() / ref.abs().max())
    del ref
    res = {"module": "Attention", "shape": dict(B=B, N=N, ch=ch, dk=ch // 8, dv=ch // 2),
           "materialize_true": {"forward_ms": t[0], "forward_backward_ms": t[2], "peak_bytes_forward_backward": peak_bytes(mat_s)},
           "materialize_false": {"forward_ms": t[1], "forward_backward_ms": t[3], "peak_bytes_forward_backward": peak_bytes(fus_s)},
           "one_map_bytes": 4 * B * N * N, "max_rel_difference_forward": diff,
           "measured_ratio_forward_fused_over_materialised": t[1]["median"] / t[0]["median"],
           "measured_ratio_forward_backward_fused_over_materialised": t[3]["median"] / t[2]["median"]}
    for k in ("forward", "forward_backward"):
        r = res["measured_ratio_%s_fused_over_materialised" % k]
        res["faster_route_" + k] = "materialize=False" if r < 1.0 else "materialize=True"
    return res


def bench_self_attn(spgan, B, N, ch=128):
    torch.manual_seed(0)
    m = spgan.Self_Attn(ch).cuda()
    with torch.no_grad():
        m.gamma.fill_(0.5)
    x, cot = _inputs(B, ch, N)

    def composed(xx):                                     # the reference's forward on the module's parameters
        query = m.query(xx).permute(0, 2, 1)
        attn = torch.softmax(torch.bmm(query, m.key(xx)), 1)
        return m.gamma * torch.bmm(m.value(xx), attn) + xx
    mod_f, mod_s = _steps(m, x, cot)
    tor_f, tor_s = _steps(m, x, cot, composed)
    t = timed_pair([mod_f, tor_f, mod_s, tor_s], warmup=3, iters=1, repeats=21)
    ref = tor_f()
    diff = float((mod_f() - ref).abs().max() / ref.abs().max())
    del ref
    return {"module": "Self_Attn", "shape": dict(B=B, N=N, in_dim=ch, dk=ch // 8, dv=ch),
            "module_forward_ms": t[0], "module_forward_backward_ms": t[2], "torch_forward_ms": t[1], "torch_forward_backward_ms": t[3],
            "peak_bytes_forward_backward": {"module": peak_bytes(mod_s), "torch": peak_bytes(tor_s)}, "one_map_bytes": 4 * B * N * N,
            "max_rel_difference_forward": diff,
            "measured_ratio_forward_torch_over_module": t[1]["median"] / t[0]["median"],
            "measured_ratio_forward_backward_torch_over_module": t[3]["median"] / t[2]["median"]}


def bench_kernel(spgan, B, N, dk, dv, kernel_ms):
    from spgan import point_attn
    g = torch.Generator().manual_seed(1)
    cat = (torch.randn(B * N, 2 * dk + dv, generator=g) * 0.4).cuda()
    dO = torch.randn(B * N, dv, generator=g).cuda()
    q, k, v = cat[:, :dk], cat[:, dk:2 * dk], cat[:, 2 * dk:]
    _, lse = point_attn.point_attn_fwd(q, k, v, B, N)
    dcat = torch.empty_like(cat)
    t = timed_pair([lambda: point_attn.point_attn_fwd(q, k, v, B, N),
                    lambda: point_attn.point_attn_bwd(q, k, v, dO, lse, B, N, dq=dcat[:, :dk], dk_out=dcat[:, dk:2 * dk], dv_out=dcat[:, 2 * dk:])],
                   warmup=3, iters=1, repeats=21)
    f_fwd, f_bwd = 2.0 * B * N * N * (dk + dv), 2.0 * B * N * N * (4 * dk + 3 * dv)
    tf = f_fwd / (t[0]["median"] * 1e-3) / 1e12
    tb = f_bwd / (t[1]["median"] * 1e-3) / 1e12
    res = {"shape": dict(B=B, N=N, dk=dk, dv=dv),
           "forward_kernel": {"ms_device_events": t[0], "flops_counted": f_fwd, "tflops": tf, "fraction_of_fp32_mfma_peak": tf / MFMA_F32_PEAK_TFLOPS},
           "backward_both_roles": {"ms_device_events": t[1], "flops_counted": f_bwd, "tflops": tb, "fraction_of_fp32_mfma_peak": tb / MFMA_F32_PEAK_TFLOPS},
           "forward_kernel_trace": "not measured"}
    if kernel_ms:
        tk = f_fwd / (kernel_ms * 1e-3) / 1e12
        res["forward_kernel_trace"] = {"ms": kernel_ms, "tflops": tk, "fraction_of_fp32_mfma_peak": tk / MFMA_F32_PEAK_TFLOPS}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_attn_bench.json"))
    ap.add_argument("--kernel-ms", type=float, default=0.0, help="the forward kernel's time at B 32, N 2048 from a separate kernel-trace run")
    a = ap.parse_args()
    import spgan
    res = {"device": torch.cuda.get_device_name(0), "timing": "device events; median / min / max of 21 repeats of 1 call after 3 warm-up rounds",
           "fp32_mfma_peak_tflops": MFMA_F32_PEAK_TFLOPS, "pair_attn_forward_fraction_of_peak": 0.52, "configs": []}
    for job in (lambda: bench_attention(spgan, 32, 2048), lambda: bench_attention(spgan, 4, 8192), lambda: bench_self_attn(spgan, 32, 2048)):
        res["configs"].append(job())
        print(json.dumps(res["configs"][-1]), flush=True)
        torch.cuda.empty_cache()
    res["kernel"] = bench_kernel(spgan, 32, 2048, 80, 320, a.kernel_ms)
    print(json.dumps(res["kernel"]), flush=True)
    txt = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
