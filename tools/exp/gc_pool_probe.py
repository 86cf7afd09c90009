#!/usr/bin/env python
"""What bounds spgan.gc_attn.pool_fwd at [32,128,40960]?  Device-event times (median of 9 x 10 back-to-back calls) of the pooling launcher
with attention and with average pooling (no logits, no exp, no rescale: a weighted sum only), in both layouts, next to streams of known
traffic on the same tensor: torch's x.sum() (|x| read), bwd_reduce (2|x| read), apply_fwd (|x| read + |x| written).

    python tools/exp/gc_pool_probe.py > profiles/gc_attn_pool_probe.txt
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "sp-gan_amd"))


def timed(fn, iters=10, repeats=9):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / iters)
    return statistics.median(ts), min(ts), max(ts)


def main():
    from spgan import gc_attn
    B, C, L = 32, 128, 40960
    g = torch.Generator().manual_seed(0)
    size = B * C * L * 4
    print("# [%d,%d,%d], |x| = %.1f MB; ms = median [min, max]; TB/s = bytes of the column 'traffic' over the median" % (B, C, L, size / 1e6))
    for layout in ("cm", "pm"):
        shape = (B, C, L) if layout == "cm" else (B * L, C)
        x = torch.randn(shape, generator=g).cuda()
        cot = torch.randn(shape, generator=g).cuda()
        w = (torch.randn(C, generator=g) / C ** 0.5).cuda()
        bias = torch.zeros(1).cuda()
        mul, add = torch.rand(B, C, generator=g).cuda(), torch.randn(B, C, generator=g).cuda()
        rows = [("pool_fwd attention", 1, lambda: gc_attn.pool_fwd(x, layout, B, L, w, bias)),
                ("pool_fwd average", 1, lambda: gc_attn.pool_fwd(x, layout, B, L)),
                ("torch x.sum()", 1, lambda: x.sum()),
                ("torch x.sum(dim=-1)", 1, lambda: x.sum(dim=-1)),
                ("bwd_reduce", 2, lambda: gc_attn.bwd_reduce(x, cot, layout, B, L)),
                ("apply_fwd", 2, lambda: gc_attn.apply_fwd(x, layout, B, L, mul, add))]
        for name, passes, fn in rows:
            med, lo, hi = timed(fn)
            print("%s  %-22s traffic %d|x|  %.3f ms [%.3f, %.3f]  %.2f TB/s" % (layout, name, passes, med, lo, hi, passes * size / med * 1e-9))
        del x, cot


if __name__ == "__main__":
    main()
