#!/usr/bin/env python3
"""Time the Frechet point-cloud distance on one GPU and print one JSON line (medians of --reps repeats with min and max):

  per shape (n1 = n2 = n activations of d features): the moments launches (both sets), the solve (sqrt, sqrt, polar; iterations per
  stage), the whole spgan.fpd.FPD call, and csrc/frechet.hip's product kernel in TFLOP/s -- as a fraction of what a register-only loop
  of v_mfma_f64_16x16x4_f64 reaches (tools/exp/run_mfma_f64_peak.py, passed in by --ceiling-json);
  torch leg: the same three stages written with torch.matmul in float64 on the device (the vendor dgemm; a host read per iteration);
  host leg: the reference's formulation (np.cov, scipy.linalg.sqrtm) on the host after copying the activations, once per shape;
  skipped if scipy does not import.

    python tools/fpd_bench.py [--reps 21] [--ceiling-json FILE] [--no-host] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sp-gan_amd"))

from spgan import _lib, fpd            # noqa: E402
from spgan.ops import _p, _s           # noqa: E402

SHAPES = [(2048, 512), (5000, 1024), (2048, 1808)]


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return {"median_ms": round(times[len(times) // 2], 4), "min_ms": round(times[0], 4), "max_ms": round(times[-1], 4)}


def torch_sqrt(S):
    d = S.shape[0]
    eye = torch.eye(d, dtype=torch.float64, device=S.device)
    nrm = torch.linalg.norm(S)
    Y, Z = S / nrm, eye.clone()
    for it in range(1, 41):
        T = 1.5 * eye - 0.5 * (Z @ Y)
        Yn, Z = Y @ T, T @ Z
        stop = (torch.linalg.norm(Yn - Y) <= 1e-13 * torch.linalg.norm(Yn)).item()
        Y = Yn
        if stop:
            break
    return Y, nrm, it


def torch_frechet(m1, s1, m2, s2):
    Y1, n1, i1 = torch_sqrt(s1)
    Y2, n2, i2 = torch_sqrt(s2)
    X0 = Y1 @ Y2
    d = X0.shape[0]
    eye = torch.eye(d, dtype=torch.float64, device=X0.device)
    t_old = torch.linalg.norm(X0)
    X = X0 / t_old
    for i3 in range(1, 41):
        X = X @ (1.5 * eye - 0.5 * (X.t() @ X))
        t = (X * X0).sum()
        stop = ((t - t_old).abs() <= 1e-14 * t.abs()).item()
        t_old = t
        if stop:
            break
    v = ((m1 - m2) ** 2).sum() + torch.trace(s1) + torch.trace(s2) - 2.0 * torch.sqrt(n1) * torch.sqrt(n2) * t_old
    return v.item(), (i1, i2, i3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--ceiling-json", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ceiling = None
    if args.ceiling_json and os.path.exists(args.ceiling_json):
        with open(args.ceiling_json) as f:
            ceiling = float(json.loads(f.readline())["ceiling_tflops"])
    try:
        import scipy.linalg
    except ImportError:
        scipy = None
    lib = _lib.load()
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "mfma_f64_register_loop_tflops": ceiling, "shapes": {}}
    g = torch.Generator().manual_seed(0)
    for n, d in SHAPES:
        mix = torch.rand((1, d), generator=g) + 0.5
        a = torch.relu(torch.randn((n, d), generator=g) * mix + 0.3 * torch.randn((n, 1), generator=g) + 0.3).cuda()
        b = torch.relu(torch.randn((n, d), generator=g) * mix + 0.3 * torch.randn((n, 1), generator=g) + 0.1).cuda()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        m1, s1 = fpd.activation_statistics(a)
        m2, s2 = fpd.activation_statistics(b)
        info = fpd.frechet_distance_info(m1, s1, m2, s2)
        peak = torch.cuda.max_memory_allocated() - base
        r = {"value": info["distance"], "iterations": list(info["iterations"]), "peak_bytes_above_inputs": int(peak)}
        r["moments_both_sets"] = timed(lambda: (fpd.activation_statistics(a), fpd.activation_statistics(b)), args.reps)
        r["solve"] = timed(lambda: fpd.frechet_distance_device(m1, s1, m2, s2), args.reps)
        r["fpd_call"] = timed(lambda: fpd.FPD(a, b), args.reps)
        A, B = torch.randn((d, d), dtype=torch.float64, generator=g).cuda(), torch.randn((d, d), dtype=torch.float64, generator=g).cuda()
        C = torch.empty_like(A)
        for ta in (0, 1):
            t = timed(lambda: _lib.check(lib.spgan_f64_gemm(_p(A), _p(B), _p(C), d, ta, 1.0, 0.0, 0.0, _s()), "f64_gemm"), args.reps)
            t["tflops"] = round(2.0 * d ** 3 / (t["median_ms"] * 1e-3) / 1e12, 3)
            if ceiling:
                t["fraction_of_register_loop"] = round(t["tflops"] / ceiling, 4)
            r["product_kernel" + ("_at" if ta else "")] = t
        t = timed(lambda: torch.matmul(A, B, out=C), args.reps)
        t["tflops"] = round(2.0 * d ** 3 / (t["median_ms"] * 1e-3) / 1e12, 3)
        r["torch_matmul_f64"] = t
        tv, tits = torch_frechet(m1, s1, m2, s2)
        r["torch_leg_solve"] = timed(lambda: torch_frechet(m1, s1, m2, s2), max(3, args.reps // 3), warmup=1)
        r["torch_leg_solve"].update(value=tv, iterations=list(tits))
        if scipy is not None and not args.no_host:
            t0 = time.perf_counter()
            x1, x2 = a.cpu().numpy(), b.cpu().numpy()
            mu1, c1 = np.mean(x1, axis=0), np.cov(x1, rowvar=False)
            mu2, c2 = np.mean(x2, axis=0), np.cov(x2, rowvar=False)
            t1 = time.perf_counter()
            covmean, _ = scipy.linalg.sqrtm(c1.dot(c2), disp=False)
            hv = float((mu1 - mu2).dot(mu1 - mu2) + np.trace(c1) + np.trace(c2) - 2.0 * np.trace(np.real(covmean)))
            t2 = time.perf_counter()
            r["host_leg_once"] = {"copy_and_moments_ms": round(1e3 * (t1 - t0), 1), "sqrtm_ms": round(1e3 * (t2 - t1), 1), "value": hv,
                                  "threads": int(os.environ.get("OMP_NUM_THREADS", "0"))}
        res["shapes"]["n%d_d%d" % (n, d)] = r
        print("done n=%d d=%d" % (n, d), file=sys.stderr, flush=True)
        del a, b, m1, s1, m2, s2, A, B, C
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
