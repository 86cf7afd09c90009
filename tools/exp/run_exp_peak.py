"""EXPERIMENT: tools/exp/exp_peak.hip -- exp evaluations per second of a register-only expf loop; prints one JSON line.

    python tools/exp/run_exp_peak.py [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SO = os.path.join(ROOT, "tools/exp/libexp_peak.so")


def measure():
    if not os.path.exists(SO):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        os.path.join(ROOT, "tools/exp/exp_peak.hip"), "-o", SO], check=True)
    import torch
    lib = C.CDLL(SO)
    lib.exp_exp_peak.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    s = torch.cuda.current_stream().cuda_stream
    res = {"device": torch.cuda.get_device_name(0), "compute_units": cus, "reps": 21}
    best = {0: 0.0, 1: 0.0}
    for fast in (0, 1):
        for acc in (4, 8):
            for wgs_per_cu in (1, 2, 4):
                blocks, iters = cus * wgs_per_cu, 4000
                out = torch.empty((blocks * 256,), dtype=torch.float32, device="cuda")
                times = []
                for rep in range(3 + 21):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    assert lib.exp_exp_peak(out.data_ptr(), blocks, iters, acc, fast, s) == 0
                    e1.record()
                    torch.cuda.synchronize()
                    if rep >= 3:
                        times.append(e0.elapsed_time(e1))
                times.sort()
                n = blocks * 256.0 * iters * acc
                rate = n / (times[len(times) // 2] * 1e-3)
                res["%s_acc%d_waves_per_simd%d" % ("fast" if fast else "expf", acc, wgs_per_cu)] = {
                    "gexp_per_s_median": round(rate / 1e9, 1), "gexp_per_s_min": round(n / (times[-1] * 1e-3) / 1e9, 1),
                    "gexp_per_s_max": round(n / (times[0] * 1e-3) / 1e9, 1)}
                best[fast] = max(best[fast], rate)
    res["ceiling_expf_gexp_per_s"] = round(best[0] / 1e9, 1)
    res["ceiling_fast_gexp_per_s"] = round(best[1] / 1e9, 1)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    line = json.dumps(measure())
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
