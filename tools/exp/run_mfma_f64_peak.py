"""EXPERIMENT: tools/exp/mfma_f64_peak.hip -- TFLOP/s of a register-only v_mfma_f64_16x16x4_f64 loop; prints one JSON line.

    python tools/exp/run_mfma_f64_peak.py [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
so = os.path.join(ROOT, "tools/exp/libmfma_f64_peak.so")
if not os.path.exists(so):
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                    os.path.join(ROOT, "tools/exp/mfma_f64_peak.hip"), "-o", so], check=True)
import torch      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()
lib = C.CDLL(so)
lib.exp_mfma_f64_peak.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
cus = torch.cuda.get_device_properties(0).multi_processor_count
s = torch.cuda.current_stream().cuda_stream
res = {"device": torch.cuda.get_device_name(0), "compute_units": cus, "reps": 21}
best = 0.0
for acc in (1, 2, 4):
    for wgs_per_cu in (1, 2, 4, 8):
        blocks, iters = cus * wgs_per_cu, 20000
        out = torch.empty((blocks * 256,), dtype=torch.float64, device="cuda")
        times = []
        for rep in range(3 + 21):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert lib.exp_mfma_f64_peak(out.data_ptr(), blocks, iters, acc, s) == 0
            e1.record()
            torch.cuda.synchronize()
            if rep >= 3:
                times.append(e0.elapsed_time(e1))
        times.sort()
        flop = blocks * 4.0 * iters * acc * 2 * 16 * 16 * 4
        tf = flop / (times[len(times) // 2] * 1e-3) / 1e12
        res["acc%d_waves_per_simd%d" % (acc, wgs_per_cu)] = {"tflops_median": round(tf, 2), "tflops_min": round(flop / (times[-1] * 1e-3) / 1e12, 2),
                                                             "tflops_max": round(flop / (times[0] * 1e-3) / 1e12, 2)}
        best = max(best, tf)
res["ceiling_tflops"] = round(best, 2)
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
