"""Times tools/exp/expansion_shapes.hip: Prim's algorithm of the expansion penalty as one wave per primitive against one workgroup per
primitive, at the shapes of tools/expansion_bench.py.  Device events, the two shapes alternating, median / min / max of 21 repeats of one
launch after 3 warm-up rounds; asserts that both produce the same tree.  Build first:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared tools/exp/expansion_shapes.hip -o tools/exp/libexpansion_shapes.so
    python tools/exp/run_expansion_shapes.py [--out profiles/expansion_shapes.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expansion_shapes.json"))
    a = ap.parse_args()
    lib = C.CDLL(os.path.join(ROOT, "tools", "exp", "libexpansion_shapes.so"))
    P_, I = C.c_void_p, C.c_int
    for fn in (lib.exp_prim_wave, lib.exp_prim_wg):
        fn.argtypes = [P_, I, I, P_, P_, P_]
        fn.restype = I
    s = torch.cuda.current_stream().cuda_stream
    res = {"device": torch.cuda.get_device_name(0), "what": "Prim's algorithm only (edge length and parent per vertex), ms per launch",
           "timing": "device events; median / min / max of 21 repeats of 1 launch after 3 warm-up rounds, shapes alternating", "configs": []}
    for B, n, p in ((32, 2048, 512), (20, 8192, 512), (32, 2048, 256), (32, 2048, 128), (32, 2048, 64)):
        x = torch.rand(B, n, 3, generator=torch.Generator().manual_seed(0)).cuda()
        P = B * n // p
        outs = [(torch.empty(P * p, device="cuda"), torch.empty(P * p, dtype=torch.int32, device="cuda")) for _ in range(2)]
        fns = [lambda f=f, o=o: f(x.data_ptr(), P, p, o[0].data_ptr(), o[1].data_ptr(), s) for f, o in zip((lib.exp_prim_wave, lib.exp_prim_wg), outs)]
        for _ in range(3):
            for fn in fns:
                assert fn() == 0
        torch.cuda.synchronize()
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "the two shapes disagree"
        t = [[], []]
        for _ in range(21):
            for i, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                t[i].append(e0.elapsed_time(e1))
        st = [{"median": statistics.median(o), "min": min(o), "max": max(o)} for o in t]
        res["configs"].append({"shape": dict(B=B, n=n, primitive_size=p, primitives=P), "wave_per_primitive_ms": st[0], "workgroup_per_primitive_ms": st[1],
                               "measured_ratio_workgroup_over_wave": st[1]["median"] / st[0]["median"]})
        print(json.dumps(res["configs"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
