#!/usr/bin/env python
"""Generate tests/golden/g24_pointconv.npz by running the REAL reference code of Common/pointconv_util.py:120-172, 199-383 on the CPU
(PointConvDensitySetAbstraction with kNN groups, with and without point features, PointConvSetAbstraction, the group_all form of the
density module, compute_density alone), each in float32 and again in float64 (`name|full` / `name|f64|full`).  Nothing of the
reference is copied: its file is read at capture time, the one import line that no longer resolves on a current scikit-learn
(`from sklearn.neighbors.kde import KernelDensity`, never used) is dropped in memory, and the module is executed.  The float64 pass
reuses the float32 pass's FPS and kNN indices (patched into the executed module), so that the two differ by rounding alone.

Conditions asserted before anything is written (a seed that fails one is skipped, the conditions stay):
  * for every centre the K-th and (K+1)-th nearest point differ by a float64 relative gap >= 1e-4;
  * the float32 neighbour set of every centre equals the float64 one;
  * the FPS indices are equal in both precisions.

    python tests/golden/make_golden_pointconv.py          (SPGAN_REFERENCE = the reference checkout, default /root/reference)
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SPGAN_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(HERE, ".."))
torch.set_num_threads(8)

import pointconv_model as pcm          # noqa: E402  (the case table only)


def load_reference():
    path = os.path.join(REF, "Common", "pointconv_util.py")
    lines = [ln for ln in open(path, encoding="utf-8").read().split("\n") if not ln.startswith("from sklearn.neighbors.kde import")]
    mod = types.ModuleType("reference_pointconv_util")
    exec(compile("\n".join(lines), path, "exec"), mod.__dict__)
    return mod


R = load_reference()
B, N, S, K, D = 2, 256, 64, 16, 6
B_ALL, N_ALL, D_ALL = 8, 96, 3          # group_all: bn_linear normalises over B values per channel, so B >= 8
OUT = {}


def put(name, t, f64=False):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    if a.dtype == np.float64 and not f64:
        a = a.astype(np.float32)
    OUT[name + ("|f64" if f64 else "") + "|full"] = a


def inputs(seed, b=B, n=N, d=D):
    rng = np.random.default_rng(seed)
    xyz = rng.random((b, 3, n), dtype=np.float64).astype(np.float32)
    pts = rng.standard_normal((b, d, n)).astype(np.float32)
    return torch.from_numpy(xyz), torch.from_numpy(pts)


class Recorder:
    """Wraps the reference's index-producing functions: records their float32 results, replays them in the float64 pass."""

    def __init__(self):
        self.fps, self.knn, self.replay = [], [], False
        self._fps, self._knn = R.farthest_point_sample, R.knn_point

    def __enter__(self):
        def fps(xyz, npoint):
            if self.replay:
                return self.fps.pop(0)
            r = self._fps(xyz, npoint); self.fps.append(r); return r

        def knn(nsample, xyz, new_xyz):
            if self.replay:
                return self.knn.pop(0)
            r = self._knn(nsample, xyz, new_xyz); self.knn.append(r); return r
        R.farthest_point_sample, R.knn_point = fps, knn
        return self

    def __exit__(self, *exc):
        R.farthest_point_sample, R.knn_point = self._fps, self._knn


def index_conditions(xyz_cm, npoint, nsample):
    """The conditions of the module docstring on one input -> (ok, smallest boundary gap)."""
    x32 = xyz_cm.permute(0, 2, 1).contiguous()
    x64 = x32.double()
    f32 = R.farthest_point_sample(x32, npoint)
    torch.set_default_dtype(torch.float64)          # the reference allocates its running distances in the default dtype (:72)
    f64 = R.farthest_point_sample(x64, npoint)
    torch.set_default_dtype(torch.float32)
    if not torch.equal(f32, f64):
        return False, 0.0
    c32, c64 = R.index_points(x32, f32), R.index_points(x64, f64)
    d64 = R.square_distance(c64, x64).sort(dim=-1)[0]
    gap = float(((d64[..., nsample] - d64[..., nsample - 1]) / d64[..., nsample].clamp_min(1e-300)).min())
    s32 = R.knn_point(nsample, x32, c32).sort(dim=-1)[0]
    s64 = R.knn_point(nsample, x64, c64).sort(dim=-1)[0]
    return gap >= 1e-4 and torch.equal(s32, s64), gap


def run_case(tag, args32, seed, store_inputs=True):
    """args32: dict name -> float32 tensor | None (forward order).  Gradients for loss = sum_i <out_i, gout_i>."""
    kind, cargs, _ = pcm.CASES[tag]

    def make():
        return getattr(R, kind)(*cargs)
    torch.manual_seed(seed)
    mod = make()
    sd0 = {k: v.clone() for k, v in mod.state_dict().items()}
    for k, v in sd0.items():
        OUT["%s|sd|%s" % (tag, k)] = v.numpy()
    gouts = None
    with Recorder() as rec:
        for f64 in (False, True):
            dt = torch.float64 if f64 else torch.float32
            torch.set_default_dtype(dt)
            m = make().to(dt)
            m.load_state_dict({k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd0.items()})
            m.train()
            xs = {k: (None if v is None else v.to(dt).clone().requires_grad_(True)) for k, v in args32.items()}
            rec.replay = f64
            outs = m(*xs.values())
            assert len(outs) == 2
            if gouts is None:
                rng = np.random.default_rng(seed + 77)
                gouts = [torch.from_numpy(rng.standard_normal(tuple(o.shape)).astype(np.float16).astype(np.float32)) for o in outs]   # float16-exact
                for i, g in enumerate(gouts):
                    OUT["%s|gout%d" % (tag, i)] = g.numpy().astype(np.float16)
                for i, r in enumerate(rec.fps):
                    OUT["%s|fps%d" % (tag, i)] = r.numpy().astype(np.int16)
                for i, r in enumerate(rec.knn):
                    OUT["%s|knn%d" % (tag, i)] = r.sort(dim=-1)[0].numpy().astype(np.int16)      # the neighbour SET: the order is unspecified
            sum((o * g.to(dt)).sum() for o, g in zip(outs, gouts)).backward()
            for i, o in enumerate(outs):
                put("%s|out%d" % (tag, i), o, f64)
            for k, p in m.named_parameters():
                put("%s|grad|%s" % (tag, k), p.grad, f64)
            for k, v in xs.items():
                if v is not None and v.grad is not None:
                    put("%s|gin|%s" % (tag, k), v.grad, f64)
            for k, v in m.named_buffers():
                if v.is_floating_point():
                    put("%s|buf|%s" % (tag, k), v, f64)
                elif not f64:
                    OUT["%s|buf|%s" % (tag, k)] = v.numpy()
            torch.set_default_dtype(torch.float32)
    for k, v in args32.items():
        if v is not None and store_inputs:
            OUT["%s|in|%s" % (tag, k)] = v.numpy()


def main():
    for seed in range(0, 64):
        xyz, pts = inputs(seed)
        ok, gap = index_conditions(xyz, S, K)
        if ok:
            break
    else:
        raise SystemExit("no seed met the index conditions")
    print("kNN cases: seed %d meets the index conditions (smallest boundary gap %.2e)" % (seed, gap))
    OUT["seed"] = np.int64(seed)
    run_case("dsa", {"xyz": xyz, "points": pts}, 21)
    run_case("dsa_nopts", {"xyz": xyz, "points": None}, 22, store_inputs=False)
    run_case("sa", {"xyz": xyz, "points": pts}, 23, store_inputs=False)
    xa, pa = inputs(100, b=B_ALL, n=N_ALL, d=D_ALL)
    run_case("dsa_all", {"xyz": xa, "points": pa}, 24)
    # ---- compute_density alone, with its gradient
    x32 = xyz.permute(0, 2, 1).contiguous()
    g = torch.from_numpy(np.random.default_rng(5).standard_normal((B, N)).astype(np.float16).astype(np.float32))
    OUT["kde|gout"] = g.numpy().astype(np.float16)
    for f64 in (False, True):
        dt = torch.float64 if f64 else torch.float32
        x = x32.to(dt).clone().requires_grad_(True)
        dens = R.compute_density(x, pcm.BANDWIDTH)
        (dens * g.to(dt)).sum().backward()
        put("kde|density", dens, f64)
        put("kde|gin|xyz", x.grad, f64)
    path = os.path.join(HERE, "g24_pointconv.npz")
    np.savez_compressed(path, **OUT)
    print("wrote %s: %d entries, %.2f MB" % (path, len(OUT), os.path.getsize(path) / 1e6))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
