#!/usr/bin/env python
"""Generate tests/golden/deform.npz by running the REAL reference `deform_edgeConv_simple` (Generation/modules.py:1432-1466) and
`deform_edgeConv_first` (:1394-1428), with conv2dbr :612-626 and get_edge_features :683-725, on the CPU, each case in float32 and again
in float64 on the float32 run's kNN graph, so that the two differ by rounding alone.  Nothing of the reference is copied: its file is
read at capture time, the two import lines that do not resolve without its CUDA extensions (`metrics.pointops`, `einops`; neither
is used by the classes captured here) are dropped in memory, and the module is executed up to `class PointTransformerLayer(`
(the file's tail runs a demo at import time).  Inputs and weights come from spgan.fixture_rng (tests/deform_model.py).

Per case `tag` (tests/deform_model.py::CASES): `tag|x`, `tag|g` (the cotangent, of the output's literal shape), `tag|idx` (int64
[B,N*k], the reference's graph), `tag|param|<state_dict key>`; results as `tag|<q>|full` (float32 run) and `tag|<q>|d64|full` (float64
run minus float32 run, stored in float32: deform_model.golden_f64 adds them up) for q in out, dx, grad|<parameter>, buf|<buffer>;
`tag|noise|<q>` = the rel-L2 distance of the two runs; `tag|near_tie_rows`.

Condition asserted before anything is written (a seed that fails it is skipped, the condition stays): at most 1 % of the rows of a
graph have a float32 distance gap below 1e-4 between consecutive ranks 0..k+1 (those rows are the ones a differently rounded kNN may
order differently; the GPU test excludes exactly them).

    python tests/golden/make_golden_deform.py          (SPGAN_REFERENCE = the reference checkout, default /root/reference)
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SPGAN_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "sp-gan_amd"))
torch.set_num_threads(8)

import deform_model as dm          # noqa: E402

DIST_GAP, MAX_NEAR_TIE = 1e-4, 0.01


def load_reference():
    path = os.path.join(REF, "Generation", "modules.py")
    drop = ("from metrics.pointops import", "from einops import")
    lines = [ln for ln in open(path, encoding="utf-8").read().split("\n") if not ln.startswith(drop)]
    lines = lines[:next(i for i, ln in enumerate(lines) if ln.startswith("class PointTransformerLayer("))]
    mod = types.ModuleType("reference_modules")
    exec(compile("\n".join(lines), path, "exec"), mod.__dict__)
    return mod


R = load_reference()


def run(tag, x, g, sd, dtype, idx=None):
    """One reference forward + backward in `dtype`; idx = the graph to replay (None: the reference builds and reports its own)."""
    c = dm.CASES[tag]
    simple = c["cls"] == "simple"
    m = (R.deform_edgeConv_simple if simple else R.deform_edgeConv_first)(c["Fin"], c["Fout"], c["k"])
    m.load_state_dict({k_: v.clone() for k_, v in sd.items()}, strict=True)
    m = m.to(dtype)
    m.train(c["train"])
    seen = {}
    orig = R.get_edge_features

    def gef(xx, k, num=-1, idx_=None, return_idx=False):
        ee, ii = orig(xx, k, idx=idx, return_idx=True)
        seen["idx"] = ii
        return ee
    R.get_edge_features = gef
    try:
        xr = x.to(dtype).clone().requires_grad_(True)
        out = m(xr, None) if simple else m(xr)
        (out * g.to(dtype)).sum().backward()
    finally:
        R.get_edge_features = orig
    assert tuple(out.shape) == dm.out_shape(c), (tag, tuple(out.shape))
    res = {"out": out.detach(), "dx": xr.grad}
    for n, p in m.named_parameters():
        res["grad|" + n] = p.grad
    for n, b in m.named_buffers():
        res["buf|" + n] = b.detach()
    return res, seen["idx"]


def near_tie_rows(x, k):
    """rows whose float32 distances (the reference's own, modules.py:695-699) of consecutive ranks 0..k+1 lie closer than DIST_GAP"""
    xt = x.permute(0, 2, 1)
    dist = -2 * torch.bmm(xt, x) + torch.sum(xt ** 2, dim=2, keepdim=True) + torch.sum(xt ** 2, dim=2, keepdim=True).permute(0, 2, 1)
    ds = torch.sort(dist, dim=2)[0][:, :, :k + 2]
    return ((ds[:, :, 1:] - ds[:, :, :-1]).min(dim=2)[0] < DIST_GAP).reshape(-1)


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def capture(tag):
    k = dm.CASES[tag]["k"]
    for seed in range(20000):
        x, g, sd = dm.case_tensors(tag, seed)
        near = near_tie_rows(x, k)
        if near.float().mean().item() <= MAX_NEAR_TIE:
            break
    else:
        raise SystemExit("no seed of case %s meets the condition" % tag)
    _, idx = R.get_edge_features(x, k, return_idx=True)
    r32, idx32 = run(tag, x, g, sd, torch.float32)
    assert torch.equal(idx, idx32)
    assert near.float().mean().item() <= MAX_NEAR_TIE
    r64, idx64 = run(tag, x, g, sd, torch.float64, idx=idx)
    assert torch.equal(idx, idx64)
    out = {"%s|x" % tag: x.numpy(), "%s|g" % tag: g.numpy(), "%s|idx" % tag: idx.numpy().astype(np.int64), "%s|seed" % tag: np.int64(seed),
           "%s|near_tie_rows" % tag: near.numpy()}
    for n, v in sd.items():
        out["%s|param|%s" % (tag, n)] = v.numpy()
    noise = {}
    for q in r32:
        out["%s|%s|full" % (tag, q)] = r32[q].numpy()
        out["%s|%s|d64|full" % (tag, q)] = (r64[q].double() - r32[q].double()).numpy().astype(np.float32)
        if r32[q].dtype.is_floating_point:
            noise[q] = out["%s|noise|%s" % (tag, q)] = np.float64(rel(r32[q], r64[q]))
    print("%s: seed %d, near-tie rows %d, noise %s" % (tag, seed, int(near.sum()), {q: "%.2e" % v for q, v in noise.items()}))
    # the quantities whose 5 x noise exceeds the GPU test's base bound (3e-6 out / dx, 5e-6 parameter gradients): they take the fallback
    need = [q for q, v in noise.items() if not q.startswith("buf|") and q[5:] not in dm.ZERO_GRAD_BIASES
            and 5 * v > (3e-6 if q in ("out", "dx") else 5e-6)]
    print("%s: quantities that need the 5 x noise fallback: %s" % (tag, need or "none"))
    return out


if __name__ == "__main__":
    OUT = {}
    for tag in dm.CASES:
        OUT.update(capture(tag))
    path = os.path.join(HERE, "deform.npz")
    np.savez_compressed(path, **OUT)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))
