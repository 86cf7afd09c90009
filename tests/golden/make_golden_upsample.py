#!/usr/bin/env python
"""Generate tests/golden/upsample.npz by running the REAL reference `upsample_edgeConv` (Generation/modules.py:799-845, with conv2dbr
:612-626 and get_edge_features :683-725) and `get_edge_features_xyz` (:727-776) on the CPU, each layer case in float32 and again in
float64 on the float32 run's kNN graph, so that the two differ by rounding alone.  Nothing of the reference is copied: its file is
read at capture time, the two import lines that do not resolve without its CUDA extensions (`metrics.pointops`, `einops`; neither
is used by the classes captured here) are dropped in memory, and the module is executed up to `class bilateral_upsample_edgeConv(`
(the file's tail runs a demo at import time).  Inputs and weights come from spgan.fixture_rng (tests/upsample_model.py).

Per case `tag` (tests/upsample_model.py::CASES): `tag|x`, `tag|g` (the cotangent), `tag|idx` (int64 [B,N*k], the reference's graph),
`tag|param|<state_dict key>`; results as `tag|<q>|full` (float32 run) and `tag|<q>|d64|full` (float64 run minus float32 run, stored
in float32: upsample_model.golden_f64 adds them up) for q in out, dx, grad|<parameter>, buf|<buffer>; `tag|noise|<q>` = the rel-L2
distance of the two runs; `tag|near_tie_rows`.  get_edge_features_xyz: `xyzfn|x`, `|pc`, `|gf`, `|gx` (cotangents), `|idx`,
`|e_fea|full`, `|e_xyz|full`, `|dx|full`, `|dpc|full` (float32 run: the values are gathers and differences), `|near_tie_rows`.

Condition asserted before anything is written (a seed that fails it is skipped, the condition stays): at most 1 % of the rows of a
graph have a float32 distance gap below 1e-4 between consecutive ranks 0..k+1 (those rows are the ones a differently rounded kNN may
order differently; the GPU test excludes exactly them).

    python tests/golden/make_golden_upsample.py          (SPGAN_REFERENCE = the reference checkout, default /root/reference)
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

import upsample_model as um          # noqa: E402

DIST_GAP, MAX_NEAR_TIE = 1e-4, 0.01


def load_reference():
    path = os.path.join(REF, "Generation", "modules.py")
    drop = ("from metrics.pointops import", "from einops import")
    lines = [ln for ln in open(path, encoding="utf-8").read().split("\n") if not ln.startswith(drop)]
    lines = lines[:next(i for i, ln in enumerate(lines) if ln.startswith("class bilateral_upsample_edgeConv("))]
    mod = types.ModuleType("reference_modules")
    exec(compile("\n".join(lines), path, "exec"), mod.__dict__)
    return mod


R = load_reference()


def run(tag, x, g, sd, dtype, idx=None):
    """One reference forward + backward in `dtype`; idx = the graph to replay (None: the reference builds and reports its own)."""
    c = um.CASES[tag]
    m = R.upsample_edgeConv(c["Fin"], c["Fout"], c["k"], -1)
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
        out = m(xr)
        (out * g.to(dtype)).sum().backward()
    finally:
        R.get_edge_features = orig
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
    k = um.CASES[tag]["k"]
    for seed in range(20000):
        x, g, sd = um.case_tensors(tag, seed)
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
    for q in r32:
        out["%s|%s|full" % (tag, q)] = r32[q].numpy()
        out["%s|%s|d64|full" % (tag, q)] = (r64[q].double() - r32[q].double()).numpy().astype(np.float32)
        if r32[q].dtype.is_floating_point:
            out["%s|noise|%s" % (tag, q)] = np.float64(rel(r32[q], r64[q]))
    print("%s: seed %d, near-tie rows %d, noise out %.2e dx %.2e dV %.2e dW1 %.2e" % (
        tag, seed, int(near.sum()), out[tag + "|noise|out"], out[tag + "|noise|dx"], out[tag + "|noise|grad|conv2.conv.weight"],
        out[tag + "|noise|grad|inte_conv_hk.0.weight"]))
    return out


def capture_xyz():
    c = um.XYZ_CASE
    for seed in range(20000):
        x, pc, gf, gx = um.xyz_tensors(seed)
        near = near_tie_rows(x, c["k"])
        if near.float().mean().item() <= MAX_NEAR_TIE:
            break
    else:
        raise SystemExit("no seed of the get_edge_features_xyz case meets the condition")
    _, idx = R.get_edge_features(x, c["k"], return_idx=True)
    xr, pr = x.clone().requires_grad_(True), pc.clone().requires_grad_(True)
    e_fea, e_xyz = R.get_edge_features_xyz(xr, pr, c["k"])
    ((e_fea * gf).sum() + (e_xyz * gx).sum()).backward()
    assert torch.equal(e_fea.detach(), R.get_edge_features(x, c["k"], idx=idx))          # the same graph as get_edge_features reports
    print("xyzfn: seed %d, near-tie rows %d" % (seed, int(near.sum())))
    t = "xyzfn|"
    return {t + "x": x.numpy(), t + "pc": pc.numpy(), t + "gf": gf.numpy(), t + "gx": gx.numpy(), t + "idx": idx.numpy().astype(np.int64),
            t + "seed": np.int64(seed), t + "near_tie_rows": near.numpy(), t + "e_fea|full": e_fea.detach().numpy(),
            t + "e_xyz|full": e_xyz.detach().numpy(), t + "dx|full": xr.grad.numpy(), t + "dpc|full": pr.grad.numpy()}


if __name__ == "__main__":
    OUT = {}
    for tag in um.CASES:
        OUT.update(capture(tag))
    OUT.update(capture_xyz())
    path = os.path.join(HERE, "upsample.npz")
    np.savez_compressed(path, **OUT)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))
