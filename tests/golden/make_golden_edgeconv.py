#!/usr/bin/env python
"""Generate tests/golden/edgeconv.npz by running the REAL reference `edgeConv` (Generation/modules.py:779-796, with conv2dbr :612-626
and get_edge_features :683-725) on the CPU, each case in float32 and again in float64 on the float32 run's kNN graph, so that the
two differ by rounding alone.  Nothing of the reference is copied: its file is read at capture time, the two import lines that do
not resolve without its CUDA extensions (`metrics.pointops`, `einops`; neither is used by the classes captured here) are dropped in
memory, and the module is executed up to the end of `edgeConv` (the file's tail runs a demo at import time).  Inputs and weights come from spgan.fixture_rng (tests/edgeconv_model.py::case_tensors).

Per case `tag` (tests/edgeconv_model.py::CASES): `tag|x`, `tag|g` (the cotangent), `tag|idx` (int64 [B,N*k], the reference's graph),
`tag|param|<state_dict key>`; results as `tag|<q>|full` (float32 run) and `tag|<q>|d64|full` (float64 run minus float32 run, stored in float32:
edgeconv_model.golden_f64 adds them up) for q in out, dx,
grad|<parameter>, buf|<buffer>; `tag|noise|<q>` = the rel-L2 distance of the two runs; `tag|gap` and `tag|near_tie_rows`.

Conditions asserted before anything is written (a seed that fails one is skipped, the conditions stay):
  * no case hinges on a tie in the max: over every (point, channel) the float64 gap between the best and the second-best pre-norm
    value y over j (best = largest for a positive bn.weight, smallest for a negative one) exceeds 1e-4 x max|y|;
  * at most 1 % of the rows of a graph have a float32 distance gap below 1e-4 between consecutive ranks 0..k+1 (those rows are the
    ones a differently rounded kNN may order differently; the GPU test excludes exactly them).

    python tests/golden/make_golden_edgeconv.py          (SPGAN_REFERENCE = the reference checkout, default /root/reference)
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

import edgeconv_model as ecm          # noqa: E402

GAP_REL, DIST_GAP, MAX_NEAR_TIE = 1e-4, 1e-4, 0.01


def load_reference():
    path = os.path.join(REF, "Generation", "modules.py")
    drop = ("from metrics.pointops import", "from einops import")
    lines = [ln for ln in open(path, encoding="utf-8").read().split("\n") if not ln.startswith(drop)]
    lines = lines[:next(i for i, ln in enumerate(lines) if ln.startswith("class upsample_edgeConv("))]      # everything up to and including edgeConv
    mod = types.ModuleType("reference_modules")
    exec(compile("\n".join(lines), path, "exec"), mod.__dict__)
    return mod


R = load_reference()


def run(tag, x, g, sd, dtype, idx=None):
    """One reference forward + backward in `dtype`; idx = the graph to replay (None: the reference builds and reports its own)."""
    c = ecm.CASES[tag]
    m = R.edgeConv(c["Fin"], c["Fout"], c["k"])
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


def checks(tag, x, sd, idx):
    c = ecm.CASES[tag]
    k = c["k"]
    d = lambda t: t.double()                                                   # noqa: E731
    f = ecm.forward(d(x), idx, k, d(sd["conv.conv.weight"]), d(sd["conv.conv.bias"]), d(sd["conv.bn.weight"]), d(sd["conv.bn.bias"]),
                    d(sd["conv.bn.running_mean"]), d(sd["conv.bn.running_var"]), c["train"])
    y = f["Q"].unsqueeze(2) + f["Pn"]                                          # [B,N,k,F]
    ys = torch.sort(y, dim=2)[0]
    up = (f["a"] >= 0).view(1, 1, -1)
    gap = torch.where(up, ys[:, :, -1] - ys[:, :, -2], ys[:, :, 1] - ys[:, :, 0]).min().item() / y.abs().max().item()
    # the reference's own float32 distances (modules.py:695-699), ranks 0..k+1
    xt = x.permute(0, 2, 1)
    dist = -2 * torch.bmm(xt, x) + torch.sum(xt ** 2, dim=2, keepdim=True) + torch.sum(xt ** 2, dim=2, keepdim=True).permute(0, 2, 1)
    ds = torch.sort(dist, dim=2)[0][:, :, :k + 2]
    near = ((ds[:, :, 1:] - ds[:, :, :-1]).min(dim=2)[0] < DIST_GAP).reshape(-1)
    return gap, near


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def capture(tag):
    k = ecm.CASES[tag]["k"]
    for seed in range(20000):                       # the cheap conditions first; the reference runs once, on the seed that meets them
        x, g, sd = ecm.case_tensors(tag, seed)
        _, idx = R.get_edge_features(x, k, return_idx=True)
        gap, near = checks(tag, x, sd, idx)
        if gap > GAP_REL and near.float().mean().item() <= MAX_NEAR_TIE:
            break
    else:
        raise SystemExit("no seed of case %s meets the conditions" % tag)
    r32, idx32 = run(tag, x, g, sd, torch.float32)
    assert torch.equal(idx, idx32)
    assert gap > GAP_REL and near.float().mean().item() <= MAX_NEAR_TIE
    r64, idx64 = run(tag, x, g, sd, torch.float64, idx=idx)
    assert torch.equal(idx, idx64)
    out = {"%s|x" % tag: x.numpy(), "%s|g" % tag: g.numpy(), "%s|idx" % tag: idx.numpy().astype(np.int64), "%s|seed" % tag: np.int64(seed),
           "%s|gap" % tag: np.float64(gap), "%s|near_tie_rows" % tag: near.numpy()}
    for n, v in sd.items():
        out["%s|param|%s" % (tag, n)] = v.numpy()
    for q in r32:
        out["%s|%s|full" % (tag, q)] = r32[q].numpy()
        # the float64 run as its distance from the float32 run, itself in float32: r64 = r32 + d64 to 1e-14 relative, at half the bytes
        out["%s|%s|d64|full" % (tag, q)] = (r64[q].double() - r32[q].double()).numpy().astype(np.float32)
        if r32[q].dtype.is_floating_point:
            out["%s|noise|%s" % (tag, q)] = np.float64(rel(r32[q], r64[q]))
    print("%s: seed %d, gap %.2e, near-tie rows %d, noise out %.2e dx %.2e dW %.2e" % (
        tag, seed, gap, int(near.sum()), out[tag + "|noise|out"], out[tag + "|noise|dx"], out[tag + "|noise|grad|conv.conv.weight"]))
    return out


if __name__ == "__main__":
    OUT = {}
    for tag in ecm.CASES:
        OUT.update(capture(tag))
    path = os.path.join(HERE, "edgeconv.npz")
    np.savez_compressed(path, **OUT)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))
