#!/usr/bin/env python
"""Generate tests/golden/bilateral.npz by running the REAL reference `bilateral_upsample_edgeConv` (Generation/modules.py:847-925, with
get_edge_features_xyz :727-776) on the CPU, each case in float32 and again in float64 on the float32 run's kNN graph, so that the two
differ by rounding alone.  Nothing of the reference is copied: its file is read at capture time exactly as make_golden_deform.py does
(same loader).  Inputs and weights come from spgan.fixture_rng (tests/bilateral_model.py).  The protocol and the storage form are
make_golden_deform_xyz.py's.

The reference's get_edge_features_xyz takes no graph.  The float32 run calls it as it is; the float64 run replaces it by two calls of the
reference's own get_edge_features(., k, idx=<the float32 graph>), one for x and one for pc -- the same gather and concatenation -- and the
float32 run is repeated through that replacement and must reproduce the unpatched run bit for bit before anything is stored.

Per case `tag` (tests/bilateral_model.py::CASES): `tag|x`, `tag|pc`, `tag|g` (the cotangent), `tag|idx` (int64 [B,N*k], the reference's
graph), `tag|param|<state_dict key>` (a conv weight of more than 1024 elements as `tag|param16|<key>`, the upper 16 bits of its bfloat16-exact
float32 values: bilateral_model.param reads both); results as `tag|<q>|full` (float32 run) and `tag|<q>|d64|full` (float64 run minus float32 run, stored
in float32, with 10 mantissa bits for more than 1024 elements) for q in out, dx, dpc, grad|<parameter>, buf|<buffer> -- results of more than
8192 elements as `|stride`, `|samples`, `|l2` and `|d64|samples`, the summarised form of helpers.check --; `tag|noise` = the rel-L2
distances of the two runs, one per floating-point quantity in the order of `noise_keys` (bilateral_model.noise looks one up: two hundred
one-number entries would cost more than the numbers); `tag|near_tie_rows`; `state_keys` = the reference's state_dict keys in its own order.

Condition asserted before anything is written (a seed that fails it is skipped, the condition stays): at most 1 % of the rows of a
graph have a float32 distance gap below 1e-4 between consecutive ranks 0..k+1.

    python tests/golden/make_golden_bilateral.py          (SPGAN_REFERENCE = the reference checkout)
"""
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "sp-gan_amd"))

import bilateral_model as xm            # noqa: E402
import make_golden_deform as mg         # noqa: E402  (the reference loader, near_tie_rows, rel; its __main__ part does not run)

R = mg.R


def run(tag, x, pc, g, sd, dtype, idx=None):
    """One reference forward + backward in `dtype`; idx = the graph to replay (None: the reference's own get_edge_features_xyz runs)."""
    c = xm.CASES[tag]
    m = R.bilateral_upsample_edgeConv(c["Fin"], c["Fout"], c["k"], -1, softmax=c["softmax"])
    keys = tuple(m.state_dict().keys())
    m.load_state_dict({k_: v.clone() for k_, v in sd.items()}, strict=True)
    m = m.to(dtype)
    m.train(c["train"])
    orig = R.get_edge_features_xyz

    def replay(xx, pp, k, num=-1):
        return R.get_edge_features(xx, k, idx=idx), R.get_edge_features(pp, k, idx=idx)
    if idx is not None:
        R.get_edge_features_xyz = replay
    try:
        xr, pr = x.to(dtype).clone().requires_grad_(True), pc.to(dtype).clone().requires_grad_(True)
        out = m(xr, pr)
        (out * g.to(dtype)).sum().backward()
    finally:
        R.get_edge_features_xyz = orig
    assert tuple(out.shape) == (c["B"], c["Fout"], 2 * c["N"]) and len(keys) == 42, (tag, tuple(out.shape), len(keys))
    res = {"out": out.detach(), "dx": xr.grad, "dpc": pr.grad}
    for n, p in m.named_parameters():
        res["grad|" + n] = p.grad
    for n, b in m.named_buffers():
        res["buf|" + n] = b.detach()
    return res, keys


def capture(tag):
    k = xm.CASES[tag]["k"]
    for seed in range(20000):
        x, pc, g, sd = xm.case_tensors(tag, seed)
        near = mg.near_tie_rows(x, k)
        if near.float().mean().item() <= mg.MAX_NEAR_TIE:
            break
    else:
        raise SystemExit("no seed of case %s meets the condition" % tag)
    _, idx = R.get_edge_features(x, k, return_idx=True)         # the graph get_edge_features_xyz builds: the same float32 operations
    r32, keys = run(tag, x, pc, g, sd, torch.float32)
    again, _ = run(tag, x, pc, g, sd, torch.float32, idx=idx)
    for q in r32:                                                # the replay is the reference's own gather on the reference's own graph
        assert torch.equal(r32[q], again[q]), (tag, q)
    assert near.float().mean().item() <= mg.MAX_NEAR_TIE
    r64, _ = run(tag, x, pc, g, sd, torch.float64, idx=idx)
    out = {"%s|x" % tag: x.numpy(), "%s|pc" % tag: pc.numpy(), "%s|g" % tag: g.numpy(), "%s|idx" % tag: idx.numpy().astype(np.int64),
           "%s|seed" % tag: np.int64(seed), "%s|near_tie_rows" % tag: near.numpy()}
    for n, v in sd.items():
        a = v.numpy()
        if a.dtype == np.float32 and a.size > 1024:     # the conv weights are bfloat16-exact: their upper halves are the whole value
            hi = (a.view(np.uint32) >> 16).astype(np.uint16)
            assert np.array_equal((hi.astype(np.uint32) << 16).view(np.float32), a), n
            out["%s|param16|%s" % (tag, n)] = hi
        else:
            out["%s|param|%s" % (tag, n)] = a
    noise = {}
    for q in r32:
        d64 = (r64[q].double() - r32[q].double()).numpy().astype(np.float32)
        if d64.size > 1024:                        # 10 mantissa bits of a large tensor's distance: 1e-10 of the value; vectors stay exact
            d64 = (d64.view(np.int32) & np.int32(-8192)).view(np.float32)
        if r32[q].numel() > xm.SAMPLE_MIN:                                         # helpers.check's summarised form
            st = xm.SAMPLE_STRIDE
            out["%s|%s|stride" % (tag, q)] = np.int64(st)
            out["%s|%s|samples" % (tag, q)] = r32[q].numpy().reshape(-1)[::st].copy()
            out["%s|%s|l2" % (tag, q)] = np.float64(r32[q].double().norm())
            out["%s|%s|d64|samples" % (tag, q)] = d64.reshape(-1)[::st].copy()
        else:
            out["%s|%s|full" % (tag, q)] = r32[q].numpy()
            out["%s|%s|d64|full" % (tag, q)] = d64
        if r32[q].dtype.is_floating_point:
            noise[q] = np.float64(mg.rel(r32[q], r64[q]))
    out["%s|noise" % tag] = np.array(list(noise.values()), dtype=np.float64)
    print("%s: seed %d, near-tie rows %d, noise %s" % (tag, seed, int(near.sum()), {q: "%.2e" % v for q, v in noise.items()}))
    # the quantities whose 5 x noise exceeds the GPU test's base bound (3e-6 out / dx / dpc, 5e-6 parameter gradients): they take the fallback
    zero = xm.ZERO_GRAD_BIASES if xm.CASES[tag]["train"] else ()
    need = {q: "%.2e" % v for q, v in noise.items() if not q.startswith("buf|") and q[5:] not in zero
            and 5 * v > (3e-6 if q in ("out", "dx", "dpc") else 5e-6)}
    print("%s: quantities that need the 5 x noise fallback: %s" % (tag, need or "none"))
    return out, keys, tuple(noise)


if __name__ == "__main__":
    OUT = {}
    for tag in xm.CASES:
        o, keys, nkeys = capture(tag)
        assert OUT.setdefault("noise_keys", np.array(nkeys)).tolist() == list(nkeys)
        OUT.update(o)
    OUT["state_keys"] = np.array(keys)
    path = os.path.join(HERE, "bilateral.npz")
    # np.savez_compressed's container at the highest deflate level: the 700 small entries and the 16-bit halves leave little room under 1 MiB
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, a in OUT.items():
            with z.open(name + ".npy", "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)
    assert os.path.getsize(path) < 2 ** 20, os.path.getsize(path)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))
