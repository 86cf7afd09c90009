#!/usr/bin/env python
"""Generate tests/golden/point_attn.npz by running the REAL reference classes on the CPU -- `Attention` of Generation/modules.py:534-558
and `Self_Attn` of Common/utilities.py:210-245 -- each case of tests/point_attn_model.py::CASES in float32 and in float64.  Nothing of the
reference is copied: its files are read at capture time and the lines of the one class are executed in a namespace that supplies torch,
nn, F and P = nn.Parameter.

Per case `tag`: `tag|x`, `tag|g` (the cotangent; both [B,ch,N]); `tag|param|<state_dict key>`; the float64 run's results as
`tag|<q>|full` for q in out, dx, grad|<parameter> -- results of more than 2048 elements as `|stride`, `|samples` (every stride-th value;
stride 16, or 64 beyond 32768 elements) and `|l2`; `tag|noise` = the rel-L2 distance of the float32 run from the float64 run (absolute norm
where the float64 quantity is all zero), one per quantity in the order of point_attn_model.quantities(tag); `tag|qbias_f32` (Self_Attn) =
|query.bias.grad| of the float32 run: query.bias adds the same number to every score of a softmax column and cancels, so its gradient
is rounding noise around an exact zero in either run and its entry of `tag|noise` means nothing.  Any float32 array of more
than 1024 bfloat16-exact values is stored as `...16|...`, the upper 16 bits of its values (`tag|x16`, `tag|g16`, `tag|param16|<key>`).
`state_keys|Attention`, `state_keys|Self_Attn` = the reference's state_dict keys in its own order.

Conditions asserted before anything is written: gamma is non-zero in every case; case b's theta and phi gradients are exact zeros; case
d's scores span at least +-30 in every row, every row's maximum sits at j = N - 1 and the prefix maximum rises across every 32-key
boundary; case g's attention is uniform and its phi gradient an exact zero.

    python tests/golden/make_golden_point_attn.py          (SPGAN_REFERENCE = the reference checkout)
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

import point_attn_model as pm         # noqa: E402

REF = os.environ.get("SPGAN_REFERENCE", os.path.join(HERE, "..", "..", "..", "reference"))      # default: a checkout beside the repository


def load_class(rel_path, name, pick):
    """The `pick`-th class of that name in the file (Generation/modules.py has a Self_Attn of its own before Attention)."""
    lines = open(os.path.join(REF, *rel_path)).read().split("\n")
    starts = [i for i, ln in enumerate(lines) if ln.startswith("class %s(" % name)]
    start = starts[pick]
    end = next((i for i in range(start + 1, len(lines)) if lines[i] and not lines[i][0].isspace()), len(lines))
    ns = {"torch": torch, "nn": nn, "F": F, "P": nn.Parameter}
    exec(compile("\n".join(lines[start:end]), "reference:" + name, "exec"), ns)
    return ns[name]


def run(cls, tag, x, g, sd, dtype):
    m = cls(pm.CASES[tag]["ch"])
    keys = tuple(m.state_dict().keys())
    m.load_state_dict({k_: v.clone() for k_, v in sd.items()}, strict=True)
    m = m.to(dtype)
    xr = x.to(dtype).clone().requires_grad_(True)
    out = m(xr)
    assert tuple(out.shape) == tuple(x.shape), (tag, tuple(out.shape))
    (out * g.to(dtype)).sum().backward()
    res = {"out": out.detach(), "dx": xr.grad}
    for n, p in m.named_parameters():
        res["grad|" + n] = p.grad
    return res, keys


def conditions(tag, x, sd, r32, r64):
    assert float(sd["gamma"].abs().min()) > 0
    for q in pm.EXACT_ZERO.get(tag, ()):
        assert not bool(r64[q].any()) and not bool(r32[q].any()), (tag, q)
    S = pm.scores(tag, sd, x.double())
    if tag == "d":
        N = S.shape[2]
        assert bool((S.max(-1).values >= 30).all()) and bool((S.min(-1).values <= -30).all())
        assert bool((S.argmax(-1) == N - 1).all())
        for m in range(32, N, 32):
            assert bool((S[:, :, m:m + 32].max(-1).values > S[:, :, :m].max(-1).values).all()), m
    if tag == "g":
        assert float(S.abs().max()) == 0.0


def put(out, name, a):
    """a float32 array of more than 1024 bfloat16-exact values goes in as its upper halves"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32 and a.size > 1024:
        hi = (a.view(np.uint32) >> 16).astype(np.uint16)
        if np.array_equal((hi.astype(np.uint32) << 16).view(np.float32), a):
            head, _, tail = name.partition("|")
            first, _, rest = tail.partition("|")
            out["%s|%s16%s" % (head, first, "|" + rest if rest else "")] = hi
            return
    out[name] = a


def capture(classes, tag):
    c = pm.CASES[tag]
    x, g, sd = pm.case_tensors(tag)
    r32, keys = run(classes[c["module"]], tag, x, g, sd, torch.float32)
    r64, _ = run(classes[c["module"]], tag, x, g, sd, torch.float64)
    assert keys == pm.STATE_KEYS[c["module"]], keys
    assert tuple(r64) == pm.quantities(tag), tuple(r64)
    conditions(tag, x, sd, r32, r64)
    out = {}
    put(out, "%s|x" % tag, x.numpy())
    put(out, "%s|g" % tag, g.numpy())
    for n, v in sd.items():
        put(out, "%s|param|%s" % (tag, n), v.numpy())
    noise = {}
    for q, v in r64.items():
        flat = v.numpy().reshape(-1)
        if flat.size > pm.SAMPLE_MIN:
            stride = pm.BIG_STRIDE if flat.size > pm.BIG else pm.SAMPLE_STRIDE
            out["%s|%s|stride" % (tag, q)] = np.int64(stride)
            out["%s|%s|samples" % (tag, q)] = flat[::stride].copy()
            out["%s|%s|l2" % (tag, q)] = np.float64(np.linalg.norm(flat))
        else:
            out["%s|%s|full" % (tag, q)] = v.numpy()
        noise[q] = np.float64(pm.rel(r32[q], v))
    out["%s|noise" % tag] = np.array(list(noise.values()), dtype=np.float64)
    if c["module"] == "Self_Attn":
        out["%s|qbias_f32" % tag] = np.float64(r32["grad|query.bias"].abs().max())
        assert float(r64["grad|query.bias"].abs().max()) < 1e-12
        noise.pop("grad|query.bias")
    print("%s: noise %s" % (tag, {q: "%.2e" % v for q, v in noise.items()}))
    need = {q: "%.2e" % v for q, v in noise.items() if 5 * v > (3e-6 if q in ("out", "dx") else 5e-6)}
    print("%s: quantities that need the 5 x noise fallback: %s" % (tag, need or "none"))
    return out, keys


if __name__ == "__main__":
    classes = {"Attention": load_class(("Generation", "modules.py"), "Attention", 0),
               "Self_Attn": load_class(("Common", "utilities.py"), "Self_Attn", 0)}
    OUT = {}
    for tag in pm.CASES:
        o, keys = capture(classes, tag)
        OUT["state_keys|" + pm.CASES[tag]["module"]] = np.array(keys)
        OUT.update(o)
    path = os.path.join(HERE, "point_attn.npz")
    np.savez_compressed(path, **OUT)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))
