#!/usr/bin/env python
"""Generate tests/golden/utilities_rest.npz by running the REAL reference `GC_attn`, `Self_Attn2`, `DenseModule2D`, `MultiDenseMLP` and
`Dense_Attn_2D` (Common/utilities.py:45-65, 92-121, 247-290, 323-426) on the CPU, each case in float32 and again in float64.  Nothing of the reference is copied: its two files are read at capture time and executed as the modules
`Common.ops` / `Common.utilities`, the way tests/golden/make_golden_dense_edge.py loads them.  Inputs and weights come from
spgan.fixture_rng (tests/gc_attn_model.py::case_tensors).

Per case `tag` (tests/gc_attn_model.py::CASES): `tag|x`, `tag|g` (the cotangent), `tag|param|<state_dict key>` in the reference's key
order; results as `tag|<q>|full` (float32 run) and `tag|<q>|d64|full` (float64 run minus float32 run, stored in float32:
gc_attn_model.golden_f64 adds them up) for q in out, dx (dx1 ..: MultiDenseMLP's side inputs, stored as `tag|x1` ..), grad|<parameter>, buf|<buffer>; `tag|noise|<q>` = the rel-L2 distance of the two runs;
`tag|seed`, `tag|kink_margin`; `tag|init|<state_dict key>` (the cases of
gc_attn_model.INIT_TAGS) = the reference module's initial values under torch.manual_seed(gc_attn_model.INIT_SEED).

The condition asserted before anything is written (a seed that fails it is skipped, the condition stays): in float64 no pre-activation in
front of a ReLU or LeakyReLU lies within 1e-5 x its column's largest (a GC branch: its tensor's, all B*O values) of zero, so that the reference's float32 and
float64 runs sit on the same side of every kink and their distance is rounding alone.

    python tests/golden/make_golden_utilities_rest.py          (SPGAN_REFERENCE = the reference checkout, default /root/reference)
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

import gc_attn_model as gm          # noqa: E402

KINK_REL, SEEDS = 1e-5, 200


def load_reference():
    pkg = types.ModuleType("Common")
    pkg.__path__ = []
    path = os.path.join(REF, "Common", "ops.py")
    src = open(path, encoding="utf-8").read()
    src = src[:src.index("if __name__ == '__main__':")]
    ops = types.ModuleType("Common.ops")
    exec(compile(src, path, "exec"), ops.__dict__)
    pkg.ops = ops
    sys.modules["Common"], sys.modules["Common.ops"] = pkg, ops
    path = os.path.join(REF, "Common", "utilities.py")
    util = types.ModuleType("Common.utilities")
    exec(compile(open(path, encoding="utf-8").read(), path, "exec"), util.__dict__)
    return util


R = load_reference()


def run(tag, x, g, sd, dtype):
    """One reference forward + backward in `dtype`"""
    m = gm.build_module(R, tag)
    assert list(m.state_dict().keys()) == list(sd.keys()), (list(m.state_dict().keys()), list(sd.keys()))
    m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    m = m.to(dtype)
    m.train(gm.CASES[tag]["train"])
    many = isinstance(x, (list, tuple))
    xs = [t.to(dtype).clone().requires_grad_(True) for t in (x if many else [x])]
    out = m(xs if many else xs[0])
    (out * g.to(dtype)).sum().backward()
    res = {"out": out.detach()}
    for n, t in zip(gm.input_names(tag), xs):
        res["d" + n] = t.grad
    for n, p in m.named_parameters():
        res["grad|" + n] = p.grad
    for n, b in m.named_buffers():
        res["buf|" + n] = b.detach()
    return res


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def capture(tag):
    for seed in range(SEEDS):
        x, g, sd = gm.case_tensors(tag, seed)
        margin = gm.kink_margin(gm.run(tag, x, g, sd)["pre"])
        if margin > KINK_REL:
            break
    else:
        raise SystemExit("no seed of case %s meets the condition" % tag)
    assert margin > KINK_REL
    r32, r64 = run(tag, x, g, sd, torch.float32), run(tag, x, g, sd, torch.float64)
    out = {"%s|g" % tag: g.numpy(), "%s|seed" % tag: np.int64(seed), "%s|kink_margin" % tag: np.float64(margin)}
    for n, t in zip(gm.input_names(tag), x if isinstance(x, (list, tuple)) else [x]):
        out["%s|%s" % (tag, n)] = t.numpy()
    for n, v in sd.items():
        out["%s|param|%s" % (tag, n)] = v.numpy()
    if tag in gm.INIT_TAGS:
        torch.manual_seed(gm.INIT_SEED)
        for n, v in gm.build_module(R, tag).state_dict().items():
            out["%s|init|%s" % (tag, n)] = v.numpy()
    for q in r32:
        out["%s|%s|full" % (tag, q)] = r32[q].numpy()
        # the float64 run as its distance from the float32 run, itself in float32: r64 = r32 + d64 to 1e-14 relative, at half the bytes
        out["%s|%s|d64|full" % (tag, q)] = (r64[q].double() - r32[q].double()).numpy().astype(np.float32)
        if r32[q].dtype.is_floating_point:
            out["%s|noise|%s" % (tag, q)] = np.float64(rel(r32[q], r64[q]))
    noise = {q: float(out["%s|noise|%s" % (tag, q)]) for q in r32 if gm.zero_gradient(tag, q) is None and not q.startswith("buf|")}
    worst = max(noise, key=lambda q: noise[q])
    print("%s: seed %d, kink margin %.2e, noise out %.2e dx %.2e worst %.2e (%s)" % (tag, seed, margin, noise["out"], noise["dx"], noise[worst], worst))
    return out


if __name__ == "__main__":
    OUT = {}
    for tag in gm.CASES:
        OUT.update(capture(tag))
    path = os.path.join(HERE, "utilities_rest.npz")
    np.savez_compressed(path, **OUT)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))
