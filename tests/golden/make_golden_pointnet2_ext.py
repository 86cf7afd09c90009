#!/usr/bin/env python
"""Generate tests/golden/pointnet2_ext.npz by running the REAL reference `PointnetSAModuleMSG`, `PointnetSAModule` and `PointnetFPModule`
(metrics/pointnet2/pointnet2_modules.py over its pointnet2_utils.py and pytorch_utils.py) on the CPU, each case in float32 and again in
float64.  Nothing of the reference is copied: its three files are imported at capture time as the package `pointnet2`, whose path is the
reference's directory.  What they need and a CPU machine lacks is supplied here:
  * `pointnet2.pointnet2_cuda`, the native extension: tests/pointnet2_ext_model.py::cuda_stand_in, written from the kernels' semantics;
  * `torch.cuda.IntTensor` / `torch.cuda.FloatTensor`: CPU constructors (of the run's float dtype) for the duration;
  * `Common.utilities` (imported for names the three files never use): an empty stand-in, as make_golden_utilities_rest.py stubs Common.

Per case `tag` (tests/pointnet2_ext_model.py::CASES): `tag|in|<name>`, `tag|gout<i>`, `tag|param|<state_dict key>` in the reference's key
order (`tag|keys`: that order as one string), `tag|seed`, `tag|margin|<which>`; results `tag|<q>|full` (float32 run) and `tag|<q>|f64|full`
(float64 run) for q in out<i>, gin|<input>, grad|<parameter>, buf|<buffer>.

Conditions asserted before anything is written (a seed that fails them is skipped, the conditions stay; found in float64 by the model, which
must first agree with the reference's float64 run to 1e-9): no normalised pre-activation within 1e-4 of the ReLU kink, no pooled
maximum's runner-up (at a slot holding another point) within 1e-4 of it, no point within 1e-6 in d2 of a ball's surface, no farthest-point
pick or third-nearest choice within 1e-6 of its runner-up.  The routing is then the same in both precisions and in every implementation.

    python tests/golden/make_golden_pointnet2_ext.py          (SPGAN_REFERENCE = the reference checkout, default /root/reference)
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

import pointnet2_ext_model as pm          # noqa: E402

FLOAT = [torch.float32]


def load_reference():
    common = types.ModuleType("Common")
    common.__path__ = []
    util = types.ModuleType("Common.utilities")
    for name in ("Self_Attn", "DenseModule2D", "Dense_Attn_2D"):
        setattr(util, name, type(name, (), {}))
    common.utilities = util
    sys.modules["Common"], sys.modules["Common.utilities"] = common, util
    pkg = types.ModuleType("pointnet2")
    pkg.__path__ = [os.path.join(REF, "metrics", "pointnet2")]
    sys.modules["pointnet2"] = pkg
    sys.modules["pointnet2.pointnet2_cuda"] = pkg.pointnet2_cuda = pm.cuda_stand_in()
    torch.cuda.IntTensor = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    torch.cuda.FloatTensor = lambda *shape: torch.zeros(*shape, dtype=FLOAT[0])
    import pointnet2.pointnet2_modules as modules
    return modules


R = load_reference()


def run_reference(cfg, sd, inputs, gouts, dtype):
    FLOAT[0] = dtype
    m = pm.build(R, cfg)
    assert list(m.state_dict().keys()) == list(sd.keys()), (list(m.state_dict().keys()), list(sd.keys()))
    m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    m = m.to(dtype)
    m.train(cfg["training"])
    names, tensors = inputs
    args = [None if t is None else t.to(dtype).clone().requires_grad_(n in pm.GRAD_INPUTS) for n, t in zip(names, tensors)]
    outs = m(*args)
    outs = [o for o in (outs if isinstance(outs, tuple) else (outs,)) if o is not None]
    sum((o * g.to(dtype)).sum() for o, g in zip(outs, gouts)).backward()
    res = {"out%d" % i: o.detach() for i, o in enumerate(outs)}
    for n, a in zip(names, args):
        if a is not None and a.requires_grad:
            res["gin|" + n] = a.grad if a.grad is not None else torch.zeros_like(a)
    for n, p in m.named_parameters():
        res["grad|" + n] = p.grad if p.grad is not None else torch.zeros_like(p)
    for n, b in m.named_buffers():
        res["buf|" + n] = b.detach()
    return res


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def capture(tag):
    cfg = pm.CASES[tag]
    keys_shapes = [(k, tuple(v.shape)) for k, v in pm.build(R, cfg).state_dict().items()]
    seed, inputs, sd, gouts, margins = pm.find_seed(cfg, pm.MARGINS, keys_shapes)
    assert all(margins[k] > pm.MARGINS[k] for k in pm.MARGINS), margins
    r32 = run_reference(cfg, sd, inputs, gouts, torch.float32)
    r64 = run_reference(cfg, sd, inputs, gouts, torch.float64)
    model = pm.run_model(cfg, sd, inputs, torch.float64, gouts)
    assert sorted(model) == sorted(r64), (sorted(model), sorted(r64))
    for q in r64:
        if r64[q].dtype.is_floating_point:
            assert rel(model[q], r64[q]) < 1e-9 or float((model[q].double() - r64[q].double()).abs().max()) < 1e-12, (tag, q, rel(model[q], r64[q]))
        else:
            assert torch.equal(model[q], r64[q]), (tag, q)
    out = {"%s|seed" % tag: np.int64(seed), "%s|keys" % tag: np.array("\n".join(sd.keys()))}
    for k, v in margins.items():
        out["%s|margin|%s" % (tag, k)] = np.float64(v)
    for n, t in zip(*inputs):
        if t is not None:
            out["%s|in|%s" % (tag, n)] = t.numpy()
    for i, g in enumerate(gouts):
        out["%s|gout%d" % (tag, i)] = g.numpy()
    for k, v in sd.items():
        out["%s|param|%s" % (tag, k)] = v.numpy()
    worst = 0.0
    for q in r32:
        out["%s|%s|full" % (tag, q)] = r32[q].numpy()
        out["%s|%s|f64|full" % (tag, q)] = r64[q].numpy()
        if r32[q].dtype.is_floating_point:
            worst = max(worst, rel(r32[q], r64[q]))
    print("%s: seed %d, margins %s, worst float32 noise %.2e" % (tag, seed, {k: "%.1e" % v for k, v in margins.items()}, worst))
    return out


if __name__ == "__main__":
    OUT = {}
    for tag in pm.CASES:
        OUT.update(capture(tag))
    path = os.path.join(HERE, "pointnet2_ext.npz")
    np.savez_compressed(path, **OUT)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))
