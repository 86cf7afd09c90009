#!/usr/bin/env python
"""Generate tests/golden/gan_layers.npz by running the REAL reference classes of Generation/modules.py:32-496 (SpectralNorm, StddevLayer,
MinibatchStdDev, PixelNorm, PixelwiseNorm, NoiseLayer, NoiseInjection, LayerEpilogue, AdaptiveInstanceNorm, WScaleLayer, Truncation) and
torch.nn.utils.spectral_norm (what the reference's snconv2d / snlinear apply) on the CPU in float64.  Nothing of the reference is copied:
its file is read at capture time, the two import lines that do not resolve without its CUDA extensions (`metrics.pointops`, `einops`;
neither is used by the classes captured here) are dropped in memory, and the module is executed up to `class Self_Attn(`.

Per case `tag`: inputs `tag|in|<name>`, parameters `tag|param|<state_dict key>`, the cotangent `tag|g`, results `tag|out`, `tag|dx`,
`tag|grad|<name>`; the spectral-norm cases also `tag|w1`, `tag|u1`, `tag|v1` (normalised weight, u, v after ONE forward), `tag|u3`, `tag|v3`,
`tag|w3` (after three consecutive forwards), `tag|weval` (hook form: an eval-mode forward after the three) and `tag|dW` (the gradient of
sum(w1 * g) taken at the first forward).  `keys|<class>`: the state_dict key lists.  Activation inputs are kept away from 0
(inputs moved so that |x + w * noise| >= 0.05).

    python tests/golden/make_golden_gan_layers.py          (SPGAN_REFERENCE = the reference checkout, default /root/reference)
"""
import os
import types
import warnings

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SPGAN_REFERENCE", "/root/reference")
torch.set_num_threads(8)
torch.set_default_dtype(torch.float64)


def load_reference():
    path = os.path.join(REF, "Generation", "modules.py")
    drop = ("from metrics.pointops import", "from einops import")
    lines = [ln for ln in open(path, encoding="utf-8").read().split("\n") if not ln.startswith(drop)]
    lines = lines[:next(i for i, ln in enumerate(lines) if ln.startswith("class Self_Attn("))]
    mod = types.ModuleType("reference_modules")
    exec(compile("\n".join(lines), path, "exec"), mod.__dict__)
    return mod


R = load_reference()
RNG = np.random.RandomState(20240607)
OUT = {}


def rnd(*shape, scale=1.0):
    return torch.from_numpy(RNG.standard_normal(shape) * scale)


def put(tag, **kv):
    for k, v in kv.items():
        OUT["%s|%s" % (tag, k)] = v.detach().clone().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def keys(name, module):
    sd = module.state_dict()
    OUT["keys|" + name] = np.array(list(sd.keys()))
    OUT["shapes|" + name] = np.array(["x".join(str(s) for s in v.shape) for v in sd.values()])


# ------------------------------------------------------------------------------------------------ spectral norm
def layer_for(shape):
    if len(shape) == 2:
        return nn.Linear(shape[1], shape[0]), rnd(2, shape[1])
    return nn.Conv2d(shape[1], shape[0], (shape[2], shape[3])), rnd(1, shape[1], shape[2], shape[3])


def sn_class_case(tag, shape, n):
    layer, x = layer_for(shape)
    layer.weight.data = rnd(*shape)
    m = R.SpectralNorm(layer, power_iterations=n)
    g = rnd(*shape)
    put(tag, **{"in|W": layer.weight_bar, "in|u": layer.weight_u, "in|v": layer.weight_v, "in|x": x, "g": g, "n": n})
    m(x)
    (layer.weight * g).sum().backward()
    put(tag, w1=layer.weight, u1=layer.weight_u, v1=layer.weight_v, dW=layer.weight_bar.grad)
    m(x); m(x)
    put(tag, w3=layer.weight, u3=layer.weight_u, v3=layer.weight_v)
    return m


def sn_hook_case(tag, shape, n):
    layer, x = layer_for(shape)
    layer.weight.data = rnd(*shape)
    m = torch.nn.utils.spectral_norm(layer, n_power_iterations=n)
    g = rnd(*shape)
    put(tag, **{"in|W": m.weight_orig, "in|u": m.weight_u.clone(), "in|v": m.weight_v.clone(), "in|x": x, "g": g, "n": n})
    m.train()
    m(x)
    (m.weight * g).sum().backward()
    put(tag, w1=m.weight, u1=m.weight_u.clone(), v1=m.weight_v.clone(), dW=m.weight_orig.grad)
    m(x); m(x)
    put(tag, w3=m.weight, u3=m.weight_u.clone(), v3=m.weight_v.clone())
    m.eval()
    m(x)
    put(tag, weval=m.weight, ueval=m.weight_u.clone())
    return m


for shape, n in (((5, 7), 1), ((5, 7), 3), ((1, 64), 1), ((8, 6, 1, 4), 1), ((64, 3), 3)):
    t = "x".join(str(s) for s in shape) + "_n%d" % n
    mc = sn_class_case("sn_class_" + t, shape, n)
    mh = sn_hook_case("sn_hook_" + t, shape, n)
keys("SpectralNorm", mc)
keys("spectral_norm", mh)
keys("snconv2d", R.snconv2d(6, 4, 1))
keys("snlinear", R.snlinear(7, 5))


# ------------------------------------------------------------------------------------------------ stddev layers
def fwd_bwd(tag, module, inputs, call=None):
    """forward + backward of sum(out * g); records inputs, out, input gradients and parameter gradients"""
    leaves = {k: v.clone().requires_grad_(True) for k, v in inputs.items()}
    out = (call or module)(*leaves.values())
    g = rnd(*out.shape)
    (out * g).sum().backward()
    put(tag, g=g, out=out)
    for k, v in leaves.items():
        put(tag, **{"in|" + k: v, "grad|" + k: v.grad if v.grad is not None else torch.zeros_like(v)})
    if isinstance(module, nn.Module):
        for k, p in module.named_parameters():
            put(tag, **{"param|" + k: p})
            if p.grad is not None:
                put(tag, **{"pgrad|" + k: p.grad})
        for k, b in module.named_buffers():
            put(tag, **{"param|" + k: b})
    return out


for (B, C, N, grp, Fn) in ((8, 5, 70, 4, 1), (3, 4, 1, 4, 1), (4, 1, 65, 2, 1)):
    fwd_bwd("mbstd_%d_%d_%d_%d" % (B, C, N, grp), R.MinibatchStdDev(grp), {"x": rnd(B, C, N)})
for (B, C, N, grp, Fn) in ((8, 5, 7, 4, 1), (8, 6, 16, 4, 2), (6, 6, 5, 3, 3)):
    fwd_bwd("stddev_%d_%d_%d_%d_%d" % (B, C, N, grp, Fn), R.StddevLayer(grp, Fn), {"x": rnd(B, C, N)})


# ------------------------------------------------------------------------------------------------ epilogue family
def away_from_zero(x, w=None, noise=None):
    """x moved by 0.05 away from the activation's kink: |x + w * noise| >= 0.05 afterwards"""
    off = 0 if w is None else w.reshape(1, -1, *([1] * (x.dim() - 2))) * noise
    x = x + 0.05 * torch.sign(x + off)
    assert (x + off).abs().min().item() >= 1e-3
    return x


fwd_bwd("pixelnorm", R.PixelNorm(), {"x": rnd(3, 5, 70)})
fwd_bwd("pixelwisenorm", R.PixelwiseNorm(), {"x": rnd(2, 6, 4, 5)})
m = R.NoiseLayer(5); m.weight.data = rnd(1, 5, 1)
fwd_bwd("noiselayer", m, {"x": rnd(3, 5, 70), "noise": rnd(3, 1, 70)})
keys("NoiseLayer", m)
m = R.NoiseInjection(6); m.weight.data = rnd(1, 6, 1, 1)
fwd_bwd("noiseinjection", m, {"image": rnd(2, 6, 4, 5), "noise": rnd(2, 1, 4, 5)})
keys("NoiseInjection", m)

for tag, actl in (("lrelu", nn.LeakyReLU(0.2)), ("relu", nn.ReLU())):
    m = R.LayerEpilogue(5, 0, False, True, True, True, False, actl)
    m.top_epi.noise.weight.data = rnd(1, 5, 1)
    x, nz = rnd(3, 5, 70), rnd(3, 1, 70)
    x = away_from_zero(x, m.top_epi.noise.weight.data, nz)
    m.top_epi.noise.noise = nz

    def call(x_, m=m):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # InstanceNorm2d(5) on what it reads as a 3-channel image
            return m(x_)
    fwd_bwd("epilogue_" + tag, m, {"x": x}, call=call)
    put("epilogue_" + tag, **{"in|noise": nz})
    keys("LayerEpilogue", m)
# the noise gradient of the full layer, through NoiseLayer's explicit argument
m = R.LayerEpilogue(5, 0, False, True, True, True, False, nn.LeakyReLU(0.2))
m.top_epi.noise.weight.data = rnd(1, 5, 1)
x, nz = rnd(3, 5, 70), rnd(3, 1, 70)
x = away_from_zero(x, m.top_epi.noise.weight.data, nz)


def call_noise(x_, n_, m=m):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t = m.top_epi.noise(x_, n_)
        for name, layer in m.top_epi.named_children():
            if name != "noise":
                t = layer(t)
        return t


fwd_bwd("epilogue_noisegrad", m, {"x": x, "noise": nz}, call=call_noise)
m = R.LayerEpilogue(6, 0, False, False, True, True, False, nn.LeakyReLU(0.2))
x = away_from_zero(rnd(2, 6, 4, 5))
fwd_bwd("epilogue_4d", m, {"x": x})
m = R.AdaptiveInstanceNorm(6, 8)
m.style.linear.weight_orig.data = rnd(12, 8)
m.style.linear.bias.data += rnd(12, scale=0.1)
fwd_bwd("adain", m, {"input": rnd(2, 6, 4, 5), "style": rnd(2, 8)})
keys("AdaptiveInstanceNorm", m)
conv = nn.Conv1d(6, 4, 1)
m = R.WScaleLayer(conv, gain=2)
fwd_bwd("wscale", m, {"input": rnd(2, 4, 9)})
put("wscale", scale=m.scale)
keys("WScaleLayer", m)
m = R.Truncation(rnd(16), max_layer=3, threshold=0.7)
fwd_bwd("truncation", m, {"x": rnd(2, 5, 16)})
m.update(rnd(16))
put("truncation", avg_updated=m.avg_latent)
keys("Truncation", m)
keys("MinibatchStdDev", R.MinibatchStdDev())
keys("StddevLayer", R.StddevLayer())
keys("PixelNorm", R.PixelNorm())

if __name__ == "__main__":
    path = os.path.join(HERE, "gan_layers.npz")
    np.savez_compressed(path, **OUT)
    print("wrote %s (%.1f KB, %d arrays)" % (path, os.path.getsize(path) / 1024, len(OUT)))
