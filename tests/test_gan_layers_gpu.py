"""GPU: the kernels of csrc/gan_layers.hip (spgan.gan_layers) against the float64 model tests/gan_layers_model.py.

Tolerance (every `near` below): the reference's own float32 formulation, composed from torch ops on the same device, is evaluated
against the float64 model -> e_ref; the HIP result must lie within max(4 * e_ref, 8 * 2^-24 * scale) of the model, scale = the largest
magnitude of the compared tensor.  The factor 4 covers a different but equally valid summation order, the floor the cases where torch
happens to be exact.  Copy paths, grouped-against-alone and captured-against-eager are compared bit for bit.  Every figure is appended to
LOG (tools/gan_layers_accuracy.py writes it to profiles/gan_layers_accuracy.json)."""
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

import gan_layers_model as glm
import spgan
from spgan import gan_layers as gl

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOG = []
GOLD = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gan_layers.npz")))


def rnd(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(DEV)


def f32(t):
    return None if t is None else t.float().contiguous()


def near(case, what, got, ref32, model):
    model = model.double()
    scale = float(model.abs().max())
    e_ref = float((ref32.double() - model).abs().max())
    err = float((got.double() - model).abs().max())
    bound = max(4 * e_ref, 8 * 2.0 ** -24 * scale)
    LOG.append({"case": case, "tensor": what, "err_hip": err, "e_ref": e_ref, "scale": scale, "bound": bound})
    print("%s %s: hip %.3e  torch-f32 %.3e  bound %.3e  scale %.3e" % (case, what, err, e_ref, bound, scale))
    assert got.shape == model.shape and err <= bound, (case, what, err, e_ref, bound)


# ------------------------------------------------------------------------------------------------ spectral norm
def sn_inputs(seed=0):
    Ws = [rnd(seed + i, *s) for i, s in enumerate(glm.SN_SHAPES)]
    us = [glm.normalise(rnd(seed + 100 + i, s[0]), 1, 1e-12) for i, s in enumerate(glm.SN_SHAPES)]
    vs = [glm.normalise(rnd(seed + 200 + i, int(np.prod(s[1:]))), 1, 1e-12) for i, s in enumerate(glm.SN_SHAPES)]
    return Ws, us, vs


def clones(ts):
    return [f32(t).clone() for t in ts]


@pytest.mark.parametrize("rule", [glm.RULE_L2NORMALIZE, glm.RULE_F_NORMALIZE])
@pytest.mark.parametrize("n", [1, 3])
def test_sn_group_against_model_and_alone(rule, n):
    Ws, us, vs = sn_inputs()
    W32 = [w.requires_grad_(True) for w in clones(Ws)]
    u32, v32 = clones(us), clones(vs)
    outs = gl.sn_group(W32, u32, v32, n, rule, 1e-12)
    Gs = [rnd(300 + i, *s) for i, s in enumerate(glm.SN_SHAPES)]
    dWs = torch.autograd.grad(sum((o * f32(g)).sum() for o, g in zip(outs, Gs)), W32)
    for i, s in enumerate(glm.SN_SHAPES):
        case = "sn %s n=%d rule=%d" % ("x".join(map(str, s)), n, rule)
        mw, msig, mu, mv = glm.sn_forward(Ws[i], us[i], vs[i], n, rule)
        Wr = f32(Ws[i]).requires_grad_(True)
        rw, rsig, ru, rv = glm.ref32_sn(Wr, f32(us[i]), f32(vs[i]), n, rule, 1e-12)
        near(case, "W/sigma", outs[i].detach(), rw.detach(), mw)
        near(case, "u", u32[i], ru, mu), near(case, "v", v32[i], rv, mv)
        (rdW,) = torch.autograd.grad((rw * f32(Gs[i])).sum(), Wr)
        mdW = glm.sn_backward(Gs[i], Ws[i], msig, mu, mv)
        near(case, "dW", dWs[i], rdW, mdW)
        # the u v^T term is part of what was compared: without it the gradient is far outside the bound
        assert float((Gs[i] / msig - mdW).abs().max()) > 100 * LOG[-1]["bound"]
        # alone: the same bits as inside the group
        Wa, ua, va = f32(Ws[i]).requires_grad_(True), f32(us[i]).clone(), f32(vs[i]).clone()
        (oa,) = gl.sn_group([Wa], [ua], [va], n, rule, 1e-12)
        (dWa,) = torch.autograd.grad((oa * f32(Gs[i])).sum(), Wa)
        assert torch.equal(oa, outs[i]) and torch.equal(ua, u32[i]) and torch.equal(va, v32[i]) and torch.equal(dWa, dWs[i]), case


def test_sn_three_consecutive_forwards():
    Ws, us, vs = sn_inputs(seed=7)
    u32, v32 = clones(us), clones(vs)
    ru, rv, mu, mv = clones(us), clones(vs), list(us), list(vs)
    for _ in range(3):
        outs = gl.sn_group(clones(Ws), u32, v32, 1, glm.RULE_L2NORMALIZE, 1e-12)
        for i in range(len(Ws)):
            rw, _, ru[i], rv[i] = glm.ref32_sn(f32(Ws[i]), ru[i], rv[i], 1, glm.RULE_L2NORMALIZE, 1e-12)
            mw, _, mu[i], mv[i] = glm.sn_forward(Ws[i], mu[i], mv[i], 1, glm.RULE_L2NORMALIZE)
    for i, s in enumerate(glm.SN_SHAPES):
        case = "sn 3 forwards %s" % "x".join(map(str, s))
        near(case, "u", u32[i], ru[i], mu[i]), near(case, "v", v32[i], rv[i], mv[i])
        # the third call's quotient is W / (u3 . W v3): the n_iter = 0 evaluation at the final vectors
        near(case, "W/sigma", outs[i], glm.ref32_sn(f32(Ws[i]), ru[i], rv[i], 0, 0, 1e-12)[0], glm.sn_forward(Ws[i], mu[i], mv[i], 0, 0)[0])


def test_sn_double_backward_and_cpu_are_refused():
    W = rnd(1, 5, 7).float().requires_grad_(True)
    (o,) = gl.sn_group([W], [f32(rnd(2, 5))], [f32(rnd(3, 7))])
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(o.sum(), W, create_graph=True)


def test_sn_wrappers_training_against_eval():
    lin = nn.Linear(7, 5)
    sd = {"weight_orig": torch.from_numpy(GOLD["sn_hook_5x7_n1|in|W"]).float(), "weight_u": torch.from_numpy(GOLD["sn_hook_5x7_n1|in|u"]).float(),
          "weight_v": torch.from_numpy(GOLD["sn_hook_5x7_n1|in|v"]).float(), "bias": lin.bias.detach().clone()}
    assert sorted(sd) == sorted(GOLD["keys|snlinear"])
    ours, theirs = spgan.spectral_norm(nn.Linear(7, 5)), torch.nn.utils.spectral_norm(nn.Linear(7, 5))
    ours.load_state_dict(sd, strict=True)
    theirs.load_state_dict(ours.state_dict(), strict=True)                  # ours -> torch, strictly
    ours.to(DEV).train(), theirs.to(DEV).train()
    x = torch.from_numpy(GOLD["sn_hook_5x7_n1|in|x"]).float().to(DEV)
    ours(x), theirs(x)
    G = lambda k: torch.from_numpy(GOLD["sn_hook_5x7_n1|" + k]).to(DEV)      # noqa: E731
    near("hook train", "weight", ours.weight.detach(), theirs.weight.detach(), G("w1"))
    near("hook train", "u", ours.weight_u, theirs.weight_u, G("u1"))
    ours(x), theirs(x), ours(x), theirs(x)
    near("hook train x3", "u", ours.weight_u, theirs.weight_u, G("u3")), near("hook train x3", "v", ours.weight_v, theirs.weight_v, G("v3"))
    ours.eval(), theirs.eval()
    u_before = ours.weight_u.clone()
    ours(x), theirs(x)
    assert torch.equal(ours.weight_u, u_before)                             # eval: no power iteration
    near("hook eval", "weight", ours.weight.detach(), theirs.weight.detach(), G("weval"))
    back = torch.nn.utils.spectral_norm(nn.Linear(7, 5))
    back.load_state_dict(ours.state_dict(), strict=True)                    # and back, after training
    ours.load_state_dict(back.state_dict(), strict=True)


def test_sn_reference_class_iterates_in_eval_mode_too():
    tag = "sn_class_5x7_n1"
    T = lambda k: torch.from_numpy(GOLD[tag + "|" + k]).to(DEV)               # noqa: E731
    lin = nn.Linear(7, 5)
    m = spgan.SpectralNorm(lin)
    assert list(m.state_dict()) == list(GOLD["keys|SpectralNorm"])
    m.load_state_dict({"module.bias": lin.bias.detach().clone(), "module.weight_bar": T("in|W").float(), "module.weight_u": T("in|u").float(),
                       "module.weight_v": T("in|v").float()}, strict=True)
    m.to(DEV).eval()
    x, g = f32(T("in|x")), T("g")
    y = m(x)
    assert torch.equal(y, torch.nn.functional.linear(x, lin.weight, lin.bias))
    Wr = f32(T("in|W")).requires_grad_(True)
    rw, _, ru, rv = glm.ref32_sn(Wr, f32(T("in|u")), f32(T("in|v")), 1, 0, 1e-12)
    near("class eval", "weight", lin.weight.detach(), rw.detach(), T("w1"))
    near("class eval", "u", lin.weight_u.data, ru, T("u1")), near("class eval", "v", lin.weight_v.data, rv, T("v1"))
    (lin.weight * f32(g)).sum().backward()
    (rdW,) = torch.autograd.grad((rw * f32(g)).sum(), Wr)
    near("class eval", "dW", lin.weight_bar.grad, rdW, T("dW"))
    m(x), m(x)
    for _ in range(2):
        _, _, ru, rv = glm.ref32_sn(f32(T("in|W")), ru, rv, 1, 0, 1e-12)
    near("class eval x3", "u", lin.weight_u.data, ru, T("u3")), near("class eval x3", "v", lin.weight_v.data, rv, T("v3"))
    # a 4-D parameter is flattened from dim 0 (the update alone: no convolution is run)
    tag = "sn_class_8x6x1x4_n1"
    conv = nn.Conv2d(6, 8, (1, 4))
    mc = spgan.SpectralNorm(conv)
    mc.load_state_dict({"module.bias": conv.bias.detach().clone(), "module.weight_bar": T("in|W").float(), "module.weight_u": T("in|u").float(),
                        "module.weight_v": T("in|v").float()}, strict=True)
    mc.to(DEV)
    mc._update_u_v()
    rw = glm.ref32_sn(f32(T("in|W")), f32(T("in|u")), f32(T("in|v")), 1, 0, 1e-12)[0]
    assert conv.weight.shape == (8, 6, 1, 4)
    near("class 4-D", "weight", conv.weight.detach(), rw, T("w1"))


def _critic():
    return nn.Sequential(nn.Conv1d(3, 64, 1), nn.LeakyReLU(0.2), nn.Conv1d(64, 128, 1), nn.LeakyReLU(0.2), nn.AdaptiveMaxPool1d(1),
                         nn.Flatten(), nn.Linear(128, 1))


def test_spectral_norm_network_equals_per_layer_application():
    torch.manual_seed(3)
    a, b = _critic(), _critic()
    b.load_state_dict(a.state_dict())
    spgan.spectral_norm_network(a)
    for sub in b:
        if isinstance(sub, (nn.Conv1d, nn.Linear)):
            spgan.spectral_norm(sub)
    b.load_state_dict(a.state_dict(), strict=True)
    a.to(DEV), b.to(DEV)
    x = f32(rnd(5, 4, 3, 33))
    for mode in (True, True, False):
        a.train(mode), b.train(mode)
        ya, yb = a(x), b(x)
        assert torch.equal(ya, yb)
        for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
            assert ka == kb and torch.equal(va, vb), ka
        # the normalised weights and their gradients (the spectral-norm backward alone: torch's convolution backward between the
        # layers is not bit-reproducible and is not what is compared)
        la, lb = ([m for m in net if hasattr(m, "weight_orig")] for net in (a, b))
        cot = [f32(rnd(70 + i, *m.weight.shape)) for i, m in enumerate(la)]
        ga = torch.autograd.grad(sum((m.weight * c).sum() for m, c in zip(la, cot)), [m.weight_orig for m in la])
        gb = torch.autograd.grad(sum((m.weight * c).sum() for m, c in zip(lb, cot)), [m.weight_orig for m in lb])
        for ma, mb, da, db in zip(la, lb, ga, gb):
            assert torch.equal(ma.weight, mb.weight) and torch.equal(da, db)
    assert len(la) == 3


def test_sn_inside_captured_body_equals_eager():
    torch.manual_seed(4)
    a, b = spgan.spectral_norm(nn.Linear(64, 16)).to(DEV), spgan.spectral_norm(nn.Linear(64, 16)).to(DEV)
    b.load_state_dict(a.state_dict(), strict=True)

    def body_of(m):
        def body(x):
            out = m(x)
            (dW,) = torch.autograd.grad(out.square().sum(), m.weight_orig)
            return out, dW, m.weight_u.clone(), m.weight_v.clone()
        return body
    cap, eager = spgan.CapturedBody(body_of(a), modules=(a,), warmup=1), body_of(b)
    x = f32(rnd(6, 8, 64))
    with warnings.catch_warnings():
        warnings.simplefilter("error")                     # a failed capture warns and falls back to eager issue: that is a failure here
        for call in range(3):                              # 1 eager warm-up call, then the capture and two replays
            got = [t.clone() for t in cap(x)]
            want = eager(x)
            for g, w in zip(got, want):
                assert torch.equal(g, w), call
    assert cap._graph is not None and not cap.eager


# ------------------------------------------------------------------------------------------------ stddev layers
@pytest.mark.parametrize("B,C,N,grp,Fn", glm.MBSTD_CASES)
def test_stddev_layers(B, C, N, grp, Fn):
    case = "mbstd %s" % ((B, C, N, grp, Fn),)
    x, g = rnd(10, B, C, N), rnd(11, B, C + Fn, N)
    layer = spgan.MinibatchStdDev(grp) if Fn == 1 else spgan.StddevLayer(grp, Fn)
    xh = f32(x).requires_grad_(True)
    out = layer(xh)
    (dx,) = torch.autograd.grad((out * f32(g)).sum(), xh)
    xr = f32(x).requires_grad_(True)
    ro = glm.ref32_mbstd(xr, grp, Fn)
    (rdx,) = torch.autograd.grad((ro * f32(g)).sum(), xr)
    mo, (mdx,) = glm.vjp(lambda x_: glm.mbstd_forward(x_, grp, Fn), [x], g)
    assert torch.equal(out[:, :C].detach(), f32(x))                         # the channel copy: bit-exact
    near(case, "new channels", out[:, C:].detach(), ro[:, C:].detach(), mo[:, C:])
    near(case, "dx", dx, rdx, mdx)
    if Fn > 1:                                                              # StddevLayer and the functional form agree
        assert torch.equal(gl.minibatch_stddev(f32(x), grp, Fn), out.detach())
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(layer(xh).sum(), xh, create_graph=True)


def test_stddev_value_errors_on_the_device():
    with pytest.raises(ValueError, match="batch_size 6"):
        spgan.MinibatchStdDev(4)(torch.zeros(6, 4, 8, device=DEV))
    with pytest.raises(ValueError, match="batch size 6"):
        spgan.StddevLayer(4)(torch.zeros(6, 4, 8, device=DEV))
    with pytest.raises(ValueError, match="5 channels"):
        spgan.StddevLayer(4, 2)(torch.zeros(8, 5, 8, device=DEV))


# ------------------------------------------------------------------------------------------------ epilogue
def epi_inputs(B, C, L, seed=20):
    x, nz, w = rnd(seed, B, C, L), rnd(seed + 1, B, L), rnd(seed + 2, C)
    x = x + 0.05 * torch.sign(x + w.view(1, -1, 1) * nz.view(B, 1, L))     # |x + w*noise| >= 0.05: away from the activation's kink
    x0 = rnd(seed, B, C, L)
    x0 = x0 + 0.05 * torch.sign(x0)                                       # the same for the cases without noise
    return x, x0, nz, w, rnd(seed + 3, B, C) + 1.0, rnd(seed + 4, B, C), rnd(seed + 5, B, C, L)


def run_epilogue(case, x, nz, w, act, slope, pn, stats, gamma, beta, g):
    """forward + backward of the HIP layer, torch float32 and the float64 model on the same inputs; compares y and every gradient"""
    ins64 = [x, nz, w, gamma, beta]
    hip = [None if t is None else f32(t).requires_grad_(True) for t in ins64]
    gb = None if gamma is None else torch.cat([hip[3], hip[4]], 1)
    y = gl.layer_epilogue(hip[0], hip[1], hip[2], act, slope, pn, 1e-8, stats, 1e-5, gb)
    ref = [None if t is None else f32(t).requires_grad_(True) for t in ins64]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ry = glm.ref32_epilogue(ref[0], ref[1], ref[2], act, slope, pn, 1e-8, stats, ref[3], ref[4])
    my, mg = glm.vjp(lambda *a: glm.epilogue_forward(a[0], a[1], a[2], act, slope, pn, 1e-8, stats, 1e-5, a[3], a[4]), ins64, g)
    near(case, "y", y.detach(), ry.detach(), my)
    hg = torch.autograd.grad((y * f32(g)).sum(), [t for t in hip if t is not None])
    rg = torch.autograd.grad((ry * f32(g)).sum(), [t for t in ref if t is not None])
    names = [n for n, t in zip(("dx", "dnoise", "dw", "dgamma", "dbeta"), ins64) if t is not None]
    for n, h, r, m in zip(names, hg, rg, [t for t in mg if t is not None]):
        near(case, n, h, r, m)


STAGES = {
    "noise": dict(noise=True), "relu": dict(act=glm.ACT_RELU), "lrelu": dict(act=glm.ACT_LRELU, slope=0.2),
    "pixelnorm": dict(pn=glm.PN_RSQRT), "pixelwisenorm": dict(pn=glm.PN_SQRT_DIV), "in_channel": dict(stats=glm.STATS_CHANNEL),
    "in_joint": dict(stats=glm.STATS_JOINT), "affine": dict(affine=True),
    "pixelwisenorm+in_channel+affine": dict(pn=glm.PN_SQRT_DIV, stats=glm.STATS_CHANNEL, affine=True, act=glm.ACT_RELU, noise=True),
    "pixelnorm+affine": dict(pn=glm.PN_RSQRT, affine=True),
}


@pytest.mark.parametrize("stage", list(STAGES))
def test_epilogue_every_stage_alone(stage):
    o = STAGES[stage]
    x, x0, nz, w, gamma, beta, g = epi_inputs(3, 5, 70)
    noise = o.get("noise", False)
    run_epilogue("stage " + stage, x if noise else x0, nz if noise else None, w if noise else None, o.get("act", glm.ACT_NONE), o.get("slope", 0.0),
                 o.get("pn", glm.PN_NONE), o.get("stats", glm.STATS_NONE), gamma if o.get("affine") else None, beta if o.get("affine") else None, g)


@pytest.mark.parametrize("B,C,L", glm.EPILOGUE_SHAPES)
@pytest.mark.parametrize("actl", [nn.LeakyReLU(0.2), nn.ReLU()], ids=["lrelu", "relu"])
def test_layer_epilogue_full(B, C, L, actl):
    case = "LayerEpilogue %s %s" % ((B, C, L), type(actl).__name__)
    x, _, nz, w, _, _, g = epi_inputs(B, C, L, seed=40)
    m = spgan.LayerEpilogue(C, 0, False, True, True, True, False, actl).to(DEV)
    m.top_epi.noise.weight.data.copy_(f32(w).view(1, C, 1))
    xh, nh = f32(x).requires_grad_(True), f32(nz).view(B, 1, L).requires_grad_(True)
    y = m(xh, noise=nh)
    m.top_epi.noise.noise = nh.detach()                                     # the attribute route gives the same bits
    assert torch.equal(m(f32(x)), y.detach())
    dx, dn, dw = torch.autograd.grad((y * f32(g)).sum(), [xh, nh, m.top_epi.noise.weight])
    act, slope = (glm.ACT_RELU, 0.0) if isinstance(actl, nn.ReLU) else (glm.ACT_LRELU, 0.2)
    ref = [f32(t).requires_grad_(True) for t in (x, nz, w)]
    # the reference's chain itself: nn.InstanceNorm2d on the 3-D tensor (joint statistics per sample)
    t = ref[0] + ref[2].view(1, -1, 1) * ref[1].view(B, 1, L)
    t = actl(t)
    t = t * torch.rsqrt(torch.mean(t ** 2, dim=1, keepdim=True) + 1e-8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ry = nn.InstanceNorm2d(C)(t)
    rg = torch.autograd.grad((ry * f32(g)).sum(), ref)
    my, mg = glm.vjp(lambda a, b, c: glm.epilogue_forward(a, b, c, act, slope, glm.PN_RSQRT, 1e-8, glm.STATS_JOINT), [x, nz, w], g)
    near(case, "y", y.detach(), ry.detach(), my)
    near(case, "dx", dx, rg[0], mg[0]), near(case, "dnoise", dn.view(B, L), rg[1], mg[1]), near(case, "dw", dw.view(C), rg[2], mg[2])
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(m(xh, noise=nh).sum(), xh, create_graph=True)


def test_layer_epilogue_4d_is_per_channel():
    B, C, H, W = 2, 6, 4, 5
    x, x0, _, _, _, _, g = epi_inputs(B, C, H * W, seed=60)
    m = spgan.LayerEpilogue(C, 0, False, False, True, True, False, nn.LeakyReLU(0.2))
    xh = f32(x0).view(B, C, H, W).requires_grad_(True)
    y = m(xh)
    (dx,) = torch.autograd.grad((y * f32(g).view(B, C, H, W)).sum(), xh)
    xr = f32(x0).view(B, C, H, W).requires_grad_(True)
    t = nn.LeakyReLU(0.2)(xr)
    ry = nn.InstanceNorm2d(C)(t * torch.rsqrt(torch.mean(t ** 2, dim=1, keepdim=True) + 1e-8))
    (rdx,) = torch.autograd.grad((ry * f32(g).view(B, C, H, W)).sum(), xr)
    my, (mdx,) = glm.vjp(lambda a: glm.epilogue_forward(a, None, None, glm.ACT_LRELU, 0.2, glm.PN_RSQRT, 1e-8, glm.STATS_CHANNEL), [x0], g)
    near("LayerEpilogue 4-D", "y", y.detach().view(B, C, -1), ry.detach().view(B, C, -1), my)
    near("LayerEpilogue 4-D", "dx", dx.view(B, C, -1), rdx.view(B, C, -1), mdx)
    with pytest.raises(ValueError, match="use_noise=False"):
        spgan.LayerEpilogue(C, 0, False, True, True, True, False, nn.ReLU()).to(DEV)(f32(x0).view(B, C, H, W))
    with pytest.raises(ValueError, match="C = 1025"):
        spgan.PixelNorm()(torch.zeros(1, 1025, 2, device=DEV))


def test_adaptive_instance_norm_and_small_layers():
    tag = "adain"
    G64 = lambda k: torch.from_numpy(GOLD[tag + "|" + k]).to(DEV)               # noqa: E731
    m = spgan.AdaptiveInstanceNorm(6, 8)
    m.load_state_dict({"style.linear.weight_orig": G64("param|style.linear.weight_orig").float(), "style.linear.bias": G64("param|style.linear.bias").float()},
                      strict=True)
    m.to(DEV)
    x, s = f32(G64("in|input")).requires_grad_(True), f32(G64("in|style")).requires_grad_(True)
    y = m(x, s)
    grads = torch.autograd.grad((y * f32(G64("g"))).sum(), [x, s, m.style.linear.weight_orig, m.style.linear.bias])
    xr, sr, Wr, br = (f32(G64(k)).requires_grad_(True) for k in ("in|input", "in|style", "param|style.linear.weight_orig", "param|style.linear.bias"))
    gbr = torch.nn.functional.linear(sr, Wr * (2.0 / 8) ** 0.5, br).unsqueeze(2).unsqueeze(3)
    ry = gbr[:, :6] * nn.InstanceNorm2d(6)(xr) + gbr[:, 6:]
    rg = torch.autograd.grad((ry * f32(G64("g"))).sum(), [xr, sr, Wr, br])
    near("AdaIN", "y", y.detach(), ry.detach(), G64("out"))
    for n, h, r, k in zip(("dx", "dstyle", "dW", "db"), grads, rg, ("grad|input", "grad|style", "pgrad|style.linear.weight_orig", "pgrad|style.linear.bias")):
        near("AdaIN", n, h, r, G64(k))
    # NoiseInjection, PixelwiseNorm on 4-D, WScaleLayer, Truncation against the golden file
    ni = spgan.NoiseInjection(6).to(DEV)
    ni.weight.data.copy_(torch.from_numpy(GOLD["noiseinjection|param|weight"]).float())
    im, nz = (torch.from_numpy(GOLD["noiseinjection|in|" + k]).to(DEV) for k in ("image", "noise"))
    near("NoiseInjection", "y", ni(f32(im), f32(nz)).detach(), f32(im) + ni.weight.detach() * f32(nz), torch.from_numpy(GOLD["noiseinjection|out"]).to(DEV))
    xp = torch.from_numpy(GOLD["pixelwisenorm|in|x"]).to(DEV)
    near("PixelwiseNorm", "y", spgan.PixelwiseNorm()(f32(xp)), f32(xp) / f32(xp).pow(2.0).mean(dim=1, keepdim=True).add(1e-8).sqrt(),
         torch.from_numpy(GOLD["pixelwisenorm|out"]).to(DEV))
    xw = torch.from_numpy(GOLD["wscale|in|input"]).to(DEV)
    ws = spgan.WScaleLayer(nn.Conv1d(6, 4, 1), gain=2)
    near("WScaleLayer", "y", ws(f32(xw)), f32(xw) * ws.scale, torch.from_numpy(GOLD["wscale|out"]).to(DEV))
    tr = spgan.Truncation(torch.from_numpy(GOLD["truncation|param|avg_latent"]).float(), max_layer=3, threshold=0.7).to(DEV)
    xt = f32(torch.from_numpy(GOLD["truncation|in|x"]).to(DEV)).requires_grad_(True)
    yt = tr(xt)
    (dxt,) = torch.autograd.grad((yt * f32(torch.from_numpy(GOLD["truncation|g"]).to(DEV))).sum(), xt)
    xr = xt.detach().clone().requires_grad_(True)
    keep = (torch.arange(5, device=DEV) < 3).view(1, -1, 1)
    ryt = torch.where(keep, torch.lerp(tr.avg_latent, xr, 0.7), xr)
    (rdxt,) = torch.autograd.grad((ryt * f32(torch.from_numpy(GOLD["truncation|g"]).to(DEV))).sum(), xr)
    near("Truncation", "y", yt.detach(), ryt.detach(), torch.from_numpy(GOLD["truncation|out"]).to(DEV))
    near("Truncation", "dx", dxt, rdxt, torch.from_numpy(GOLD["truncation|grad|x"]).to(DEV))
    assert torch.equal(yt[:, 3:].detach(), xt[:, 3:].detach())                 # the rows past max_layer: copied
    tr.update(torch.from_numpy(GOLD["truncation|param|avg_latent"]).float().to(DEV) * 0 + 1)
    assert tr.avg_latent.shape == (16,)


def test_noise_layer_draws_on_the_device():
    m = spgan.NoiseLayer(4).to(DEV)
    m.weight.data.fill_(1.0)
    x = torch.zeros(2, 4, 512, device=DEV)
    y = m(x)                                                                # no argument, no attribute: 0.2 * randn on the device
    assert y.is_cuda and torch.equal(y[:, 0], y[:, 3]) and 0.15 < float(y.detach().std()) < 0.25
    m.noise = torch.ones(2, 1, 512, device=DEV)
    assert torch.equal(m(x), torch.ones_like(x)) and torch.equal(m(x, noise=2 * m.noise), 2 * torch.ones_like(x))
