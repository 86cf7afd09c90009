"""CPU: the float64 model of the GAN-stabiliser layers (tests/gan_layers_model.py) reproduces tests/golden/gan_layers.npz, the reference's
own classes run in float64; spgan's modules have the reference's state_dict keys and shapes and load strictly both ways; the grouped
problem packing and the layers' domain checks reject what they must, before any GPU is touched."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import gan_layers_model as glm
import spgan
from spgan import gan_layers as gl

GOLD = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gan_layers.npz")))
TOL = 1e-11          # float64 against float64: a few hundred roundings of 1.1e-16 on values of order 1..10


def G(key):
    return torch.from_numpy(GOLD[key])


def close(a, b, what):
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max())
    assert err <= TOL * scale, (what, err, scale)


SN_TAGS = sorted({k.split("|")[0] for k in GOLD if k.startswith("sn_")})


@pytest.mark.parametrize("tag", SN_TAGS)
def test_model_spectral_norm_matches_golden(tag):
    rule = glm.RULE_L2NORMALIZE if tag.startswith("sn_class") else glm.RULE_F_NORMALIZE
    W, u, v, g, n = G(tag + "|in|W"), G(tag + "|in|u"), G(tag + "|in|v"), G(tag + "|g"), int(GOLD[tag + "|n"])
    w1, sigma, u1, v1 = glm.sn_forward(W, u, v, n, rule)
    close(w1, G(tag + "|w1"), "w1"), close(u1, G(tag + "|u1"), "u1"), close(v1, G(tag + "|v1"), "v1")
    close(glm.sn_backward(g, W, sigma, u1, v1), G(tag + "|dW"), "dW (explicit formula)")
    _, (dW,) = glm.vjp(lambda W_: glm.sn_forward(W_, u, v, n, rule)[0], [W], g)
    close(dW, G(tag + "|dW"), "dW (autograd, u and v constant)")
    uu, vv = u1, v1
    for _ in range(2):
        w3, _, uu, vv = glm.sn_forward(W, uu, vv, n, rule)
    close(w3, G(tag + "|w3"), "w3"), close(uu, G(tag + "|u3"), "u3"), close(vv, G(tag + "|v3"), "v3")
    if tag + "|weval" in GOLD:                 # the hook form in eval mode: no iteration, u and v untouched
        we, _, ue, _ = glm.sn_forward(W, uu, vv, 0, rule)
        close(we, G(tag + "|weval"), "weval")
        assert torch.equal(ue, uu) and torch.equal(G(tag + "|ueval"), G(tag + "|u3"))


MB_TAGS = sorted({k.split("|")[0] for k in GOLD if k.startswith(("mbstd_", "stddev_"))})


@pytest.mark.parametrize("tag", MB_TAGS)
def test_model_stddev_matches_golden(tag):
    p = [int(s) for s in tag.split("_")[1:]]
    grp, Fn = p[3], (p[4] if len(p) > 4 else 1)
    x, g = G(tag + "|in|x"), G(tag + "|g")
    out, (dx,) = glm.vjp(lambda x_: glm.mbstd_forward(x_, grp, Fn), [x], g)
    close(out, G(tag + "|out"), "out"), close(dx, G(tag + "|grad|x"), "dx")
    assert torch.equal(out[:, :x.shape[1]], x)


def _epi_case(tag):
    """-> (model call over (x, noise, w, gamma, beta), inputs, golden gradient keys)"""
    cm3 = lambda t: t.reshape(t.shape[0], t.shape[1], -1)                        # noqa: E731
    if tag in ("epilogue_lrelu", "epilogue_relu", "epilogue_noisegrad"):
        act = glm.ACT_RELU if tag.endswith("relu") and tag != "epilogue_lrelu" else glm.ACT_LRELU
        x, nz, w = G(tag + "|in|x"), G(tag + "|in|noise").reshape(3, 70), G(tag + "|param|top_epi.noise.weight").reshape(-1)
        f = lambda x_, n_, w_: glm.epilogue_forward(x_, n_, w_, act, 0.2, glm.PN_RSQRT, 1e-8, glm.STATS_JOINT)      # noqa: E731
        return f, [x, nz, w], ["grad|x", "grad|noise" if tag == "epilogue_noisegrad" else None, "pgrad|top_epi.noise.weight"]
    if tag == "epilogue_4d":
        f = lambda x_: glm.epilogue_forward(x_, None, None, glm.ACT_LRELU, 0.2, glm.PN_RSQRT, 1e-8, glm.STATS_CHANNEL)   # noqa: E731
        return f, [cm3(G(tag + "|in|x"))], ["grad|x"]
    if tag == "pixelnorm":
        return (lambda x_: glm.epilogue_forward(x_, pn=glm.PN_RSQRT)), [G(tag + "|in|x")], ["grad|x"]
    if tag == "pixelwisenorm":
        return (lambda x_: glm.epilogue_forward(x_, pn=glm.PN_SQRT_DIV)), [cm3(G(tag + "|in|x"))], ["grad|x"]
    if tag == "noiselayer":
        f = lambda x_, n_, w_: glm.epilogue_forward(x_, n_, w_)                  # noqa: E731
        return f, [G(tag + "|in|x"), G(tag + "|in|noise").reshape(3, 70), G(tag + "|param|weight").reshape(-1)], ["grad|x", "grad|noise", "pgrad|weight"]
    if tag == "noiseinjection":
        f = lambda x_, n_, w_: glm.epilogue_forward(x_, n_, w_)                  # noqa: E731
        return f, [cm3(G(tag + "|in|image")), G(tag + "|in|noise").reshape(2, 20), G(tag + "|param|weight").reshape(-1)], \
            ["grad|image", "grad|noise", "pgrad|weight"]
    raise KeyError(tag)


@pytest.mark.parametrize("tag", ["epilogue_lrelu", "epilogue_relu", "epilogue_noisegrad", "epilogue_4d", "pixelnorm", "pixelwisenorm",
                                 "noiselayer", "noiseinjection"])
def test_model_epilogue_matches_golden(tag):
    f, inputs, gkeys = _epi_case(tag)
    g = G(tag + "|g")
    out, grads = glm.vjp(f, inputs, g.reshape(inputs[0].shape))
    close(out, G(tag + "|out").reshape(out.shape), "out")
    for got, key in zip(grads, gkeys):
        if key is not None:
            close(got, G(tag + "|" + key).reshape(got.shape), key)


def test_joint_statistics_are_what_the_reference_computes():
    """LayerEpilogue on [B,C,N]: nn.InstanceNorm2d reads it as ONE image with B channels; per-(b,c) statistics are far off"""
    tag = "epilogue_lrelu"
    x, nz, w = G(tag + "|in|x"), G(tag + "|in|noise").reshape(3, 70), G(tag + "|param|top_epi.noise.weight").reshape(-1)
    per_channel = glm.epilogue_forward(x, nz, w, glm.ACT_LRELU, 0.2, glm.PN_RSQRT, 1e-8, glm.STATS_CHANNEL)
    assert float((per_channel - G(tag + "|out")).abs().max()) > 0.1


def test_model_adain_wscale_truncation_match_golden():
    tag = "adain"
    x, style = G(tag + "|in|input"), G(tag + "|in|style")
    W, b = G(tag + "|param|style.linear.weight_orig"), G(tag + "|param|style.linear.bias")

    def f(x_, s_, W_, b_):
        gb = s_ @ (W_ * (2.0 / 8) ** 0.5).t() + b_
        return glm.epilogue_forward(x_.reshape(2, 6, 20), stats=glm.STATS_CHANNEL, gamma=gb[:, :6], beta=gb[:, 6:]).reshape(x_.shape)
    out, grads = glm.vjp(f, [x, style, W, b], G(tag + "|g"))
    close(out, G(tag + "|out"), "out")
    for got, key in zip(grads, ["grad|input", "grad|style", "pgrad|style.linear.weight_orig", "pgrad|style.linear.bias"]):
        close(got, G(tag + "|" + key), key)
    close(G("wscale|in|input") * float(GOLD["wscale|scale"]), G("wscale|out"), "wscale")
    assert abs(float(GOLD["wscale|scale"]) - spgan.WScaleLayer(nn.Conv1d(6, 4, 1), gain=2).scale) < 1e-15
    x = G("truncation|in|x")
    out, (dx,) = glm.vjp(lambda x_: glm.truncation_forward(x_, G("truncation|param|avg_latent"), 3, 0.7), [x], G("truncation|g"))
    close(out, G("truncation|out"), "truncation"), close(dx, G("truncation|grad|x"), "truncation dx")


# ------------------------------------------------------------------------------------------------ state_dicts
def _keys(m):
    sd = m.state_dict()
    return list(sd.keys()), ["x".join(str(s) for s in v.shape) for v in sd.values()]


@pytest.mark.parametrize("name,build", [
    ("SpectralNorm", lambda: spgan.SpectralNorm(nn.Linear(3, 64), power_iterations=3)),
    ("spectral_norm", lambda: spgan.spectral_norm(nn.Linear(3, 64), n_power_iterations=3)),
    ("snconv2d", lambda: spgan.snconv2d(6, 4, 1)),
    ("snlinear", lambda: spgan.snlinear(7, 5)),
    ("NoiseLayer", lambda: spgan.NoiseLayer(5)),
    ("NoiseInjection", lambda: spgan.NoiseInjection(6)),
    ("LayerEpilogue", lambda: spgan.LayerEpilogue(5, 0, False, True, True, True, False, nn.ReLU())),
    ("AdaptiveInstanceNorm", lambda: spgan.AdaptiveInstanceNorm(6, 8)),
    ("WScaleLayer", lambda: spgan.WScaleLayer(nn.Conv1d(6, 4, 1))),
    ("Truncation", lambda: spgan.Truncation(torch.zeros(16), max_layer=3)),
    ("MinibatchStdDev", lambda: spgan.MinibatchStdDev()),
    ("StddevLayer", lambda: spgan.StddevLayer()),
    ("PixelNorm", lambda: spgan.PixelNorm()),
])
def test_state_dict_keys_and_shapes_equal_the_reference(name, build):
    keys, shapes = _keys(build())
    assert keys == list(GOLD["keys|" + name]) and shapes == list(GOLD["shapes|" + name])


def test_spectral_norm_state_dict_round_trips_with_torch():
    for make in (lambda: nn.Linear(7, 5), lambda: nn.Conv2d(6, 4, (1, 3)), lambda: nn.Conv1d(3, 8, 1)):
        ours, theirs = spgan.spectral_norm(make()), torch.nn.utils.spectral_norm(make())
        theirs.load_state_dict(ours.state_dict(), strict=True)
        for k, v in ours.state_dict().items():
            assert torch.equal(theirs.state_dict()[k], v)
        ours2 = spgan.spectral_norm(make())
        ours2.load_state_dict(theirs.state_dict(), strict=True)
    # u and v: unit vectors, not trainable
    m = spgan.SpectralNorm(nn.Conv1d(4, 3, 1))
    assert not m.module.weight_u.requires_grad and not m.module.weight_v.requires_grad and m.module.weight_bar.requires_grad
    assert abs(float(m.module.weight_u.norm()) - 1) < 1e-5 and abs(float(spgan.l2normalize(torch.ones(4)).norm()) - 1) < 1e-6
    with pytest.raises(RuntimeError, match="two spectral_norm hooks"):
        spgan.spectral_norm(spgan.spectral_norm(nn.Linear(2, 2)))


def test_spectral_norm_network_has_the_per_layer_keys():
    def net():
        return nn.Sequential(nn.Conv1d(3, 8, 1), nn.ReLU(), nn.Conv2d(8, 4, 1), nn.Flatten(), nn.Linear(4, 2), nn.BatchNorm1d(2))
    a, b = spgan.spectral_norm_network(net()), net()
    for sub in b:
        if isinstance(sub, (nn.Conv1d, nn.Conv2d, nn.Linear)):
            torch.nn.utils.spectral_norm(sub)
    assert _keys(a) == _keys(b)
    b.load_state_dict(a.state_dict(), strict=True), a.load_state_dict(b.state_dict(), strict=True)


# ------------------------------------------------------------------------------------------------ rejected inputs
def test_group_packing_rejects_bad_groups():
    geo, nsave, nws = gl.pack_sn_group([(512, 1024), (8, 6, 1, 4), (1, 64)], [512, 8, 1], [1024, 24, 64])
    assert [g[:2] for g in geo] == [(512, 1024), (8, 24), (1, 64)]
    assert nsave == sum(1 + h + w for h, w, _, _ in geo) and geo[1][2] == 1 + 512 + 1024
    lib = spgan._lib.load()
    assert nws == sum(lib.spgan_sn_ws_floats(h, w) for h, w, _, _ in geo) and geo[2][3] == sum(lib.spgan_sn_ws_floats(h, w) for h, w, _, _ in geo[:2])
    for bad in (([], [], []), ([(4, 0)], [4], [0]), ([()], [1], [1]), ([(4, 3)], [3], [3]), ([(4, 3)], [4], [4]), ([(4, 3), (2, 2)], [4], [3])):
        with pytest.raises(ValueError):
            gl.pack_sn_group(*bad)
    with pytest.raises(ValueError):
        gl.sn_group([torch.zeros(4, 3)], [torch.zeros(4)], [torch.zeros(3)], n_iter=-1)
    with pytest.raises(RuntimeError, match="no CPU"):
        gl.sn_group([torch.zeros(4, 3)], [torch.zeros(4)], [torch.zeros(3)])
    # the C entries: -22 before any launch
    a = spgan._lib.SnArgs()
    assert lib.spgan_sn_forward(a, 1, 1, 1e-12, None) == -22 and lib.spgan_sn_backward(a, None) == -22
    a.count = spgan._lib.SN_MAX + 1
    assert lib.spgan_sn_forward(a, 1, 1, 1e-12, None) == -22
    a.count = 1
    a.h[0], a.w[0] = 4, 3
    assert lib.spgan_sn_forward(a, 1, 1, 1e-12, None) == -22                        # missing pointers
    assert lib.spgan_sn_ws_floats(0, 3) == 0 and lib.spgan_sn_ws_floats(512, 1024) == 32 * 1024 + 512 + 256
    assert lib.spgan_mbstd_forward(1, 8, 5, 70, 3, 1, 1e-8, 1, 1, None) == -22      # 8 % 3
    assert lib.spgan_mbstd_forward(1, 8, 5, 70, 4, 2, 1e-8, 1, 1, None) == -22      # 5 % 2
    assert lib.spgan_mbstd_backward(None, 1, 8, 5, 70, 4, 1, 1e-8, 1, 1, None) == -22
    e = spgan._lib.EpilogueArgs()
    assert lib.spgan_epilogue_forward(e, 1, None) == -22
    e.x, e.B, e.C, e.L = 1, 2, 1025, 3
    assert lib.spgan_epilogue_forward(e, 1, None) == -22                            # C > 1024
    e.C, e.stats = 4, 1
    assert lib.spgan_epilogue_forward(e, 1, None) == -22                            # statistics without their buffers
    assert lib.spgan_epilogue_backward(e, None, 1, None, None, None, None, 0, None, None) == -22
    assert lib.spgan_truncation(None, None, 0, 1, 1, 1, 1, 0.7, 0, None, None) == -22


def test_value_errors_name_the_sizes():
    with pytest.raises(ValueError, match="batch_size 6 .* group_size 4"):
        gl.mbstd_groups(6, 5, 4, 1, strict=True)
    assert gl.mbstd_groups(3, 5, 4, 1, strict=True) == (3, 1) and gl.mbstd_groups(8, 6, 4, 2) == (4, 2)
    with pytest.raises(ValueError, match="batch size 6 .* 4"):
        gl.mbstd_groups(6, 5, 4, 1)
    with pytest.raises(ValueError, match="5 channels .* num_new_features = 2"):
        gl.mbstd_groups(8, 5, 4, 2)
    with pytest.raises(ValueError, match="C = 1025"):
        gl.epilogue_domain(1025, 3, gl.STATS_NONE)
    with pytest.raises(ValueError, match="C = 1, L = 1"):
        gl.epilogue_domain(1, 1, gl.STATS_JOINT)
    with pytest.raises(ValueError, match="L = 0"):
        gl.epilogue_domain(4, 0, gl.STATS_NONE)
    gl.epilogue_domain(1, 1, gl.STATS_NONE), gl.epilogue_domain(1024, 1, gl.STATS_CHANNEL)
    with pytest.raises(ValueError, match="activation_layer"):
        spgan.LayerEpilogue(4, 0, False, False, False, False, False, nn.Tanh())


def test_cpu_tensors_raise_runtime_error():
    x = torch.zeros(4, 4, 8)
    for call in (lambda: spgan.MinibatchStdDev()(x), lambda: spgan.StddevLayer()(x), lambda: spgan.PixelNorm()(x),
                 lambda: spgan.PixelwiseNorm()(x), lambda: spgan.NoiseLayer(4)(x), lambda: spgan.NoiseInjection(4)(x[..., None], x[:, :1, :, None]),
                 lambda: spgan.LayerEpilogue(4, 0, False, True, True, True, False, nn.ReLU())(x),
                 lambda: spgan.AdaptiveInstanceNorm(4, 3)(x[..., None], torch.zeros(4, 3)), lambda: spgan.WScaleLayer(nn.Conv1d(4, 4, 1))(x),
                 lambda: spgan.Truncation(torch.zeros(8))(x), lambda: spgan.SpectralNorm(nn.Conv1d(4, 4, 1))(x),
                 lambda: spgan.snlinear(8, 2)(x), lambda: spgan.spectral_norm_network(nn.Sequential(nn.Conv1d(4, 4, 1)))(x)):
        with pytest.raises(RuntimeError, match="no CPU"):
            call()
