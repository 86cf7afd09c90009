"""CPU: the float64 model of GC_attn, Self_Attn2, DenseModule2D, MultiDenseMLP and Dense_Attn_2D (tests/gc_attn_model.py) against the
reference's golden results (tests/golden/utilities_rest.npz), the modules' parameter surface against the golden's recorded keys, shapes and
initial values, constructor refusals, the argument checks of every spgan_gc_attn_* entry point and the weight images of MultiDenseMLP's
side-input layout -- none of which needs a GPU."""
import os

import numpy as np
import pytest
import torch

import gc_attn_model as gm

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "utilities_rest.npz")


@pytest.fixture(scope="module")
def d():
    return np.load(GOLD)


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


@pytest.mark.parametrize("tag", list(gm.CASES))
def test_model_reproduces_golden(d, tag):
    """the model in float64 against the reference's float64 run: rel-L2 1e-10; gradients that are zero in exact arithmetic below 1e-9
    absolute in both; the stored inputs are case_tensors' under the stored seed"""
    x, g, sd = gm.case_tensors(tag, int(d["%s|seed" % tag]))
    assert torch.equal(g, torch.from_numpy(d["%s|g" % tag]))
    for n, t in zip(gm.input_names(tag), x if isinstance(x, list) else [x]):
        assert torch.equal(t, torch.from_numpy(d["%s|%s" % (tag, n)])), n
    gsd = gm.golden_state_dict(d, tag)
    assert list(gsd) == list(sd) and all(torch.equal(gsd[n], sd[n]) for n in sd)
    res = gm.run(tag, x, g, sd)
    qs = gm.quantities(d, tag)
    assert sorted(qs) == sorted(q for q in res if q != "pre")
    assert gm.kink_margin(res["pre"]) > 1e-5 and abs(gm.kink_margin(res["pre"]) / float(d["%s|kink_margin" % tag]) - 1) < 1e-9
    for q in qs:
        ref = gm.golden_f64(d, tag, q)
        if gm.zero_gradient(tag, q) is not None:
            assert float(res[q].abs().max()) < 1e-9 and float(ref.abs().max()) < 1e-9, q
            continue
        if q.endswith("num_batches_tracked"):
            assert int(res[q]) == int(d["%s|%s|full" % (tag, q)]), q
            continue
        assert _rel(res[q], ref) < 1e-10, (tag, q, _rel(res[q], ref))


def test_zero_gradients_are_listed(d):
    assert gm.zero_gradient("gc_att", "grad|conv_mask.bias") == "exact" and gm.zero_gradient("gc_att", "grad|conv_mask.weight") is None
    assert "grad|conv_mask.bias" in gm.quantities(d, "gc_att") and "grad|conv_mask.bias" not in gm.quantities(d, "gc_avg")
    zeros = {tag: sorted(q for q in gm.quantities(d, tag) if gm.zero_gradient(tag, q)) for tag in gm.CASES}
    assert zeros["sa2_train"] == ["grad|key.0.bias", "grad|query.0.bias", "grad|value.0.bias"] and zeros["sa2_eval"] == [] and zeros["d2_eval"] == []
    assert zeros["d2_train"] == ["grad|dense_modules.%d.0.bias" % l for l in range(3)] == zeros["mdm"]
    assert zeros["da_gc"] == ["grad|atten.conv_mask.bias", "grad|dense.dense_modules.0.0.bias", "grad|dense.dense_modules.1.0.bias"]
    assert zeros["da_sa"] == ["grad|atten.query.bias", "grad|dense.dense_modules.0.0.bias", "grad|dense.dense_modules.1.0.bias"]


@pytest.mark.parametrize("tag,entries", [("gc_att", 14), ("gc_add", 8), ("gc_mul", 8), ("gc_avg", 12), ("gc_4d", 14), ("sa2_train", 22), ("sa2_eval", 22),
                                         ("d2_train", 21), ("d2_eval", 21), ("mdm", 21), ("da_gc", 28), ("da_sa", 21)])
def test_state_dict_surface(d, tag, entries):
    """keys in the reference's order, shapes and dtypes as recorded; strict loading; the reference's initial values under its seed"""
    import spgan
    torch.manual_seed(gm.INIT_SEED)
    m = gm.build_module(spgan, tag)
    sd, gsd = m.state_dict(), gm.golden_state_dict(d, tag)
    assert len(sd) == entries and list(sd) == list(gsd)
    for n in sd:
        assert sd[n].shape == gsd[n].shape and sd[n].dtype == gsd[n].dtype, n
    if tag in gm.INIT_TAGS:
        init = gm.golden_state_dict(d, tag, "init")
        assert list(init) == list(sd)
        for n in sd:
            assert torch.equal(sd[n], init[n]), n                       # the same seed gives the reference's initial parameters
    m.load_state_dict(gsd, strict=True)
    assert all(torch.equal(m.state_dict()[n], gsd[n]) for n in gsd)
    c = gm.CASES[tag]
    if c["kind"] == "sa2":
        assert list(sd)[0] == "gamma"
    if c["kind"] == "da":
        assert [n for n, _ in m.named_children()] == ["atten", "dense"]
    if c["kind"] != "gc":
        return
    assert hasattr(m, "conv_mask") == (c["pool"] == "att") and hasattr(m, "softmax") == (c["pool"] == "att") and hasattr(m, "avg_pool") == (c["pool"] != "att")
    assert (m.channel_add_conv is None) == ("channel_add" not in c["fusions"]) and (m.channel_mul_conv is None) == ("channel_mul" not in c["fusions"])
    assert [n for n, _ in m.named_children()] == (["conv_mask", "softmax"] if c["pool"] == "att" else ["avg_pool"]) + \
        [b for b in ("channel_add_conv", "channel_mul_conv") if b[:-5] in c["fusions"]]
    assert not any(True for _ in m.buffers())


def test_constructor_refusals():
    import spgan
    for bad in ("attention", "att2", "satt", None, 3):
        with pytest.raises(ValueError, match="pool"):
            spgan.GC_attn(16, pool=bad)
    for kw in (dict(in_dim=0), dict(in_dim=1025), dict(in_dim=16, out_dim=0), dict(in_dim=16, out_dim=1025)):
        with pytest.raises(ValueError, match="gc_attn serves"):
            spgan.GC_attn(**kw)
    m = spgan.GC_attn(1024, out_dim=1, pool="max", fusions=[])
    assert len(m.state_dict()) == 0 and m.pool == "max"
    with pytest.raises(RuntimeError, match="GPU"):
        spgan.GC_attn(16)(torch.zeros(2, 16, 5))


def test_other_constructor_refusals():
    import spgan
    for mlps in ([], [64]):
        with pytest.raises(ValueError, match="mlps"):
            spgan.DenseModule2D(mlps=mlps)
        with pytest.raises(ValueError, match="mlps"):
            spgan.Dense_Attn_2D(mlps=mlps)
    with pytest.raises(ValueError):
        spgan.MultiDenseMLP([8, 5], [6, 3, 2])
    with pytest.raises(ValueError):
        spgan.MultiDenseMLP([], [])
    for bad in (4, 1024):
        with pytest.raises(ValueError, match="Self_Attn2"):
            spgan.Self_Attn2(bad)
    assert isinstance(spgan.Dense_Attn_2D(6, mlps=[6, 8, 16]).atten, spgan.GC_attn)
    assert isinstance(spgan.Dense_Attn_2D(6, mlps=[6, 8, 16], atten="self").atten, spgan.Self_Attn)
    d2 = spgan.DenseModule2D(in_dim=6, levels=9, growth_rate=1, mlps=[99, 8, 5, 7])                 # levels, growth_rate, mlps[0]: ignored
    assert [m[0].weight.shape[:2] for m in d2.dense_modules] == [(8, 6), (5, 14), (7, 19)]
    for m in (d2, spgan.MultiDenseMLP([8], [6]), spgan.Self_Attn2(16)):
        with pytest.raises(RuntimeError, match="GPU"):
            m([torch.zeros(2, 6, 3, 3)] if isinstance(m, spgan.MultiDenseMLP) else torch.zeros(2, 16 if isinstance(m, spgan.Self_Attn2) else 6, 3, 3))


def test_side_input_weight_images():
    """MultiDenseMLP's weights over the buffer [x_0 x_1 x_2 | y_0 y_1 ..]: zero columns for the side inputs a level does not see yet, and the
    same product as the reference's column order cat[x_0, y_0, x_1, y_1, x_2] in float64"""
    from spgan import edge_conv
    mlps, mlps2 = [8, 5, 7], [6, 3, 2]
    rng = np.random.default_rng(3)
    cin, Ws = mlps2[0], []
    for i, w in enumerate(mlps):
        Ws.append(torch.from_numpy(rng.standard_normal((w, cin, 1, 1)).astype(np.float32)))
        if i < 2:
            cin += w + mlps2[i + 1]
    (Wm, Wx_t, Wback), maps = edge_conv.dense_side_images(Ws, mlps2)
    Cin = sum(mlps2)
    xs = [torch.from_numpy(rng.standard_normal((9, c))) for c in mlps2]
    ys = [torch.from_numpy(rng.standard_normal((9, w))) for w in mlps]
    buf = torch.cat(xs + ys, dim=1)
    pc = xs[0]
    zoff = [0, 8, 13, 20]
    for l in range(3):
        assert Wm[l].shape == (mlps[l], Cin + zoff[l]) and maps[l].numel() == Ws[l].shape[1]
        ref = pc @ Ws[l].reshape(mlps[l], -1).double().t()
        got = buf[:, :Cin + zoff[l]] @ Wm[l].double().t()
        assert float((ref - got).abs().max()) < 1e-12
        unseen = sum(mlps2[:l + 1])
        assert float(Wm[l][:, unseen:Cin].abs().max() if unseen < Cin else 0.0) == 0.0           # side inputs not seen yet
        assert torch.equal(Wm[l][:, maps[l]], Ws[l].reshape(mlps[l], -1))
        if l < 2:
            pc = torch.cat([pc, ys[l], xs[l + 1]], dim=1)
    assert Wx_t.shape == (Cin, sum(mlps)) and torch.equal(Wx_t, torch.cat([w[:, :Cin].t() for w in Wm], dim=1))
    assert [tuple(w.shape) for w in Wback] == [(8, 12), (5, 7)]
    assert torch.equal(Wback[0], torch.cat([Wm[1][:, Cin:Cin + 8].t(), Wm[2][:, Cin:Cin + 8].t()], dim=1))


def test_abi_argument_checks():
    """every new entry returns -22 on null pointers and on sizes outside the domain, before any launch"""
    from spgan import _lib
    lib = _lib.load()
    assert lib.spgan_gc_attn_chunk_points(0) > 0 and lib.spgan_gc_attn_chunk_points(1) > 0 and lib.spgan_gc_attn_chunk_points(2) == 0
    p = 64                                                                 # a non-null address that no check dereferences
    br = _lib.GcBranch(p, p, p, p, p, p)
    half = _lib.GcBranch(p, p, p, None, p, p)
    import ctypes
    r, h = ctypes.byref(br), ctypes.byref(half)
    ok = dict(layout=0, ld=8, B=2, C=8, L=5)
    for bad in (dict(layout=2), dict(layout=-1), dict(B=0), dict(B=65536), dict(C=0), dict(C=1025), dict(L=0), dict(layout=1, ld=7)):
        a = dict(ok, **bad)
        assert lib.spgan_gc_attn_pool_fwd(p, a["layout"], a["ld"], a["B"], a["C"], a["L"], p, p, p, p, p, p, p, None) == -22, bad
        assert lib.spgan_gc_attn_apply_fwd(p, a["layout"], a["ld"], a["B"], a["C"], a["L"], p, p, p, a["ld"], None) == -22, bad
        assert lib.spgan_gc_attn_bwd_reduce(p, a["ld"], p, a["ld"], a["layout"], a["B"], a["C"], a["L"], p, p, p, None) == -22, bad
        assert lib.spgan_gc_attn_bwd_apply(p, a["ld"], p, a["ld"], a["layout"], a["B"], a["C"], a["L"], p, p, p, p, p, p, p, a["ld"], p, None) == -22, bad
    assert lib.spgan_gc_attn_pool_fwd(None, 0, 8, 2, 8, 5, p, p, p, p, p, p, p, None) == -22
    assert lib.spgan_gc_attn_pool_fwd(p, 0, 8, 2, 8, 5, p, p, p, None, p, p, p, None) == -22          # attention pooling without the logits' buffer
    assert lib.spgan_gc_attn_pool_fwd(p, 0, 8, 2, 8, 5, p, p, None, p, p, p, p, None) == -22
    assert lib.spgan_gc_attn_apply_fwd(p, 0, 8, 2, 8, 5, None, None, p, 8, None) == -22                # neither mul nor add
    assert lib.spgan_gc_attn_apply_fwd(p, 0, 8, 2, 8, 5, p, p, None, 8, None) == -22
    assert lib.spgan_gc_attn_apply_fwd(p, 1, 8, 2, 8, 5, p, p, p, 7, None) == -22                      # an output row shorter than C
    assert lib.spgan_gc_attn_bwd_reduce(p, 8, None, 8, 0, 2, 8, 5, p, p, p, None) == -22
    assert lib.spgan_gc_attn_bwd_reduce(p, 8, p, 8, 0, 2, 8, 5, p, None, None, None) == -22           # nothing to compute
    assert lib.spgan_gc_attn_bwd_reduce(p, 8, p, 8, 1, 2, 8, 5, None, p, p, None) == -22              # point-major needs the records
    assert lib.spgan_gc_attn_bwd_apply(p, 8, p, 8, 0, 2, 8, 5, p, None, p, p, p, p, p, 8, p, None) == -22
    assert lib.spgan_gc_attn_bwd_apply(p, 8, p, 8, 0, 2, 8, 5, p, p, p, p, None, p, p, 8, p, None) == -22   # attention pooling without the logits
    assert lib.spgan_gc_attn_bwd_apply(p, 8, p, 8, 1, 2, 8, 5, p, p, p, p, p, p, p, 7, p, None) == -22
    for B, C, O in ((0, 8, 4), (65536, 8, 4), (2, 0, 4), (2, 1025, 4), (2, 8, 0), (2, 8, 1025)):
        assert lib.spgan_gc_attn_channel_fwd(p, B, C, O, r, r, 1e-5, p, p, p, p, None) == -22
        assert lib.spgan_gc_attn_channel_bwd(p, p, p, p, p, B, C, O, r, r, p, p, None) == -22
    assert lib.spgan_gc_attn_channel_fwd(p, 2, 8, 4, None, None, 1e-5, p, p, p, p, None) == -22        # no branch
    assert lib.spgan_gc_attn_channel_fwd(p, 2, 8, 4, h, None, 1e-5, p, p, p, p, None) == -22           # a branch with a missing tensor
    assert lib.spgan_gc_attn_channel_fwd(p, 2, 8, 4, r, None, 1e-5, p, p, None, p, None) == -22        # a branch without its output
    assert lib.spgan_gc_attn_channel_fwd(p, 2, 8, 4, r, r, 0.0, p, p, p, p, None) == -22
    assert lib.spgan_gc_attn_channel_fwd(None, 2, 8, 4, r, r, 1e-5, p, p, p, p, None) == -22
    assert lib.spgan_gc_attn_channel_bwd(p, p, p, p, p, 2, 8, 4, None, None, p, p, None) == -22
    assert lib.spgan_gc_attn_channel_bwd(None, p, p, p, p, 2, 8, 4, r, None, p, p, None) == -22        # the add branch without dadd
    assert lib.spgan_gc_attn_channel_bwd(p, p, None, p, p, 2, 8, 4, None, r, p, p, None) == -22        # the mul branch without mul
    assert lib.spgan_gc_attn_channel_bwd(p, p, p, p, p, 2, 8, 4, r, r, None, p, None) == -22
