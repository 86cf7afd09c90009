"""CPU: the float64 model of the dense family (tests/dense_edge_model.py) against the reference's golden results
(tests/golden/dense_edge.npz), the operand images of spgan.edge_conv against the split of the conv weights, and what the modules
promise without a GPU (state_dict layout, refusals)."""
import os

import numpy as np
import pytest
import torch

import dense_edge_model as dem

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_edge.npz")


@pytest.fixture(scope="module")
def d():
    return np.load(GOLD)


@pytest.mark.parametrize("tag", list(dem.CASES))
def test_model_reproduces_golden_f64(d, tag):
    """rel-L2 1e-10 against the reference's float64 run (stored as the float32 run plus a float32 difference: 1e-14); the gradients
    that are zero in exact arithmetic (dense_edge_model.zero_gradient) are rounding noise in both: absolute 1e-9."""
    x, g = torch.from_numpy(d[tag + "|x"]), torch.from_numpy(d[tag + "|g"])
    idx = torch.from_numpy(d[tag + "|idx"]) if (tag + "|idx") in d.files else None
    res = dem.run(tag, x, g, dem.golden_state_dict(d, tag), idx)
    qs = dem.quantities(d, tag)
    assert "out" in qs and "dx" in qs and len(qs) >= 2 + 7
    for q in qs:
        ref, got = dem.golden_f64(d, tag, q), res[q]
        if q.endswith("num_batches_tracked"):
            assert int(got) == int(ref)
        elif dem.zero_gradient(tag, q):
            assert float(got.abs().max()) < 1e-9 and float(ref.abs().max()) < 1e-9, q
        else:
            e = float((got.double() - ref).norm() / max(float(ref.norm()), 1e-30))
            assert e < 1e-10, (tag, q, e)


def test_golden_conditions(d):
    for tag in dem.EDGE_CASES:
        assert float(d[tag + "|gap"]) > 1e-4
        near = d[tag + "|near_tie_rows"]
        assert near.mean() <= 0.01 and near.shape == (dem.CASES[tag]["B"] * dem.CASES[tag]["N"],)
        idx = d[tag + "|idx"]
        c = dem.CASES[tag]
        assert idx.shape == (c["B"], c["N"], c["k"]) and idx.min() >= 0 and idx.max() < c["N"]
    for tag in dem.CASES:
        x, g, sd = dem.case_tensors(tag, int(d[tag + "|seed"]), d[tag + "|row_salts"] if tag in dem.EDGE_CASES else None)
        assert np.array_equal(d[tag + "|x"], x.numpy()) and np.array_equal(d[tag + "|g"], g.numpy())
        for n, v in sd.items():
            assert np.array_equal(d["%s|param|%s" % (tag, n)], v.numpy()), n


def test_dense_edge_images_match_the_split_of_W():
    """PQ = x Wst^T reproduces W_l . e0 on every edge; Wy / Wback are the y columns and their transposed stacks."""
    from spgan import edge_conv
    C, G, L, M = 5, 6, 3, 9
    gen = torch.Generator().manual_seed(3)
    Ws = [torch.randn(G, 2 * C + l * G, 1, 1, generator=gen, dtype=torch.float64) for l in range(L)]
    Wst, Wst_t, Wy, Wback = edge_conv.dense_edge_images(Ws, C)
    assert tuple(Wst.shape) == (2 * L * G, C) and torch.equal(Wst_t, Wst.t())
    x = torch.randn(M, C, generator=gen, dtype=torch.float64)
    PQ = x @ Wst.t()
    i, j = 2, 7
    e0 = torch.cat([x[j] - x[i], x[i]])
    for l in range(L):
        Wm = Ws[l].reshape(G, -1)
        got = PQ[j, l * G:(l + 1) * G] + PQ[i, (L + l) * G:(L + l + 1) * G]
        assert torch.allclose(got, Wm[:, :2 * C] @ e0, rtol=1e-12, atol=1e-12)
        if l:
            assert torch.equal(Wy[l - 1], Wm[:, 2 * C:])
    for m in range(L - 1):
        assert tuple(Wback[m].shape) == (G, (L - 1 - m) * G)
        for l in range(m + 1, L):
            blk = Wback[m][:, (l - m - 1) * G:(l - m) * G]
            assert torch.equal(blk, Ws[l].reshape(G, -1)[:, 2 * C + m * G:2 * C + (m + 1) * G].t())
    # the gradient of the e0 columns from the stacked gradient: the adjoint of the split
    dWst = torch.randn(2 * L * G, C, generator=gen, dtype=torch.float64)
    for l in range(L):
        dW = edge_conv.dense_edge_unstacked_grad(dWst, l, L, G)
        Wl = torch.randn(G, 2 * C, generator=gen, dtype=torch.float64)
        lhs = (dW * Wl).sum()
        rhs = (dWst[l * G:(l + 1) * G] * Wl[:, :C]).sum() + (dWst[(L + l) * G:(L + l + 1) * G] * (Wl[:, C:] - Wl[:, :C])).sum()
        assert torch.allclose(lhs, rhs, rtol=1e-12)
    # cached per weight set, rebuilt after an in-place write
    assert edge_conv.dense_edge_images(Ws, C)[0] is Wst
    Ws[0].mul_(2.0)
    assert edge_conv.dense_edge_images(Ws, C)[0] is not Wst


def test_dense_rows_images():
    from spgan import edge_conv
    Cin, widths = 4, [3, 5, 4]
    gen = torch.Generator().manual_seed(4)
    Ws, cin = [], Cin
    for w in widths:
        Ws.append(torch.randn(w, cin, 1, generator=gen, dtype=torch.float64))
        cin += w
    Wm, Wx_t, Wback = edge_conv.dense_rows_images(Ws, Cin)
    assert tuple(Wx_t.shape) == (Cin, sum(widths))
    off = [0, 3, 8, 12]
    for l, w in enumerate(Ws):
        assert torch.equal(Wm[l], w.reshape(w.shape[0], -1))
        assert torch.equal(Wx_t[:, off[l]:off[l + 1]], Wm[l][:, :Cin].t())
    assert torch.equal(Wback[0], torch.cat([Wm[1][:, Cin:Cin + 3].t(), Wm[2][:, Cin:Cin + 3].t()], dim=1))
    assert torch.equal(Wback[1], Wm[2][:, Cin + 3:Cin + 8].t())


@pytest.mark.parametrize("tag", list(dem.CASES))
def test_state_dict_layout_and_strict_loading(d, tag):
    import spgan
    m = dem.build_module(spgan, tag)
    gold = dem.golden_state_dict(d, tag)
    own = m.state_dict()
    assert sorted(own) == sorted(gold)
    for n, v in own.items():
        assert tuple(v.shape) == tuple(gold[n].shape) and v.dtype == gold[n].dtype, n
    m.load_state_dict(gold, strict=True)
    back = {n: v.clone() for n, v in m.state_dict().items()}
    assert all(torch.equal(back[n], gold[n]) for n in gold)
    if dem.kind_of(tag) == "edge":
        assert len(own) == 7 * dem.CASES[tag]["L"] and m.last_idx is None


def test_constructor_defaults_and_refusals():
    import spgan
    m = spgan.DenseEdgeModule()
    assert m.k == 20 and len(m.dense_modules) == 4 and tuple(m.dense_modules[3][0].weight.shape) == (64, 64 + 3 * 64, 1, 1)
    assert isinstance(m.dense_modules[0][2], torch.nn.LeakyReLU) and m.dense_modules[0][2].negative_slope == 0.2
    r = spgan.DenseModule1D()
    assert [tuple(s[0].weight.shape) for s in r.dense_modules] == [(64, 64, 1), (64, 128, 1), (64, 192, 1)]
    r = spgan.DenseModule1D(12, 3, 20)
    assert [tuple(s[0].weight.shape) for s in r.dense_modules] == [(20, 12, 1), (20, 32, 1), (12, 52, 1)]
    a = spgan.Dense_Attn(16, activation="anything")
    assert isinstance(a.atten, spgan.Self_Attn) and isinstance(a.dense, spgan.DenseModule1D) and len(a.dense.dense_modules) == 3
    for k in (0, 1, 33, 2.0):
        with pytest.raises(ValueError, match="2..32"):
            spgan.DenseEdgeModule(6, 3, 16, k)
    with pytest.raises(ValueError):
        spgan.DenseEdgeModule(7, 3, 16, 5)                                    # input_channel = 2*C is even
    with pytest.raises(ValueError):
        spgan.DenseEdgeModule(6, 0, 16, 5)
    with pytest.raises(RuntimeError, match="GPU"):
        spgan.DenseEdgeModule(6, 3, 16, 5)(torch.zeros(2, 3, 64))
    with pytest.raises(RuntimeError, match="GPU"):
        spgan.DenseModule1D(12, 3, 20)(torch.zeros(2, 12, 70))
    with pytest.raises(RuntimeError, match="GPU"):
        spgan.Dense_Attn(16)(torch.zeros(2, 16, 48))
    with pytest.raises(RuntimeError, match="GPU"):
        spgan.get_graph_feature(torch.zeros(2, 3, 64), 5)


def test_launchers_refuse_before_any_launch():
    """status codes on bad arguments (no GPU needed), and the tile of the records"""
    from spgan import _lib
    lib = _lib.load()
    assert lib.spgan_edge_dense_tile_rows() == 128
    one = 1                                                                    # any non-null address: nothing is launched
    assert lib.spgan_edge_dense_level(None, 0, 0, None, None, 0.2, None, 0, None, None, 0, 0, None, 1, 4, 4, 0, None, 4, None, None) == -22     # no Y
    assert lib.spgan_edge_dense_level(None, 0, 0, None, None, 0.2, None, 0, None, None, 0, 0, None, 1, 4, 4, 0, one, 4, None, None) == -22      # nothing to add
    assert lib.spgan_edge_dense_level(one, 8, 9, None, None, 0.2, one, 8, None, None, 0, 0, None, 1, 4, 4, 8, one, 4, None, None) == -22        # raw_cols > K
    assert lib.spgan_edge_dense_level(one, 8, 2, None, None, 0.2, one, 8, None, None, 0, 0, None, 1, 4, 4, 8, one, 4, None, None) == -22        # no scale
    assert lib.spgan_edge_dense_level(one, 8, 8, None, None, 0.2, one, 8, None, one, 8, 4, one, 3, 4, 4, 8, one, 4, None, None) == -22          # M % k
    assert lib.spgan_edge_dense_level(one, 8, 8, None, None, 0.2, one, 8, None, one, 8, 2, one, 2, 4, 4, 8, one, 4, None, None) == -22          # Q overlaps P
    assert lib.spgan_edge_dense_level(one, 4, 4, None, None, 0.2, one, 8, None, None, 0, 0, None, 1, 4, 4, 8, one, 4, None, None) == -22        # lda < K
    assert lib.spgan_edge_dense_scatter(one, 4, one, one, 4, 0, 4, one, 8, None) == -22
    assert lib.spgan_edge_dense_scatter(one, 4, one, one, 4, 2, 4, one, 7, None) == -22
    assert lib.spgan_edge_dense_bn_apply(one, 4, one, 3, 4, 4, one, one, None, one, 5, one, 4, None) == -22
    assert lib.spgan_edge_dense_bn_apply(one, 4, one, 4, 4, 4, one, one, None, one, 0, one, 4, None) == -22
