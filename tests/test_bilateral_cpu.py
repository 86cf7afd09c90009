"""CPU: the decomposed bilateral upsampling edge convolution (tests/bilateral_model.py: upsample_edgeConv's rank-window products, deform_edgeConv's
weight branch with 2C output channels, their element-wise product in front of conv2's taps k..2k-1) against the vectors captured from the
reference's bilateral_upsample_edgeConv (golden bilateral.npz); the written-out backward of the stored-operand launchers against autograd;
the operand images (spgan.edge_conv.bilateral_images) against the reference's transpose / view chain evaluated on an index tensor, and
their cache; the module's parameter layout against the reference's.

Tolerances, as tests/test_deform_xyz_cpu.py.  float64: the model runs in float64 on float32 inputs, the golden holds the reference's float64
run on the same inputs and graph (its distance from the float32 run stored with 10 mantissa bits: 1e-10 of the value): 1e-9 rel-L2.
float32: within 5 x the reference's own float32-vs-float64 distance of that quantity.  Every conv bias sits in front of a train-mode
BatchNorm: its gradient is zero up to rounding in both, compared absolutely (1e-12 in float64; 2e-3 in float32), in the train-mode cases."""
import numpy as np
import pytest
import torch

import bilateral_model as bm
import upsample_model as um
from helpers import golden

TAGS = list(bm.CASES)


@pytest.fixture(scope="module")
def d():
    return golden("bilateral.npz")


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _module(d, tag):
    """spgan.bilateral_upsample_edgeConv of the case, holding the reference's checkpoint (strict loading)"""
    import spgan
    c = bm.CASES[tag]
    m = spgan.bilateral_upsample_edgeConv(c["Fin"], c["Fout"], c["k"], -1, softmax=c["softmax"])
    m.load_state_dict(bm.golden_state_dict(d, tag), strict=True)
    return m


@pytest.fixture(scope="module")
def runs(d):
    """The model's float64 and float32 results per case, computed once, on the parameters and buffers as the module holds them after loading
    the reference's checkpoint"""
    out = {}
    for tag in TAGS:
        c = bm.CASES[tag]
        for dt in (torch.float64, torch.float32):
            sd = {k: v.to(dt) if v.dtype.is_floating_point else v for k, v in _module(d, tag).state_dict().items()}
            assert tuple(sd) == bm.STATE_KEYS
            t = lambda n: torch.from_numpy(d[tag + n]).to(dt)
            out[tag, dt] = bm.run(t("|x"), t("|pc"), torch.from_numpy(d[tag + "|idx"]), t("|g"), c["k"], sd, c["train"], c["softmax"])
    return out


def _stored(d, tag):
    return {k[len(tag) + 1:].rsplit("|", 1)[0] for k in d.files if k.startswith(tag + "|") and k.endswith(("|full", "|samples"))
            and "|d64|" not in k and "num_batches_tracked" not in k}


@pytest.mark.parametrize("tag", TAGS)
def test_model_matches_reference_float64(d, runs, tag):
    got = runs[tag, torch.float64]
    assert set(got) == _stored(d, tag)                                          # every stored quantity
    for q, v in got.items():
        ref64, mine = bm.golden_pair(d, tag, q, v)
        err = _rel(mine, ref64)
        print("%s %s: model vs reference float64 rel-L2 %.3e" % (tag, q, err))
        if (q[5:] in bm.ZERO_GRAD_BIASES and bm.CASES[tag]["train"]) or float(ref64.abs().max()) == 0.0:
            assert float((mine - ref64).abs().max()) < 1e-12, (tag, q)
        else:
            assert err < 1e-9, (tag, q, err)


@pytest.mark.parametrize("tag", TAGS)
def test_model_float32_within_reference_noise(d, runs, tag):
    for q, v in runs[tag, torch.float32].items():
        ref64, mine = bm.golden_pair(d, tag, q, v)
        if q[5:] in bm.ZERO_GRAD_BIASES and bm.CASES[tag]["train"]:
            assert float((mine.double() - ref64).abs().max()) <= 2e-3, (tag, q)
            continue
        err, noise = _rel(mine, ref64), bm.noise(d, tag, q)
        print("%s %s: float32 model vs reference float64 %.3e (reference float32: %.3e)" % (tag, q, err, noise))
        assert err <= max(5.0 * noise, 1e-12), (tag, q, err, noise)


def test_golden_conditions(d):
    assert tuple(str(k) for k in d["state_keys"]) == bm.STATE_KEYS and len(bm.STATE_KEYS) == 42
    quantities = ["out", "dx", "dpc"] + ["grad|" + n for n in bm.STATE_KEYS if n.endswith((".weight", ".bias"))] + \
        ["buf|" + n for n in bm.BUFFERS if "num_batches" not in n]
    assert sorted(str(n) for n in d["noise_keys"]) == sorted(quantities)
    for tag in TAGS:
        c = bm.CASES[tag]
        assert d[tag + "|near_tie_rows"].mean() <= 0.01
        assert tuple(d[tag + "|x"].shape) == (c["B"], c["Fin"], c["N"]) and tuple(d[tag + "|pc"].shape) == (c["B"], 3, c["N"])
        assert tuple(d[tag + "|g"].shape) == (c["B"], c["Fout"], 2 * c["N"])
        assert tuple(d[tag + "|idx"].shape) == (c["B"], c["N"] * c["k"]) and d[tag + "|noise"].shape == d["noise_keys"].shape
        m = _module(d, tag)                                                     # the capture and the layer agree on every shape
        assert tuple(m.state_dict()) == bm.STATE_KEYS
        assert tuple(m.conv2.conv.weight.shape) == (2 * c["Fout"], 2 * c["Fin"], 1, 2 * c["k"])
        assert (m.k, m.Fin, m.Fout, m.softmax, m.num, m.training) == (c["k"], c["Fin"], c["Fout"], c["softmax"], -1, True)
        for conv in bm.CONVS:
            bf = torch.from_numpy(bm.param(d, tag, conv + ".weight"))
            assert torch.equal(bf.bfloat16().float(), bf), conv                 # what the 16-bit storage relies on
    assert np.any(d["b|dpc|full"]) and np.any(d["b|grad|conv_xyz.0.weight|full"])
    for n in bm.BUFFERS:                                                        # eval mode: the reference leaves its buffers alone
        assert np.array_equal(d["e|buf|%s|full" % n], bm.param(d, "e", n)), n


# ---------------------------------------------------------------- the launchers' written-out backward against autograd
@pytest.mark.parametrize("soft", [True, False])
@pytest.mark.parametrize("k,F1", [(2, 3), (4, 6), (10, 5)])
def test_stored_backward_against_autograd(k, F1, soft):
    g = torch.Generator().manual_seed(k * 10 + F1)
    M, O = 7, 4
    U = torch.randn(M, k, F1, generator=g, dtype=torch.float64).requires_grad_(True)
    z3 = torch.randn(M, k, F1, generator=g, dtype=torch.float64).requires_grad_(True)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    sc1, sh1, sc3, sh3 = r(2 * F1), r(2 * F1) * 0.3, r(F1), r(F1) * 0.3
    mean1, inv1, mean3, inv3 = r(2 * F1), r(2 * F1).abs() + 0.5, r(F1), r(F1).abs() + 0.5
    W2i = r(O, k * F1).requires_grad_(True)
    dy = r(M, O)
    y = bm.stored_gemm(U, sc1, sh1, z3, sc3, sh3, soft, W2i)
    (y * dy).sum().backward()
    gU, su, g3, s3 = bm.stored_dgrad(dy, W2i.detach(), U.detach(), sc1, sh1, mean1, inv1, z3.detach(), sc3, sh3, mean3, inv3, soft)
    par = torch.arange(k) % 2
    # gU and g3 are the gradients with respect to the BatchNorm outputs: the affine's scale is the chain to U and z3
    assert _rel(gU * sc1.view(2, F1)[par], U.grad) < 1e-12 and _rel(g3 * sc3, z3.grad) < 1e-12
    assert _rel(bm.stored_wgrad(U.detach(), sc1, sh1, z3.detach(), sc3, sh3, soft, dy), W2i.grad) < 1e-12
    uhat = (U.detach() - mean1.view(2, F1)[par]) * inv1.view(2, F1)[par]
    for h in range(2):
        assert _rel(su[h * F1:(h + 1) * F1], gU[:, h::2].sum(dim=(0, 1))) < 1e-12
        assert _rel(su[2 * F1 + h * F1:2 * F1 + (h + 1) * F1], (gU * uhat)[:, h::2].sum(dim=(0, 1))) < 1e-12
    assert _rel(s3[:F1], g3.sum(dim=(0, 1))) < 1e-12 and _rel(s3[F1:], (g3 * (z3.detach() - mean3) * inv3).sum(dim=(0, 1))) < 1e-12


# ---------------------------------------------------------------- the operand images
def _ids(shape, start=0):
    n = int(np.prod(shape))
    return (torch.arange(n, dtype=torch.float32) + start).reshape(shape).clone()


IMG_SHAPES = lambda C, k, F2: [(4 * C, 2 * C, 1, k // 2 + 1), (3, 2 * C, 1, 1), (3, 6, 1, 1), (5, 3, 1, 1), (2 * C, 5, 1, 1), (F2, 2 * C, 1, 2 * k)]


def _weights(C, k, F2, start=0):
    return [_ids(s, start + 100000 * i) for i, s in enumerate(IMG_SHAPES(C, k, F2))]


@pytest.fixture
def cache():
    from spgan import edge_conv
    held = {name: dict(c) for name, c in edge_conv._IMAGES.items()}
    for c in edge_conv._IMAGES.values():
        c.clear()
    yield edge_conv._IMAGES["bilateral"]
    for name, c in edge_conv._IMAGES.items():
        c.clear()
        c.update(held[name])


@pytest.mark.parametrize("C,k", [(2, 2), (2, 4), (3, 10), (1, 28)])
def test_images_against_the_reference_view_chain(cache, C, k):
    """The reference multiplies element (c', j) of its reshuffled [2C, k] block by the weight of rank j and feeds it to conv2's tap k + j of
    channel c'.  Here the same source element (o, t) of inte_conv_hk's output sits at row r', channel c' of the [k, 2C] block the kernels
    read: the weight branch's rank at r' and the tap V2i carries in column r'*2C + c' must be that j."""
    from spgan import edge_conv
    T, F2 = k // 2, 2
    ws = _weights(C, k, F2)
    W1, V = ws[0], ws[5]
    img = edge_conv.bilateral_images(*ws, C, k)
    Wc1, Wd1, Wd1t, Vc, Vd, Vdt, Vct, V2i, V2it, Wst_f, Wst_x, Wst_xt, Wcat_t, Wm2, Wm2t, Wm3, Wm3t = img
    # the reference's chain on the ids o*T + t of one point's [4C, T] block  (B = N = 1)
    src = torch.arange(4 * C * T).view(1, 4 * C, 1, T)
    chain = src.transpose(2, 1).contiguous().view(1, 1, 2 * C, 2, T).contiguous().view(1, 1, 2 * C, k).permute(0, 2, 1, 3)[0, :, 0, :]      # [2C, k]
    # the same ids as the layer stores them: rows (t), channels in the order of the permuted weight, read as [k, 2C]
    rows = torch.arange(4 * C * T).view(4 * C, T).t()                                   # rows[t, o] = o*T + t: what the reference's order gives
    ours = edge_conv.parity_major(rows, 1).reshape(k, 2 * C)
    ranks = edge_conv.paired_ranks(torch.arange(k).view(1, k))[0]
    for f in range(F2):
        for rp in range(k):
            for cp in range(2 * C):
                fid, c2, _, tap = np.unravel_index(int(V2i[f, rp * 2 * C + cp]) - 500000, V.shape)
                j = tap - k
                assert fid == f and c2 == cp and 0 <= j < k
                assert int(chain[cp, j]) == int(ours[rp, cp]) and int(ranks[rp]) == j, (f, rp, cp)
    # the interpolation's images are upsample_images' with permuted output channels; the rest as the siblings build them
    uWc1, uWd1, uVc, uVd, _ = um.images(W1, V, C, k)
    assert torch.equal(Wc1, edge_conv.parity_major(uWc1)) and torch.equal(Wd1, edge_conv.parity_major(uWd1)) and torch.equal(Wd1t, Wd1.t())
    assert torch.equal(edge_conv.channel_major(edge_conv.parity_major(W1)), W1)
    assert torch.equal(Vc, uVc) and torch.equal(Vd, uVd) and torch.equal(Vdt, uVd.t()) and torch.equal(Vct, uVc.t()) and torch.equal(V2it, V2i.t())
    assert torch.equal(Wst_f, edge_conv.stacked(ws[1])) and torch.equal(Wst_x, edge_conv.stacked(ws[2])) and torch.equal(Wst_xt, Wst_x.t())
    assert torch.equal(Wcat_t, torch.cat([Wc1, Wst_f]).t())
    assert torch.equal(Wm2, ws[3][:, :, 0, 0]) and torch.equal(Wm2t, Wm2.t()) and torch.equal(Wm3, ws[4][:, :, 0, 0]) and torch.equal(Wm3t, Wm3.t())
    assert all(t.is_contiguous() for t in img)


def _fresh(new, old):
    assert new is not old and all(a is not b for a, b in zip(new, old))


def test_images_cache(cache):
    """The staleness rule of the sibling images (tests/test_edge_images_cpu.py): a hit returns the very tensors; an in-place write or an
    optimiser epoch on any of the six weights, or another (C, k) at the same addresses, rebuilds; the dictionary holds at most 64 entries."""
    from spgan import edge_conv, ops
    C, k, F2 = 2, 4, 2
    call = lambda ws, C_=C, k_=k: edge_conv.bilateral_images(*ws, C_, k_)
    ws = _weights(C, k, F2)
    img = call(ws)
    again = call(ws)
    assert again is img and all(a is b for a, b in zip(again, img)) and len(cache) == 1
    for i in range(6):
        ws = _weights(C, k, F2)
        old = call(ws)
        ws[i].view(-1)[1:3].add_(7.0)
        new = call(ws)
        _fresh(new, old)
        assert torch.equal(new[7], call([w.clone() for w in ws])[7])
        old = new
        versions = [w._version for w in ws]
        ws[i].data.copy_(_ids(ws[i].shape, 5 + i))
        assert [w._version for w in ws] == versions
        ops.bump_weights_epoch(ws[i])
        new = call(ws)
        _fresh(new, old)
        assert torch.equal(new[0], call([w.clone() for w in ws])[0]) and torch.equal(new[7], call([w.clone() for w in ws])[7])
    # k = 2 reads the same conv2 storage differently: (C, k) is part of the key
    ws = _weights(C, 4, F2)
    a = call(ws)
    small = [ws[0].view(-1)[:4 * C * 2 * C * 2].view(4 * C, 2 * C, 1, 2)] + ws[1:5] + [ws[5].view(-1)[:F2 * 2 * C * 4].view(F2, 2 * C, 1, 4)]
    b = call(small, C, 2)
    _fresh(b, a)
    assert tuple(b[7].shape) == (F2, 2 * 2 * C)
    cache.clear()
    keep = []
    for n in range(65):
        keep.append(_weights(C, k, F2, start=n))
        img = call(keep[-1])
        assert len(cache) <= 64
    assert call(keep[-1]) is img


def test_module_layout_and_refusals():
    import spgan
    m = spgan.bilateral_upsample_edgeConv(3, 8, 4, 7, softmax=False)
    assert [n for n, _ in m.named_children()] == ["conv2", "conv_xyz", "conv_fea", "conv_all", "inte_conv_hk"]
    assert len(m.state_dict()) == 42 and (m.k, m.Fin, m.Fout, m.softmax, m.num, m.last_idx) == (4, 3, 8, False, 7, None)
    for k in (3, 0, 30, -2):
        with pytest.raises(ValueError, match="k=%d" % k):
            spgan.bilateral_upsample_edgeConv(4, 4, k, 1)
    with pytest.raises(RuntimeError, match="no CPU"):
        m(torch.zeros(1, 3, 8), torch.zeros(1, 3, 8))
