"""CPU: the decomposed weighted full-rank edge convolution (tests/deform_feat_model.py: two per-point GEMMs, gathered rows, the weight MLP
over edge rows, the softmax normaliser per (point, channel), a product with K = k*Fin over h*s) against the vectors captured from the
reference's deform_edgeConv_feat (golden deform_feat.npz); the written-out backward of the new launchers against autograd; the module's
parameter layout against the reference's; the new entry points' argument checks.

Tolerances.  float64: the model runs in float64 on float32 inputs, the golden holds the reference's float64 run on the same inputs and
graph (its distance from the float32 run stored with 10 mantissa bits: 1e-10 of the value), so the two differ by float64 rounding and
that storage alone: 1e-9 rel-L2.  float32: within 5 x the reference's own float32-vs-float64 distance of that quantity (`tag|noise|q`).
Every conv bias sits in front of a train-mode BatchNorm: its gradient is zero up to rounding in both, compared absolutely (1e-12 in
float64; 2e-3 in float32, the ZERO_GRAD_BIASES rule), in the train-mode cases.  Case d (k = 1): the softmax weight is 1, every conv_fea
gradient is an exact zero in the reference and in the model."""
import numpy as np
import pytest
import torch

import deform_feat_model as fm
from helpers import golden

TAGS = list(fm.CASES)


@pytest.fixture(scope="module")
def d():
    return golden("deform_feat.npz")


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _module(d, tag):
    """spgan.deform_edgeConv_feat of the case, holding the reference's checkpoint (strict loading)"""
    import spgan
    c = fm.CASES[tag]
    m = spgan.deform_edgeConv_feat(c["Fin"], c["Fout"], c["k"], softmax=c["softmax"])
    m.load_state_dict(fm.golden_state_dict(d, tag), strict=True)
    return m


def _model(d, tag, dt):
    """The model on the parameters and buffers as the module holds them after loading the reference's checkpoint: what the golden checks
    is the layer's own layout, not a list of names kept beside it."""
    c = fm.CASES[tag]
    sd = {k: v.to(dt) if v.dtype.is_floating_point else v for k, v in _module(d, tag).state_dict().items()}
    assert tuple(sd) == fm.STATE_KEYS
    return fm.run(torch.from_numpy(d[tag + "|x"]).to(dt), torch.from_numpy(d[tag + "|idx"]), torch.from_numpy(d[tag + "|g"]).to(dt), c["k"], sd,
                  c["train"], c["softmax"])


def _stored(d, tag):
    return {k[len(tag) + 1:].rsplit("|", 1)[0] for k in d.files if k.startswith(tag + "|") and k.endswith(("|full", "|samples"))
            and "|d64|" not in k and "num_batches_tracked" not in k}


@pytest.mark.parametrize("tag", TAGS)
def test_model_matches_reference_float64(d, tag):
    got = _model(d, tag, torch.float64)
    assert set(got) == _stored(d, tag)                                          # every stored quantity
    for q, v in got.items():
        ref64, mine = fm.golden_pair(d, tag, q, v)
        err = _rel(mine, ref64)
        print("%s %s: model vs reference float64 rel-L2 %.3e" % (tag, q, err))
        if (q[5:] in fm.ZERO_GRAD_BIASES and fm.CASES[tag]["train"]) or float(ref64.abs().max()) == 0.0:
            assert float((mine - ref64).abs().max()) < 1e-12, (tag, q)
        else:
            assert err < 1e-9, (tag, q, err)


@pytest.mark.parametrize("tag", TAGS)
def test_model_float32_within_reference_noise(d, tag):
    got = _model(d, tag, torch.float32)
    for q, v in got.items():
        ref64, mine = fm.golden_pair(d, tag, q, v)
        if q[5:] in fm.ZERO_GRAD_BIASES and fm.CASES[tag]["train"]:
            assert float((mine.double() - ref64).abs().max()) <= 2e-3, (tag, q)
            continue
        err, noise = _rel(mine, ref64), float(d["%s|noise|%s" % (tag, q)])
        print("%s %s: float32 model vs reference float64 %.3e (reference float32: %.3e)" % (tag, q, err, noise))
        assert err <= max(5.0 * noise, 1e-12), (tag, q, err, noise)


def test_golden_conditions(d):
    assert tuple(str(k) for k in d["state_keys"]) == fm.STATE_KEYS
    for tag in TAGS:
        c = fm.CASES[tag]
        assert d[tag + "|near_tie_rows"].mean() <= 0.01
        assert tuple(d[tag + "|x"].shape) == (c["B"], c["Fin"], c["N"]) and tuple(d[tag + "|idx"].shape) == (c["B"], c["N"] * c["k"])
        m = _module(d, tag)                                                     # the capture and the layer agree on every shape
        assert tuple(m.conv2.conv.weight.shape) == (c["Fout"], c["Fin"], 1, c["k"]) == tuple(d[tag + "|param|conv2.conv.weight"].shape)
        assert (m.k, m.Fin, m.Fout, m.softmax, m.training) == (c["k"], c["Fin"], c["Fout"], c["softmax"], True)
    for n in fm.STATE_KEYS:                                                     # case d: conv_fea's gradients vanish
        if n.startswith("conv_fea") and n.endswith((".weight", ".bias")):
            assert not np.any(d["d|grad|%s|full" % n]), n
    assert not np.array_equal(d["e|param|conv_fea.7.running_mean"], np.zeros(32, np.float32))
    for n in fm.BUFFERS:                                                        # eval mode: the reference leaves its buffers alone
        assert np.array_equal(d["e|buf|%s|full" % n], d["e|param|" + n]), n


@pytest.mark.parametrize("soft", [True, False])
def test_written_out_backward_matches_autograd(soft):
    """fm.wdgrad / fm.wwgrad (what the GPU launchers are compared with) against autograd over fm.wgemm, float64: the yardstick of the
    wrappers in spgan.edge_weight, whose argument order the model's functions follow."""
    import inspect
    import spgan
    ew = spgan.edge_weight
    assert list(inspect.signature(ew.edge_weight_dgrad).parameters)[:14] == ["dy", "W2t", "PQ", "idx", "scale1", "shift1", "mean1", "invstd1", "z3",
                                                                           "scale3", "shift3", "mean3", "invstd3", "norm"]
    assert list(inspect.signature(ew.edge_weight_wgrad).parameters)[:9] == ["PQ", "idx", "scale1", "shift1", "z3", "scale3", "shift3", "norm", "dy"]
    g = torch.Generator().manual_seed(5)
    M, k, F, O = 23, 4, 6, 5
    PQ = torch.randn(M, 2 * F, generator=g, dtype=torch.float64)
    gidx = torch.randint(0, M, (M, k), generator=g)
    z3 = torch.randn(M, k, F, generator=g, dtype=torch.float64)
    sc1, sh1, sc3, sh3 = (torch.randn(F, generator=g, dtype=torch.float64) for _ in range(4))
    mean1, inv1, mean3, inv3 = (torch.rand(F, generator=g, dtype=torch.float64) + 0.5 for _ in range(4))
    W = torch.randn(O, k * F, generator=g, dtype=torch.float64).requires_grad_(True)
    dy = torch.randn(M, O, generator=g, dtype=torch.float64)
    # autograd reaches the two pre-activation BatchNorm outputs through explicit leaves
    u = fm.pre_norm(PQ, gidx)
    ah = (u * sc1 + sh1).requires_grad_(True)
    a3 = (z3 * sc3 + sh3).requires_grad_(True)
    a3l = fm.lrelu(a3)
    s = torch.softmax(a3l, dim=1) if soft else a3l
    y = (fm.lrelu(ah) * s).reshape(M, -1) @ W.t()
    (y * dy).sum().backward()
    assert _rel(y.detach(), fm.wgemm(PQ, gidx, sc1, sh1, z3, sc3, sh3, soft, W.detach())) < 1e-12
    du, su, g3, s3 = fm.wdgrad(dy, W.detach(), PQ, gidx, sc1, sh1, mean1, inv1, z3, sc3, sh3, mean3, inv3, soft)
    assert _rel(du, ah.grad) < 1e-12 and _rel(g3, a3.grad) < 1e-12
    assert _rel(su, torch.cat([ah.grad.sum(dim=(0, 1)), (ah.grad * (u - mean1) * inv1).sum(dim=(0, 1))])) < 1e-12
    assert _rel(s3, torch.cat([a3.grad.sum(dim=(0, 1)), (a3.grad * (z3 - mean3) * inv3).sum(dim=(0, 1))])) < 1e-12
    assert _rel(fm.wwgrad(PQ, gidx, sc1, sh1, z3, sc3, sh3, soft, dy), W.grad) < 1e-12
    wmax, wrs = fm.norm(z3, sc3, sh3)
    assert _rel(torch.exp(a3l.detach() - wmax[:, None]) * wrs[:, None], torch.softmax(a3l.detach(), dim=1)) < 1e-12


def test_state_dict_layout_and_strict_loading(d):
    import spgan
    for tag in TAGS:
        c = fm.CASES[tag]
        m = spgan.deform_edgeConv_feat(c["Fin"], c["Fout"], c["k"], softmax=c["softmax"])
        sd = m.state_dict()
        assert tuple(sd.keys()) == tuple(str(k) for k in d["state_keys"])       # the reference's own list, in its order
        for n in fm.STATE_KEYS:
            assert tuple(sd[n].shape) == tuple(d["%s|param|%s" % (tag, n)].shape), n
        m.load_state_dict(fm.golden_state_dict(d, tag), strict=True)
        assert (m.k, m.Fin, m.Fout, m.softmax) == (c["k"], c["Fin"], c["Fout"], c["softmax"])
    assert [n for n, _ in m.named_children()] == ["conv2", "conv_fea", "inte_conv_hk"]
    assert isinstance(m.conv2, spgan.conv2dbr) and m.conv_fea[8].negative_slope == 0.01 and m.inte_conv_hk[2].negative_slope == 0.01
    assert "deform_edgeConv_feat" in spgan.__all__ and spgan.deform_edgeConv_feat(4, 4, 3).softmax is True
    with pytest.raises(RuntimeError):                                           # a deform_edgeConv_simple checkpoint does not fit
        spgan.deform_edgeConv_feat(16, 32, 10).load_state_dict(spgan.deform_edgeConv_simple(16, 32, 10).state_dict(), strict=True)


def test_constructor_and_cpu_refusal():
    import spgan
    for k in (0, 33):
        with pytest.raises(ValueError, match="k=%d" % k):
            spgan.deform_edgeConv_feat(4, 4, k)
    with pytest.raises(ValueError, match="Fin=0"):
        spgan.deform_edgeConv_feat(0, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU"):
        spgan.deform_edgeConv_feat(3, 8, 4)(torch.zeros(2, 3, 16))


def test_entry_points_declared():
    import os
    from spgan import _lib
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "spgan_hip.h")).read()
    lib = _lib.load()
    for n in ("gather", "norm", "gemm", "wgrad", "dgrad"):
        assert "int spgan_edge_weight_%s(" % n in header, n
        assert callable(getattr(lib, "spgan_edge_weight_" + n))


def test_launchers_reject_bad_sizes_without_gpu():
    from spgan import _lib
    lib = _lib.load()
    p = 16                                                                      # any non-null address: the checks come before every launch
    #                                   PQ ld idx M  k  F  Z  stream
    assert lib.spgan_edge_weight_gather(None, 8, p, 8, 4, 4, p, None) == -22
    assert lib.spgan_edge_weight_gather(p, 8, p, 8, 33, 4, p, None) == -22                                               # k > 32
    assert lib.spgan_edge_weight_gather(p, 7, p, 8, 4, 4, p, None) == -22                                                # ld < 2*F
    #                                 z3 M  k  F1 sc sh slope wmax wrs
    assert lib.spgan_edge_weight_norm(None, 8, 4, 4, p, p, 0.01, p, p, None) == -22
    assert lib.spgan_edge_weight_norm(p, 8, 33, 4, p, p, 0.01, p, p, None) == -22
    assert lib.spgan_edge_weight_norm(p, 8, 4, 4, p, p, 0.01, p, None, None) == -22
    #                                 PQ ld idx M  k  F1 sc1 sh1 slope z3 sc3 sh3 wmax wrs W2i ldw b2   O  Y ldy part stream
    assert lib.spgan_edge_weight_gemm(None, 8, None, 8, 4, 4, None, None, 0.01, None, None, None, None, None, None, 16, None, 8, None, 8, None, None) == -22
    assert lib.spgan_edge_weight_gemm(p, 8, p, 8, 33, 4, p, p, 0.01, p, p, p, p, p, p, 132, None, 8, p, 8, None, None) == -22      # k > 32
    assert lib.spgan_edge_weight_gemm(p, 7, p, 8, 4, 4, p, p, 0.01, p, p, p, p, p, p, 16, None, 8, p, 8, None, None) == -22        # ld < 2*F1
    assert lib.spgan_edge_weight_gemm(p, 8, p, 8, 4, 4, p, p, 0.01, p, p, p, p, p, p, 15, None, 8, p, 8, None, None) == -22        # ldw < k*F1
    assert lib.spgan_edge_weight_gemm(p, 8, p, 8, 4, 4, p, p, 0.01, p, p, p, p, p, p, 16, None, 8, p, 7, None, None) == -22        # ldy < O
    assert lib.spgan_edge_weight_gemm(p, 8, p, 8, 4, 4, p, p, 0.01, None, p, p, p, p, p, 16, None, 8, p, 8, None, None) == -22     # no z3
    assert lib.spgan_edge_weight_gemm(p, 8, p, 8, 4, 4, p, p, 0.01, p, p, p, p, None, p, 16, None, 8, p, 8, None, None) == -22     # wmax without wrs
    #                                  PQ ld idx M  k  F1 sc1 sh1 slope z3 sc3 sh3 wmax wrs dY ldg O dW lddw ws ws_bytes
    assert lib.spgan_edge_weight_wgrad(p, 8, p, 8, 4, 4, p, p, 0.01, p, p, p, p, p, p, 8, 8, p, 16, p, 4, None) == -22             # workspace too small
    assert lib.spgan_edge_weight_wgrad(p, 8, p, 8, 4, 4, p, p, 0.01, p, p, p, p, p, p, 7, 8, p, 16, p, 1 << 30, None) == -22       # ldg < O
    assert lib.spgan_edge_weight_wgrad(p, 8, p, 8, 4, 4, p, p, 0.01, p, p, p, p, p, p, 8, 8, p, 15, p, 1 << 30, None) == -22       # lddw < k*F1
    assert lib.spgan_edge_weight_wgrad(p, 8, p, 8, 33, 4, p, p, 0.01, p, p, p, p, p, p, 8, 8, p, 132, p, 1 << 30, None) == -22     # k > 32
    assert lib.spgan_edge_weight_wgrad(None, 8, p, 8, 4, 4, p, p, 0.01, p, p, p, p, p, p, 8, 8, p, 16, p, 1 << 30, None) == -22
    #                                  dY ldg W2t ldwt PQ ld idx M k F1 O sc1 sh1 mu1 inv1 slope z3 sc3 sh3 mu3 inv3 wmax wrs dU G3 pu p3
    ok = [p, 8, p, 8, p, 8, p, 8, 4, 4, 8, p, p, p, p, 0.01, p, p, p, p, p, p, p, p, 32, p, p, None]
    for pos, bad in ((1, 7), (3, 7), (5, 7), (8, 33), (0, None), (16, None), (19, None), (22, None), (23, None), (24, p), (25, None), (26, None)):
        a = list(ok)
        a[pos] = bad                          # ldg < O, ldwt < O, ld < 2*F1, k > 32, null operands, wmax without wrs, dU == G3, no records
        assert lib.spgan_edge_weight_dgrad(*a) == -22, pos
