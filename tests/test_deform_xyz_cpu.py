"""CPU: the decomposed coordinate-guided full-rank edge convolution (tests/deform_xyz_model.py: three per-point GEMMs, the product of two
activated 16-channel branches gathered through one graph, the weight MLP over edge rows, the softmax normaliser, a product with
K = k*Fin over h*s) against the vectors captured from the reference's deform_edgeConv (golden deform_xyz.npz); the written-out backward
of the two new launchers against autograd; the module's parameter layout against the reference's; the new entry points' argument checks.

Tolerances, as tests/test_deform_feat_cpu.py.  float64: the model runs in float64 on float32 inputs, the golden holds the reference's
float64 run on the same inputs and graph (its distance from the float32 run stored with 10 mantissa bits: 1e-10 of the value), so the
two differ by float64 rounding and that storage alone: 1e-9 rel-L2.  float32: within 5 x the reference's own float32-vs-float64 distance
of that quantity.  Every conv bias sits in front of a train-mode BatchNorm: its gradient is zero up to rounding in both, compared
absolutely (1e-12 in float64; 2e-3 in float32, the ZERO_GRAD_BIASES rule), in the train-mode cases.  Case d (k = 1): the softmax weight
is 1, dpc and every conv_fea / conv_xyz / conv_all gradient is an exact zero in the reference and in the model."""
import numpy as np
import pytest
import torch

import deform_xyz_model as xm
from helpers import golden

TAGS = list(xm.CASES)


@pytest.fixture(scope="module")
def d():
    return golden("deform_xyz.npz")


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _module(d, tag):
    """spgan.deform_edgeConv of the case, holding the reference's checkpoint (strict loading)"""
    import spgan
    c = xm.CASES[tag]
    m = spgan.deform_edgeConv(c["F"], c["F"], c["k"], softmax=c["softmax"])
    m.load_state_dict(xm.golden_state_dict(d, tag), strict=True)
    return m


@pytest.fixture(scope="module")
def runs(d):
    """The model's float64 and float32 results per case, computed once: on the parameters and buffers as the module holds them after
    loading the reference's checkpoint, so what the golden checks is the layer's own layout, not a list of names kept beside it."""
    out = {}
    for tag in TAGS:
        c = xm.CASES[tag]
        for dt in (torch.float64, torch.float32):
            sd = {k: v.to(dt) if v.dtype.is_floating_point else v for k, v in _module(d, tag).state_dict().items()}
            assert tuple(sd) == xm.STATE_KEYS
            t = lambda n: torch.from_numpy(d[tag + n]).to(dt)
            out[tag, dt] = xm.run(t("|x"), t("|pc"), torch.from_numpy(d[tag + "|idx"]), t("|g"), c["k"], sd, c["train"], c["softmax"])
    return out


def _stored(d, tag):
    return {k[len(tag) + 1:].rsplit("|", 1)[0] for k in d.files if k.startswith(tag + "|") and k.endswith(("|full", "|samples"))
            and "|d64|" not in k and "num_batches_tracked" not in k}


@pytest.mark.parametrize("tag", TAGS)
def test_model_matches_reference_float64(d, runs, tag):
    got = runs[tag, torch.float64]
    assert set(got) == _stored(d, tag)                                          # every stored quantity
    for q, v in got.items():
        ref64, mine = xm.golden_pair(d, tag, q, v)
        err = _rel(mine, ref64)
        print("%s %s: model vs reference float64 rel-L2 %.3e" % (tag, q, err))
        if (q[5:] in xm.ZERO_GRAD_BIASES and xm.CASES[tag]["train"]) or float(ref64.abs().max()) == 0.0:
            assert float((mine - ref64).abs().max()) < 1e-12, (tag, q)
        else:
            assert err < 1e-9, (tag, q, err)


@pytest.mark.parametrize("tag", TAGS)
def test_model_float32_within_reference_noise(d, runs, tag):
    for q, v in runs[tag, torch.float32].items():
        ref64, mine = xm.golden_pair(d, tag, q, v)
        if q[5:] in xm.ZERO_GRAD_BIASES and xm.CASES[tag]["train"]:
            assert float((mine.double() - ref64).abs().max()) <= 2e-3, (tag, q)
            continue
        err, noise = _rel(mine, ref64), xm.noise(d, tag, q)
        print("%s %s: float32 model vs reference float64 %.3e (reference float32: %.3e)" % (tag, q, err, noise))
        assert err <= max(5.0 * noise, 1e-12), (tag, q, err, noise)


def test_golden_conditions(d):
    assert tuple(str(k) for k in d["state_keys"]) == xm.STATE_KEYS
    quantities = ["out", "dx", "dpc"] + ["grad|" + n for n in xm.STATE_KEYS if n.endswith((".weight", ".bias"))] + \
        ["buf|" + n for n in xm.BUFFERS if "num_batches" not in n]
    assert sorted(str(n) for n in d["noise_keys"]) == sorted(quantities)
    for tag in TAGS:
        c = xm.CASES[tag]
        assert d[tag + "|near_tie_rows"].mean() <= 0.01
        assert tuple(d[tag + "|x"].shape) == (c["B"], c["F"], c["N"]) and tuple(d[tag + "|pc"].shape) == (c["B"], 3, c["N"])
        assert tuple(d[tag + "|idx"].shape) == (c["B"], c["N"] * c["k"]) and d[tag + "|noise"].shape == d["noise_keys"].shape
        m = _module(d, tag)                                                     # the capture and the layer agree on every shape
        assert tuple(m.conv2[0].weight.shape) == (c["F"], c["F"], 1, c["k"]) == tuple(xm.param(d, tag, "conv2.0.weight").shape)
        assert (m.k, m.Fin, m.Fout, m.softmax, m.training) == (c["k"], c["F"], c["F"], c["softmax"], True)
        bf = torch.from_numpy(xm.param(d, tag, "conv2.0.weight"))
        assert torch.equal(bf.bfloat16().float(), bf)                           # what the 16-bit storage relies on
    assert not np.any(d["d|dpc|full"])                                          # case d: nothing reaches the weight side
    for n in xm.STATE_KEYS:
        if n.startswith(xm.SINGLE_RANK_ZERO) and n.endswith((".weight", ".bias")):
            assert not np.any(d["d|grad|%s|full" % n]), n
    assert np.any(d["b|dpc|full"]) and np.any(d["b|grad|conv_xyz.0.weight|full"])
    assert not np.array_equal(xm.param(d, "e", "conv_all.4.running_mean"), np.zeros(32, np.float32))
    for n in xm.BUFFERS:                                                        # eval mode: the reference leaves its buffers alone
        assert np.array_equal(d["e|buf|%s|full" % n], xm.param(d, "e", n)), n


@pytest.mark.parametrize("soft", [True, False])
def test_written_out_backward_matches_autograd(soft):
    """xm.gather2 / xm.split (what the GPU launchers are compared with) against autograd, float64: the yardstick of the wrappers in
    spgan.edge_weight, whose argument order the model's functions follow.  The product feeds a softmax over the ranks (or not), so that
    the cotangent reaching it is not a plain constant."""
    import inspect
    import spgan
    ew = spgan.edge_weight
    assert list(inspect.signature(ew.edge_weight_gather2).parameters)[:7] == ["PQa", "PQb", "idx", "scale_a", "shift_a", "scale_b", "shift_b"]
    assert list(inspect.signature(ew.edge_weight_split).parameters)[:12] == ["dw0", "PQa", "PQb", "idx", "scale_a", "shift_a", "mean_a", "invstd_a",
                                                                           "scale_b", "shift_b", "mean_b", "invstd_b"]
    g = torch.Generator().manual_seed(7)
    M, k, F = 23, 4, 6
    PQa, PQb = (torch.randn(M, 2 * F, generator=g, dtype=torch.float64) for _ in range(2))
    gidx = torch.randint(0, M, (M, k), generator=g)
    sca, sha, scb, shb = (torch.randn(F, generator=g, dtype=torch.float64) for _ in range(4))
    mua, inva, mub, invb = (torch.rand(F, generator=g, dtype=torch.float64) + 0.5 for _ in range(4))
    cot = torch.randn(M, k, F, generator=g, dtype=torch.float64)
    # autograd reaches the two pre-activation BatchNorm outputs through explicit leaves
    za, zb = xm.pre_norm(PQa, gidx), xm.pre_norm(PQb, gidx)
    prea, preb = (za * sca + sha).requires_grad_(True), (zb * scb + shb).requires_grad_(True)
    w0 = xm.lrelu(prea) * xm.lrelu(preb)
    w0.retain_grad()
    y = torch.softmax(w0, dim=1) if soft else w0 * w0
    (y * cot).sum().backward()
    assert _rel(w0.detach().reshape(M * k, F), xm.gather2(PQa, PQb, gidx, sca, sha, scb, shb)) < 1e-12
    ga, sa, gb, sb = xm.split(w0.grad.reshape(M * k, F), PQa, PQb, gidx, sca, sha, mua, inva, scb, shb, mub, invb)
    assert _rel(ga, prea.grad) < 1e-12 and _rel(gb, preb.grad) < 1e-12
    assert _rel(sa, torch.cat([prea.grad.sum(dim=(0, 1)), (prea.grad * (za - mua) * inva).sum(dim=(0, 1))])) < 1e-12
    assert _rel(sb, torch.cat([preb.grad.sum(dim=(0, 1)), (preb.grad * (zb - mub) * invb).sum(dim=(0, 1))])) < 1e-12


def test_state_dict_layout_and_strict_loading(d):
    import spgan
    from torch import nn
    for tag in TAGS:
        c = xm.CASES[tag]
        m = spgan.deform_edgeConv(c["F"], c["F"], c["k"], softmax=c["softmax"])
        sd = m.state_dict()
        assert tuple(sd.keys()) == tuple(str(k) for k in d["state_keys"])       # the reference's own list, in its order
        for n in xm.STATE_KEYS:
            assert tuple(sd[n].shape) == tuple(xm.param(d, tag, n).shape), n
        m.load_state_dict(xm.golden_state_dict(d, tag), strict=True)
        assert (m.k, m.Fin, m.Fout, m.softmax, m.last_idx) == (c["k"], c["F"], c["F"], c["softmax"], None)
    assert [n for n, _ in m.named_children()] == ["conv2", "conv_xyz", "conv_fea", "conv_all", "inte_conv_hk"]
    # conv2 is a plain Sequential that ends in LeakyReLU, not a conv2dbr
    assert type(m.conv2) is nn.Sequential and isinstance(m.conv2[2], nn.LeakyReLU) and m.conv2[2].negative_slope == 0.01
    assert "deform_edgeConv" in spgan.__all__ and spgan.deform_edgeConv(4, 4, 3).softmax is True
    # the reference's BatchNorm2d(Fin) over Fout channels: any pair constructs, with the reference's shapes, and loads strictly both ways
    a, b = spgan.deform_edgeConv(8, 12, 5), spgan.deform_edgeConv(8, 12, 5)
    assert tuple(a.conv2[0].weight.shape) == (12, 8, 1, 5) and a.conv2[1].num_features == 8
    b.load_state_dict(a.state_dict(), strict=True)
    with pytest.raises(RuntimeError):                                           # a deform_edgeConv_feat checkpoint does not fit
        spgan.deform_edgeConv(16, 16, 10).load_state_dict(spgan.deform_edgeConv_feat(16, 16, 10).state_dict(), strict=True)


def test_constructor_and_cpu_refusal():
    import spgan
    for k in (0, 33):
        with pytest.raises(ValueError, match="k=%d" % k):
            spgan.deform_edgeConv(4, 4, k)
    with pytest.raises(ValueError, match="Fin=0"):
        spgan.deform_edgeConv(0, 4, 4)
    with pytest.raises(ValueError, match="Fout=0"):
        spgan.deform_edgeConv(4, 0, 4)
    with pytest.raises(ValueError, match="Fin=3.*Fout=8"):                      # constructs, but does not run: the reference's rule
        spgan.deform_edgeConv(3, 8, 4)(torch.zeros(2, 3, 16), torch.zeros(2, 3, 16))
    with pytest.raises(RuntimeError, match="no CPU"):
        spgan.deform_edgeConv(3, 3, 4)(torch.zeros(2, 3, 16), torch.zeros(2, 3, 16))


def test_entry_points_declared():
    import os
    from spgan import _lib
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "spgan_hip.h")).read()
    lib = _lib.load()
    for n in ("gather2", "split"):
        assert "int spgan_edge_weight_%s(" % n in header, n
        assert callable(getattr(lib, "spgan_edge_weight_" + n))


def test_launchers_reject_bad_sizes_without_gpu():
    from spgan import _lib
    lib = _lib.load()
    p = 16                                                                      # any non-null address: the checks come before every launch
    #     PQa lda PQb ldb idx M  k  F  sca sha scb shb slope W0 stream
    ok = [p, 8, p, 8, p, 8, 4, 4, p, p, p, p, 0.01, p, None]
    for pos, bad in ((0, None), (2, None), (4, None), (8, None), (9, None), (10, None), (11, None), (13, None), (6, 0), (6, 33), (1, 7), (3, 7),
                     (5, 0), (7, 0)):
        a = list(ok)
        a[pos] = bad                          # null operands, k outside 1..32, lda / ldb < 2*F, M = 0, F = 0
        assert lib.spgan_edge_weight_gather2(*a) == -22, pos
    #     dW0 PQa lda PQb ldb idx M  k  F  sca sha mua inva scb shb mub invb slope GA  GB  pa  pb  stream
    ok = [p, p, 8, p, 8, p, 8, 4, 4, p, p, p, p, p, p, p, p, 0.01, p, 32, p, 32, None]
    for pos, bad in ((0, None), (1, None), (3, None), (5, None), (9, None), (10, None), (11, None), (12, None), (13, None), (14, None), (15, None),
                     (16, None), (18, None), (19, None), (20, None), (21, None), (19, p), (21, p), (7, 0), (7, 33), (2, 7), (4, 7), (6, 0), (8, 0)):
        a = list(ok)
        a[pos] = bad                          # null operands, GA == GB, one record buffer for both, k outside 1..32, ld < 2*F, M = 0, F = 0
        assert lib.spgan_edge_weight_split(*a) == -22, pos
