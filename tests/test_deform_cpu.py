"""CPU: the decomposed full-rank edge convolution (tests/deform_model.py: one per-point GEMM, gathered rows, a product with K = k*F1,
closed-form backward with the BatchNorm correction applied per edge) against the vectors captured from the reference's
deform_edgeConv_simple / deform_edgeConv_first (golden deform.npz); the modules' parameter layout against the reference's.

Tolerances.  float64: the model runs in float64 on float32 inputs, the golden holds the reference's float64 run on the same inputs and
graph, so the two differ by float64 rounding alone: 1e-9 rel-L2 (the decomposition IS the reference).  float32: the model's distance from
the reference's float64 run stays within 5 x the reference's own float32-vs-float64 distance of that quantity (`tag|noise|q`).  The two
conv biases sit in front of a train-mode BatchNorm: their gradient is zero up to rounding in both, so they are compared absolutely
(1e-12 in float64; 2e-3 in float32, the ZERO_GRAD_BIASES rule)."""
import numpy as np
import pytest
import torch

import deform_model as dm
from helpers import golden

TAGS = list(dm.CASES)


@pytest.fixture(scope="module")
def d():
    return golden("deform.npz")


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _model(d, tag, dt):
    c = dm.CASES[tag]
    sd = {k: v.to(dt) if v.dtype.is_floating_point else v for k, v in dm.golden_state_dict(d, tag).items()}
    f = dm.forward(torch.from_numpy(d[tag + "|x"]).to(dt), torch.from_numpy(d[tag + "|idx"]), c["k"], sd, c["train"])
    bwd = dm.backward(f, torch.from_numpy(d[tag + "|g"]).to(dt))
    got = {"out": f["out"].reshape(dm.out_shape(c)), "dx": bwd["dx"]}
    got.update({q: v for q, v in bwd.items() if q.startswith("grad|")})
    for pre, bn in (("conv2.bn", f["bn2"]), ("inte_conv_hk.1", f["bn1"])):
        got["buf|%s.running_mean" % pre], got["buf|%s.running_var" % pre] = bn["running_mean"], bn["running_var"]
    return got


@pytest.mark.parametrize("tag", TAGS)
def test_model_matches_reference_float64(d, tag):
    got = _model(d, tag, torch.float64)
    assert set(got) == {k[len(tag) + 1:-5] for k in d.files if k.startswith(tag + "|") and k.endswith("|full") and "|d64|" not in k
                        and "num_batches_tracked" not in k}                     # every stored quantity
    for q, v in got.items():
        ref64 = dm.golden_f64(d, tag, q)
        assert tuple(v.shape) == tuple(ref64.shape), (tag, q)
        err = _rel(v, ref64)
        print("%s %s: model vs reference float64 rel-L2 %.3e" % (tag, q, err))
        if q[5:] in dm.ZERO_GRAD_BIASES and dm.CASES[tag]["train"]:
            assert float((v - ref64).abs().max()) < 1e-12, (tag, q)
        else:
            assert err < 1e-9, (tag, q, err)


@pytest.mark.parametrize("tag", TAGS)
def test_model_float32_within_reference_noise(d, tag):
    got = _model(d, tag, torch.float32)
    for q, v in got.items():
        ref64 = dm.golden_f64(d, tag, q)
        if q[5:] in dm.ZERO_GRAD_BIASES and dm.CASES[tag]["train"]:
            assert float((v.double() - ref64).abs().max()) <= 2e-3, (tag, q)
            continue
        err, noise = _rel(v, ref64), float(d["%s|noise|%s" % (tag, q)])
        print("%s %s: float32 model vs reference float64 %.3e (reference float32: %.3e)" % (tag, q, err, noise))
        assert err <= 5.0 * noise, (tag, q, err, noise)


def test_golden_conditions(d):
    for tag in TAGS:
        assert d[tag + "|near_tie_rows"].mean() <= 0.01
        assert tuple(d[tag + "|out|full"].shape) == dm.out_shape(dm.CASES[tag])
    for n in ("conv2.bn.weight", "inte_conv_hk.1.weight"):
        w = d["simple/feat|param|" + n]
        assert (w[::3] < 0).all() and (np.delete(w, np.s_[::3]) > 0).all()
    assert not np.array_equal(d["simple/eval|param|conv2.bn.running_mean"], np.zeros(8, np.float32))
    assert d["simple/k1|param|conv2.conv.weight"].shape == (4, 4, 1, 1) and d["first/odd|param|conv2.conv.weight"].shape == (12, 7, 1, 5)


def test_state_dict_layout_and_strict_loading(d):
    import spgan
    for tag in TAGS:
        c = dm.CASES[tag]
        cls = spgan.deform_edgeConv_simple if c["cls"] == "simple" else spgan.deform_edgeConv_first
        m = cls(c["Fin"], c["Fout"], c["k"])
        sd = m.state_dict()
        assert tuple(sd.keys()) == dm.STATE_KEYS
        for n in dm.STATE_KEYS:
            assert tuple(sd[n].shape) == tuple(d["%s|param|%s" % (tag, n)].shape), n
        m.load_state_dict(dm.golden_state_dict(d, tag), strict=True)
        assert (m.k, m.Fin, m.Fout) == (c["k"], c["Fin"], c["Fout"])
    assert isinstance(m.conv2, spgan.conv2dbr) and isinstance(m.inte_conv_hk[2], torch.nn.LeakyReLU) and m.inte_conv_hk[2].negative_slope == 0.01
    assert "deform_edgeConv_simple" in spgan.__all__ and "deform_edgeConv_first" in spgan.__all__
    with pytest.raises(RuntimeError):                                             # an upsample_edgeConv checkpoint does not fit
        spgan.deform_edgeConv_simple(16, 32, 10).load_state_dict(spgan.upsample_edgeConv(16, 32, 10, -1).state_dict(), strict=True)


def test_constructor_and_cpu_refusal():
    import spgan
    for k in (0, 33):
        with pytest.raises(ValueError, match="k=%d" % k):
            spgan.deform_edgeConv_simple(4, 4, k)
        with pytest.raises(ValueError, match="k=%d" % k):
            spgan.deform_edgeConv_first(4, 4, k)
    with pytest.raises(RuntimeError, match="no CPU"):
        spgan.deform_edgeConv_simple(3, 8, 4)(torch.zeros(2, 3, 16), None)
    with pytest.raises(RuntimeError, match="no CPU"):
        spgan.deform_edgeConv_first(3, 8, 4)(torch.zeros(2, 3, 16))


def test_launchers_reject_bad_sizes_without_gpu():
    from spgan import _lib
    lib = _lib.load()
    assert lib.spgan_edge_rank_tile_points(1) > 0 and lib.spgan_edge_rank_tile_points(32) > 0
    assert lib.spgan_edge_rank_tile_points(33) == 0 and lib.spgan_edge_rank_tile_points(0) == 0
    #                               PQ  ld idx M  k  F1 sc  sh  slope W2i ldw b2   O  Y  ldy part stream
    assert lib.spgan_edge_rank_gemm(None, 8, None, 8, 4, 4, None, None, 0.01, None, 16, None, 8, None, 8, None, None) == -22
    assert lib.spgan_edge_rank_gemm(16, 8, 16, 8, 33, 4, 16, 16, 0.01, 16, 132, None, 8, 16, 8, None, None) == -22       # k > 32
    assert lib.spgan_edge_rank_gemm(16, 7, 16, 8, 4, 4, 16, 16, 0.01, 16, 16, None, 8, 16, 8, None, None) == -22         # ld < 2*F1
    assert lib.spgan_edge_rank_gemm(16, 8, 16, 8, 4, 4, 16, 16, 0.01, 16, 15, None, 8, 16, 8, None, None) == -22         # ldw < k*F1
    assert lib.spgan_edge_rank_wgrad_ws_bytes(0, 4, 4, 8) == 0 and lib.spgan_edge_rank_wgrad_ws_bytes(8, 33, 4, 8) == 0
    assert lib.spgan_edge_rank_wgrad_ws_bytes(100, 4, 4, 8) >= 8 * 16 * 4
    assert lib.spgan_edge_rank_wgrad(16, 8, 16, 8, 4, 4, 16, 16, 0.01, 16, 8, 8, 16, 16, 16, 4, None) == -22             # workspace too small
    assert lib.spgan_edge_rank_dgrad(16, 7, 16, 8, 16, 8, 16, 8, 4, 4, 8, 16, 16, 16, 16, 0.01, 16, 16, None) == -22     # ldg < O
    assert lib.spgan_edge_rank_scatter(16, 16, 16, None, 8, None, 8, 4, 4, 16, None, None, None, 16, 7, None) == -22     # ldd < 2*F1
    assert lib.spgan_edge_rank_scatter(16, 16, 16, None, 8, None, 8, 4, 4, 16, None, None, 16, 16, 8, None) == -22       # train mode without PQ
