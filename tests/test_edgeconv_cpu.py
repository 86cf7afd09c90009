"""CPU: the decomposed max-aggregation edge convolution (tests/edgeconv_model.py: P/Q per point, max / min selection by the sign of
gamma*invstd, closed-form backward) against the vectors captured from the reference's edgeConv (golden edgeconv.npz), in float64;
the module's parameter layout against the reference's; the refusal of CPU tensors.

Tolerance: the model runs in float64 on float32 inputs, the golden holds the reference's float64 run on the same inputs and graph, so
the two differ by float64 rounding through a BatchNorm and two small GEMMs: 1e-10 relative (1e-12 absolute for the conv bias, whose
gradient in front of a train-mode BatchNorm is zero up to rounding).  The float32 golden is then within the stored float32-vs-float64
divergence (x 1.5) of the model."""
import numpy as np
import pytest
import torch

import edgeconv_model as ecm
from helpers import golden

TAGS = list(ecm.CASES)


@pytest.fixture(scope="module")
def d():
    return golden("edgeconv.npz")


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _model64(d, tag):
    c = ecm.CASES[tag]
    sd = {k: v.double() if v.dtype.is_floating_point else v for k, v in ecm.golden_state_dict(d, tag).items()}
    x = torch.from_numpy(d[tag + "|x"]).double()
    idx = torch.from_numpy(d[tag + "|idx"])
    f = ecm.forward(x, idx, c["k"], sd["conv.conv.weight"], sd["conv.conv.bias"], sd["conv.bn.weight"], sd["conv.bn.bias"],
                    sd["conv.bn.running_mean"], sd["conv.bn.running_var"], c["train"])
    bwd = ecm.backward(f, torch.from_numpy(d[tag + "|g"]).double())
    return f, bwd


@pytest.mark.parametrize("tag", TAGS)
def test_model_matches_reference_float64(d, tag):
    f, bwd = _model64(d, tag)
    got = {"out": f["out"], "dx": bwd["dx"], "grad|conv.conv.weight": bwd["dW"], "grad|conv.conv.bias": bwd["db"],
           "grad|conv.bn.weight": bwd["dgamma"], "grad|conv.bn.bias": bwd["dbeta"],
           "buf|conv.bn.running_mean": f["running_mean"], "buf|conv.bn.running_var": f["running_var"]}
    for q, v in got.items():
        ref64 = ecm.golden_f64(d, tag, q)
        err = _rel(v, ref64)
        print("%s %s: model vs reference float64 rel-L2 %.3e" % (tag, q, err))
        if q == "grad|conv.conv.bias" and ecm.CASES[tag]["train"]:
            assert float((v - ref64).abs().max()) < 1e-12, (tag, q)
        else:
            assert err < 1e-10, (tag, q, err)
        noise = float(d["%s|noise|%s" % (tag, q)])
        ref32 = torch.from_numpy(d["%s|%s|full" % (tag, q)])
        if not (q == "grad|conv.conv.bias" and ecm.CASES[tag]["train"]):
            assert _rel(ref32, v) <= 1.5 * noise + 1e-12, (tag, q)


@pytest.mark.parametrize("tag", TAGS)
def test_decomposition_equals_composition(d, tag):
    """max_j relu(bn(conv(edge tensor))) == relu(a (Q + ext_j P_n) + s): the identity the kernels rest on, in float64."""
    c = ecm.CASES[tag]
    f, _ = _model64(d, tag)
    sd = {k: v.double() if v.dtype.is_floating_point else v for k, v in ecm.golden_state_dict(d, tag).items()}
    out, y = ecm.composition(f["x"], f["idx"], c["k"], sd["conv.conv.weight"], sd["conv.conv.bias"], sd["conv.bn.weight"], sd["conv.bn.bias"],
                             sd["conv.bn.running_mean"], sd["conv.bn.running_var"], c["train"])
    assert _rel(f["out"], out) < 1e-12
    assert _rel(f["Q"].unsqueeze(2) + f["Pn"], y) < 1e-12


def test_golden_conditions(d):
    for tag in TAGS:
        assert float(d[tag + "|gap"]) > 1e-4                         # no case hinges on a tie in the max
        assert d[tag + "|near_tie_rows"].mean() <= 0.01
    assert (d["neg|param|conv.bn.weight"] < 0).sum() >= 3          # several negative bn.weight entries
    f, _ = _model64(d, "neg")
    neg = torch.from_numpy(d["neg|param|conv.bn.weight"]) < 0
    assert torch.equal(f["sel"][..., neg], f["jmin"][..., neg]) and torch.equal(f["sel"][..., ~neg], f["jmax"][..., ~neg])
    assert not torch.equal(f["jmin"][..., neg], f["jmax"][..., neg])
    assert not np.array_equal(d["eval|param|conv.bn.running_mean"], np.zeros(32, np.float32))    # non-initial running statistics


def test_state_dict_layout_and_strict_loading(d):
    import spgan
    m = spgan.edgeConv(16, 32, 10)
    sd = m.state_dict()
    assert list(sd.keys()) == ["conv.conv.weight", "conv.conv.bias", "conv.bn.weight", "conv.bn.bias", "conv.bn.running_mean",
                               "conv.bn.running_var", "conv.bn.num_batches_tracked"]
    assert tuple(sd["conv.conv.weight"].shape) == (32, 32, 1, 1) and tuple(sd["conv.bn.weight"].shape) == (32,)
    assert isinstance(m.conv, spgan.conv2dbr) and isinstance(m.conv.ac, torch.nn.ReLU)
    for tag in TAGS:
        c = ecm.CASES[tag]
        m = spgan.edgeConv(c["Fin"], c["Fout"], c["k"])
        m.load_state_dict(ecm.golden_state_dict(d, tag), strict=True)
        assert int(m.conv.bn.num_batches_tracked) == int(d[tag + "|param|conv.bn.num_batches_tracked"])
    assert (m.k, m.Fin, m.Fout) == (10, 16, 32)
    c2 = spgan.conv2dbr(6, 8, [1, 3], [1, 2])
    assert tuple(c2.conv.weight.shape) == (8, 6, 1, 3) and tuple(c2.conv.stride) == (1, 2)


def test_cpu_tensors_are_refused():
    import spgan
    m = spgan.edgeConv(3, 8, 4)
    with pytest.raises(RuntimeError, match="no CPU"):
        m(torch.zeros(2, 3, 16))
    with pytest.raises(RuntimeError, match="no CPU"):
        spgan.conv2dbr(6, 8, 1)(torch.zeros(2, 6, 16, 4))
    with pytest.raises(ValueError):
        spgan.edgeConv(3, 8, 128)


def test_launchers_reject_bad_sizes_without_gpu():
    from spgan import _lib
    lib = _lib.load()
    assert lib.spgan_edge_max_tile_points() > 0
    assert lib.spgan_edge_max_gather(None, 8, None, 4, 2, 4, None, None, None, None, None, None, None, None, None, None) == -22
    assert lib.spgan_edge_max_gather(16, 8, 16, 4, 128, 4, 16, 16, 16, 16, 16, None, None, None, None, None) == -22      # k > 127
    assert lib.spgan_edge_max_gather(16, 7, 16, 4, 2, 4, 16, 16, 16, 16, 16, None, None, None, None, None) == -22        # ld < 2F
    assert lib.spgan_edge_max_gather(16, 8, 16, 4, 2, 4, 16, 16, 16, 16, 16, 16, None, None, None, None) == -22          # scale without shift / out
    assert lib.spgan_edge_max_finish(16, 8, 16, 16, 16, 16, 16, 16, 0, 4, 16, 16, None) == -22                               # M = 0
    assert lib.spgan_edge_max_bwd_point(16, 16, 16, 8, 16, 4, 0, 4, 16, 16, 16, None) == -22                                 # k = 0
    assert lib.spgan_edge_max_bwd_graph(16, 16, 16, 8, 16, 16, None, 4, 2, 4, 16, 16, 16, 16, 16, 8, None) == -22            # sums without idx
    assert lib.spgan_edge_max_bwd_graph(16, 16, 16, 8, 16, 16, 16, 4, 2, 4, 16, 16, 16, 16, 16, 7, None) == -22              # ldd < 2F
