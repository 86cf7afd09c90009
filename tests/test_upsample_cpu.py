"""CPU: the decomposed upsampling edge convolution (tests/upsample_model.py: rank-window products, per-point central halves, the
column permutation that replaces the reference's transpose / view chain, closed-form backward) against the vectors captured from the
reference's upsample_edgeConv (golden upsample.npz), in float64; the module's parameter layout against the reference's.

Tolerance: the model runs in float64 on float32 inputs, the golden holds the reference's float64 run on the same inputs and graph, so
the two differ by float64 rounding through two BatchNorms and products of up to 2*C*k terms: 1e-10 relative (1e-12 absolute for the
two conv biases in train mode, whose gradient in front of a BatchNorm is zero up to rounding)."""
import numpy as np
import pytest
import torch

import upsample_model as um
from helpers import golden

TAGS = list(um.CASES)


@pytest.fixture(scope="module")
def d():
    return golden("upsample.npz")


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _sd64(d, tag):
    return {k: v.double() if v.dtype.is_floating_point else v for k, v in um.golden_state_dict(d, tag).items()}


def _model64(d, tag):
    c = um.CASES[tag]
    f = um.forward(torch.from_numpy(d[tag + "|x"]).double(), torch.from_numpy(d[tag + "|idx"]), c["k"], _sd64(d, tag), c["train"])
    return f, um.backward(f, torch.from_numpy(d[tag + "|g"]).double())


@pytest.mark.parametrize("tag", TAGS)
def test_model_matches_reference_float64(d, tag):
    f, bwd = _model64(d, tag)
    got = {"out": f["out"], "dx": bwd["dx"]}
    got.update({q: v for q, v in bwd.items() if q.startswith("grad|")})
    for pre, bn in (("conv2.bn", f["bn2"]), ("inte_conv_hk.1", f["bn1"])):
        got["buf|%s.running_mean" % pre], got["buf|%s.running_var" % pre] = bn["running_mean"], bn["running_var"]
    assert set(got) == {k[len(tag) + 1:-5] for k in d.files if k.startswith(tag + "|") and k.endswith("|full") and "|d64|" not in k
                        and "num_batches_tracked" not in k}                     # every stored quantity
    for q, v in got.items():
        ref64 = um.golden_f64(d, tag, q)
        err = _rel(v, ref64)
        print("%s %s: model vs reference float64 rel-L2 %.3e" % (tag, q, err))
        if q[5:] in um.ZERO_GRAD_BIASES and um.CASES[tag]["train"]:
            assert float((v - ref64).abs().max()) < 1e-12, (tag, q)
        else:
            assert err < 1e-10, (tag, q, err)


@pytest.mark.parametrize("tag", TAGS)
def test_weight_column_permutation_against_literal_views(d, tag):
    """Step 2 of the decomposition: conv2 over cat(ee, inte) with inte pushed through the reference's transpose / view / permute chain
    equals the permuted-column product of the model; evaluated literally (conv2d, batch_norm, views) in float64."""
    c = um.CASES[tag]
    sd = _sd64(d, tag)
    x, idx = torch.from_numpy(d[tag + "|x"]).double(), torch.from_numpy(d[tag + "|idx"])
    f = um.forward(x, idx, c["k"], sd, c["train"])
    assert _rel(f["out"], um.literal(x, idx, c["k"], sd, c["train"])) < 1e-12
    # the permutation alone, on an arbitrary tensor: V2 . view-chain(h) == V2p . rows(h)
    g = torch.Generator().manual_seed(1)
    C, k, B, N = c["Fin"], c["k"], c["B"], c["N"]
    T = k // 2
    h = torch.randn(B, 4 * C, N, T, generator=g, dtype=torch.float64)              # inte_conv_hk's output layout
    V = sd["conv2.conv.weight"]
    lit = h.transpose(2, 1).contiguous().view(B, N, 2 * C, 2, T).contiguous().view(B, N, 2 * C, k).permute(0, 2, 1, 3)   # [B,2C,N,k]
    want = torch.einsum("fcj,bcnj->bnf", V[:, :, 0, k:], lit)
    rows = h.permute(0, 2, 3, 1).reshape(B * N, T * 4 * C)                         # rows (i,t), columns o
    V2p = um.images(sd["inte_conv_hk.0.weight"], V, C, k)[4]
    assert _rel((rows @ V2p.t()).view(B, N, -1), want) < 1e-13


def test_golden_conditions(d):
    for tag in TAGS + ["xyzfn"]:
        assert d[tag + "|near_tie_rows"].mean() <= 0.01
    for n in ("conv2.bn.weight", "inte_conv_hk.1.weight"):
        w = d["feat|param|" + n]
        assert (w[::3] < 0).all() and (np.delete(w, np.s_[::3]) > 0).all()
    assert not np.array_equal(d["eval|param|conv2.bn.running_mean"], np.zeros(16, np.float32))
    assert um.CASES["k2"]["k"] // 2 + 1 == 2 and d["k2|param|inte_conv_hk.0.weight"].shape[3] == 2


def test_state_dict_layout_and_strict_loading(d):
    import spgan
    for tag in TAGS:
        c = um.CASES[tag]
        m = spgan.upsample_edgeConv(c["Fin"], c["Fout"], c["k"], -1)
        sd = m.state_dict()
        assert tuple(sd.keys()) == um.STATE_KEYS
        for n in um.STATE_KEYS:
            assert tuple(sd[n].shape) == tuple(d["%s|param|%s" % (tag, n)].shape), n
        m.load_state_dict(um.golden_state_dict(d, tag), strict=True)
        assert (m.k, m.Fin, m.Fout, m.num) == (c["k"], c["Fin"], c["Fout"], -1)
    assert isinstance(m.conv2, spgan.conv2dbr) and isinstance(m.inte_conv_hk[2], torch.nn.LeakyReLU) and m.inte_conv_hk[2].negative_slope == 0.01
    assert "upsample_edgeConv" in spgan.__all__ and "get_edge_features_xyz" in spgan.__all__


def test_constructor_and_cpu_refusal():
    import spgan
    with pytest.raises(ValueError):
        spgan.upsample_edgeConv(4, 4, 5, -1)                                       # odd k: the reference's view fails as well
    m = spgan.upsample_edgeConv(3, 8, 4, -1)
    with pytest.raises(RuntimeError, match="no CPU"):
        m(torch.zeros(2, 3, 16))
    with pytest.raises(RuntimeError, match="no CPU"):
        spgan.get_edge_features_xyz(torch.zeros(1, 4, 16), torch.zeros(1, 3, 16), 4)


def test_launchers_reject_bad_sizes_without_gpu():
    from spgan import _lib
    lib = _lib.load()
    assert lib.spgan_edge_window_tile_points(10, 5) > 0 and lib.spgan_edge_window_tile_points(10, 1) > 0
    assert lib.spgan_edge_window_tile_points(64, 1) == 0
    assert lib.spgan_edge_window_gemm(None, 4, None, 8, 4, 4, None, 12, 8, 3, None, 0, None, 0, None, 8, None, None) == -22
    assert lib.spgan_edge_window_gemm(16, 4, 16, 8, 4, 4, 16, 12, 8, 5, None, 0, None, 0, 16, 8, None, None) == -22      # w > k
    assert lib.spgan_edge_window_gemm(16, 4, 16, 8, 4, 4, 16, 11, 8, 3, None, 0, None, 0, 16, 8, None, None) == -22      # ldw < w*C
    assert lib.spgan_edge_window_wgrad_ws_bytes(0, 4, 4, 8, 3) == 0
    assert lib.spgan_edge_window_wgrad(16, 4, 16, 8, 4, 4, 16, 8, 8, 3, 16, 12, 16, 4, None) == -22                      # workspace too small
    assert lib.spgan_edge_window_dgrad(16, 7, 16, 8, 8, 4, 4, 8, 3, 16, 0, None) == -22                                  # ldg < O
    assert lib.spgan_edge_window_scatter(16, 16, 16, 8, 4, 4, None, 0, None, 0, 16, 3, None) == -22                      # lddx < C
