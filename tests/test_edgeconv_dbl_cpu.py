"""CPU: the closed-form double backward of the max-aggregation edge convolution (tests/edgeconv_dbl_model.py) against float64 autograd
through the materialised composition (edgeconv_model.composition): grad(create_graph=True), then grad of <v, dx>; the new launchers'
argument checks; the constructor keyword.

Tolerance: both sides run in float64 on the same inputs and the same brute-force graph, and the selection is the same discrete choice
on both (no case hinges on a tie), so they differ by float64 rounding through a BatchNorm, its two derivatives and small products:
1e-10 relative."""
import pytest
import torch

import edgeconv_dbl_model as edm
import edgeconv_model as ecm

TAGS = list(ecm.CASES)


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _case64(tag, seed=0):
    c = ecm.CASES[tag]
    x, g, sd = ecm.case_tensors(tag, seed)
    sd = {n: (t.double() if t.dtype.is_floating_point else t) for n, t in sd.items()}
    from spgan import fixture_rng as fr
    v = fr.normal("edgeconv.%s.v" % tag, tuple(x.shape), salt=seed).double()
    return c, x.double(), g.double(), v, sd, edm.brute_force_graph(x, c["k"])


@pytest.mark.parametrize("tag", TAGS)
def test_model_matches_float64_autograd(tag):
    c, x, g, v, sd, idx = _case64(tag)
    names = ("conv.conv.weight", "conv.conv.bias", "conv.bn.weight", "conv.bn.bias")
    W, b, gamma, beta = (sd[n].clone().requires_grad_(True) for n in names)
    rm, rv = sd["conv.bn.running_mean"], sd["conv.bn.running_var"]
    xa, ga = x.clone().requires_grad_(True), g.clone().requires_grad_(True)
    out, _ = ecm.composition(xa, idx, c["k"], W, b, gamma, beta, rm, rv, c["train"])
    (dx,) = torch.autograd.grad(out, xa, ga, create_graph=True)
    want = dict(zip(("xbar", "Wbar", "gammabar", "ghat", "bbar", "betabar"),
                    torch.autograd.grad((v * dx).sum(), (xa, W, gamma, ga, b, beta), allow_unused=True)))

    f = ecm.forward(x, idx, c["k"], sd[names[0]], sd[names[1]], sd[names[2]], sd[names[3]], rm, rv, c["train"])
    assert _rel(ecm.backward(f, g)["dx"], dx.detach()) < 1e-10
    got = edm.double_backward(f, g, v)
    for q in ("Wbar", "gammabar", "ghat"):
        err = _rel(got[q], want[q])
        print("%s %s: model vs float64 autograd rel-L2 %.3e" % (tag, q, err))
        assert err < 1e-10, (tag, q, err)
    if c["train"]:
        err = _rel(got["xbar"], want["xbar"])
        print("%s xbar: model vs float64 autograd rel-L2 %.3e" % (tag, err))
        assert err < 1e-10, (tag, err)
    else:                                                   # statistics constant: dx does not depend on x (piecewise)
        assert want["xbar"] is None or float(want["xbar"].abs().max()) == 0.0
        assert float(got["xbar"].abs().max()) == 0.0
    # the conv bias and beta only shift z resp. the output: no second derivative (up to float64 rounding in autograd's chain)
    scale = float(want["gammabar"].abs().max())
    for q in ("bbar", "betabar"):
        assert want[q] is None or float(want[q].abs().max()) < 1e-10 * scale, (tag, q)
    if tag == "neg":
        assert int((sd["conv.bn.weight"] < 0).sum()) == 7


def test_model_accepts_outside_selection():
    c, x, g, v, sd, idx = _case64("feat")
    f = ecm.forward(x, idx, c["k"], sd["conv.conv.weight"], sd["conv.conv.bias"], sd["conv.bn.weight"], sd["conv.bn.bias"],
                    sd["conv.bn.running_mean"], sd["conv.bn.running_var"], True)
    own = edm.double_backward(f, g, v)
    same = edm.double_backward(f, g, v, sel=f["sel"].clone(), active=f["out_pm"] > 0)
    other = edm.double_backward(f, g, v, sel=(f["sel"] + 1) % c["k"], active=f["out_pm"] > 0)
    assert torch.equal(own["xbar"], same["xbar"]) and not torch.equal(own["xbar"], other["xbar"])


def test_launchers_reject_bad_sizes_without_gpu():
    from spgan import _lib
    lib = _lib.load()
    # r, sel, PQ, ld, VPQ, ldv, idx, M, k, F, mean, invstd, partials_t, partials_s, stream
    assert lib.spgan_edge_max_dbl_point(None, 16, 16, 8, 16, 8, 16, 4, 2, 4, 16, 16, 16, 16, None) == -22               # no r
    assert lib.spgan_edge_max_dbl_point(16, 16, 16, 8, None, 8, 16, 4, 2, 4, 16, 16, 16, 16, None) == -22               # no VPQ
    assert lib.spgan_edge_max_dbl_point(16, 16, 16, 8, 16, 7, 16, 4, 2, 4, 16, 16, 16, 16, None) == -22                 # ldv < 2F
    assert lib.spgan_edge_max_dbl_point(16, 16, 16, 8, 16, 8, 16, 4, 128, 4, 16, 16, 16, 16, None) == -22               # k > 127
    assert lib.spgan_edge_max_dbl_point(16, 16, 16, 8, 16, 8, 16, 0, 2, 4, 16, 16, 16, 16, None) == -22                 # M = 0
    assert lib.spgan_edge_max_dbl_point(16, 16, 16, 8, 16, 8, 16, 4, 2, 4, None, None, 16, 16, None) == -22             # edge records without statistics
    assert lib.spgan_edge_max_dbl_point(16, 16, 16, 8, 16, 8, 16, 4, 2, 4, 16, 16, None, 16, None) == -22               # statistics without edge records
    assert lib.spgan_edge_max_dbl_point(16, 16, 16, 8, 16, 8, 16, 4, 2, 4, None, None, None, None, None) == -22         # no partials_s
    # r, sel, PQ, ld, VPQ, ldv, rowptr, src, idx, M, k, F, scale, mean, invstd, sums, dsums, ghat, PQbar, ldb, stream
    assert lib.spgan_edge_max_dbl_graph(16, 16, 16, 8, 16, 8, 16, 16, 16, 4, 2, 4, 16, 16, 16, 16, 16, None, 16, 8, None) == -22    # no ghat
    assert lib.spgan_edge_max_dbl_graph(16, 16, 16, 8, 16, 8, 16, 16, 16, 4, 2, 4, 16, 16, 16, 16, None, 16, 16, 8, None) == -22    # sums without dsums
    assert lib.spgan_edge_max_dbl_graph(16, 16, 16, 8, 16, 8, None, 16, 16, 4, 2, 4, 16, 16, 16, 16, 16, 16, 16, 8, None) == -22    # train without rowptr
    assert lib.spgan_edge_max_dbl_graph(16, 16, 16, 8, 16, 8, 16, 16, 16, 4, 2, 4, 16, 16, 16, 16, 16, 16, 16, 7, None) == -22      # ldb < 2F
    assert lib.spgan_edge_max_dbl_graph(16, 16, 16, 8, 16, 8, 16, 16, 16, 4, 2, 4, 16, 16, 16, 16, 16, 16, None, 8, None) == -22    # train without PQbar
    assert lib.spgan_edge_max_dbl_graph(16, 16, 16, 8, 16, 8, None, None, 16, 4, 2, 4, 16, None, None, None, 16, 16, None, 8, None) == -22   # dsums without sums
    assert lib.spgan_edge_max_dbl_graph(16, 16, 16, 8, 16, 8, None, None, 16, 4, 2, 4, 16, None, None, None, None, 16, 16, 8, None) == -22   # eval with PQbar
    assert lib.spgan_edge_max_dbl_graph(16, 16, 16, 8, 16, 8, None, None, None, 4, 2, 4, 16, None, None, None, None, 16, None, 8, None) == -22  # no idx
    assert lib.spgan_edge_max_dbl_graph(16, 16, 16, 7, 16, 8, None, None, 16, 4, 2, 4, 16, None, None, None, None, 16, None, 8, None) == -22    # ld < 2F


def test_constructor_keyword_and_state_dict():
    import spgan
    m = spgan.edgeConv(16, 32, 10)
    assert m.double_backward is False
    m2 = spgan.edgeConv(16, 32, 10, double_backward=True)
    assert m2.double_backward is True
    assert list(m2.state_dict().keys()) == list(m.state_dict().keys())
    assert not any("double_backward" in n for n in m2.state_dict())
    m.load_state_dict(m2.state_dict(), strict=True)                    # both directions, strictly
    m2.load_state_dict(m.state_dict(), strict=True)
    _, _, sd = ecm.case_tensors("feat", 0)
    m2.load_state_dict(sd, strict=True)
    m2.double_backward = False                                        # a plain attribute
    assert m2.double_backward is False
