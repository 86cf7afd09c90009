"""GPU: spgan.modules.deform_edgeConv_feat (csrc/edge_rank.hip's spgan_edge_weight_* launchers) against the vectors captured from the
reference (golden deform_feat.npz) and each new launcher against the float64 model of tests/deform_feat_model.py.

Tolerances.  Module vs golden with the reference's graph injected: the project's bounds (rel-L2 3e-6 for the output and dx, 5e-6 for
parameter gradients, buffers rtol 1e-5 / atol 1e-6), or 5 x the golden's stored float32-vs-float64 distance of the quantity where that
is larger.  The generator lists the quantities whose 5 x distance exceeds the base bound: a `grad|conv_fea.7.weight` (stored 1.10e-06),
b `grad|conv_fea.1.bias` (1.08e-06), e `grad|conv_fea.7.weight` (2.45e-06); every other quantity keeps the base bound.
Every conv bias sits in front of a train-mode BatchNorm: its gradient is an exact zero here and rounding noise in the reference (2e-3
absolute, the ZERO_GRAD_BIASES rule), in the train-mode cases only.
Launchers vs the float64 model on the same float32 operands: the larger of the project's launcher bounds (2e-6 forward, 1e-5 backward)
and 5 x the rel-L2 distance between a float32 and a float64 CPU evaluation of the model on those operands."""
import numpy as np
import pytest
import torch

import deform_feat_model as fm
import deform_model as dm
from helpers import check, golden

pytestmark = pytest.mark.gpu
TAGS = list(fm.CASES)


@pytest.fixture(scope="module")
def sp():
    import spgan
    from spgan import _lib
    _lib.load()
    return spgan


@pytest.fixture(scope="module")
def d():
    return golden("deform_feat.npz")


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _module(sp, d, tag):
    c = fm.CASES[tag]
    m = sp.deform_edgeConv_feat(c["Fin"], c["Fout"], c["k"], softmax=c["softmax"])
    m.load_state_dict(fm.golden_state_dict(d, tag), strict=True)
    return m.cuda().train(c["train"])


def _run(m, d, tag, inject=True):
    x = torch.from_numpy(d[tag + "|x"]).cuda().requires_grad_(True)
    idx = torch.from_numpy(d[tag + "|idx"]).cuda() if inject else None
    out = m(x, idx=idx)
    (out * torch.from_numpy(d[tag + "|g"]).cuda()).sum().backward()
    return x, out


def _bound(d, tag, q, base):
    return max(base, 5.0 * float(d["%s|noise|%s" % (tag, q)]))


# ---------------------------------------------------------------- module against the reference (golden)
@pytest.mark.parametrize("tag", TAGS)
def test_module_golden_with_injected_graph(sp, d, tag):
    """The 5 x noise fallback applies to a `grad|conv_fea.7.weight` (1.10e-06 stored), b `grad|conv_fea.1.bias` (1.08e-06) and
    e `grad|conv_fea.7.weight` (2.45e-06) only (see the module docstring)."""
    c = fm.CASES[tag]
    train = c["train"]
    m = _module(sp, d, tag)
    x, out = _run(m, d, tag)
    assert tuple(out.shape) == (c["B"], c["Fout"], c["N"])
    e = {"out": check(d, tag + "|out", out, rtol=_bound(d, tag, "out", 3e-6), atol=1e-7),
         "dx": check(d, tag + "|dx", x.grad, rtol=_bound(d, tag, "dx", 3e-6), atol=1e-7)}
    for n, p in m.named_parameters():
        if n in fm.ZERO_GRAD_BIASES and train:
            assert float(p.grad.abs().max()) == 0.0, n                      # exact zeros here
            assert float(np.abs(d["%s|grad|%s|full" % (tag, n)]).max()) <= 2e-3, n
            continue
        if tag == "d" and n.startswith("conv_fea"):                         # k = 1: s == 1, nothing reaches the weight MLP
            assert float(p.grad.abs().max()) == 0.0 and not np.any(d["%s|grad|%s|full" % (tag, n)]), n
            continue
        e[n] = check(d, "%s|grad|%s" % (tag, n), p.grad, rtol=_bound(d, tag, "grad|" + n, 5e-6), atol=1e-7)
    print("%s: rel-L2 vs reference float32 %s" % (tag, {k: "%.2e" % v for k, v in e.items()}))
    bufs = dict(m.named_buffers())
    for n in fm.BUFFERS:
        np.testing.assert_allclose(bufs[n].cpu().numpy(), d["%s|buf|%s|full" % (tag, n)], rtol=1e-5, atol=1e-6, err_msg=n)
        if not train:                                                        # eval mode leaves the buffers untouched (bit for bit)
            assert np.array_equal(bufs[n].cpu().numpy(), d["%s|param|%s" % (tag, n)]), n
        elif n.endswith("num_batches_tracked"):
            assert int(bufs[n]) == int(d["%s|param|%s" % (tag, n)]) + 1, n


@pytest.mark.parametrize("tag", TAGS)
def test_module_own_graph_matches_reference(sp, d, tag):
    c = fm.CASES[tag]
    m = _module(sp, d, tag)
    with torch.no_grad():
        m(torch.from_numpy(d[tag + "|x"]).cuda())
    own = sp.ops.idx_to_local64(m.last_idx, c["B"], c["N"]).view(-1, c["k"]).cpu().numpy()
    ref = d[tag + "|idx"].reshape(-1, c["k"])
    near = d[tag + "|near_tie_rows"].astype(bool)
    assert near.mean() <= 0.01
    assert np.array_equal(own[~near], ref[~near]), int((own[~near] != ref[~near]).any(axis=1).sum())


# ---------------------------------------------------------------- each launcher against the model
def _graph(B, N, k, g, hand=False):
    """int64 [B*N,k] global rows: random permutation prefixes; hand: repeated neighbours, a point nobody gathers, a hub all gather
    (the constructed graph of test_deform_gpu.py)."""
    loc = torch.stack([torch.stack([torch.randperm(N, generator=g)[:k] for _ in range(N)]) for _ in range(B)])       # [B,N,k]
    if hand:
        loc[loc == 1] = 2                              # point 1 of every shape: in-degree 0
        loc[:, :, 0] = 0                               # point 0: gathered by every point (itself included)
        loc[:, 3, :] = 5                               # point 3 gathers the same neighbour k times
        loc[:, 1, 0] = 0
    return (loc + torch.arange(B).view(B, 1, 1) * N).view(B * N, k)


SHAPES = [(2, 50, 5, 3, 20), (1, 77, 20, 16, 24), (3, 43, 1, 64, 256), (1, 70, 8, 72, 64), (1, 40, 32, 16, 9)]


@pytest.mark.parametrize("B,N,k,F1,O", SHAPES)
@pytest.mark.parametrize("hand,soft", [(False, True), (True, True), (False, False)])
def test_launchers_against_model(sp, B, N, k, F1, O, hand, soft):
    """(2,50,5,3,20): the scalar staging path, M no multiple of the tile; (1,77,20,16,24): the workload's k, five rank steps;
    (3,43,1,64,256): k = 1, the vector path, two column groups, M = 129; (1,70,8,72,64): two staging chunks, the second ragged;
    (1,40,32,16,9): the largest k, O no multiple of 4 (the scalar dgrad path).  hand: the constructed graph.  soft=False: s = a3.
    dy is a column slice of a wider tensor (a strided operand).  Every third scale1 / scale3 entry is negative."""
    ew = sp.edge_weight
    g = torch.Generator().manual_seed(B * 1000 + N + F1)
    M = B * N
    PQ = torch.randn(M, 2 * F1, generator=g) * 0.7
    z3 = torch.randn(M, k, F1, generator=g)
    gidx = _graph(B, N, k, g, hand)
    W2i = (torch.rand(O, k * F1, generator=g) * 2 - 1) / np.sqrt(k * F1)
    b2 = torch.randn(O, generator=g) * 0.3
    dy_wide = torch.randn(M, O + 8, generator=g)
    dy = dy_wide[:, 4:4 + O]

    def affine(z):
        mean, var = dm.colstats(z)
        inv = 1.0 / torch.sqrt(var + dm.EPS)
        gamma = torch.rand(F1, generator=g).double() + 0.5
        gamma[::3] *= -1.0
        beta = torch.randn(F1, generator=g).double() * 0.2
        return (gamma * inv).float(), (beta - gamma * inv * mean).float(), mean.float(), inv.float()
    sc1, sh1, mu1, iv1 = affine(dm.pre_norm(PQ.double(), gidx).reshape(M * k, F1))
    sc3, sh3, mu3, iv3 = affine(z3.double().reshape(M * k, F1))

    def model(dt):
        t = lambda v: v.to(dt)
        a = (t(PQ), gidx, t(sc1), t(sh1), t(z3), t(sc3), t(sh3), soft)
        du, su, g3, s3 = fm.wdgrad(t(dy), t(W2i), t(PQ), gidx, t(sc1), t(sh1), t(mu1), t(iv1), t(z3), t(sc3), t(sh3), t(mu3), t(iv3), soft)
        wmax, wrs = fm.norm(t(z3), t(sc3), t(sh3))
        return dict(y=fm.wgemm(*a, t(W2i), t(b2)), yplain=fm.wgemm(*a, t(W2i)), dW=fm.wwgrad(*a, t(dy)), du=du, su=su, g3=g3, s3=s3, wmax=wmax, wrs=wrs,
                    z=fm.gather(t(PQ), gidx))
    m64, m32 = model(torch.float64), model(torch.float32)
    base = dict(y=2e-6, yplain=2e-6, wmax=2e-6, wrs=2e-6, z=2e-6, dW=1e-5, du=1e-5, su=1e-5, g3=1e-5, s3=1e-5)
    bound = {q: max(b, 5.0 * _rel(m32[q], m64[q])) for q, b in base.items()}
    PQg, z3g, Wg, dyg = PQ.cuda(), z3.reshape(M * k, F1).cuda(), W2i.cuda(), dy_wide.cuda()[:, 4:4 + O]
    s1, t1, m1, i1, s3_, t3, m3, i3 = (v.cuda() for v in (sc1, sh1, mu1, iv1, sc3, sh3, mu3, iv3))
    idx = gidx.to(torch.int32).cuda()
    err = {"z": _rel(ew.edge_weight_gather(PQg, idx), m64["z"])}
    wmax, wrs = ew.edge_weight_norm(z3g, k, s3_, t3)
    err["wmax"], err["wrs"] = _rel(wmax, m64["wmax"]), _rel(wrs, m64["wrs"])
    nrm = (wmax, wrs) if soft else None
    y, part, rows = ew.edge_weight_gemm(PQg, idx, s1, t1, z3g, s3_, t3, nrm, Wg, b2.cuda(), stats=True)
    assert tuple(y.shape) == (M, O) and rows == sp.edge_rank.tile_points(k) and tuple(part.shape) == ((M + rows - 1) // rows, O, 2)
    err["y"], err["yplain"] = _rel(y, m64["y"]), _rel(ew.edge_weight_gemm(PQg, idx, s1, t1, z3g, s3_, t3, nrm, Wg), m64["yplain"])
    st = sp.edge_max.edge_max_bn(part, rows, M, torch.ones(O, device="cuda"), torch.zeros(O, device="cuda"), torch.zeros(O, device="cuda"),
                                 torch.ones(O, device="cuda"))
    ymean, yvar = dm.colstats(m64["y"])
    err["mean"], err["invstd"] = _rel(st[3], ymean), _rel(st[2], 1.0 / torch.sqrt(yvar + dm.EPS))
    err["dW"] = _rel(ew.edge_weight_wgrad(PQg, idx, s1, t1, z3g, s3_, t3, nrm, dyg), m64["dW"])
    du, su, g3, s3s = ew.edge_weight_dgrad(dyg, Wg.t().contiguous(), PQg, idx, s1, t1, m1, i1, z3g, s3_, t3, m3, i3, nrm)
    assert tuple(du.shape) == (M, k, F1) and tuple(g3.shape) == (M * k, F1)
    err["du"], err["su"], err["g3"], err["s3"] = _rel(du, m64["du"]), _rel(su, m64["su"]), _rel(g3.view(M, k, F1), m64["g3"]), _rel(s3s, m64["s3"])
    print("B %d N %d k %d F1 %d O %d hand %s soft %s: %s" % (B, N, k, F1, O, hand, soft, {q: "%.2e" % v for q, v in err.items()}))
    if soft and k == 1:                                                      # the weight is exactly 1: the unweighted route's bits
        assert float(g3.abs().max()) == 0.0 and float((wrs - 1).abs().max()) == 0.0
        assert torch.equal(y, sp.edge_rank.edge_rank_gemm(PQg, idx, s1, t1, Wg, b2.cuda()))
    for q in base:
        if float(m64[q].abs().max()) == 0.0:
            assert err[q] == 0.0, q
        else:
            assert err[q] <= bound[q], (q, err[q], bound[q])
    assert err["mean"] < 2e-6 and err["invstd"] < 2e-6, err


# ---------------------------------------------------------------- properties of the module
def test_deterministic(sp, d):
    for tag in ("b", "c"):
        res = []
        for _ in range(2):
            m = _module(sp, d, tag)
            x, out = _run(m, d, tag, inject=False)
            res.append([out.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in m.parameters()] + [b.clone() for b in m.buffers()])
        for a, b in zip(*res):
            assert torch.equal(a, b), tag


def test_single_rank_equals_unweighted_route(sp, d):
    """Case d (k = 1): s == 1 exactly, so the pre-norm output is spgan.edge_rank.edge_rank_gemm's on the same operands (forward bound 2e-6;
    the bits agree in fact, asserted in test_launchers_against_model) and the layer equals deform_edgeConv_first on the shared parameters."""
    m = _module(sp, d, "d")
    ref = sp.deform_edgeConv_first(16, 32, 1).cuda().train()
    ref.load_state_dict({n: v for n, v in m.state_dict().items() if not n.startswith("conv_fea")}, strict=True)
    x = torch.from_numpy(d["d|x"]).cuda()
    idx = torch.from_numpy(d["d|idx"]).cuda()
    with torch.no_grad():
        a, b = m(x, idx=idx), ref(x, idx=idx).view(2, 32, 64)
    err = _rel(a, b)
    print("k = 1: weighted vs unweighted route %.2e" % err)
    assert err <= 2e-6


def test_capture(sp, d):
    """One forward + backward with an injected int32 graph inside spgan.CapturedBody, replayed twice, equals the eager result bit for bit."""
    c = fm.CASES["b"]
    x = torch.from_numpy(d["b|x"]).cuda()
    cot = torch.from_numpy(d["b|g"]).cuda()
    idx = sp.ops.idx_from_local64(torch.from_numpy(d["b|idx"]).cuda(), c["B"], c["N"], c["k"])

    def make():
        m = _module(sp, d, "b")

        def body(x_, cot_, idx_):
            for p in m.parameters():
                p.grad = None
            xg = x_.detach().requires_grad_(True)
            out = m(xg, idx=idx_)
            (out * cot_).sum().backward()
            return (out.detach(), xg.grad) + tuple(p.grad for p in m.parameters())
        return m, body
    m_e, body_e = make()
    eager = [t.clone() for t in body_e(x, cot, idx)]
    m_c, body_c = make()
    cap = sp.CapturedBody(body_c, modules=(m_c,), warmup=1)
    for call in range(4):                                # one eager warm-up, the capture, two replays
        res = cap(x, cot, idx)
        assert not cap.eager
        for a, b in zip(eager, res):
            assert torch.equal(a, b), call
    assert int(m_c.conv2.bn.num_batches_tracked) == 4 and int(m_c.conv_fea[7].num_batches_tracked) == 4


def test_follows_no_operand_mode(sp, d):
    """ops.set_mfma_operands does not reach the layer: the 'f16' mode gives the bits of the default mode."""
    res = []
    for kind in ("f32", "f16"):
        sp.ops.set_mfma_operands(kind)
        try:
            m = _module(sp, d, "b")
            x, out = _run(m, d, "b")
            res.append([out.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in m.parameters()])
        finally:
            sp.ops.set_mfma_operands("f32")
    for a, b in zip(*res):
        assert torch.equal(a, b)


def _composed(x, idx, k, m):
    """The materialised route: spgan.get_edge_features, then torch's conv2d / batch_norm / leaky_relu / softmax and the product."""
    import spgan
    import torch.nn.functional as F_
    e = spgan.get_edge_features(x, k, idx=idx)

    def block(t, conv, bn):
        return F_.leaky_relu(F_.batch_norm(F_.conv2d(t, conv.weight, conv.bias), None, None, bn.weight, bn.bias, True, 0.1, 1e-5), 0.01)
    w = e
    for i in (0, 3, 6):
        w = block(w, m.conv_fea[i], m.conv_fea[i + 1])
    if m.softmax:
        w = F_.softmax(w, dim=-1)
    hs = block(e, m.inte_conv_hk[0], m.inte_conv_hk[1]) * w
    y = F_.conv2d(hs, m.conv2.conv.weight, m.conv2.conv.bias)
    return torch.relu(F_.batch_norm(y, None, None, m.conv2.bn.weight, m.conv2.bn.bias, True, 0.1, 1e-5)).squeeze(3)


def test_memory_against_composed_route(sp):
    """deform_edgeConv_feat(64,128,10) at B = 4, N = 2048: E1 = 21 MB is one [M,k,Fin] tensor, E = 2 E1 the edge tensor.  The peak of one
    forward + backward lies at least 2 E below the composed torch route's, measured here on the same graph (the composed route saves e,
    u, h, z3, a3, s and h*s = 8 E1; the layer z3, du and g3 = 3 E1)."""
    from spgan import fixture_rng as fr
    B, N, Fin, Fout, k = 4, 2048, 64, 128, 10
    m = sp.deform_edgeConv_feat(Fin, Fout, k).cuda().train()
    x0 = fr.normal("deform_feat.mem.x", (B, Fin, N), 0.7).cuda()
    cot = fr.normal("deform_feat.mem.g", (B, Fout, N)).cuda()
    with torch.no_grad():
        m(x0)
    idx = sp.ops.idx_to_local64(m.last_idx, B, N)
    E = B * 2 * Fin * N * k * 4
    peaks, outs = {}, {}
    for name in ("layer", "composed"):
        m.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = m(x, idx=idx) if name == "layer" else _composed(x, idx, k, m)
        (out * cot).sum().backward()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
        outs[name] = (out.detach(), x.grad.clone())
        del out, x
    print("peak layer %.1f MB, composed %.1f MB, E %.1f MB" % (peaks["layer"] / 2**20, peaks["composed"] / 2**20, E / 2**20))
    assert peaks["layer"] <= peaks["composed"] - 2 * E, peaks
    # the two routes are the same function (a plausibility check of the yardstick, not an accuracy test)
    assert _rel(outs["layer"][0], outs["composed"][0]) < 1e-4
    print("dx layer vs composed: %.2e" % _rel(outs["layer"][1], outs["composed"][1]))


def test_refusals(sp, d):
    m = _module(sp, d, "b")
    xg = torch.from_numpy(d["b|x"]).cuda().requires_grad_(True)
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(m(xg).sum(), xg, create_graph=True)
    with pytest.raises(ValueError, match="k=33"):
        sp.deform_edgeConv_feat(4, 4, 33)
    with pytest.raises(RuntimeError, match="no CPU"):
        m(torch.from_numpy(d["b|x"]))
    with pytest.raises(ValueError):
        m(xg[:, :8])                                                         # wrong channel count
    with pytest.raises(IndexError):
        m(xg, idx=torch.full((2, 96 * 20), 96, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        m(xg, idx=torch.zeros(2 * 96, 19, dtype=torch.int32, device="cuda"))
    m.conv_fea[4].momentum = None
    with pytest.raises(NotImplementedError):
        m(xg)
    m.conv_fea[4].momentum = 0.1
    m.conv_fea[7].track_running_stats = False
    with pytest.raises(NotImplementedError):
        m(xg)
