"""GPU: spgan.modules.deform_edgeConv (csrc/edge_rank.hip's spgan_edge_weight_gather2 / spgan_edge_weight_split beside the weighted layer's
launchers) against the vectors captured from the reference (golden deform_xyz.npz) and the two new launchers against the float64 model
of tests/deform_xyz_model.py.

Tolerances, taken from tests/test_deform_feat_gpu.py.  Module vs golden with the reference's graph injected: rel-L2 3e-6 for the output,
dx and dpc, 5e-6 for parameter gradients, buffers rtol 1e-5 / atol 1e-6 -- or 5 x the golden's stored float32-vs-float64 distance of the
quantity where that is larger.  The generator lists the quantities whose 5 x distance exceeds the base bound: a `dpc` (stored 6.28e-07),
b `dpc` (7.88e-07), `grad|conv_fea.1.weight` and `grad|conv_all.4.weight` (1.08e-06 each), e the conv_all gradients and
`grad|conv_xyz.0.bias` (1.0e-06 .. 2.8e-06); every other quantity keeps the base bound.
Every conv bias sits in front of a train-mode BatchNorm: its gradient is an exact zero here and rounding noise in the reference (2e-3
absolute, the ZERO_GRAD_BIASES rule), in the train-mode cases only.  Case d (k = 1): the softmax weight is 1, dpc and every conv_fea /
conv_xyz / conv_all gradient is an exact zero here and in the reference.
Launchers vs the float64 model on the same float32 operands: 2e-6 for w0, 1e-5 for GA, GB and their column sums (the weighted layer's
launcher bounds), or 5 x the rel-L2 distance between a float32 and a float64 CPU evaluation of the model on those operands where that
is larger."""
import numpy as np
import pytest
import torch

import deform_model as dm
import deform_xyz_model as xm
from helpers import check, golden

pytestmark = pytest.mark.gpu
TAGS = list(xm.CASES)


@pytest.fixture(scope="module")
def sp():
    import spgan
    from spgan import _lib
    _lib.load()
    return spgan


@pytest.fixture(scope="module")
def d():
    return golden("deform_xyz.npz")


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _module(sp, d, tag):
    c = xm.CASES[tag]
    m = sp.deform_edgeConv(c["F"], c["F"], c["k"], softmax=c["softmax"])
    m.load_state_dict(xm.golden_state_dict(d, tag), strict=True)
    return m.cuda().train(c["train"])


def _run(m, d, tag, inject=True):
    x = torch.from_numpy(d[tag + "|x"]).cuda().requires_grad_(True)
    pc = torch.from_numpy(d[tag + "|pc"]).cuda().requires_grad_(True)
    idx = torch.from_numpy(d[tag + "|idx"]).cuda() if inject else None
    out = m(x, pc, idx=idx)
    (out * torch.from_numpy(d[tag + "|g"]).cuda()).sum().backward()
    return x, pc, out


def _bound(d, tag, q, base):
    return max(base, 5.0 * xm.noise(d, tag, q))


def _single_rank_zero(tag, n):
    return tag == "d" and n.startswith(xm.SINGLE_RANK_ZERO)


# ---------------------------------------------------------------- module against the reference (golden)
@pytest.mark.parametrize("tag", TAGS)
def test_module_golden_with_injected_graph(sp, d, tag):
    c = xm.CASES[tag]
    train = c["train"]
    m = _module(sp, d, tag)
    x, pc, out = _run(m, d, tag)
    assert tuple(out.shape) == (c["B"], c["F"], c["N"])
    e = {"out": check(d, tag + "|out", out, rtol=_bound(d, tag, "out", 3e-6), atol=1e-7),
         "dx": check(d, tag + "|dx", x.grad, rtol=_bound(d, tag, "dx", 3e-6), atol=1e-7)}
    if tag == "d":                                                          # k = 1: s == 1, nothing reaches the weight side
        assert float(pc.grad.abs().max()) == 0.0 and not np.any(d["d|dpc|full"])
    else:
        e["dpc"] = check(d, tag + "|dpc", pc.grad, rtol=_bound(d, tag, "dpc", 3e-6), atol=1e-7)
    for n, p in m.named_parameters():
        if n in xm.ZERO_GRAD_BIASES and train:
            assert float(p.grad.abs().max()) == 0.0, n                      # exact zeros here
            assert float(np.abs(d["%s|grad|%s|full" % (tag, n)]).max()) <= 2e-3, n
            continue
        if _single_rank_zero(tag, n):
            assert float(p.grad.abs().max()) == 0.0 and not np.any(d["%s|grad|%s|full" % (tag, n)]), n
            continue
        e[n] = check(d, "%s|grad|%s" % (tag, n), p.grad, rtol=_bound(d, tag, "grad|" + n, 5e-6), atol=1e-7)
    print("%s: rel-L2 vs reference float32 %s" % (tag, {k: "%.2e" % v for k, v in e.items()}))
    bufs = dict(m.named_buffers())
    for n in xm.BUFFERS:
        np.testing.assert_allclose(bufs[n].cpu().numpy(), d["%s|buf|%s|full" % (tag, n)], rtol=1e-5, atol=1e-6, err_msg=n)
        if not train:                                                        # eval mode leaves the buffers untouched (bit for bit)
            assert np.array_equal(bufs[n].cpu().numpy(), xm.param(d, tag, n)), n
        elif n.endswith("num_batches_tracked"):
            assert int(bufs[n]) == int(xm.param(d, tag, n)) + 1, n


@pytest.mark.parametrize("tag", ["a", "b"])
def test_module_own_graph_matches_reference(sp, d, tag):
    """The layer's own kNN graph (a: the fp64 coordinate mode, b: the feature mode): every row that differs from the reference's graph is
    a near-tie row, and where no row differs the results are the injected graph's, bit for bit."""
    c = xm.CASES[tag]
    m = _module(sp, d, tag)
    x, pc, out = _run(m, d, tag, inject=False)
    own = sp.ops.idx_to_local64(m.last_idx, c["B"], c["N"]).view(-1, c["k"]).cpu().numpy()
    ref = d[tag + "|idx"].reshape(-1, c["k"])
    near = d[tag + "|near_tie_rows"].astype(bool)
    assert near.mean() <= 0.01
    differ = (own != ref).any(axis=1)
    assert not differ[~near].any(), int(differ[~near].sum())
    if not differ.any():                                                     # the same graph: the injected route's bits
        m2 = _module(sp, d, tag)
        x2, pc2, out2 = _run(m2, d, tag)
        assert torch.equal(out, out2) and torch.equal(x.grad, x2.grad) and torch.equal(pc.grad, pc2.grad)
    print("%s: %d rows differ from the reference's graph (%d near-tie rows)" % (tag, int(differ.sum()), int(near.sum())))


# ---------------------------------------------------------------- the two launchers against the model
def _graph(B, N, k, g, hand=False):
    """int64 [B*N,k] global rows: random permutation prefixes; hand: point 0 is also a neighbour of every point (a hub with in-degree
    N), points nobody gathers, a point that gathers one neighbour k times."""
    loc = torch.stack([torch.stack([torch.randperm(N, generator=g)[:k] for _ in range(N)]) for _ in range(B)])       # [B,N,k]
    if hand:
        loc[loc == 1] = 2                              # points 1 and 4 of every shape: in-degree 0
        loc[loc == 4] = 6
        loc[:, :, 0] = 0                               # point 0: gathered by every point (itself included)
        loc[:, 3, :] = 5                               # point 3 gathers the same neighbour k times
    return (loc + torch.arange(B).view(B, 1, 1) * N).view(B * N, k)


SHAPES = [(2, 50, 5, 16), (1, 77, 20, 16), (3, 43, 1, 16), (1, 40, 32, 8), (1, 33, 7, 5)]


@pytest.mark.parametrize("B,N,k,F", SHAPES)
@pytest.mark.parametrize("hand", [False, True])
def test_launchers_against_model(sp, B, N, k, F, hand):
    """(2,50,5,16): M no multiple of the record tile, four tiles; (1,77,20,16): the workload's k; (3,43,1,16): k = 1, M = 129;
    (1,40,32,8): the largest k, two 16-byte pieces per row; (1,33,7,5): rows that are no multiple of four floats (the scalar path, the
    channel groups do not divide a wave).  hand: the constructed graph.  Every third scale entry is negative."""
    ew = sp.edge_weight
    g = torch.Generator().manual_seed(B * 1000 + N + F)
    M = B * N
    PQa, PQb = torch.randn(M, 2 * F, generator=g) * 0.7, torch.randn(M, 2 * F, generator=g) * 0.7
    dw0 = torch.randn(M * k, F, generator=g)
    gidx = _graph(B, N, k, g, hand)

    def affine(z):
        mean, var = dm.colstats(z)
        inv = 1.0 / torch.sqrt(var + dm.EPS)
        gamma = torch.rand(F, generator=g).double() + 0.5
        gamma[::3] *= -1.0
        beta = torch.randn(F, generator=g).double() * 0.2
        return (gamma * inv).float(), (beta - gamma * inv * mean).float(), mean.float(), inv.float()
    sa, ta, ma, ia = affine(dm.pre_norm(PQa.double(), gidx).reshape(M * k, F))
    sb, tb, mb, ib = affine(dm.pre_norm(PQb.double(), gidx).reshape(M * k, F))

    def model(dt):
        t = lambda v: v.to(dt)
        ga, sua, gb, sub = xm.split(t(dw0), t(PQa), t(PQb), gidx, t(sa), t(ta), t(ma), t(ia), t(sb), t(tb), t(mb), t(ib))
        return dict(w0=xm.gather2(t(PQa), t(PQb), gidx, t(sa), t(ta), t(sb), t(tb)), ga=ga, sua=sua, gb=gb, sub=sub)
    m64, m32 = model(torch.float64), model(torch.float32)
    base = dict(w0=2e-6, ga=1e-5, sua=1e-5, gb=1e-5, sub=1e-5)
    bound = {q: max(b, 5.0 * _rel(m32[q], m64[q])) for q, b in base.items()}
    idx = gidx.to(torch.int32).cuda()
    dev = [v.cuda() for v in (sa, ta, ma, ia, sb, tb, mb, ib)]
    w0 = ew.edge_weight_gather2(PQa.cuda(), PQb.cuda(), idx, dev[0], dev[1], dev[4], dev[5])
    ga, sua, gb, sub = ew.edge_weight_split(dw0.cuda(), PQa.cuda(), PQb.cuda(), idx, *dev)
    assert tuple(w0.shape) == (M * k, F) and tuple(ga.shape) == tuple(gb.shape) == (M, k, F) and tuple(sua.shape) == tuple(sub.shape) == (2 * F,)
    err = dict(w0=_rel(w0, m64["w0"]), ga=_rel(ga, m64["ga"]), sua=_rel(sua, m64["sua"]), gb=_rel(gb, m64["gb"]), sub=_rel(sub, m64["sub"]))
    print("B %d N %d k %d F %d hand %s: %s" % (B, N, k, F, hand, {q: "%.2e" % v for q, v in err.items()}))
    for q in base:
        assert err[q] <= bound[q], (q, err[q], bound[q])
    # the backward multiplies with the forward's activations, bit for bit: with dw0 = 1 and both pre-activations positive GA is a_b and GB
    # is a_a, so their product is the forward's w0
    one = torch.ones_like(dw0).cuda()
    ga1, _, gb1, _ = ew.edge_weight_split(one, PQa.cuda(), PQb.cuda(), idx, *dev)
    both = (ga1.view(M * k, F) > 0) & (gb1.view(M * k, F) > 0) & (w0 > 0)          # both pre-activations positive: ga1 = a_b, gb1 = a_a
    assert torch.equal((ga1.view(M * k, F) * gb1.view(M * k, F))[both], w0[both])
    # the scatter launch takes the records unchanged: dPQ of branch a against the model
    rowptr, src = sp.ops.csr_build(idx, B, N)
    dPQ = sp.edge_rank.edge_rank_scatter(ga, rowptr, src, dev[0], PQa.cuda(), idx, dev[2], dev[3], sua)
    ref = dm.rank_scatter(m64["ga"], gidx, sa.double(), PQa.double(), ma.double(), ia.double(), m64["sua"])
    assert _rel(dPQ, ref) <= max(1e-5, 5.0 * _rel(dm.rank_scatter(m32["ga"], gidx, sa, PQa, ma, ia, m32["sua"]), ref))


# ---------------------------------------------------------------- properties of the module
def test_deterministic(sp, d):
    for tag in ("b", "c"):
        res = []
        for _ in range(2):
            m = _module(sp, d, tag)
            x, pc, out = _run(m, d, tag, inject=False)
            res.append([out.detach().clone(), x.grad.clone(), pc.grad.clone()] + [p.grad.clone() for p in m.parameters()] +
                       [b.clone() for b in m.buffers()])
        for a, b in zip(*res):
            assert torch.equal(a, b), tag


def test_capture(sp, d):
    """One forward + backward with an injected int32 graph inside spgan.CapturedBody, replayed twice, equals the eager result bit for bit."""
    c = xm.CASES["b"]
    x = torch.from_numpy(d["b|x"]).cuda()
    pc = torch.from_numpy(d["b|pc"]).cuda()
    cot = torch.from_numpy(d["b|g"]).cuda()
    idx = sp.ops.idx_from_local64(torch.from_numpy(d["b|idx"]).cuda(), c["B"], c["N"], c["k"])

    def make():
        m = _module(sp, d, "b")

        def body(x_, pc_, cot_, idx_):
            for p in m.parameters():
                p.grad = None
            xg, pg = x_.detach().requires_grad_(True), pc_.detach().requires_grad_(True)
            out = m(xg, pg, idx=idx_)
            (out * cot_).sum().backward()
            return (out.detach(), xg.grad, pg.grad) + tuple(p.grad for p in m.parameters())
        return m, body
    m_e, body_e = make()
    eager = [t.clone() for t in body_e(x, pc, cot, idx)]
    m_c, body_c = make()
    cap = sp.CapturedBody(body_c, modules=(m_c,), warmup=1)
    for call in range(4):                                # one eager warm-up, the capture, two replays
        res = cap(x, pc, cot, idx)
        assert not cap.eager
        for a, b in zip(eager, res):
            assert torch.equal(a, b), call
    assert int(m_c.conv2[1].num_batches_tracked) == 4 and int(m_c.conv_xyz[1].num_batches_tracked) == 4


def test_follows_no_operand_mode(sp, d):
    """ops.set_mfma_operands does not reach the layer: the 'f16' mode gives the bits of the default mode."""
    res = []
    for kind in ("f32", "f16"):
        sp.ops.set_mfma_operands(kind)
        try:
            m = _module(sp, d, "b")
            x, pc, out = _run(m, d, "b")
            res.append([out.detach().clone(), x.grad.clone(), pc.grad.clone()] + [p.grad.clone() for p in m.parameters()])
        finally:
            sp.ops.set_mfma_operands("f32")
    for a, b in zip(*res):
        assert torch.equal(a, b)


def _composed(x, pc, idx, k, m):
    """The materialised route: spgan.get_edge_features for both tensors on one graph, then torch's conv2d / batch_norm / leaky_relu /
    softmax and the product -- the reference's formulation."""
    import spgan
    import torch.nn.functional as F_
    e, y = spgan.get_edge_features(x, k, idx=idx), spgan.get_edge_features(pc, k, idx=idx)

    def block(t, conv, bn):
        return F_.leaky_relu(F_.batch_norm(F_.conv2d(t, conv.weight, conv.bias), None, None, bn.weight, bn.bias, True, 0.1, 1e-5), 0.01)
    w = block(e, m.conv_fea[0], m.conv_fea[1]) * block(y, m.conv_xyz[0], m.conv_xyz[1])
    for i in (0, 3):
        w = block(w, m.conv_all[i], m.conv_all[i + 1])
    if m.softmax:
        w = F_.softmax(w, dim=-1)
    hs = block(e, m.inte_conv_hk[0], m.inte_conv_hk[1]) * w
    return block(hs, m.conv2[0], m.conv2[1]).squeeze(3)


def test_memory_against_composed_route(sp):
    """deform_edgeConv(64,64,10) at B = 4, N = 2048: E1 = 21 MB is one [M,k,Fin] tensor, E = 2 E1 = 4 M k Fin bytes the edge tensor.  The
    peak of one forward + backward lies at least 2 E below the composed torch route's, measured here on the same graph."""
    from spgan import fixture_rng as fr
    B, N, F, k = 4, 2048, 64, 10
    m = sp.deform_edgeConv(F, F, k).cuda().train()
    x0 = fr.normal("deform_xyz.mem.x", (B, F, N), 0.7).cuda()
    pc0 = fr.uniform("deform_xyz.mem.pc", (B, 3, N), -1.0, 1.0).cuda()
    cot = fr.normal("deform_xyz.mem.g", (B, F, N)).cuda()
    with torch.no_grad():
        m(x0, pc0)
    idx = sp.ops.idx_to_local64(m.last_idx, B, N)
    E = B * 2 * F * N * k * 4
    peaks, outs = {}, {}
    for name in ("layer", "composed"):
        m.zero_grad(set_to_none=True)
        x, pc = x0.clone().requires_grad_(True), pc0.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = m(x, pc, idx=idx) if name == "layer" else _composed(x, pc, idx, k, m)
        (out * cot).sum().backward()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
        outs[name] = (out.detach(), x.grad.clone(), pc.grad.clone())
        del out, x, pc
    print("peak layer %.1f MB, composed %.1f MB, E %.1f MB, margin %.2f E" % (peaks["layer"] / 2**20, peaks["composed"] / 2**20, E / 2**20,
                                                                             (peaks["composed"] - peaks["layer"]) / E))
    assert peaks["layer"] <= peaks["composed"] - 2 * E, peaks
    # the two routes are the same function (a plausibility check of the yardstick, not an accuracy test)
    assert _rel(outs["layer"][0], outs["composed"][0]) < 1e-4
    print("dx layer vs composed: %.2e, dpc: %.2e" % (_rel(outs["layer"][1], outs["composed"][1]), _rel(outs["layer"][2], outs["composed"][2])))


def test_refusals(sp, d):
    m = _module(sp, d, "b")
    xg = torch.from_numpy(d["b|x"]).cuda().requires_grad_(True)
    pc = torch.from_numpy(d["b|pc"]).cuda()
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(m(xg, pc).sum(), xg, create_graph=True)
    with pytest.raises(ValueError, match="k=33"):
        sp.deform_edgeConv(4, 4, 33)
    with pytest.raises(ValueError, match="Fin=32.*Fout=48"):
        sp.deform_edgeConv(32, 48, 20).cuda()(xg, pc)
    with pytest.raises(RuntimeError, match="no CPU"):
        m(torch.from_numpy(d["b|x"]), pc)
    with pytest.raises(RuntimeError, match="no CPU"):
        m(xg, torch.from_numpy(d["b|pc"]))
    with pytest.raises(ValueError):
        m(xg[:, :8], pc)                                                     # wrong channel count
    for bad in (pc[:, :2], pc[:, :, :50], pc[:1], pc[0]):
        with pytest.raises(ValueError, match=r"pc must be \[B,3,N\]"):
            m(xg, bad)
    with pytest.raises(IndexError):
        m(xg, pc, idx=torch.full((2, 96 * 20), 96, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        m(xg, pc, idx=torch.zeros(2 * 96, 19, dtype=torch.int32, device="cuda"))
    m.conv2[2].negative_slope = 0.2
    with pytest.raises(NotImplementedError, match="slope"):
        m(xg, pc)
    m.conv2[2].negative_slope = 0.01
    m.conv_xyz[1].momentum = None
    with pytest.raises(NotImplementedError):
        m(xg, pc)
    m.conv_xyz[1].momentum = 0.1
    m.conv_all[4].track_running_stats = False
    with pytest.raises(NotImplementedError):
        m(xg, pc)
