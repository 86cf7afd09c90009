"""GPU: spgan.modules.bilateral_upsample_edgeConv (csrc/edge_rank.hip's spgan_edge_stored_gemm / _wgrad / _dgrad beside the rank-window and
weighted-layer launchers) against the vectors captured from the reference (golden bilateral.npz), the three new launchers against the
float64 model of tests/bilateral_model.py, and the layer against spgan.upsample_edgeConv where the weight is the constant 1/k.

Tolerances, the siblings' (tests/test_deform_xyz_gpu.py).  Module vs golden with the reference's graph injected: rel-L2 3e-6 for the output,
dx and dpc, 5e-6 for parameter gradients, buffers rtol 1e-5 / atol 1e-6 -- or 5 x the golden's stored float32-vs-float64 distance of the
quantity where that is larger (`_bound`; the capture script lists the quantities that take the fallback: e `grad|conv_all.4.weight`, stored
1.25e-06).  Every conv bias sits in front of a train-mode BatchNorm: its gradient is an exact zero here and rounding noise in the
reference (2e-3 absolute), in the train-mode cases only.
Launchers vs the float64 model on the same float32 operands: 2e-6 for the product and the gradients, 1e-5 for the column sums (the
weighted layer's launcher bounds), or 5 x the rel-L2 distance between a float32 and a float64 CPU evaluation of the model on those
operands where that is larger."""
import numpy as np
import pytest
import torch

import bilateral_model as bm
import deform_model as dm
import upsample_model as um
from helpers import check, golden

pytestmark = pytest.mark.gpu
TAGS = list(bm.CASES)


@pytest.fixture(scope="module")
def sp():
    import spgan
    from spgan import _lib
    _lib.load()
    return spgan


@pytest.fixture(scope="module")
def d():
    return golden("bilateral.npz")


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _module(sp, d, tag):
    c = bm.CASES[tag]
    m = sp.bilateral_upsample_edgeConv(c["Fin"], c["Fout"], c["k"], -1, softmax=c["softmax"])
    m.load_state_dict(bm.golden_state_dict(d, tag), strict=True)
    return m.cuda().train(c["train"])


def _run(m, d, tag, inject=True):
    x = torch.from_numpy(d[tag + "|x"]).cuda().requires_grad_(True)
    pc = torch.from_numpy(d[tag + "|pc"]).cuda().requires_grad_(True)
    idx = torch.from_numpy(d[tag + "|idx"]).cuda() if inject else None
    out = m(x, pc, idx=idx)
    (out * torch.from_numpy(d[tag + "|g"]).cuda()).sum().backward()
    return x, pc, out


def _bound(d, tag, q, base):
    return max(base, 5.0 * bm.noise(d, tag, q))


# ---------------------------------------------------------------- module against the reference (golden)
@pytest.mark.parametrize("tag", TAGS)
def test_module_golden_with_injected_graph(sp, d, tag):
    c = bm.CASES[tag]
    train = c["train"]
    m = _module(sp, d, tag)
    assert tuple(m.state_dict()) == bm.STATE_KEYS and len(bm.STATE_KEYS) == 42
    x, pc, out = _run(m, d, tag)
    assert tuple(out.shape) == (c["B"], c["Fout"], 2 * c["N"])
    e = {"out": check(d, tag + "|out", out, rtol=_bound(d, tag, "out", 3e-6), atol=1e-7),
         "dx": check(d, tag + "|dx", x.grad, rtol=_bound(d, tag, "dx", 3e-6), atol=1e-7),
         "dpc": check(d, tag + "|dpc", pc.grad, rtol=_bound(d, tag, "dpc", 3e-6), atol=1e-7)}
    for n, p in m.named_parameters():
        if n in bm.ZERO_GRAD_BIASES and train:
            assert float(p.grad.abs().max()) == 0.0, n                      # exact zeros here
            assert float(np.abs(d["%s|grad|%s|full" % (tag, n)]).max()) <= 2e-3, n
            continue
        e[n] = check(d, "%s|grad|%s" % (tag, n), p.grad, rtol=_bound(d, tag, "grad|" + n, 5e-6), atol=1e-7)
    print("%s: rel-L2 vs reference float32 %s" % (tag, {k: "%.2e" % v for k, v in e.items()}))
    print("%s: reference noise out %.2e" % (tag, bm.noise(d, tag, "out")))
    bufs = dict(m.named_buffers())
    for n in bm.BUFFERS:
        np.testing.assert_allclose(bufs[n].cpu().numpy(), d["%s|buf|%s|full" % (tag, n)], rtol=1e-5, atol=1e-6, err_msg=n)
        if not train:                                                        # eval mode leaves the buffers untouched (bit for bit)
            assert np.array_equal(bufs[n].cpu().numpy(), bm.param(d, tag, n)), n
        elif n.endswith("num_batches_tracked"):
            assert int(bufs[n]) == int(bm.param(d, tag, n)) + 1, n
    # the reference's checkpoint format, both ways
    back = sp.bilateral_upsample_edgeConv(c["Fin"], c["Fout"], c["k"], -1, softmax=c["softmax"])
    back.load_state_dict(m.state_dict(), strict=True)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_module_own_graph_matches_reference(sp, d, tag):
    """The layer's own kNN graph (a: the fp64 coordinate mode, b: the feature mode): every row that differs from the reference's graph is
    a near-tie row, and where no row differs the results are the injected graph's, bit for bit."""
    c = bm.CASES[tag]
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


# ---------------------------------------------------------------- the three launchers against the model
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


def _operands(B, N, k, C, hand, seed):
    """U and z3 [M,k,2C] as the layer makes them from a graph: U = the rank-window product over the graph's differences (rows (i,t), 4C
    channels, read as rows (i, 2t+h)), z3 = rows gathered through the graph in the paired rank order -- a repeated neighbour gives equal
    rows, and with them ties inside the softmax.  The BatchNorm vectors come from the tensors' own statistics; every third gamma is
    negative."""
    g = torch.Generator().manual_seed(seed)
    M, F1, T, w = B * N, 2 * C, k // 2, k // 2 + 1
    gidx = _graph(B, N, k, g, hand)
    x = torch.randn(M, C, generator=g) * 0.7
    U = um.window_gemm(x, gidx, torch.randn(4 * C, w * C, generator=g) / np.sqrt(w * C), w, rowadd=torch.randn(M, 4 * C, generator=g) * 0.3)
    U = U.reshape(M, k, F1).contiguous()
    gp = gidx.view(M, 2, T).transpose(1, 2).reshape(M, k)
    z3 = dm.pre_norm(torch.randn(M, 2 * F1, generator=g) * 0.7, gp).contiguous()

    def affine(z, n):
        mean, var = dm.colstats(z.double())
        inv = 1.0 / torch.sqrt(var + dm.EPS)
        gamma = torch.rand(n, generator=g).double() + 0.5
        gamma[::3] *= -1.0
        beta = torch.randn(n, generator=g).double() * 0.2
        return (gamma * inv).float(), (beta - gamma * inv * mean).float(), mean.float(), inv.float()
    st1 = affine(U.view(M * T, 2 * F1), 2 * F1)
    st3 = affine(z3.view(M * k, F1), F1)
    return U, z3, st1, st3, g


SHAPES = [(1, 33, 2, 3), (2, 50, 4, 3), (1, 70, 8, 40), (2, 64, 28, 16), (2, 96, 10, 32)]


@pytest.mark.parametrize("B,N,k,C", SHAPES)
@pytest.mark.parametrize("hand,soft", [(False, True), (True, True), (True, False)])
def test_launchers_against_model(sp, B, N, k, C, hand, soft):
    """(1,33,2,3): one window position, two ranks, the scalar path, two point tiles with one point in the second; (2,50,4,3): the scalar
    path, M no multiple of the tile; (1,70,8,40): a full staging chunk and a ragged one; (2,64,28,16): the largest k; (2,96,10,32): the
    workload's k.  hand: the constructed graph.  soft=False: s = a3."""
    ew = sp.edge_weight
    U, z3, (sc1, sh1, mu1, inv1), (sc3, sh3, mu3, inv3), g = _operands(B, N, k, C, hand, B * 1000 + N + C)
    M, F1, O = B * N, 2 * C, 24 if C != 32 else 136                          # 136: two groups of output columns, the second ragged
    W2i = (torch.randn(O, k * F1, generator=g) / np.sqrt(k * F1))
    dy = torch.randn(M, O, generator=g)

    def model(dt):
        t = lambda v: v.to(dt)
        gU, su, g3, s3 = bm.stored_dgrad(t(dy), t(W2i), t(U), t(sc1), t(sh1), t(mu1), t(inv1), t(z3), t(sc3), t(sh3), t(mu3), t(inv3), soft)
        return dict(y=bm.stored_gemm(t(U), t(sc1), t(sh1), t(z3), t(sc3), t(sh3), soft, t(W2i)),
                    dW=bm.stored_wgrad(t(U), t(sc1), t(sh1), t(z3), t(sc3), t(sh3), soft, t(dy)), gU=gU, su=su, g3=g3, s3=s3)
    m64, m32 = model(torch.float64), model(torch.float32)
    base = dict(y=2e-6, dW=2e-6, gU=2e-6, g3=2e-6, su=1e-5, s3=1e-5)
    bound = {q: max(b, 5.0 * _rel(m32[q], m64[q])) for q, b in base.items()}
    dev = lambda *ts: [t.cuda() for t in ts]
    Ud, zd, W2d, dyd = dev(U, z3.view(M * k, F1), W2i, dy)
    a1, a3 = dev(sc1, sh1, mu1, inv1), dev(sc3, sh3, mu3, inv3)
    norm = ew.edge_weight_norm(zd, k, a3[0], a3[1]) if soft else None
    y = ew.edge_stored_gemm(Ud, k, a1[0], a1[1], zd, a3[0], a3[1], norm, W2d)
    dW = ew.edge_stored_wgrad(Ud, k, a1[0], a1[1], zd, a3[0], a3[1], norm, dyd)
    gU, su, g3, s3 = ew.edge_stored_dgrad(dyd, W2d.t().contiguous(), Ud, k, *a1, zd, *a3, norm)
    assert tuple(y.shape) == (M, O) and tuple(dW.shape) == (O, k * F1) and tuple(gU.shape) == (M, k, F1) and tuple(g3.shape) == (M * k, F1)
    assert tuple(su.shape) == (4 * F1,) and tuple(s3.shape) == (2 * F1,)
    err = dict(y=_rel(y, m64["y"]), dW=_rel(dW, m64["dW"]), gU=_rel(gU, m64["gU"]), g3=_rel(g3.view(M, k, F1), m64["g3"]), su=_rel(su, m64["su"]),
               s3=_rel(s3, m64["s3"]))
    print("B %d N %d k %d C %d hand %s soft %s: %s" % (B, N, k, C, hand, soft, {q: "%.2e" % v for q, v in err.items()}))
    for q in base:
        assert err[q] <= bound[q], (q, err[q], bound[q])
    # the product with bias and statistics records, as the siblings' launcher hands them to the BatchNorm finalize
    b2 = torch.randn(O, generator=g).cuda()
    yb, part, tile_rows = ew.edge_stored_gemm(Ud, k, a1[0], a1[1], zd, a3[0], a3[1], norm, W2d, b2, stats=True)
    assert torch.equal(yb, y + b2) and part.shape[1:] == (O, 2) and tile_rows == sp.edge_rank.tile_points(k)
    assert _rel(part[:, :, 0].sum(dim=0), yb.double().sum(dim=0)) <= 1e-5


@pytest.mark.parametrize("B,N,k,C", [(1, 33, 2, 3), (2, 50, 4, 3), (2, 64, 28, 16), (1, 70, 8, 40)])
def test_launchers_share_the_weight_bits(sp, B, N, k, C):
    """Forward product, weight gradient and input gradient form h and s with the same bits.  With dm = 1 (dy = 1 [M,1], W2t = 1) the
    input gradient hands out s (softmax on: gU = s where a1 > 0) and h (softmax off: g3 = h where a3 > 0); their float32 product must be
    the h*s that the product launch stages (W2i = the identity: y = (h*s).flat, sums of one product and zeros) and that the weight
    gradient stages (dy = one point's indicator: row 0 of dW2i = that point's h*s)."""
    ew = sp.edge_weight
    U, z3, (sc1, sh1, mu1, inv1), (sc3, sh3, mu3, inv3), g = _operands(B, N, k, C, True, 77 + k)
    M, F1 = B * N, 2 * C
    K = k * F1
    Ud, zd = U.cuda(), z3.view(M * k, F1).cuda()
    a1, a3 = [t.cuda() for t in (sc1, sh1, mu1, inv1)], [t.cuda() for t in (sc3, sh3, mu3, inv3)]
    norm = ew.edge_weight_norm(zd, k, a3[0], a3[1])
    one, onesK = torch.ones(M, 1, device="cuda"), torch.ones(K, 1, device="cuda")
    s_bits = ew.edge_stored_dgrad(one, onesK, Ud, k, *a1, zd, *a3, norm)[0].view(M, K)
    h_bits = ew.edge_stored_dgrad(one, onesK, Ud, k, *a1, zd, *a3, None)[2].view(M, K)
    par = (torch.arange(k) % 2).cuda()
    # the sign of the kernels' fused multiply-add: the product is exact in float64, and rounding the sum keeps its sign
    pos1 = ((Ud.double() * a1[0].double().view(2, F1)[par] + a1[1].double().view(2, F1)[par]) > 0).view(M, K)
    pos3 = ((zd.double() * a3[0].double() + a3[1].double()) > 0).view(M, K)
    both = pos1 & pos3 & (s_bits > 0) & (h_bits > 0)
    assert float(both.float().mean()) > 0.05
    hs = ew.edge_stored_gemm(Ud, k, a1[0], a1[1], zd, a3[0], a3[1], norm, torch.eye(K, device="cuda"))
    assert torch.equal((h_bits * s_bits)[both], hs[both])
    for i0 in (0, M - 1):
        ind = torch.zeros(M, 1, device="cuda")
        ind[i0, 0] = 1.0
        row = ew.edge_stored_wgrad(Ud, k, a1[0], a1[1], zd, a3[0], a3[1], norm, ind)[0]
        assert torch.equal(row, hs[i0])


def test_launcher_argument_checks(sp):
    ew = sp.edge_weight
    M, k, F1, O = 8, 4, 4, 4
    U, z3 = torch.zeros(M, k, F1, device="cuda"), torch.zeros(M * k, F1, device="cuda")
    v1, v3, W = torch.ones(2 * F1, device="cuda"), torch.ones(F1, device="cuda"), torch.zeros(O, k * F1, device="cuda")
    with pytest.raises(ValueError, match="k=3"):
        ew.edge_stored_gemm(U, 3, v1, v1, z3, v3, v3, None, W)
    with pytest.raises(ValueError, match="k=30"):
        ew.edge_stored_gemm(U, 30, v1, v1, z3, v3, v3, None, W)
    with pytest.raises(ValueError):
        ew.edge_stored_gemm(U[:, :2], k, v1, v1, z3, v3, v3, None, W)               # U and z3 disagree
    with pytest.raises(ValueError):
        ew.edge_stored_gemm(U, k, v3, v1, z3, v3, v3, None, W)                      # scale1 needs 2*F1 entries
    with pytest.raises(ValueError):
        ew.edge_stored_wgrad(U, k, v1, v1, z3, v3, v3, None, torch.zeros(M + 1, O, device="cuda"))
    with pytest.raises(ValueError):
        ew.edge_stored_dgrad(torch.zeros(M, O, device="cuda"), W, U, k, v1, v1, v1, v1, z3, v3, v3, v3, v3, None)      # W2t is [k*F1, O]
    lib = sp._lib.load()
    assert lib.spgan_edge_stored_gemm(None, M, k, F1, None, None, 0.01, None, None, None, None, None, None, 0, None, O, None, 0, None, None) != 0


# ---------------------------------------------------------------- against the existing layer
@pytest.mark.parametrize("k", [4, 8])
def test_constant_weight_equals_upsample_edgeconv(sp, k):
    """conv_all's last BatchNorm with weight = bias = 0: a3 = 0, the softmax weight is 1/k everywhere (exact for k = 4, 8), and the layer
    is upsample_edgeConv with the same inte_conv_hk and conv2's taps k..2k-1 scaled by 1/k.  Two fp32 routes, each within the 2e-6 launcher
    bound of the float64 model: 4e-6.  Nothing reaches the weight branch: dpc and the conv_xyz / conv_fea gradients are exact zeros."""
    from spgan import fixture_rng as fr
    B, N, C, F = 2, 64, 16, 16
    torch.manual_seed(k)
    m = sp.bilateral_upsample_edgeConv(C, F, k, -1).cuda().train()
    u = sp.upsample_edgeConv(C, F, k, -1).cuda().train()
    with torch.no_grad():
        m.conv_all[4].weight.zero_()
        m.conv_all[4].bias.zero_()
        u.inte_conv_hk.load_state_dict(m.inte_conv_hk.state_dict())
        u.conv2.load_state_dict(m.conv2.state_dict())
        u.conv2.conv.weight[:, :, :, k:] *= 1.0 / k
    x0 = fr.normal("bilateral.const.x", (B, C, N), 0.7, salt=k).cuda()
    pc0 = fr.uniform("bilateral.const.pc", (B, 3, N), -1.0, 1.0, salt=k).cuda()
    cot = fr.normal("bilateral.const.g", (B, F, 2 * N), salt=k).cuda()
    x, pc, xu = x0.clone().requires_grad_(True), pc0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    out = m(x, pc)
    (out * cot).sum().backward()
    out_u = u(xu, idx=m.last_idx)
    (out_u * cot).sum().backward()
    e = (_rel(out, out_u), _rel(x.grad, xu.grad))
    print("k %d: out %.2e dx %.2e" % ((k,) + e))
    assert e[0] <= 4e-6 and e[1] <= 4e-6
    assert _rel(m.inte_conv_hk[0].weight.grad, u.inte_conv_hk[0].weight.grad) <= 4e-6
    assert _rel(m.conv2.conv.weight.grad[:, :, :, :k], u.conv2.conv.weight.grad[:, :, :, :k]) <= 4e-6
    assert float(pc.grad.abs().max()) == 0.0
    for seq in (m.conv_xyz, m.conv_fea):
        for p in seq.parameters():
            assert float(p.grad.abs().max()) == 0.0


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
    c = bm.CASES["b"]
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
    assert int(m_c.conv2.bn.num_batches_tracked) == 4 and int(m_c.inte_conv_hk[1].num_batches_tracked) == 4


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
    softmax, the reference's transpose / view chain, the product and the concatenation -- the reference's formulation."""
    import spgan
    import torch.nn.functional as F_
    B, C, N = x.shape
    e, y = spgan.get_edge_features(x, k, idx=idx), spgan.get_edge_features(pc, k, idx=idx)

    def block(t, conv, bn, slope=0.01):
        return F_.leaky_relu(F_.batch_norm(F_.conv2d(t, conv.weight, conv.bias), None, None, bn.weight, bn.bias, True, 0.1, 1e-5), slope)
    w = block(e, m.conv_fea[0], m.conv_fea[1]) * block(y, m.conv_xyz[0], m.conv_xyz[1])
    for i in (0, 3):
        w = block(w, m.conv_all[i], m.conv_all[i + 1])
    if m.softmax:
        w = F_.softmax(w, dim=-1)
    inte = block(e, m.inte_conv_hk[0], m.inte_conv_hk[1])
    inte = inte.transpose(2, 1).contiguous().view(B, N, 2 * C, 2, k // 2).contiguous().view(B, N, 2 * C, k).permute(0, 2, 1, 3)
    out = block(torch.cat((e, inte * w), 3), m.conv2.conv, m.conv2.bn, 0.0)
    return out.unsqueeze(3).contiguous().view(B, m.Fout, 2, N).contiguous().view(B, m.Fout, 2 * N)


def test_memory_against_composed_route(sp):
    """bilateral_upsample_edgeConv(64,128,10) at B = 4, N = 2048: E = 4 M k 2Fin bytes = 42 MB is the edge tensor.  The peak of one forward
    + backward lies at least 2 E below the composed torch route's, measured here on the same graph."""
    from spgan import fixture_rng as fr
    B, N, C, F, k = 4, 2048, 64, 128, 10
    m = sp.bilateral_upsample_edgeConv(C, F, k, -1).cuda().train()
    x0 = fr.normal("bilateral.mem.x", (B, C, N), 0.7).cuda()
    pc0 = fr.uniform("bilateral.mem.pc", (B, 3, N), -1.0, 1.0).cuda()
    cot = fr.normal("bilateral.mem.g", (B, F, 2 * N)).cuda()
    with torch.no_grad():
        m(x0, pc0)
    idx = sp.ops.idx_to_local64(m.last_idx, B, N)
    E = B * 2 * C * N * k * 4
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
    for k in (5, 0, 30):
        with pytest.raises(ValueError, match="k=%d .Fin=4, Fout=6." % k):
            sp.bilateral_upsample_edgeConv(4, 6, k, -1)
    with pytest.raises(RuntimeError, match="no CPU"):
        m(torch.from_numpy(d["b|x"]), pc)
    with pytest.raises(RuntimeError, match="no CPU"):
        m(xg, torch.from_numpy(d["b|pc"]))
    with pytest.raises(ValueError, match="8 channels"):
        m(xg[:, :8], pc)                                                     # wrong channel count
    for bad in (pc[:, :2], pc[:, :, :50], pc[:1], pc[0]):
        with pytest.raises(ValueError, match=r"pc must be \[B,3,N\]"):
            m(xg, bad)
    with pytest.raises(IndexError):
        m(xg, pc, idx=torch.full((2, 96 * 10), 96, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        m(xg, pc, idx=torch.zeros(2 * 96, 9, dtype=torch.int32, device="cuda"))
    m.conv_all[5].negative_slope = 0.2
    with pytest.raises(NotImplementedError, match="slope"):
        m(xg, pc)
    m.conv_all[5].negative_slope = 0.01
    m.conv_xyz[1].momentum = None
    with pytest.raises(NotImplementedError):
        m(xg, pc)
    m.conv_xyz[1].momentum = 0.1
    m.inte_conv_hk[1].track_running_stats = False
    with pytest.raises(NotImplementedError):
        m(xg, pc)
