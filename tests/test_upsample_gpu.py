"""GPU: spgan.modules.upsample_edgeConv / get_edge_features_xyz (csrc/edge_window.hip) against the vectors captured from the reference
(golden upsample.npz) and each launcher against the float64 model of tests/upsample_model.py on small and awkward sizes.

Tolerances.  Module vs golden with the reference's graph injected: the bounds of the edgeConv golden test (rel-L2 3e-6 for the output
and dx, 5e-6 for parameter gradients, buffers rtol 1e-5 / atol 1e-6), or 5 x the golden's stored float32-vs-float64 distance of the
quantity where that is larger.  The stored distances are 0.7e-7 .. 4.0e-7 over the four cases, so 5 x noise stays below the base bound
for every quantity: NO quantity takes the fallback.  The two conv biases sit in front of a train-mode BatchNorm: their gradients are
exact zeros here and rounding noise in the reference (2e-3 absolute, the ZERO_GRAD_BIASES rule), in the train-mode cases only.
Launchers vs the float64 model on the same float32 operands: the larger of the project's launcher bounds (2e-6 forward, 1e-5 backward)
and 5 x the rel-L2 distance between a float32 and a float64 CPU evaluation of the model on those operands."""
import numpy as np
import pytest
import torch

import upsample_model as um
from helpers import check, golden

pytestmark = pytest.mark.gpu
TAGS = list(um.CASES)


@pytest.fixture(scope="module")
def sp():
    import spgan
    from spgan import _lib
    _lib.load()
    return spgan


@pytest.fixture(scope="module")
def d():
    return golden("upsample.npz")


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _module(sp, d, tag):
    c = um.CASES[tag]
    m = sp.upsample_edgeConv(c["Fin"], c["Fout"], c["k"], -1)
    m.load_state_dict(um.golden_state_dict(d, tag), strict=True)
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
    train = um.CASES[tag]["train"]
    m = _module(sp, d, tag)
    x, out = _run(m, d, tag)
    e = {"out": check(d, tag + "|out", out, rtol=_bound(d, tag, "out", 3e-6), atol=1e-7),
         "dx": check(d, tag + "|dx", x.grad, rtol=_bound(d, tag, "dx", 3e-6), atol=1e-7)}
    for n, p in m.named_parameters():
        if n in um.ZERO_GRAD_BIASES and train:
            assert float(p.grad.abs().max()) == 0.0, n                      # exact zeros here
            assert float(np.abs(d["%s|grad|%s|full" % (tag, n)]).max()) <= 2e-3, n
            continue
        e[n] = check(d, "%s|grad|%s" % (tag, n), p.grad, rtol=_bound(d, tag, "grad|" + n, 5e-6), atol=1e-7)
    print("%s: rel-L2 vs reference float32 %s" % (tag, {k: "%.2e" % v for k, v in e.items()}))
    bufs = dict(m.named_buffers())
    for n in um.BUFFERS:
        np.testing.assert_allclose(bufs[n].cpu().numpy(), d["%s|buf|%s|full" % (tag, n)], rtol=1e-5, atol=1e-6, err_msg=n)
        if not train:                                                        # eval mode leaves the buffers untouched (bit for bit)
            assert np.array_equal(bufs[n].cpu().numpy(), d["%s|param|%s" % (tag, n)]), n
    if train:
        assert int(m.conv2.bn.num_batches_tracked) == int(d[tag + "|param|conv2.bn.num_batches_tracked"]) + 1
        assert int(m.inte_conv_hk[1].num_batches_tracked) == int(d[tag + "|param|inte_conv_hk.1.num_batches_tracked"]) + 1


@pytest.mark.parametrize("tag", TAGS)
def test_module_own_graph_matches_reference(sp, d, tag):
    c = um.CASES[tag]
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
    """int64 [B*N,k] global rows: random permutation prefixes; hand: repeated neighbours, a point nobody gathers, a hub all gather."""
    loc = torch.stack([torch.stack([torch.randperm(N, generator=g)[:k] for _ in range(N)]) for _ in range(B)])       # [B,N,k]
    if hand:
        loc[loc == 1] = 2                              # point 1 of every shape: in-degree 0
        loc[:, :, 0] = 0                               # point 0: gathered by every point (itself included)
        loc[:, 3, :] = 5                               # point 3 gathers the same neighbour k times
        loc[:, 1, 0] = 0
    return (loc + torch.arange(B).view(B, 1, 1) * N).view(B * N, k)


SHAPES = [(2, 50, 4, 3, 12), (1, 77, 6, 7, 20), (3, 64, 10, 64, 256), (2, 33, 2, 16, 8)]


def _launcher_case(sp, B, N, k, C, O, w, hand, seed):
    ops, ew, em = sp.ops, sp.edge_window, sp.edge_max
    g = torch.Generator().manual_seed(seed)
    M, T = B * N, k - w + 1
    x = torch.randn(M, C, generator=g) * 0.7
    gidx = _graph(B, N, k, g, hand)
    W = (torch.rand(O, w * C, generator=g) * 2 - 1) / np.sqrt(w * C)
    rowadd = torch.randn(M, O, generator=g) * 0.3
    add2 = torch.randn(M * T, O, generator=g) * 0.3
    G = torch.randn(M * T, O, generator=g)
    gamma, beta = torch.rand(O, generator=g) + 0.5, torch.randn(O, generator=g) * 0.2

    def model(dt):
        xx, WW, GG = x.to(dt), W.to(dt), G.to(dt)
        Y = um.window_gemm(xx, gidx, WW, w, rowadd.to(dt), add2.to(dt))
        S = um.window_dgrad(GG, WW, k, C, w)
        return dict(Y=Y, Yplain=um.window_gemm(xx, gidx, WW, w), dW=um.window_wgrad(xx, gidx, GG, w), S=S,
                    dx=um.window_scatter(S, gidx, xx, None))
    m64, m32 = model(torch.float64), model(torch.float32)
    bound = {q: max(base, 5.0 * _rel(m32[q], m64[q])) for q, base in (("Y", 2e-6), ("Yplain", 2e-6), ("dW", 1e-5), ("S", 1e-5), ("dx", 1e-5))}
    xg, Wg, Gg = x.cuda(), W.cuda(), G.cuda()
    idx = gidx.to(torch.int32).cuda()
    rm, rv = torch.zeros(O, device="cuda"), torch.ones(O, device="cuda")
    Y, part, rows = ew.edge_window_gemm(xg, idx, Wg, rowadd=rowadd.cuda(), add2=add2.cuda(), stats=True)
    err = {"Y": _rel(Y, m64["Y"]), "Yplain": _rel(ew.edge_window_gemm(xg, idx, Wg), m64["Yplain"])}
    assert tuple(Y.shape) == (M * T, O) and rows == ew.tile_points(k, T) * T
    st = em.edge_max_bn(part, rows, M * T, gamma.cuda(), beta.cuda(), rm, rv)
    mean, var = um.colstats(m64["Y"])
    err["mean"], err["invstd"] = _rel(st[3], mean), _rel(st[2], 1.0 / torch.sqrt(var + um.EPS))
    err["dW"] = _rel(ew.edge_window_wgrad(xg, idx, Gg, w), m64["dW"])
    S = ew.edge_window_dgrad(Gg, Wg.t().contiguous(), k, C)
    err["S"] = _rel(S, m64["S"])
    S2 = ew.edge_window_dgrad(Gg, Wg.t().contiguous(), k, C, out=S.clone())          # accumulate: twice the slot gradients
    assert _rel(S2, 2.0 * m64["S"]) <= bound["S"]
    rowptr, src = ops.csr_build(idx, B, N)
    err["dx"] = _rel(ew.edge_window_scatter(S, rowptr, src, xg), um.window_scatter(S.cpu().double(), gidx, x.double()))
    print("B %d N %d k %d C %d O %d w %d hand %s: %s" % (B, N, k, C, O, w, hand, {q: "%.2e" % v for q, v in err.items()}))
    for q in ("Y", "Yplain", "dW", "S", "dx"):
        assert err[q] <= bound[q], (q, err[q], bound[q])
    assert err["mean"] < 2e-6 and err["invstd"] < 2e-6, err


@pytest.mark.parametrize("B,N,k,C,O", SHAPES)
@pytest.mark.parametrize("hand", [False, True])
def test_launchers_against_model(sp, B, N, k, C, O, hand):
    """(2,50,4,3,12): the scalar staging path; (1,77,6,7,20): C and O no multiples of 4, M no multiple of a tile; (3,64,10,64,256): several
    K blocks, channel chunks and output-column passes; (2,33,2,16,8): T = 1 and w = 2.  hand: the constructed graph."""
    _launcher_case(sp, B, N, k, C, O, k // 2 + 1, hand, seed=B * 1000 + N + C)


@pytest.mark.parametrize("B,N,k,C,O", [SHAPES[0], SHAPES[2]])
def test_launchers_full_window_form(sp, B, N, k, C, O):
    """(w, T) = (k, 1): the first k taps of conv2."""
    _launcher_case(sp, B, N, k, C, O, k, False, seed=B * 1000 + N + C + 7)


# ---------------------------------------------------------------- properties of the module
@pytest.mark.parametrize("tag", ["feat", "eval"])
def test_deterministic(sp, d, tag):
    res = []
    for _ in range(2):
        m = _module(sp, d, tag)
        x, out = _run(m, d, tag, inject=False)
        res.append([out.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in m.parameters()] + [b.clone() for b in m.buffers()])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_output_layout(sp):
    """Weights that make y(i,o) identifiable: only the central taps of conv2 see the input, x is one-hot in the channel that carries
    the point number, BatchNorm is the identity in eval mode up to the rounding of 1/sqrt(var + eps): y[b,o,n] = (o+1) * (n+1), small
    integers that rounding to the nearest integer recovers exactly, and out[b,f,s*N+n] == y[b,2f+s,n]."""
    B, C, N, Fout, k = 2, 4, 16, 3, 4
    m = sp.upsample_edgeConv(C, Fout, k, -1)
    with torch.no_grad():
        for p in m.parameters():
            p.zero_()
        m.conv2.conv.weight[:, 0, 0, 0] = torch.arange(1, 2 * Fout + 1, dtype=torch.float32)
        m.conv2.bn.weight.fill_(1.0)
        m.inte_conv_hk[1].weight.fill_(1.0)
    m = m.cuda().eval()
    x = torch.zeros(B, C, N)
    x[:, 0, :] = torch.arange(1, N + 1, dtype=torch.float32)
    out = m(x.cuda()).detach().cpu()
    y = torch.arange(1, 2 * Fout + 1, dtype=torch.float32).view(1, -1, 1) * x[:, :1, :]          # [B,2Fout,N]
    assert tuple(out.shape) == (B, Fout, 2 * N)
    for f in range(Fout):
        for s in range(2):
            got = out[:, f, s * N:(s + 1) * N]
            assert torch.equal(torch.round(got), y[:, 2 * f + s, :]) and float((got - y[:, 2 * f + s, :]).abs().max()) < 1e-2, (f, s)


def test_checkpoints(sp, d):
    m = _module(sp, d, "feat")
    _run(m, d, "feat")
    m2 = sp.upsample_edgeConv(16, 32, 10, -1).cuda()
    m2.load_state_dict(m.state_dict(), strict=True)
    for (n, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), n
    m.train(); m2.train()
    x = torch.from_numpy(d["feat|x"]).cuda()
    idx = torch.from_numpy(d["feat|idx"]).cuda()
    with torch.no_grad():
        assert torch.equal(m(x, idx=idx), m2(x, idx=idx))


def test_error_behaviour(sp, d):
    with pytest.raises(ValueError):
        sp.upsample_edgeConv(4, 4, 7, -1)
    m = _module(sp, d, "feat")
    x = torch.from_numpy(d["feat|x"]).cuda()
    with pytest.raises(ValueError):
        m(x[:, :8])                                                        # wrong channel count
    with pytest.raises(ValueError):
        m(x, idx=torch.zeros(2, 5, dtype=torch.int64, device="cuda"))
    with pytest.raises(IndexError):
        m(x, idx=torch.full((2, 64 * 10), 64, dtype=torch.int64, device="cuda"))
    with pytest.raises(NotImplementedError):
        m.conv2(torch.zeros(1, 32, 8, 20, device="cuda"))                  # conv2dbr on its own still refuses the [1,2k] kernel
    m.conv2.bn.momentum = None
    with pytest.raises(NotImplementedError):
        m(x)
    m = _module(sp, d, "feat")
    xg = x.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(m(xg).sum(), xg, create_graph=True)


def test_get_edge_features_xyz_golden(sp, d):
    c = um.XYZ_CASE
    x = torch.from_numpy(d["xyzfn|x"]).cuda().requires_grad_(True)
    pc = torch.from_numpy(d["xyzfn|pc"]).cuda().requires_grad_(True)
    e_fea, e_xyz = sp.get_edge_features_xyz(x, pc, c["k"])
    assert tuple(e_fea.shape) == (c["B"], 2 * c["C"], c["N"], c["k"]) and tuple(e_xyz.shape) == (c["B"], 6, c["N"], c["k"])
    near = torch.from_numpy(d["xyzfn|near_tie_rows"].astype(bool))
    assert near.float().mean() <= 0.01
    keep = (~near).view(c["B"], 1, c["N"], 1)
    for got, name in ((e_fea, "e_fea"), (e_xyz, "e_xyz")):
        ref = torch.from_numpy(d["xyzfn|%s|full" % name])
        assert torch.equal(torch.where(keep, got.detach().cpu(), ref), ref), name            # exact outside the near-tie rows
    assert not near.any()          # the gradient comparison below needs the whole graph to agree (the stored case has no near-tie row)
    ((e_fea * torch.from_numpy(d["xyzfn|gf"]).cuda()).sum() + (e_xyz * torch.from_numpy(d["xyzfn|gx"]).cuda()).sum()).backward()
    assert _rel(x.grad, torch.from_numpy(d["xyzfn|dx|full"])) < 3e-6              # the get_edge_features bounds of tests/test_pointnet_gpu.py
    assert _rel(pc.grad, torch.from_numpy(d["xyzfn|dpc|full"])) < 3e-6


def _composed(x, idx, k, m):
    """The materialised route: spgan.get_edge_features, then torch's conv2d / batch_norm / leaky_relu and the views of the reference."""
    import spgan
    import torch.nn.functional as F_
    B, C, N = x.shape
    conv1, bn1 = m.inte_conv_hk[0], m.inte_conv_hk[1]
    ee = spgan.get_edge_features(x, k, idx=idx)
    h = F_.leaky_relu(F_.batch_norm(F_.conv2d(ee, conv1.weight, conv1.bias), None, None, bn1.weight, bn1.bias, True, 0.1, 1e-5), 0.01, inplace=True)
    h = h.transpose(2, 1).contiguous().view(B, N, 2 * C, 2, k // 2).contiguous().view(B, N, 2 * C, k).permute(0, 2, 1, 3)
    y = F_.conv2d(torch.cat((ee, h), 3), m.conv2.conv.weight, m.conv2.conv.bias)
    y = torch.relu(F_.batch_norm(y, None, None, m.conv2.bn.weight, m.conv2.bn.bias, True, 0.1, 1e-5))
    return y.contiguous().view(B, -1, 2, N).contiguous().view(B, -1, 2 * N)


def test_memory_against_composed_route(sp):
    """upsample_edgeConv(64,128,10) at B = 4, N = 2048: with E the bytes of one [B,2Fin,N,k] tensor, the peak of one forward + backward
    lies at least 2 E below the composed torch route's (which holds ee and the 2 E merged tensor for its backward)."""
    from spgan import fixture_rng as fr
    B, N, Fin, Fout, k = 4, 2048, 64, 128, 10
    m = sp.upsample_edgeConv(Fin, Fout, k, -1).cuda().train()
    x0 = fr.normal("upsample.mem.x", (B, Fin, N), 0.7).cuda()
    cot = fr.normal("upsample.mem.g", (B, Fout, 2 * N)).cuda()
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
    # the two routes are the same function (a plausibility check of the yardstick, not an accuracy test: the layer's accuracy is
    # asserted against the reference above, and torch's convolution backward on this device is no fp32-exact reference)
    assert _rel(outs["layer"][0], outs["composed"][0]) < 1e-4
    print("dx layer vs composed: %.2e" % _rel(outs["layer"][1], outs["composed"][1]))


def test_capture(sp, d):
    """One forward + backward with an injected int32 graph inside spgan.CapturedBody, replayed twice, equals the eager result bit for bit."""
    c = um.CASES["feat"]
    x = torch.from_numpy(d["feat|x"]).cuda()
    cot = torch.from_numpy(d["feat|g"]).cuda()
    idx = sp.ops.idx_from_local64(torch.from_numpy(d["feat|idx"]).cuda(), c["B"], c["N"], c["k"])

    def make():
        m = _module(sp, d, "feat")

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
    assert int(m_c.conv2.bn.num_batches_tracked) == 4
