"""GPU: spgan.modules.edgeConv / conv2dbr (csrc/edge_max.hip) against the vectors captured from the reference's edgeConv (golden
edgeconv.npz) and each launcher against the float64 model of tests/edgeconv_model.py on small and awkward sizes.

Tolerances.  Module vs golden with the reference's graph injected: those of the EdgeBlock-vs-golden checks of tests/test_parity_gpu.py
(rel-L2 3e-6 for the output and dx, 5e-6 for parameter gradients with the absolute bound 2e-3 for the conv bias, whose gradient in front
of a train-mode BatchNorm is exactly zero here and rounding noise in the reference -- in the train-mode cases only; buffers rtol 1e-5 / atol 1e-6).  Launchers vs the
float64 model on the same float32 operands: float32 arithmetic on sums of k (or in-degree) well-conditioned terms, 2e-6 forward and 1e-5
backward, as in tests/test_pointconv_gpu.py; the extremes, ranks and clip flags are discrete and must be equal."""
import numpy as np
import pytest
import torch

import edgeconv_model as ecm
from helpers import check, golden

pytestmark = pytest.mark.gpu
TAGS = list(ecm.CASES)


@pytest.fixture(scope="module")
def sp():
    import spgan
    from spgan import _lib
    _lib.load()
    return spgan


@pytest.fixture(scope="module")
def d():
    return golden("edgeconv.npz")


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _module(sp, d, tag):
    c = ecm.CASES[tag]
    m = sp.edgeConv(c["Fin"], c["Fout"], c["k"])
    m.load_state_dict(ecm.golden_state_dict(d, tag), strict=True)
    return m.cuda().train(c["train"])


def _run(m, d, tag, inject=True):
    x = torch.from_numpy(d[tag + "|x"]).cuda().requires_grad_(True)
    idx = torch.from_numpy(d[tag + "|idx"]).cuda() if inject else None
    out = m(x, idx=idx)
    (out * torch.from_numpy(d[tag + "|g"]).cuda()).sum().backward()
    return x, out


def _atol(n, train):
    """2e-3 only for the conv bias in front of a TRAIN-mode BatchNorm (zero here, rounding noise in the reference: test_parity_gpu's
    ZERO_GRAD_BIASES rule); in eval mode the bias gradient is an ordinary quantity."""
    return 2e-3 if (n == "conv.conv.bias" and train) else 1e-7


# ---------------------------------------------------------------- each launcher against the model
def _problem(B, N, k, F, seed, neg=True):
    g = torch.Generator().manual_seed(seed)
    P, Q = torch.randn(B, N, F, generator=g), torch.randn(B, N, F, generator=g) * 0.5 + 0.3
    idx = torch.stack([torch.stack([torch.randperm(N, generator=g)[:k] for _ in range(N)]).reshape(-1) for _ in range(B)])      # int64 [B,N*k]
    gamma = torch.rand(F, generator=g) + 0.5
    if neg:
        gamma[::3] *= -1
    beta = torch.randn(F, generator=g) * 0.2
    rm, rv = torch.randn(F, generator=g) * 0.1, torch.rand(F, generator=g) + 0.5
    cot = torch.randn(B, N, F, generator=g)
    return P, Q, idx, gamma, beta, rm, rv, cot


@pytest.mark.parametrize("B,N,k,F", [(2, 50, 5, 12), (1, 77, 3, 7), (3, 64, 10, 64), (2, 33, 20, 260)])
@pytest.mark.parametrize("training", [True, False])
def test_launchers_against_model(sp, B, N, k, F, training):
    """F = 12: float4 path with a partly idle channel group; F = 7 and 260: the scalar path / more than one channel pass; M not a multiple
    of the 32-point tile."""
    ops, em = sp.ops, sp.edge_max
    P, Q, idx, gamma, beta, rm, rv, cot = _problem(B, N, k, F, seed=B * 1000 + N + F)
    f = ecm.forward_pq(P.double(), Q.double(), idx, k, gamma.double(), beta.double(), rm.double(), rv.double(), training)
    M = B * N
    PQ = torch.cat([P, Q], dim=2).reshape(M, 2 * F).cuda().contiguous()
    gidx = ops.idx_from_local64(idx.cuda(), B, N, k)
    rm_g, rv_g = rm.cuda(), rv.cuda()
    if training:
        pmax, pmin, rmax, rmin, part, tile_rows = em.edge_max_gather(PQ, gidx)
        assert torch.equal(pmax.cpu().double(), f["pmax"].reshape(M, F)) and torch.equal(pmin.cpu().double(), f["pmin"].reshape(M, F))
        assert torch.equal(rmax.cpu().long(), f["jmax"].reshape(M, F)) and torch.equal(rmin.cpu().long(), f["jmin"].reshape(M, F))
        st = em.edge_max_bn(part, tile_rows, M * k, gamma.cuda(), beta.cuda(), rm_g, rv_g)
        assert _rel(st[3], f["mean"]) < 2e-6 and _rel(st[2], f["invstd"]) < 2e-6
        assert _rel(rm_g, f["running_mean"]) < 2e-6 and _rel(rv_g, f["running_var"]) < 2e-6
        out, sel = em.edge_max_finish(PQ, pmax, pmin, rmax, rmin, st[0], st[1])
    else:
        st = ops.bn_prepare(None, None, gamma.cuda(), beta.cuda(), M * k, False, rm_g, rv_g)
        out, sel = em.edge_max_eval(PQ, gidx, st[0], st[1])
        assert torch.equal(rm_g.cpu(), rm) and torch.equal(rv_g.cpu(), rv)
    assert _rel(st[0], f["a"]) < 2e-6 and _rel(st[1], f["s"]) < 2e-5          # s = beta - a*mean: one cancellation
    assert _rel(out, f["out_pm"].reshape(M, F)) < 2e-6
    rank, clipped = (sel & 0x7f).cpu().long().view(B, N, F), (sel & 0x80).cpu().view(B, N, F) != 0
    assert torch.equal(rank, f["sel"])
    # the clip flag is the sign of the float32 output: it may differ from the float64 model's only where the output is a rounding residue
    assert torch.equal(clipped, out.cpu().view(B, N, F) <= 0)
    flips = clipped != (f["out_pm"] <= 0)
    assert float(f["out_pm"][flips].abs().max() if flips.any() else 0.0) < 1e-5
    # backward with the kernel's own selection and mask
    r = cot.reshape(M, F).cuda().contiguous()
    sums = em.edge_max_bwd_point(r, sel, PQ, gidx, st[3], st[2])
    bw = ecm.backward_pq(f, cot.double(), sel=rank, active=~clipped)
    assert torch.equal(r.cpu(), (cot * (~clipped).float()).reshape(M, F))
    assert _rel(sums[:F], bw["dbeta"]) < 1e-5 and _rel(sums[F:], bw["dgamma"]) < 1e-5
    rowptr, src = ops.csr_build(gidx, B, N)
    if training:
        dPQ = em.edge_max_bwd_graph(r, sel, PQ, k, rowptr, src, st[0], gidx, st[3], st[2], sums)
    else:
        dPQ = em.edge_max_bwd_graph(r, sel, PQ, k, rowptr, src, st[0])
    assert _rel(dPQ[:, :F], bw["dP"].reshape(M, F)) < 1e-5
    assert _rel(dPQ[:, F:], bw["dQ"].reshape(M, F)) < 1e-5


def test_first_rank_wins_exact_ties(sp):
    ops, em = sp.ops, sp.edge_max
    B, N, k, F = 1, 40, 6, 8
    P, Q, idx, gamma, beta, rm, rv, _ = _problem(B, N, k, F, seed=5)
    P = torch.round(P)                                               # integers in a narrow range: many exact ties among the k values
    PQ = torch.cat([P, Q], dim=2).reshape(N, 2 * F).cuda().contiguous()
    _, _, rmax, rmin, _, _ = em.edge_max_gather(PQ, ops.idx_from_local64(idx.cuda(), B, N, k))
    Pn = ecm.gather_neighbours(P, idx, k)[0]                         # [N,k,F]
    first_max = (Pn == Pn.max(dim=1, keepdim=True)[0]).float().argmax(dim=1)
    first_min = (Pn == Pn.min(dim=1, keepdim=True)[0]).float().argmax(dim=1)
    assert ((Pn == Pn.max(dim=1, keepdim=True)[0]).sum(dim=1) > 1).any() and ((Pn == Pn.min(dim=1, keepdim=True)[0]).sum(dim=1) > 1).any()
    assert torch.equal(rmax.cpu().long(), first_max) and torch.equal(rmin.cpu().long(), first_min)


# ---------------------------------------------------------------- module against the reference (golden)
@pytest.mark.parametrize("tag", TAGS)
def test_module_golden_with_injected_graph(sp, d, tag):
    m = _module(sp, d, tag)
    x, out = _run(m, d, tag)
    e = {"out": check(d, tag + "|out", out, rtol=3e-6),           # measured (MI355X) 1.2e-7 .. 1.5e-7 over the four cases
         "dx": check(d, tag + "|dx", x.grad, rtol=3e-6)}           # measured 1.7e-7 .. 2.1e-7
    for n, p in m.named_parameters():
        e[n] = check(d, "%s|grad|%s" % (tag, n), p.grad, rtol=5e-6, atol=_atol(n, ecm.CASES[tag]["train"]))   # measured <= 4.4e-7 (eval conv bias 2.4e-7)
    print("%s: rel-L2 vs reference float32 %s" % (tag, {k: "%.2e" % v for k, v in e.items()}))
    for n, b in m.state_dict().items():
        if n in dict(m.named_buffers()):
            np.testing.assert_allclose(b.cpu().numpy(), d["%s|buf|%s|full" % (tag, n)], rtol=1e-5, atol=1e-6, err_msg=n)
    if not ecm.CASES[tag]["train"]:                                   # eval mode leaves the buffers untouched (bit for bit)
        for n in ecm.BUFFERS:
            assert np.array_equal(m.state_dict()[n].cpu().numpy(), d["%s|param|%s" % (tag, n)]), n
    else:
        assert int(m.conv.bn.num_batches_tracked) == int(d[tag + "|param|conv.bn.num_batches_tracked"]) + 1


@pytest.mark.parametrize("tag", TAGS)
def test_module_own_graph_matches_reference(sp, d, tag):
    c = ecm.CASES[tag]
    m = _module(sp, d, tag)
    with torch.no_grad():
        m(torch.from_numpy(d[tag + "|x"]).cuda())
    own = sp.ops.idx_to_local64(m.last_idx, c["B"], c["N"]).view(-1, c["k"]).cpu().numpy()
    ref = d[tag + "|idx"].reshape(-1, c["k"])
    near = d[tag + "|near_tie_rows"].astype(bool)
    assert near.mean() <= 0.01
    assert np.array_equal(own[~near], ref[~near]), int((own[~near] != ref[~near]).any(axis=1).sum())


def test_negative_gamma_takes_the_min_branch(sp, d):
    m = _module(sp, d, "neg")
    _run(m, d, "neg")
    c = ecm.CASES["neg"]
    sd = {k: v.double() if v.dtype.is_floating_point else v for k, v in ecm.golden_state_dict(d, "neg").items()}
    f = ecm.forward(torch.from_numpy(d["neg|x"]).double(), torch.from_numpy(d["neg|idx"]), c["k"], sd["conv.conv.weight"], sd["conv.conv.bias"],
                    sd["conv.bn.weight"], sd["conv.bn.bias"], sd["conv.bn.running_mean"], sd["conv.bn.running_var"], True)
    neg = sd["conv.bn.weight"] < 0
    assert int(neg.sum()) >= 3
    rank = (m.last_sel & 0x7f).cpu().long().view(c["B"], c["N"], c["Fout"])
    assert torch.equal(rank[..., neg], f["jmin"][..., neg]) and torch.equal(rank[..., ~neg], f["jmax"][..., ~neg])
    assert not torch.equal(f["jmin"][..., neg], f["jmax"][..., neg])


@pytest.mark.parametrize("tag", ["feat", "eval"])
def test_deterministic(sp, d, tag):
    res = []
    for _ in range(2):
        m = _module(sp, d, tag)
        x, out = _run(m, d, tag, inject=False)
        res.append([out.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in m.parameters()] + [b.clone() for b in m.buffers()])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_requires_grad_off_and_no_grad(sp, d):
    m = _module(sp, d, "feat")
    x = torch.from_numpy(d["feat|x"]).cuda()
    idx = torch.from_numpy(d["feat|idx"]).cuda()
    with torch.no_grad():
        o1 = m(x, idx=idx)
    assert not o1.requires_grad
    check(d, "feat|out", o1, rtol=3e-6)
    for p in m.parameters():
        p.requires_grad_(False)
    m2 = _module(sp, d, "feat")
    for p in m2.parameters():
        p.requires_grad_(False)
    xg = x.clone().requires_grad_(True)
    (m2(xg, idx=idx) * torch.from_numpy(d["feat|g"]).cuda()).sum().backward()
    check(d, "feat|dx", xg.grad, rtol=3e-6)
    assert all(p.grad is None for p in m2.parameters())


def test_double_backward_raises(sp, d):
    m = _module(sp, d, "feat")
    x = torch.from_numpy(d["feat|x"]).cuda().requires_grad_(True)
    out = m(x)
    with pytest.raises(RuntimeError, match="once differentiable"):           # the gradient-penalty pattern: refused where it is asked for
        torch.autograd.grad(out.sum(), x, create_graph=True)
    (gx,) = torch.autograd.grad(m(x).sum(), x)                                # the first derivative alone is served
    assert gx.shape == x.shape and not gx.requires_grad


def test_bad_arguments_are_rejected(sp, d):
    ops, em = sp.ops, sp.edge_max
    m = _module(sp, d, "feat")
    x = torch.from_numpy(d["feat|x"]).cuda()
    with pytest.raises(ValueError):
        m(x[:, :8])                                                        # wrong channel count
    with pytest.raises(ValueError):
        m(x, idx=torch.zeros(2, 5, dtype=torch.int64, device="cuda"))      # wrong idx size
    with pytest.raises(IndexError):
        m(x, idx=torch.full((2, 128 * 10), 128, dtype=torch.int64, device="cuda"))
    with pytest.raises(RuntimeError, match="no CPU"):
        m(x.cpu())
    PQ = torch.zeros(64, 16, device="cuda")
    with pytest.raises(RuntimeError):
        em.edge_max_gather(PQ, torch.zeros(64, 128, dtype=torch.int32, device="cuda"))      # k > 127: status -22 from the launcher
    with pytest.raises(ValueError):
        em.edge_max_gather(PQ[:, :15], torch.zeros(64, 4, dtype=torch.int32, device="cuda"))
    with pytest.raises(NotImplementedError):
        sp.conv2dbr(4, 8, [1, 3]).cuda()(torch.zeros(1, 4, 8, 8, device="cuda"))


def test_conv2dbr_1x1_against_torch(sp):
    g = torch.Generator().manual_seed(3)
    B, Fi, Fo, H, W = 2, 6, 12, 17, 5
    m = sp.conv2dbr(Fi, Fo, 1).cuda().train()
    ref = torch.nn.Sequential(torch.nn.Conv2d(Fi, Fo, 1), torch.nn.BatchNorm2d(Fo), torch.nn.ReLU()).double()
    ref[0].load_state_dict({k: v.double().cpu() for k, v in m.conv.state_dict().items()})
    x = torch.randn(B, Fi, H, W, generator=g)
    cot = torch.randn(B, Fo, H, W, generator=g)
    xg = x.cuda().requires_grad_(True)
    out = m(xg)
    (out * cot.cuda()).sum().backward()
    xr = x.double().requires_grad_(True)
    outr = ref(xr)
    (outr * cot.double()).sum().backward()
    assert out.shape == outr.shape and _rel(out, outr) < 2e-6 and _rel(xg.grad, xr.grad) < 1e-5
    assert _rel(m.conv.weight.grad, ref[0].weight.grad) < 1e-5 and _rel(m.bn.weight.grad, ref[1].weight.grad) < 1e-5
    assert _rel(m.bn.running_var, ref[1].running_var) < 2e-6 and int(m.bn.num_batches_tracked) == 1


# ---------------------------------------------------------------- full size
def test_full_size_properties(sp):
    """edgeConv(64,128,10) at B = 4, N = 2048 on its own graph: forward against a float64 composition evaluated shape by shape, the saved
    selection against max_j y, backward against the model evaluated with the kernel's own selection, and the point of the feature: the
    peak memory of forward + backward stays below ONE [B,Fout,N,k] float32 tensor plus the input and the output."""
    from spgan import fixture_rng as fr
    B, N, Fin, F, k = 4, 2048, 64, 128, 10
    m = sp.edgeConv(Fin, F, k).cuda().train()
    with torch.no_grad():
        m.conv.bn.weight.copy_(fr.uniform("edgeconv.full.gamma", (F,), 0.5, 1.5))
        m.conv.bn.weight[::5] *= -1
        m.conv.bn.bias.copy_(fr.uniform("edgeconv.full.beta", (F,), -0.2, 0.2))
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    x = fr.normal("edgeconv.full.x", (B, Fin, N), 0.7).cuda().requires_grad_(True)
    cot = fr.normal("edgeconv.full.g", (B, F, N)).cuda()
    torch.cuda.reset_peak_memory_stats()
    out = m(x)
    (out * cot).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    edge_bytes = B * F * N * k * 4
    bound = edge_bytes + x.numel() * 4 + out.numel() * 4
    print("peak %.1f MB over forward+backward; one edge tensor %.1f MB; bound %.1f MB" % (peak / 2**20, edge_bytes / 2**20, bound / 2**20))
    assert peak < bound, (peak, bound)                                           # measured 41.8 MB against 46.0 MB

    # float64 model on the module's own graph, shape by shape for the per-edge tensors, statistics over all shapes
    idx = sp.ops.idx_to_local64(m.last_idx, B, N)
    sd = {n: (v.double() if v.dtype.is_floating_point else v) for n, v in m.state_dict().items()}
    f = ecm.forward(x.detach().double(), idx, k, sd["conv.conv.weight"], sd["conv.conv.bias"], sd["conv.bn.weight"], sd["conv.bn.bias"],
                    torch.zeros(F, dtype=torch.float64, device="cuda"), torch.ones(F, dtype=torch.float64, device="cuda"), True)
    W, b = sd["conv.conv.weight"], sd["conv.conv.bias"]
    ys = []
    for s in range(B):
        _, y = ecm.composition(x.detach()[s:s + 1].double(), idx[s:s + 1], k, W, b, sd["conv.bn.weight"], sd["conv.bn.bias"], None, None, True)
        ys.append(y)
    y = torch.cat(ys)                                                            # [B,N,k,F] float64
    mean, var = y.mean(dim=(0, 1, 2)), y.var(dim=(0, 1, 2), unbiased=False)
    z = torch.relu((y - mean) / torch.sqrt(var + 1e-5) * sd["conv.bn.weight"] + sd["conv.bn.bias"]).max(dim=2)[0].transpose(1, 2)
    err = _rel(out, z)
    print("forward vs float64 composition: %.2e" % err)
    assert err < 3e-6                                                            # measured 1.5e-7
    sel = m.last_sel.view(B, N, F)
    rank, clipped = (sel & 0x7f).long(), (sel & 0x80) != 0
    a = sd["conv.bn.weight"] / torch.sqrt(var + 1e-5)
    ysel = torch.gather(y, 2, rank.unsqueeze(2)).squeeze(2)
    best = torch.where(a >= 0, y.max(dim=2)[0], y.min(dim=2)[0])
    slack = 4 * torch.finfo(torch.float32).eps * y.abs().max()                   # fp32 rounding of y = Q + P (two rounded terms and their sum)
    assert bool((torch.where(a >= 0, ysel >= best - slack, ysel <= best + slack)).all())
    bw = ecm.backward(f, cot.double(), sel=rank, active=~clipped)
    errs = {"dx": _rel(x.grad, bw["dx"]), "dW": _rel(m.conv.conv.weight.grad, bw["dW"]), "dgamma": _rel(m.conv.bn.weight.grad, bw["dgamma"]),
            "dbeta": _rel(m.conv.bn.bias.grad, bw["dbeta"])}
    print("backward vs model with the kernel's selection: %s" % {n: "%.2e" % v for n, v in errs.items()})
    assert max(errs.values()) < 1e-5                                             # measured dx 2.8e-7, dW 2.0e-7, dgamma 1.9e-7, dbeta 9.6e-8
    assert float(m.conv.conv.bias.grad.abs().max()) == 0.0
