"""GPU: the opt-in double backward of spgan.edgeConv (edgeConv(double_backward=True); csrc/edge_max.hip's dbl passes, edge_conv.EdgeMaxConvBwdFn)
against the float64 closed form of tests/edgeconv_dbl_model.py, which tests/test_edgeconv_dbl_cpu.py ties to float64 autograd.

Tolerances.  Launchers vs the float64 model on the same float32 operands and the kernel's own selection: rel-L2 1e-5, the launcher-backward
bound of tests/test_edgeconv_gpu.py -- the arithmetic is the same: sums over k or in-degree terms plus E-long record sums.  The module is
held to the same bound (its products are exact-fp32 GEMMs with K <= 2F in front of and behind the same passes).  The stacked critic
chains four such stages (two double backwards, the torch ops between them, two first-order backwards fed by xbar) and the penalty's
(||g|| - gamma) in front: 1e-4, with the penalty's amplification ||g|| / | ||g|| - gamma | asserted to stay below 10."""
import pytest
import torch
import torch.nn as nn

import edgeconv_dbl_model as edm
import edgeconv_model as ecm

pytestmark = pytest.mark.gpu
TAGS = list(ecm.CASES)
NAMES = ("conv.conv.weight", "conv.conv.bias", "conv.bn.weight", "conv.bn.bias")


@pytest.fixture(scope="module")
def sp():
    import spgan
    from spgan import _lib
    _lib.load()
    return spgan


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


# ---------------------------------------------------------------- each launcher against the model
def _problem(B, N, k, F, seed):
    """test_edgeconv_gpu's launcher problem (every third gamma negative) with a direction [VP | VQ]"""
    g = torch.Generator().manual_seed(seed)
    P, Q = torch.randn(B, N, F, generator=g), torch.randn(B, N, F, generator=g) * 0.5 + 0.3
    idx = torch.stack([torch.stack([torch.randperm(N, generator=g)[:k] for _ in range(N)]).reshape(-1) for _ in range(B)])      # int64 [B,N*k]
    gamma = torch.rand(F, generator=g) + 0.5
    gamma[::3] *= -1
    beta = torch.randn(F, generator=g) * 0.2
    rm, rv = torch.randn(F, generator=g) * 0.1, torch.rand(F, generator=g) + 0.5
    cot = torch.randn(B, N, F, generator=g)
    VP, VQ = torch.randn(B, N, F, generator=g), torch.randn(B, N, F, generator=g) * 0.7 - 0.2
    return P, Q, idx, gamma, beta, rm, rv, cot, VP, VQ


@pytest.mark.parametrize("B,N,k,F", [(2, 50, 5, 12), (1, 77, 3, 7), (3, 64, 10, 64), (2, 33, 20, 260)])
@pytest.mark.parametrize("training", [True, False])
def test_launchers_against_model(sp, B, N, k, F, training):
    """F = 12: float4 path with a partly idle channel group; F = 7 and 260: the scalar path / more than one channel pass; M not a multiple
    of the 32-point tile.  Measured maxima over the eight cases (MI355X): T1 1.8e-7, T2 3.8e-7, S 1.8e-7, A 1.8e-7, ghat 3.4e-7, Pbar 8.4e-7,
    Qbar 8.8e-7 (the largest at F = 260, k = 20)."""
    ops, em = sp.ops, sp.edge_max
    P, Q, idx, gamma, beta, rm, rv, cot, VP, VQ = _problem(B, N, k, F, seed=B * 1000 + N + F)
    f = ecm.forward_pq(P.double(), Q.double(), idx, k, gamma.double(), beta.double(), rm.double(), rv.double(), training)
    M = B * N
    PQ = torch.cat([P, Q], dim=2).reshape(M, 2 * F).cuda().contiguous()
    VPQ = torch.cat([VP, VQ], dim=2).reshape(M, 2 * F).cuda().contiguous()
    gidx = ops.idx_from_local64(idx.cuda(), B, N, k)
    rm_g, rv_g = rm.cuda(), rv.cuda()
    if training:
        pmax, pmin, rmax, rmin, part, tile_rows = em.edge_max_gather(PQ, gidx)
        st = em.edge_max_bn(part, tile_rows, M * k, gamma.cuda(), beta.cuda(), rm_g, rv_g)
        _, sel = em.edge_max_finish(PQ, pmax, pmin, rmax, rmin, st[0], st[1])
    else:
        st = ops.bn_prepare(None, None, gamma.cuda(), beta.cuda(), M * k, False, rm_g, rv_g)
        _, sel = em.edge_max_eval(PQ, gidx, st[0], st[1])
    rank, clipped = (sel & 0x7f).cpu().long().view(B, N, F), (sel & 0x80).cpu().view(B, N, F) != 0
    r = cot.reshape(M, F).cuda().contiguous()
    sums = em.edge_max_bwd_point(r, sel, PQ, gidx, st[3], st[2])
    want = edm.double_backward_pq(f, cot.double(), VP.double(), VQ.double(), sel=rank, active=~clipped)
    errs = {}
    if training:
        dsums = em.edge_max_dbl_point(r, sel, PQ, VPQ, gidx, st[3], st[2])
        assert dsums.shape == (3 * F,)
        errs.update(T1=_rel(dsums[:F], want["T1"]), T2=_rel(dsums[F:2 * F], want["T2"]), S=_rel(dsums[2 * F:], want["S"]))
        rowptr, src = ops.csr_build(gidx, B, N)
        ghat, PQbar = em.edge_max_dbl_graph(r, sel, PQ, VPQ, gidx, st[0], k, rowptr, src, st[3], st[2], sums, dsums)
        errs.update(Pbar=_rel(PQbar[:, :F], want["Pbar"].reshape(M, F)), Qbar=_rel(PQbar[:, F:], want["Qbar"].reshape(M, F)))
        E = float(M * k)
        A = dsums[2 * F:] - sums[:F] * dsums[:F] / E - sums[F:] * dsums[F:2 * F] / E      # as edge_conv.EdgeMaxConvBwdFn forms it
        errs.update(A=_rel(A, want["A"]))
    else:
        S = em.edge_max_dbl_point(r, sel, PQ, VPQ, gidx)
        assert S.shape == (F,)
        errs.update(S=_rel(S, want["S"]))
        ghat, PQbar = em.edge_max_dbl_graph(r, sel, PQ, VPQ, gidx, st[0], k)
        assert PQbar is None
    errs.update(ghat=_rel(ghat, want["ghat"].reshape(M, F)))
    assert float(ghat.cpu()[clipped.reshape(M, F)].abs().max() if clipped.any() else 0.0) == 0.0      # exactly zero where the ReLU clipped
    print("launchers (%d,%d,%d,%d) %s: rel-L2 vs float64 model %s" % (B, N, k, F, "train" if training else "eval",
                                                                     {n: "%.2e" % e for n, e in errs.items()}))
    for n, e in errs.items():
        assert e < 1e-5, (n, e)


# ---------------------------------------------------------------- module against the model
def _layer(sp, tag, double_backward=True):
    c = ecm.CASES[tag]
    x, g, sd = ecm.case_tensors(tag, 0)
    m = sp.edgeConv(c["Fin"], c["Fout"], c["k"], double_backward=double_backward)
    m.load_state_dict(sd, strict=True)
    return c, x, g, sd, m.cuda().train(c["train"])


def _direction(tag, x):
    from spgan import fixture_rng as fr
    return fr.normal("edgeconv.%s.v" % tag, tuple(x.shape), salt=0)


@pytest.mark.parametrize("tag", TAGS)
def test_module_against_model(sp, tag):
    c, x, g, sd, m = _layer(sp, tag)
    idx = edm.brute_force_graph(x, c["k"])
    v = _direction(tag, x)
    xg, gg = x.cuda().requires_grad_(True), g.cuda().requires_grad_(True)
    out = m(xg, idx=idx.cuda())
    (dx,) = torch.autograd.grad(out, xg, gg, create_graph=True)
    assert dx.requires_grad and dx.grad_fn is not None
    params = dict(m.named_parameters())
    got = dict(zip(("xbar", "ghat") + NAMES,
                   torch.autograd.grad((v.cuda() * dx).sum(), [xg, gg] + [params[n] for n in NAMES], allow_unused=True)))

    sd64 = {n: (t.double() if t.dtype.is_floating_point else t) for n, t in sd.items()}
    f = ecm.forward(x.double(), idx, c["k"], sd64[NAMES[0]], sd64[NAMES[1]], sd64[NAMES[2]], sd64[NAMES[3]], sd64["conv.bn.running_mean"],
                    sd64["conv.bn.running_var"], c["train"])
    sel = m.last_sel.cpu().view(c["B"], c["N"], c["Fout"])
    rank, clipped = (sel & 0x7f).long(), (sel & 0x80) != 0
    # a condition, not a tolerance: the kernel's selection is the model's own up to float32 rounding at a tie
    differ = int(((rank != f["sel"]) | (clipped != (f["out_pm"] <= 0))).sum())
    print("%s: last_sel differs from the float64 model's selection in %d of %d entries" % (tag, differ, sel.numel()))
    assert differ * 1000 <= sel.numel()
    assert _rel(dx, ecm.backward(f, g.double(), sel=rank, active=~clipped)["dx"]) < 1e-5
    want = edm.double_backward(f, g.double(), v.double(), sel=rank, active=~clipped)
    errs = {"Wbar": _rel(got[NAMES[0]], want["Wbar"]), "gammabar": _rel(got[NAMES[2]], want["gammabar"]), "ghat": _rel(got["ghat"], want["ghat"])}
    if c["train"]:
        errs["xbar"] = _rel(got["xbar"], want["xbar"])
    else:
        assert got["xbar"] is None
    print("%s: rel-L2 vs float64 model with the layer's selection %s" % (tag, {n: "%.2e" % e for n, e in errs.items()}))
    for n, e in errs.items():
        assert e < 1e-5, (tag, n, e)                                 # measured (MI355X) <= 2.6e-7 over the four cases; 0 selection differences
    for n in (NAMES[1], NAMES[3]):                                  # conv bias, beta: no second derivative
        assert got[n] is None or float(got[n].abs().max()) == 0.0, n


# ---------------------------------------------------------------- a stacked critic under GradientPenalty
B2, N2, K2 = 2, 64, 8


class _Critic(nn.Module):
    def __init__(self, sp, idx, double_backward=True):
        super().__init__()
        self.l1 = sp.edgeConv(3, 16, K2, double_backward=double_backward)
        self.l2 = sp.edgeConv(16, 32, K2, double_backward=double_backward)
        self.fc = nn.Linear(32, 1)
        self.idx = idx

    def forward(self, x):
        h = self.l2(self.l1(x, idx=self.idx), idx=self.idx)             # a shared graph
        return self.fc(h.max(dim=2)[0])


def _critic_problem(sp):
    from spgan import fixture_rng as fr
    real = fr.uniform("edgeconv.critic.real", (B2, 3, N2), -1.0, 1.0)
    fake = fr.uniform("edgeconv.critic.fake", (B2, 3, N2), -1.0, 1.0)
    alpha = fr.uniform("edgeconv.critic.alpha", (B2, 1, 1), 0.2, 0.8)
    idx = edm.brute_force_graph(real, K2)
    torch.manual_seed(11)
    net = _Critic(sp, idx.cuda())
    with torch.no_grad():                                              # statistics-sensitive parameters away from their initial 1 / 0
        for l in (net.l1, net.l2):
            l.conv.bn.weight.copy_(fr.uniform("edgeconv.critic.gamma%d" % l.Fin, (l.Fout,), 0.5, 1.5))
            l.conv.bn.weight[::4] *= -1
            l.conv.bn.bias.copy_(fr.uniform("edgeconv.critic.beta%d" % l.Fin, (l.Fout,), -0.2, 0.2))
    return net.cuda().train(), real, fake, alpha, idx


def _penalty_grads(sp, net, real, fake, alpha):
    for p in net.parameters():
        p.grad = None
    pen = sp.GradientPenalty(10)(net, real.cuda(), fake.cuda(), alpha=alpha.cuda())
    pen.backward()
    return pen.detach(), {n: (None if p.grad is None else p.grad.clone()) for n, p in net.named_parameters()}


def _critic_float64(net, real, fake, alpha, idx):
    """the same critic with edgeconv_model.composition in float64 torch, under the penalty of Common/gradient_penalty.py"""
    sd = {n: t.detach().double().cpu().requires_grad_(True) for n, t in net.named_parameters()}
    x_hat = (real.double() + alpha.double() * (fake.double() - real.double())).requires_grad_(True)
    h = x_hat
    for l in ("l1", "l2"):
        h, _ = ecm.composition(h, idx, K2, sd[l + ".conv.conv.weight"], sd[l + ".conv.conv.bias"], sd[l + ".conv.bn.weight"],
                               sd[l + ".conv.bn.bias"], None, None, True)
    disc = h.max(dim=2)[0] @ sd["fc.weight"].t() + sd["fc.bias"]
    (g,) = torch.autograd.grad(disc, x_hat, torch.ones_like(disc), create_graph=True)
    norms = g.reshape(B2, -1).norm(2, dim=1)
    pen = 10.0 * ((norms - 1.0) ** 2).mean()
    grads = torch.autograd.grad(pen, list(sd.values()), allow_unused=True)
    return pen.detach(), dict(zip(sd.keys(), grads)), norms.detach()


def test_stacked_critic_under_gradient_penalty(sp):
    """edgeConv(3,16,8) -> edgeConv(16,32,8) on a shared graph -> max over points -> Linear(32,1) under spgan.GradientPenalty(10): the chained
    cotangent (layer 2's ghat is layer 1's direction) and the first-order backward fed by xbar, against float64 torch.
    Measured (MI355X): parameter gradients 3.6e-7 .. 8.9e-7, penalty 3e-7, amplification 2.1."""
    net, real, fake, alpha, idx = _critic_problem(sp)
    pen, got = _penalty_grads(sp, net, real, fake, alpha)
    pen64, want, norms = _critic_float64(net, real, fake, alpha, idx)
    amp = float((norms / (norms - 1.0).abs()).max())
    print("penalty %.6f (float64 %.6f); ||g|| %s; amplification %.2f" % (float(pen), float(pen64), [round(float(n), 4) for n in norms], amp))
    assert amp < 10.0
    assert abs(float(pen) - float(pen64)) < 1e-5 * abs(float(pen64))
    errs = {}
    # l1's beta shifts l2's input: it has a gradient here, through xbar and l1's first-order backward
    for n in ("l1.conv.conv.weight", "l1.conv.bn.weight", "l1.conv.bn.bias", "l2.conv.conv.weight", "l2.conv.bn.weight", "fc.weight"):
        errs[n] = _rel(got[n], want[n])
    print("critic parameter gradients: rel-L2 vs float64 torch %s" % {n: "%.2e" % e for n, e in errs.items()})
    for n, e in errs.items():
        assert e < 1e-4, (n, e)
    # a conv bias in front of a train-mode BatchNorm, the last layer's beta and the critic's bias: no gradient
    for n in ("l1.conv.conv.bias", "l2.conv.conv.bias", "l2.conv.bn.bias", "fc.bias"):
        assert got[n] is None or float(got[n].abs().max()) == 0.0, n
        assert want[n] is None or float(want[n].abs().max()) < 1e-12, n


def test_penalty_repeats_bit_for_bit(sp):
    net, real, fake, alpha, _ = _critic_problem(sp)
    p1, g1 = _penalty_grads(sp, net, real, fake, alpha)
    p2, g2 = _penalty_grads(sp, net, real, fake, alpha)
    assert torch.equal(p1, p2)
    for n in g1:
        assert (g1[n] is None and g2[n] is None) or torch.equal(g1[n], g2[n]), n
    assert g1["l1.conv.conv.weight"] is not None and float(g1["l1.conv.conv.weight"].abs().max()) > 0.0


# ---------------------------------------------------------------- behaviour
@pytest.mark.parametrize("tag", ["feat", "eval"])
def test_first_order_is_bit_identical_to_the_default_layer(sp, tag):
    res = []
    for dbl in (False, True):
        c, x, g, _, m = _layer(sp, tag, double_backward=dbl)
        xg = x.cuda().requires_grad_(True)
        out = m(xg)
        (out * g.cuda()).sum().backward()
        res.append([out.detach().clone(), xg.grad.clone(), m.last_sel.clone()] + [p.grad.clone() for p in m.parameters()] +
                   [b.clone() for b in m.buffers()])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    with torch.no_grad():                                              # and nothing is kept without a graph
        assert not m(x.cuda()).requires_grad


def test_third_derivative_raises(sp):
    c, x, g, _, m = _layer(sp, "feat")
    xg = x.cuda().requires_grad_(True)
    (dx,) = torch.autograd.grad(m(xg), xg, g.cuda(), create_graph=True)
    L = (dx * _direction("feat", x).cuda()).sum()
    with pytest.raises(RuntimeError, match="third derivative"):
        torch.autograd.grad(L, xg, create_graph=True)


def test_cotangent_on_parameter_gradient_raises(sp):
    c, x, g, _, m = _layer(sp, "feat")
    xg = x.cuda().requires_grad_(True)
    dx, dW = torch.autograd.grad(m(xg), (xg, m.conv.conv.weight), g.cuda(), create_graph=True)
    assert dW.requires_grad
    with pytest.raises(NotImplementedError, match="dW"):
        torch.autograd.grad(dW.sum(), xg)


def test_default_layer_still_refuses(sp):
    c, x, g, _, m = _layer(sp, "feat", double_backward=False)
    xg = x.cuda().requires_grad_(True)
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(m(xg).sum(), xg, create_graph=True)
    m.double_backward = True                                          # a plain attribute: read at every forward
    (dx,) = torch.autograd.grad(m(xg).sum(), xg, create_graph=True)
    assert dx.requires_grad
