"""GPU: the bilateral / deform blocks of spgan.modules (edge_conv.BlockTailFn over csrc/block_tail.hip behind the edge convolutions) against
the vectors captured from the reference (golden blocks.npz / blocks2.npz), and the four block-tail launchers against the float64 model of
tests/blocks_model.py.

Tolerances, the siblings' (tests/test_bilateral_gpu.py).  Modules vs golden with the reference's graph injected: rel-L2 3e-6 for the
outputs, dx and dpc, 5e-6 for parameter gradients, buffers rtol 1e-5 / atol 1e-6 -- or 5 x the golden's stored float32-vs-float64 distance of
the quantity where that is larger (`_bound`; the capture script lists the quantities that take the fallback: behind the BatchNorm1d's over
the four rows of the global branch the reference's own float32 run is up to 1.2e-5 from its float64 run).  A conv / linear bias in front
of a train-mode BatchNorm: its gradient is an exact zero here and rounding noise in the reference (2e-3 absolute).
Launchers vs the float64 model on the same float32 operands: 2e-6 for outputs and gradients, 1e-5 for statistics and sums (the weighted
layer's launcher bounds), or 5 x the rel-L2 distance between a float32 and a float64 CPU evaluation of the model on those operands where
that is larger."""
import numpy as np
import pytest
import torch

import blocks_model as km
from helpers import check

pytestmark = pytest.mark.gpu
TAGS = list(km.CASES)


@pytest.fixture(scope="module")
def sp():
    import spgan
    from spgan import _lib
    _lib.load()
    return spgan


@pytest.fixture(scope="module")
def d():
    return km.load_golden()


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _module(sp, d, tag):
    m = km.make_module(km.CASES[tag], sp)
    m.load_state_dict(km.golden_state_dict(d, tag), strict=True)
    return m.cuda().train(km.CASES[tag]["train"])


def _run(m, d, tag, inject=True, use=(True, True)):
    """forward + backward of the case -> (x, pc | None, x_out, g_out | None); use: which outputs' cotangents enter the loss"""
    c = km.CASES[tag]
    takes_pc = km.BLOCKS[c["block"]][3]
    x = torch.from_numpy(d[tag + "|x"]).cuda().requires_grad_(True)
    pc = torch.from_numpy(d[tag + "|pc"]).cuda().requires_grad_(True) if takes_pc else None
    idx = torch.from_numpy(d[tag + "|idx"]).cuda() if inject else None
    out = m(x, pc, idx=idx) if takes_pc else m(x, idx=idx)
    x_out, g_out = out if isinstance(out, tuple) else (out, None)
    gx, gg = km.golden_cotangents(d, tag)
    loss = 0.0
    if use[0]:
        loss = loss + (x_out * gx.cuda()).sum()
    if use[1] and g_out is not None:
        loss = loss + (g_out * gg.cuda()).sum()
    loss.backward()
    return x, pc, x_out, g_out


def _bound(d, tag, q, base):
    return max(base, 5.0 * km.noise(d, tag, q))


# ---------------------------------------------------------------- modules against the reference (golden)
@pytest.mark.parametrize("tag", TAGS)
def test_module_golden_with_injected_graph(sp, d, tag):
    c = km.CASES[tag]
    train = c["train"]
    m = _module(sp, d, tag)
    keys = tuple(str(n) for n in d["state_keys|" + c["block"]])
    assert tuple(m.state_dict()) == keys and len(keys) == km.STATE_COUNTS[c["block"]]
    before = {n: b.clone() for n, b in m.named_buffers()}
    x, pc, x_out, g_out = _run(m, d, tag)
    sx, sg = km.out_shapes(c)
    assert tuple(x_out.shape) == sx and (None if g_out is None else tuple(g_out.shape)) == sg
    e = {"x_out": check(d, tag + "|x_out", x_out, rtol=_bound(d, tag, "x_out", 3e-6), atol=1e-7),
         "dx": check(d, tag + "|dx", x.grad, rtol=_bound(d, tag, "dx", 3e-6), atol=1e-7)}
    if g_out is not None:
        e["g_out"] = check(d, tag + "|g_out", g_out, rtol=_bound(d, tag, "g_out", 3e-6), atol=1e-7)
    if pc is not None:
        e["dpc"] = check(d, tag + "|dpc", pc.grad, rtol=_bound(d, tag, "dpc", 3e-6), atol=1e-7)
    zero = km.zero_grad_biases(keys) if train else ()
    for n, p in m.named_parameters():
        if n in zero:
            assert float(p.grad.abs().max()) == 0.0, n                      # exact zeros here
            assert float(np.abs(d["%s|grad|%s|full" % (tag, n)]).max()) <= 2e-3, n
            continue
        e[n] = check(d, "%s|grad|%s" % (tag, n), p.grad, rtol=_bound(d, tag, "grad|" + n, 5e-6), atol=1e-7)
    print("%s: rel-L2 vs reference float32 %s" % (tag, {k: "%.2e" % v for k, v in e.items()}))
    for n, b in m.named_buffers():
        np.testing.assert_allclose(b.cpu().numpy(), d["%s|buf|%s|full" % (tag, n)], rtol=1e-5, atol=1e-6, err_msg=n)
        if not train:                                                        # eval mode leaves the buffers untouched (bit for bit)
            assert torch.equal(b, before[n]), n
        elif n.endswith("num_batches_tracked"):
            assert int(b) == int(before[n]) + 1, n
    assert m.last_idx is not None and tuple(m.last_idx.shape) == (c["B"] * c["N"], km.layer_k(c))
    # the reference's checkpoint format, both ways
    back = km.make_module(c, sp)
    back.load_state_dict(m.state_dict(), strict=True)


@pytest.mark.parametrize("tag", ["l2", "df"])
def test_module_own_graph_matches_reference(sp, d, tag):
    """The block's own kNN graph: every row that differs from the reference's graph is a near-tie row, and where no row differs the
    results are the injected graph's, bit for bit."""
    c = km.CASES[tag]
    k = km.layer_k(c)
    m = _module(sp, d, tag)
    x, pc, x_out, g_out = _run(m, d, tag, inject=False)
    own = sp.ops.idx_to_local64(m.last_idx, c["B"], c["N"]).view(-1, k).cpu().numpy()
    ref = d[tag + "|idx"].reshape(-1, k)
    near = d[tag + "|near_tie_rows"].astype(bool)
    assert near.mean() <= 0.01
    differ = (own != ref).any(axis=1)
    assert not differ[~near].any(), int(differ[~near].sum())
    if not differ.any():                                                     # the same graph: the injected route's bits
        x2, pc2, x_out2, g_out2 = _run(_module(sp, d, tag), d, tag)
        assert torch.equal(x_out, x_out2) and torch.equal(g_out, g_out2) and torch.equal(x.grad, x2.grad)
    print("%s: %d rows differ from the reference's graph (%d near-tie rows)" % (tag, int(differ.sum()), int(near.sum())))


def _grads(m, x, pc):
    out = {"dx": x.grad, "dpc": None if pc is None else pc.grad}
    out.update({n: p.grad for n, p in m.named_parameters()})
    return out


@pytest.mark.parametrize("tag", ["l2", "dm"])
def test_single_output_backward(sp, d, tag):
    """Backward through x_out alone / g_out alone (the other cotangent reaches the kernels as NULL) equals the two-cotangent backward with
    the other cotangent zero."""
    gx, gg = km.golden_cotangents(d, tag)
    for use in ((True, False), (False, True)):
        m1 = _module(sp, d, tag)
        x1, pc1, _, _ = _run(m1, d, tag, use=use)
        m2 = _module(sp, d, tag)
        x2 = torch.from_numpy(d[tag + "|x"]).cuda().requires_grad_(True)
        pc2 = torch.from_numpy(d[tag + "|pc"]).cuda().requires_grad_(True)
        x_out, g_out = m2(x2, pc2, idx=torch.from_numpy(d[tag + "|idx"]).cuda())
        ((x_out * (gx.cuda() if use[0] else torch.zeros_like(x_out))).sum() + (g_out * (gg.cuda() if use[1] else torch.zeros_like(g_out))).sum()).backward()
        a, b = _grads(m1, x1, pc1), _grads(m2, x2, pc2)
        for n in b:
            ga = a[n] if a[n] is not None else torch.zeros_like(b[n])        # a parameter only the unused output reaches: no gradient at all
            assert torch.equal(ga, b[n]), (tag, use, n, _rel(ga, b[n]))


def test_eval_mode_single_shape(sp, d):
    """Eval mode with B = 1 runs (train mode raises ValueError, as the reference fails in BatchNorm1d)."""
    m = _module(sp, d, "dfe")
    x = torch.from_numpy(d["dfe|x"][:1]).cuda()
    x_out, g_out = m(x)
    assert tuple(x_out.shape) == (1, 16, 24) and tuple(g_out.shape) == (1, 528, 24) and bool(torch.isfinite(x_out).all())
    with pytest.raises(ValueError, match="B=1"):
        m.train()(x)


# ---------------------------------------------------------------- the four launchers against the model
SHAPES = [(3, 5, 23, 7, 0), (2, 16, 48, 16, 512), (2, 3, 4100, 0, 512), (1, 4, 1, 4, 0)]


def _operands(B, C, L, Cs, Cg):
    g = torch.Generator().manual_seed(B * 1000 + C * 10 + L)
    r = lambda *s: torch.randn(*s, generator=g)
    Y = r(B, C, L) * 0.7 + r(1, C, 1)
    xs, gv = (r(B, Cs) if Cs else None), (r(B, Cg) if Cg else None)
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[::3] *= -1.0
    beta = r(C) * 0.2
    return Y, xs, gv, gamma, beta, r(B, Cs + C, L), r(B, Cg + C, L), r(B, C, L)


def _model(dt, Y, xs, gv, gamma, beta, dx, dg, ex, Cs, Cg, train):
    t = lambda v: None if v is None else v.to(dt)
    Y, xs, gv, gamma, beta, dx, dg, ex = [t(v) for v in (Y, xs, gv, gamma, beta, dx, dg, ex)]
    if train:
        mean, var = km.cm_stats(Y)
    else:
        mean, var = torch.zeros_like(gamma) + 0.1, torch.ones_like(gamma) * 0.8
    invstd = 1.0 / torch.sqrt(var + km.EPS)
    scale = gamma * invstd
    shift = beta - mean * scale
    out_x, out_g = km.tail_fwd(Y, xs, gv, scale, shift)
    return dict(mean=mean, invstd=invstd, scale=scale, shift=shift, out_x=out_x, out_g=out_g)


def _dev(*ts):
    return [None if t is None else t.cuda() for t in ts]


@pytest.mark.parametrize("B,C,L,Cs,Cg", SHAPES)
def test_launchers_against_model(sp, B, C, L, Cs, Cg):
    """(3,5,23,7,0): the scalar path, no g; (2,16,48,16,512): the vector path, both outputs; (2,3,4100,0,512): a row longer than one pass
    of a wave (and of a workgroup), no xs; (1,4,1,4,0): one value per channel."""
    bt, em = sp.block_tail, sp.edge_max
    Y, xs, gv, gamma, beta, dx, dg, ex = _operands(B, C, L, Cs, Cg)
    if not Cg:
        dg = None
    f64, f32 = (_model(dt, Y, xs, gv, gamma, beta, dx, dg, ex, Cs, Cg, True) for dt in (torch.float64, torch.float32))

    def bwd(f, dt, dx_, dg_, ex_, train=True):
        t = lambda v: None if v is None else v.to(dt)
        sums, dxs, dgs, dY = km.tail_bwd(t(Y), t(dx_), t(dg_), t(ex_), Cs, Cg, f["scale"], f["shift"], f["mean"], f["invstd"], t(gamma), train)
        return dict(sums=sums, dxs=dxs, dg=dgs, dY=dY)
    base = dict(mean=1e-5, invstd=1e-5, scale=1e-5, shift=1e-5, out_x=2e-6, out_g=2e-6, sums=1e-5, dxs=1e-5, dg=1e-5, dY=2e-6)

    def bounds(m32, m64):
        return {q: max(base[q], 5.0 * _rel(m32[q], m64[q])) for q in m64 if m64[q] is not None}
    Yd, xsd, gvd, gammad, betad, dxd, dgd, exd = _dev(Y, xs, gv, gamma, beta, dx, dg, ex)
    # statistics: the records go through the existing finalize
    part, tile_rows = bt.cm_stats(Yd)
    assert tuple(part.shape) == (B, C, 2) and tile_rows == L
    scale, shift, invstd, mean = em.edge_max_bn(part, tile_rows, B * L, gammad, betad, None, None)
    out_x, out_g = bt.block_tail_fwd(Yd, xsd, gvd, scale, shift, want_g=Cg > 0)
    got = dict(mean=mean, invstd=invstd, scale=scale, shift=shift, out_x=out_x, out_g=out_g)
    bd = bounds(f32, f64)
    err = {q: _rel(got[q], f64[q]) for q in bd}
    print("B %d C %d L %d Cs %d Cg %d forward: %s" % (B, C, L, Cs, Cg, {q: "%.2e" % v for q, v in err.items()}))
    for q in bd:
        assert err[q] <= bd[q], (q, err[q], bd[q])
    assert tuple(out_x.shape) == (B, Cs + C, L) and (out_g is None) == (Cg == 0)
    if Cs:                                                                       # the broadcast channels are the vectors' bits
        assert torch.equal(out_x[:, :Cs], xsd.view(B, Cs, 1).expand(B, Cs, L))
    if Cg:
        assert torch.equal(out_g[:, :Cg], gvd.view(B, Cg, 1).expand(B, Cg, L)) and torch.equal(out_g[:, Cg:], out_x[:, Cs:])
    # backward on the model's own float32 statistics (so that the mask is the model's): every cotangent absent in turn, and eval mode
    st = _dev(f32["scale"], f32["shift"], f32["mean"], f32["invstd"])
    st64 = {q: f32[q].double() for q in ("scale", "shift", "mean", "invstd")}
    for name, (hx, hg, he) in dict(all=(1, 1, 1), no_x=(0, 1, 1), no_g=(1, 0, 1), no_extra=(1, 1, 0), extra_only=(0, 0, 1)).items():
        for train in (True, False):
            cpu = (dx if hx else None, dg if hg else None, ex if he else None)
            gpu = (dxd if hx else None, dgd if hg else None, exd if he else None)
            ref, m32 = bwd(st64, torch.float64, *cpu, train=train), bwd(f32, torch.float32, *cpu, train=train)
            sums, dxs, dgs = bt.block_tail_bwd_reduce(Yd, *gpu, Cs, Cg, *st)
            dY = bt.block_tail_bwd_apply(Yd, *gpu, Cs, Cg, *st, gammad, sums if train else None)
            got = dict(sums=sums, dxs=dxs, dg=dgs, dY=dY)
            bd = {q: max(base[q], 5.0 * _rel(m32[q], ref[q])) for q in ("sums", "dxs", "dg", "dY")}
            for q in bd:
                if (q == "dxs" and not Cs) or (q == "dg" and not Cg):
                    assert got[q] is None
                    continue
                e_ = _rel(got[q], ref[q])
                assert e_ <= bd[q], (name, train, q, e_, bd[q])
            # two runs: the same bits
            sums2, dxs2, dgs2 = bt.block_tail_bwd_reduce(Yd, *gpu, Cs, Cg, *st)
            dY2 = bt.block_tail_bwd_apply(Yd, *gpu, Cs, Cg, *st, gammad, sums2 if train else None)
            assert torch.equal(sums, sums2) and torch.equal(dY, dY2)
    part2, _ = bt.cm_stats(Yd)
    ox2, og2 = bt.block_tail_fwd(Yd, xsd, gvd, scale, shift, want_g=Cg > 0)
    assert torch.equal(part, part2) and torch.equal(out_x, ox2) and (og2 is None or torch.equal(out_g, og2))
    # the middle blocks' call: g_out alone, no xs
    if Cg:
        nx, og3 = bt.block_tail_fwd(Yd, None, gvd, scale, shift, want_x=False)
        assert nx is None and torch.equal(og3, out_g)
