"""GPU: the dense family (spgan.DenseEdgeModule, DenseModule1D, Dense_Attn, get_graph_feature; csrc/edge_dense.hip) against the float64
model (tests/dense_edge_model.py) and the reference's golden results (tests/golden/dense_edge.npz).

Bounds.  Launchers vs the float64 model on the same float32 operands: float32 arithmetic on sums of K (or in-degree) well-conditioned
terms, rel-L2 2e-6 forward and 1e-5 backward, as the edge family's launcher tests carry.  Modules vs the golden: rel-L2 against the
reference's float64 run, bounded per case and quantity by 10 x the reference's OWN float32-vs-float64 distance stored in the golden
(`tag|noise|q`) -- the margin the edge family's tests carry between their bounds (3e-6 / 5e-6) and what was measured on the MI355X
(1.2e-7 .. 4.4e-7): the GPU sums in another order at the same precision.  A conv bias in front of a train-mode BatchNorm has a gradient
that is exactly zero here and rounding noise in the reference: asserted zero, with the absolute bound 2e-3 (test_edgeconv_gpu._atol).
Buffers: rtol 1e-5 / atol 1e-6.  Measured errors: next to each bound below and in DESIGN.md section 29."""
import os

import numpy as np
import pytest
import torch

import dense_edge_model as dem

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_edge.npz")
MARGIN = 10.0
FWD, BWD = 2e-6, 1e-5


@pytest.fixture(scope="module")
def sp():
    import spgan
    return spgan


@pytest.fixture(scope="module")
def d():
    return np.load(GOLD)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _rand(name, shape, std=1.0):
    from spgan import fixture_rng as fr
    return fr.normal("dense_edge_gpu." + name, shape, std)


# ---------------------------------------------------------------- the level kernel against the model
LEVEL_SHAPES = [(250, 12, 24, 5), (231, 7, 7, 3), (640, 64, 192, 20), (660, 72, 144, 20)]       # M, N, K, k (M % k == 0)


@pytest.mark.parametrize("addend", [False, True])
@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("M,N,K,k", LEVEL_SHAPES)
def test_level_kernel(sp, M, N, K, k, raw, addend):
    """Y = op(A) W^T (+ Q + P[idx]) written IN PLACE into a slice of the buffer A is read from; the records, finalised, are the column
    mean / variance.  Measured on the MI355X over the 16 cases: Y rel-L2 4.3e-8 .. 2.6e-7 (bound 2e-6), mean <= 9.5e-8 of the column's scale (2e-6), variance <= 3.1e-7 relative (1e-5)."""
    from spgan import edge_dense, edge_max
    tag = "level.%d.%d.%d" % (M, N, K)
    raw_cols = (K + 2) // 3 if raw else 0
    # with the addend: a row stride that is a multiple of 4 floats (the 16-byte staging path); without: an odd one (element by element)
    pad = 4 + (-(K + N)) % 4 + (0 if addend else 1)
    buf0 = _rand(tag + ".buf", (M, K + N + pad))
    assert ((K + N + pad) % 4 == 0) == addend
    W = _rand(tag + ".W", (N, K), 1.0 / np.sqrt(K)).cuda()
    if addend:                                                              # W too with a row stride of a multiple of 4 floats: K = 7 ends inside a 16-byte group
        W = torch.cat([W, torch.full((N, (-K) % 4), float("nan"), device="cuda")], dim=1)[:, :K]
    scale, shift = _rand(tag + ".sc", (K,), 0.5, ) + 1.0, _rand(tag + ".sh", (K,), 0.3)
    scale[K // 2] *= -1.0
    bias = _rand(tag + ".bias", (N,)) if raw else None
    PQ = idx = None
    if addend:
        PQ = _rand(tag + ".PQ", (M // k, 2 * N + 1)).cuda()
        idx = torch.from_numpy(np.random.default_rng(M).integers(0, M // k, size=(M // k, k)).astype(np.int32)).cuda()
    buf = buf0.cuda()
    A, out = buf[:, :K], buf[:, K:K + N]
    ad = (PQ[:, :N], PQ[:, N + 1:], idx) if addend else None
    _, part, tile_rows = edge_dense.edge_dense_level(A, W, out, raw_cols=raw_cols, scale=scale.cuda(), shift=shift.cuda(), bias=None if bias is None else bias.cuda(),
                                                     addend=ad, stats=True)
    ref = dem.level_model(buf0[:, :K], W, raw_cols, scale, shift, bias, None if PQ is None else PQ[:, :N], None if PQ is None else PQ[:, N + 1:], idx)
    torch.cuda.synchronize()
    assert torch.equal(buf[:, :K].cpu(), buf0[:, :K]) and torch.equal(buf[:, K + N:].cpu(), buf0[:, K + N:])     # nothing but the slice was written
    e = _rel(out, ref)
    print("%s raw=%d addend=%d: Y rel-L2 %.2e" % (tag, raw_cols, addend, e))
    assert e < FWD
    # the same product into a tensor of its own: bit-identical
    own = torch.empty((M, N), dtype=torch.float32, device="cuda")
    edge_dense.edge_dense_level(buf0[:, :K].cuda(), W, own, raw_cols=raw_cols, scale=scale.cuda(), shift=shift.cuda(), bias=None if bias is None else bias.cuda(), addend=ad)
    assert torch.equal(own, out)
    st = edge_max.edge_max_bn(part, tile_rows, M, torch.ones(N, device="cuda"), torch.zeros(N, device="cuda"), None, None)
    mean, var = st[3].double().cpu(), (1.0 / st[2].double().cpu() ** 2 - 1e-5)
    rmean, rvar = ref.mean(dim=0), ref.var(dim=0, unbiased=False)
    em = float(((mean - rmean).abs() / (rmean.abs() + rvar.sqrt())).max())
    ev = float(((var - rvar).abs() / rvar).max())
    print("%s: mean %.2e of the column's scale, variance %.2e relative" % (tag, em, ev))
    assert em < FWD and ev < BWD


def test_level_kernel_gather_only_and_refusals(sp):
    """A = None: the addend alone, the first level of DenseEdgeModule (equal to edge_weight_gather bit for bit); overlapping slices and
    misfits are refused before any launch."""
    from spgan import edge_dense, edge_weight
    M_, k, N = 77, 3, 20
    PQ = _rand("gather.PQ", (M_, 2 * N)).cuda()
    idx = torch.from_numpy(np.random.default_rng(1).integers(0, M_, size=(M_, k)).astype(np.int32)).cuda()
    Z = torch.zeros((M_ * k, 3 * N), device="cuda")
    edge_dense.edge_dense_level(None, None, Z[:, N:2 * N], addend=(PQ[:, :N], PQ[:, N:], idx))
    assert torch.equal(Z[:, N:2 * N], edge_weight.edge_weight_gather(PQ, idx))
    assert float(Z[:, :N].abs().max()) == 0.0 and float(Z[:, 2 * N:].abs().max()) == 0.0
    W = torch.zeros((N, 2 * N), device="cuda")
    with pytest.raises(ValueError, match="overlaps"):
        edge_dense.edge_dense_level(Z[:, :2 * N], W, Z[:, N:2 * N], raw_cols=2 * N)
    with pytest.raises(ValueError):
        edge_dense.edge_dense_level(Z[:, :N], W, Z[:, N:2 * N])                   # W does not fit
    with pytest.raises(ValueError, match="scale"):
        edge_dense.edge_dense_level(Z[:, :2 * N], W, Z[:, 2 * N:], raw_cols=3)
    with pytest.raises(RuntimeError, match="GPU"):
        edge_dense.edge_dense_level(Z[:, :2 * N].cpu(), W, Z[:, 2 * N:], raw_cols=2 * N)
    lib = sp._lib.load()
    assert lib.spgan_edge_dense_level(None, 0, 0, None, None, 0.2, None, 0, None, None, 0, 0, None, 1, 4, 4, 0, Z.data_ptr(), 4, None, None) == -22
    assert lib.spgan_edge_dense_scatter(None, 4, None, None, 4, 1, 4, None, 8, None) == -22


# ---------------------------------------------------------------- the scatter and the strided BatchNorm backward against the model
@pytest.mark.parametrize("C", [50, 300])
def test_scatter_kernel(sp, C):
    """a graph with an isolated point and a point that every row gathers.  Measured: rel-L2 6.1e-8 and 5.4e-8 (bound 1e-5)."""
    from spgan import edge_dense
    M_, k, hub, iso = 37, 4, 5, 11
    rng = np.random.default_rng(C)
    nb = rng.integers(0, M_ - 1, size=(M_, k))
    nb[nb >= iso] += 1                                                     # nobody gathers `iso`
    nb[:, 0] = hub
    idx = torch.from_numpy(nb.astype(np.int32)).cuda()
    wide = _rand("scatter.%d" % C, (M_ * k, C + 7))
    D = wide.cuda()[:, 3:3 + C]
    rowptr, src = sp.ops.csr_build(idx, 1, M_)
    dPQ = edge_dense.edge_dense_scatter(D, rowptr, src, k)
    ref = dem.scatter_model(wide[:, 3:3 + C], idx)
    e = _rel(dPQ, ref)
    print("scatter C=%d: rel-L2 %.2e" % (C, e))
    assert e < BWD
    assert float(dPQ[iso, :C].abs().max()) == 0.0
    assert torch.equal(dPQ, edge_dense.edge_dense_scatter(D, rowptr, src, k))


def test_bn_apply_strided(sp):
    from spgan import edge_dense
    M_, C = 301, 23
    g, z = _rand("apply.g", (M_, C)), _rand("apply.z", (M_, C + 9))
    mean, invstd, gamma, sums = _rand("apply.m", (C,), 0.1), _rand("apply.i", (C,), 0.1) + 1.0, _rand("apply.ga", (C,)), _rand("apply.s", (2 * C,), 5.0)
    out = torch.zeros((M_, 3 * C), device="cuda")
    edge_dense.edge_dense_bn_apply(g.cuda(), z.cuda()[:, 4:4 + C], mean.cuda(), invstd.cuda(), gamma.cuda(), sums.cuda(), 777, out[:, C:2 * C])
    ref = dem.bn_apply_model(g, z[:, 4:4 + C], mean, invstd, gamma, sums, 777)
    assert _rel(out[:, C:2 * C], ref) < FWD
    assert float(out[:, :C].abs().max()) == 0.0 and float(out[:, 2 * C:].abs().max()) == 0.0


# ---------------------------------------------------------------- the modules against the golden
def _module(sp, d, tag, sd=None):
    m = dem.build_module(sp, tag)
    m.load_state_dict(dem.golden_state_dict(d, tag) if sd is None else sd, strict=True)
    return m.cuda().train(dem.CASES[tag]["train"])


def _run(m, tag, x, g, idx=None, x_grad=True):
    xr = x.cuda().clone().requires_grad_(x_grad)
    out = m(xr, idx=idx) if dem.kind_of(tag) == "edge" else m(xr)
    (out * g.cuda()).sum().backward()
    res = {"out": out.detach(), "dx": xr.grad}
    for n, p in m.named_parameters():
        res["grad|" + n] = p.grad
    for n, b in m.named_buffers():
        res["buf|" + n] = b.detach()
    return res


def _golden_inputs(d, tag):
    x, g = torch.from_numpy(d[tag + "|x"]), torch.from_numpy(d[tag + "|g"])
    idx = torch.from_numpy(d[tag + "|idx"]).cuda() if (tag + "|idx") in d.files else None
    return x, g, idx


def _zero_bias(q, tag):
    """a conv bias in front of a train-mode BatchNorm"""
    return dem.zero_gradient(tag, q) == "exact"


def _check_against_golden(d, tag, res, what):
    worst = {}
    for q in dem.quantities(d, tag):
        ref, got = dem.golden_f64(d, tag, q), res[q]
        if q.endswith("num_batches_tracked"):
            assert int(got) == int(ref), q
        elif q.startswith("buf|"):
            assert torch.allclose(got.double().cpu(), ref, rtol=1e-5, atol=1e-6), (tag, q)
        elif _zero_bias(q, tag):
            assert int(torch.count_nonzero(got)) == 0, (tag, q)
            assert float(ref.abs().max()) < 2e-3, (tag, q)
        elif dem.zero_gradient(tag, q) == "noise":                     # zero in exact arithmetic, computed like any gradient: the same absolute bound
            assert float(got.abs().max()) < 2e-3 and float(ref.abs().max()) < 2e-3, (tag, q)
        else:
            e, bound = _rel(got, ref), MARGIN * float(d["%s|noise|%s" % (tag, q)])
            key = q if not q.startswith("grad|") else "grad"
            if e / bound >= worst.get(key, (0.0, 0.0, 0.0, ""))[0]:
                worst[key] = (e / bound, e, bound, q[5:] if key == "grad" else "")
            assert e < bound, (what, tag, q, e, bound)
    print("%s %s: " % (what, tag) + ", ".join("%s %.2e (bound %.2e) %s" % (k_, v[1], v[2], v[3]) for k_, v in sorted(worst.items())))


@pytest.mark.parametrize("tag", list(dem.CASES))
def test_module_vs_golden_injected_graph(sp, d, tag):
    """Measured on the MI355X (rel-L2 against the float64 golden | bound = 10 x the reference's own float32 noise), worst quantity per kind:
      a  out 1.91e-7 | 1.81e-6   dx 2.51e-7 | 1.61e-6   parameter gradients 3.97e-7 | 1.99e-6
      b  out 1.91e-7 | 2.60e-6   dx 3.55e-7 | 2.16e-6   parameter gradients 4.26e-7 | 5.61e-6
      c  out 9.94e-8 | 1.35e-6   dx 1.17e-7 | 1.21e-6   parameter gradients 3.28e-7 | 1.32e-6
      d  out 9.04e-8 | 7.99e-7   dx 1.37e-7 | 1.30e-6   parameter gradients 2.26e-7 | 1.74e-6
      e  out 1.02e-7 | 1.17e-6   dx 2.00e-7 | 9.83e-7   parameter gradients 8.62e-8 | 4.36e-7
      rows_train  out 2.06e-7 | 1.88e-6   dx 1.85e-7 | 1.27e-6   parameter gradients 2.98e-7 | 1.93e-6
      rows_eval   out 1.91e-7 | 1.87e-6   dx 1.33e-7 | 1.15e-6   parameter gradients 3.09e-7 | 1.69e-6
      attn        out 1.17e-7 | 1.25e-6   dx 1.09e-7 | 8.87e-7   parameter gradients 3.40e-6 | 3.50e-6 (atten.gamma, Self_Attn's gate: one float32
                  sum over all B*C*N products; the closest of all)
    (the parameter-gradient column is the gradient closest to its own bound).  With the module's own graph no row differs from the
    reference's in any case, and the figures are the same."""
    x, g, idx = _golden_inputs(d, tag)
    m = _module(sp, d, tag)
    res = _run(m, tag, x, g, idx)
    _check_against_golden(d, tag, res, "injected")
    if idx is not None:
        B, N, k = idx.shape
        assert torch.equal(sp.ops.idx_to_local64(m.last_idx, B, N).view(B, N, k), idx)


@pytest.mark.parametrize("tag", list(dem.EDGE_CASES))
def test_module_own_graph(sp, d, tag):
    """On rows not flagged near-tie the neighbour sets equal the reference's exactly; if no row differs, the outputs meet the same bound."""
    x, g, idx = _golden_inputs(d, tag)
    m = _module(sp, d, tag)
    res = _run(m, tag, x, g)
    B, N, k = idx.shape
    own = sp.ops.idx_to_local64(m.last_idx, B, N).view(B * N, k)
    assert torch.equal(own[:, 0].cpu(), torch.arange(N).repeat(B)), "the point itself comes first"
    same = (torch.sort(own, dim=1)[0] == torch.sort(idx.view(B * N, k), dim=1)[0]).all(dim=1).cpu()
    near = torch.from_numpy(d[tag + "|near_tie_rows"])
    assert bool(same[~near].all()), "%d rows outside the near-tie set differ" % int((~same[~near]).sum())
    print("own graph %s: %d of %d rows differ (all near-tie)" % (tag, int((~same).sum()), B * N))
    if bool(same.all()):
        _check_against_golden(d, tag, res, "own graph")


@pytest.mark.parametrize("levels", [(2,), (1,), (0, 2)])
def test_negative_bn_weight_vs_model(sp, d, levels):
    """negative bn.weight entries at the last and at a middle level (case a: L = 3), against the float64 model on the same operands;
    the edge family's module bounds (3e-6 output and dx, 5e-6 parameter gradients).  Measured: out <= 1.96e-7, dx <= 2.74e-7, gradients <= 5.12e-7."""
    tag = "a"
    x, g, idx = _golden_inputs(d, tag)
    sd = dem.golden_state_dict(d, tag)
    for l in levels:
        sd["dense_modules.%d.1.weight" % l][1::3] *= -1.0
    res = _run(_module(sp, d, tag, sd), tag, x, g, idx)
    ref = dem.run(tag, x, g, sd, idx.cpu())
    errs = {}
    for q, r in ref.items():
        if q == "zs" or q.startswith("buf|"):
            continue
        if _zero_bias(q, tag):
            assert int(torch.count_nonzero(res[q])) == 0 and float(r.abs().max()) < 1e-9
            continue
        e = _rel(res[q], r)
        errs[q] = e
        assert e < (3e-6 if q in ("out", "dx") else 5e-6), (q, e)
    print("negative gamma at %s: out %.2e dx %.2e worst gradient %.2e" % (levels, errs["out"], errs["dx"], max(v for q, v in errs.items() if q.startswith("grad|"))))


def test_runs_repeat_bit_for_bit(sp, d):
    for tag in ("b", "rows_train"):
        x, g, idx = _golden_inputs(d, tag)
        r1 = _run(_module(sp, d, tag), tag, x, g, idx)
        r2 = _run(_module(sp, d, tag), tag, x, g, idx)
        for q in r1:
            assert torch.equal(r1[q], r2[q]), (tag, q)


def test_no_grad_paths(sp, d):
    for tag in ("a", "rows_train"):
        x, g, idx = _golden_inputs(d, tag)
        full = _run(_module(sp, d, tag), tag, x, g, idx)
        part = _run(_module(sp, d, tag), tag, x, g, idx, x_grad=False)            # requires_grad=False on x: the parameter gradients alone
        assert part["dx"] is None
        for q in full:
            if q != "dx":
                assert torch.equal(full[q], part[q]), (tag, q)
        m = _module(sp, d, tag)
        with torch.no_grad():
            out = m(x.cuda(), idx=idx) if idx is not None else m(x.cuda())
        assert not out.requires_grad and torch.equal(out, full["out"])
        for p in m.parameters():
            p.requires_grad_(False)
        out = m(x.cuda(), idx=idx) if idx is not None else m(x.cuda())            # nothing to differentiate: no node
        assert not out.requires_grad


def test_create_graph_raises(sp, d):
    for tag in ("d", "rows_train"):
        x, g, idx = _golden_inputs(d, tag)
        m = _module(sp, d, tag)
        xr = x.cuda().requires_grad_(True)
        out = m(xr, idx=idx) if idx is not None else m(xr)
        with pytest.raises(RuntimeError, match="once differentiable"):
            torch.autograd.grad(out.sum(), xr, create_graph=True)


def test_refusals(sp, d):
    x, g, idx = _golden_inputs(d, "a")
    m = _module(sp, d, "a")
    with pytest.raises(ValueError, match="input_channel"):
        m(torch.zeros(2, 4, 64, device="cuda"))
    with pytest.raises(RuntimeError, match="GPU|CPU"):
        m(x)
    with pytest.raises(RuntimeError, match="GPU|CPU"):
        m(x.cuda(), idx=idx.cpu())
    bad = idx.clone()
    bad[0, 0, 0] = 64
    with pytest.raises(IndexError):
        m(x.cuda(), idx=bad)
    with pytest.raises(ValueError):
        m(x.cuda(), idx=idx[:, :, :4].contiguous())
    with pytest.raises(ValueError):
        m(x.cuda(), idx=idx.to(torch.int32))
    for k in (1, 33):
        with pytest.raises(ValueError, match="2..32"):
            sp.DenseEdgeModule(6, 3, 16, k)
        with pytest.raises(ValueError, match="2..32"):
            sp.get_graph_feature(x.cuda(), k)
    with pytest.raises(RuntimeError, match="GPU|CPU"):
        sp.DenseModule1D(12, 3, 20)(torch.zeros(2, 12, 70))
    with pytest.raises(RuntimeError, match="GPU|CPU"):
        sp.Dense_Attn(16)(torch.zeros(2, 16, 48))
    # the layer's own int32 format is accepted
    B, N, k = idx.shape
    out = m(x.cuda(), idx=sp.ops.idx_from_local64(idx.reshape(B, N * k), B, N, k))
    assert torch.equal(out, m(x.cuda(), idx=idx.reshape(B, N * k)))


def test_get_graph_feature(sp, d):
    """equal to the reference's gathered tensor on its graph (differences of float32 numbers: exact), its gradient against the float64
    model (3e-6, the family's bound for dx), and the own graph against the golden's."""
    tag = "c"
    x, g, idx = _golden_inputs(d, tag)
    B, C, N = x.shape
    k = idx.shape[2]
    xr = x.cuda().requires_grad_(True)
    ee = sp.get_graph_feature(xr, k, idx=idx)
    assert tuple(ee.shape) == (B, 2 * C, N, k)
    assert torch.equal(ee.detach().cpu(), dem.graph_feature(x, idx.cpu(), k))
    cot = _rand("ggf.cot", (B, 2 * C, N, k))
    ee.backward(cot.cuda())
    x64 = x.double().requires_grad_(True)
    dem.graph_feature(x64, idx.cpu(), k).backward(cot.double())
    assert _rel(xr.grad, x64.grad) < 3e-6
    own = sp.get_graph_feature(x.cuda(), k)
    near = torch.from_numpy(d[tag + "|near_tie_rows"]).view(B, N)
    assert torch.equal(own.cpu()[:, C:], ee.detach().cpu()[:, C:])
    rows = ~near
    assert torch.equal(own.cpu().permute(0, 2, 1, 3)[rows], ee.detach().cpu().permute(0, 2, 1, 3)[rows])       # rank order included: ascending distance


def test_memory_contract(sp):
    """Peak memory of forward + backward above the level before the call stays below (2L + 3) E G 4 bytes + 32 MiB: the pre-norm buffer
    Z [E, LG], the gradient buffer D [E, LG], the [E,G] result of the max backward, one spare [E,G] and the per-point tensors.  The
    materialised formulation holds the edge tensor and the concatenations, (2C (L+1) + G L (L+1) / 2) E 4 bytes (here 960 E 4 bytes = 15 E G 4),
    plus every level's convolution, BatchNorm and LeakyReLU outputs (3L E G 4 more) and cannot meet it.  Measured: 100.0 MiB against the bound of 142.0 MiB (E G 4 bytes = 10.0 MiB)."""
    B, N, C, k, L, G = 2, 1024, 32, 20, 4, 64
    m = sp.DenseEdgeModule(2 * C, L, G, k).cuda().train()
    x = _rand("mem.x", (B, C, N)).cuda().requires_grad_(True)
    g = _rand("mem.g", (B, G, N)).cuda()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = m(x)
    (out * g).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    E = B * N * k
    bound = (2 * L + 3) * E * G * 4 + 32 * 2 ** 20
    print("peak %.1f MiB over forward+backward; E*G*4 = %.1f MiB; bound %.1f MiB" % (peak / 2 ** 20, E * G * 4 / 2 ** 20, bound / 2 ** 20))
    assert peak < bound, (peak, bound)
    assert torch.isfinite(x.grad).all() and torch.isfinite(out).all()
