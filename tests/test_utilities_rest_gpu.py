"""GPU: spgan.GC_attn, Self_Attn2, DenseModule2D, MultiDenseMLP, Dense_Attn_2D and the launchers of spgan.gc_attn (csrc/gc_attn.hip) against
the float64 model (tests/gc_attn_model.py) and the reference's golden results (tests/golden/utilities_rest.npz).

Bounds.  Launchers vs the float64 model on the same float32 operands: float32 arithmetic on sums of well-conditioned terms, rel-L2 2e-6
forward and 1e-5 backward, as the edge family's launcher tests carry.  The extreme-logit case: the larger of those and 10 x the distance
between a float32 CPU evaluation of the model's formulas and the float64 model on the same operands.  Modules vs the golden: rel-L2
against the reference's float64 run, bounded per case and quantity by 10 x the reference's OWN float32-vs-float64 distance stored in the
golden (`tag|noise|q`), the MARGIN of test_dense_edge_gpu.py with the same reasoning: the GPU sums in another order at the same
precision.  Gradients that are exactly zero here and rounding noise in the reference (gc_attn_model.zero_gradient) are asserted zero.
Buffers: rtol 1e-5 / atol 1e-6; num_batches_tracked exact.
Measured errors: printed next to each bound, and in DESIGN.md section 30."""
import os

import numpy as np
import pytest
import torch

import gc_attn_model as gm

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "utilities_rest.npz")
MARGIN = 10.0
FWD, BWD = 2e-6, 1e-5
MiB = 1 << 20


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
    return fr.normal("utilities_rest_gpu." + name, shape, std)


def _chunk(layout):
    from spgan import gc_attn
    return gc_attn.chunk_points("pm" if layout.startswith("pm") else "cm")


def _shapes(layout):
    c = _chunk(layout)
    # the last two: C beyond the 64- and the 32-position LDS tiles of the channel-major kernels (the two-walk kernels; three pieces per lane in rows)
    return [(1, 1, 1), (3, 16, 37), (2, 5, 257), (2, 130, c + 1), (1, 64, 2 * c + 3), (4, 128, c - 1), (1, 300, c + 5), (1, 520, c + 5)]


def _to_layout(t, layout):
    """[B,C,L] on the CPU -> the GPU operand of `layout`: "cm", "pm" (rows [B*L,C]) or "pm_pad" (rows with a stride of C + 3)"""
    if layout == "cm":
        return t.cuda().contiguous()
    B, C, L = t.shape
    rows = t.permute(0, 2, 1).reshape(B * L, C)
    if layout == "pm":
        return rows.cuda().contiguous()
    wide = torch.full((B * L, C + 3), float("nan"))
    wide[:, :C] = rows
    return wide.cuda()[:, :C]


def _from_layout(t, layout, B, L):
    return t.cpu() if layout == "cm" else t.cpu().reshape(B, L, -1).permute(0, 2, 1)


def _branch(tag, C, O):
    from spgan import fixture_rng as fr
    n = "utilities_rest_gpu.%s" % tag
    return (fr.uniform(n + ".W1", (O, C), -1, 1) / np.sqrt(C), fr.uniform(n + ".b1", (O,), -0.5, 0.5), fr.uniform(n + ".lnw", (O,), 0.5, 1.5),
            fr.uniform(n + ".lnb", (O,), -0.2, 0.2), fr.uniform(n + ".W2", (C, O), -1, 1) / np.sqrt(O), fr.uniform(n + ".b2", (C,), -0.5, 0.5))


def _cuda(p):
    return None if p is None else tuple(t.cuda() for t in p)


# ---------------------------------------------------------------- every launcher against the model, both layouts
@pytest.mark.parametrize("pool", ["att", "avg"])
@pytest.mark.parametrize("case", range(8))
@pytest.mark.parametrize("layout", ["cm", "pm", "pm_pad"])
def test_launchers(sp, layout, case, pool):
    """Every forward and backward quantity of every launcher, with mul only, add only and both.  Measured on the MI355X: see DESIGN 30."""
    from spgan import gc_attn
    B, C, L = _shapes(layout)[case]
    lay = "cm" if layout == "cm" else "pm"
    O = max(1, C // 2 + 1)
    tag = "launch.%d.%d.%d" % (B, C, L)
    x, g = _rand(tag + ".x", (B, C, L)), _rand(tag + ".g", (B, C, L))
    w = _rand(tag + ".w", (C,), 1.0 / np.sqrt(C)) if pool == "att" else None
    bias = _rand(tag + ".bias", (1,)) if pool == "att" else None
    xg, gg = _to_layout(x, layout), _to_layout(g, layout)
    wg, bg = (None if w is None else w.cuda()), (None if bias is None else bias.cuda())
    worst = {"fwd": 0.0, "bwd": 0.0}

    def chk(kind, name, got, ref):
        assert torch.isfinite(got).all(), name
        if float(ref.double().norm()) < 1e-12:                      # a quantity that is zero in exact arithmetic (L = 1, or C = O = 1)
            assert float(got.abs().max()) < 1e-6, name
            return
        e = _rel(got, ref)
        worst[kind] = max(worst[kind], e)
        assert e < (FWD if kind == "fwd" else BWD), "%s %s: rel-L2 %.2e" % (tag, name, e)

    # the pooling
    ctx, lse, stat, m = gc_attn.pool_fwd(xg, lay, B, L, wg, bg)
    pm_ = gm.pool_model(x.double(), None if w is None else w.double(), None if bias is None else bias.double())
    chk("fwd", "ctx", ctx, pm_["ctx"])
    assert float((lse.double().cpu() - pm_["lse"]).abs().max()) < FWD * max(1.0, float(pm_["lse"].abs().max()))
    if pool == "att":
        chk("fwd", "m", m, pm_["m"])
        chk("fwd", "p", torch.exp(m - stat[:, :1]) / stat[:, 1:], pm_["p"])
    else:
        assert m is None
    for fus in (("mul",), ("add",), ("add", "mul")):
        add_p = _branch(tag + ".add", C, O) if "add" in fus else None
        mul_p = _branch(tag + ".mul", C, O) if "mul" in fus else None
        # the branches on the model's ctx (float32), so that each launcher is checked on operands it shares with the model
        ctx32 = pm_["ctx"].float()
        add, mul, hid, lnstat = gc_attn.channel_fwd(ctx32.cuda(), _cuda(add_p), _cuda(mul_p))
        cm_ = gm.channel_model(ctx32, add_p, mul_p)
        for nm, got in (("add", add), ("mul", mul)):
            assert (got is None) == (cm_[nm] is None)
            if got is not None:
                chk("fwd", nm, got, cm_[nm])
        wide = torch.full((B * L, C + 3), float("nan"), device="cuda") if layout == "pm_pad" else None
        out = gc_attn.apply_fwd(xg, lay, B, L, mul, add, out=None if wide is None else wide[:, :C])
        chk("fwd", "out", _from_layout(out.contiguous(), layout, B, L), gm.apply_model(x, mul, add))
        assert wide is None or torch.isnan(wide[:, C:]).all()               # nothing beyond the C columns of a row was written
        # backward
        dmul, dadd = gc_attn.bwd_reduce(xg, gg, lay, B, L, want_mul="mul" in fus, want_add="add" in fus)
        rm, ra = gm.bwd_reduce_model(x, g)
        if dmul is not None:
            chk("bwd", "dmul", dmul, rm)
        if dadd is not None:
            chk("bwd", "dadd", dadd, ra)
        G, dctx = gc_attn.channel_bwd(None if dadd is None else ra.float().cuda(), None if dmul is None else rm.float().cuda(), mul, hid, lnstat,
                                      _cuda(add_p), _cuda(mul_p))
        bm_ = gm.channel_model(ctx32, add_p, mul_p, ra.float(), rm.float())
        chk("bwd", "dctx", dctx, bm_["dctx"])
        sl = gc_attn.channel_slices(C, O, add_p, mul_p)[0]
        G64 = G.double().cpu()
        for nm in sl:
            col = {k: G64[:, lo:hi] for k, (lo, hi) in sl[nm].items()}
            mine = [col["dh"].t() @ ctx32.double(), col["dh"].sum(0), col["dlnw"].sum(0), col["dlnb"].sum(0), col["dt"].t() @ col["r"], col["dt"].sum(0)]
            for k, (a, b_) in enumerate(zip(mine, bm_["grads"][nm])):
                chk("bwd", "%s grad %d" % (nm, k), a, b_.reshape(a.shape))
        dctx32 = bm_["dctx"].float()
        dx, dwpart = gc_attn.bwd_apply(xg, gg, lay, B, L, mul, dctx32.cuda(), ctx, wg, m, stat)
        rdx, rdw = gm.bwd_apply_model(x, g, mul, dctx32, w, bias)
        chk("bwd", "dx", _from_layout(dx, layout, B, L), rdx)
        if pool == "att":
            chk("bwd", "dw", dwpart.double().sum(0), rdw)
        else:
            assert dwpart is None
    print("%s %s %s: worst rel-L2 forward %.2e (bound %.0e), backward %.2e (bound %.0e)" % (tag, layout, pool, worst["fwd"], FWD, worst["bwd"], BWD))


# ---------------------------------------------------------------- extreme logits
@pytest.mark.parametrize("layout", ["cm", "pm"])
def test_extreme_logits(sp, layout):
    """x on a grid of 1/4, conv_mask.weight on a grid of 1/2 and an integer bias: every logit is exact in float32.  Sample 0 holds a
    logit of +96 (one-hot: the next one is tens below), sample 1 one of -100; the rest spread over tens.  Everything must be finite, and
    within the larger of the launcher bounds and 10 x the float32 CPU evaluation's own distance from the float64 model."""
    from spgan import gc_attn
    lay = "cm" if layout == "cm" else "pm"
    B, C, L = 3, 16, 2 * _chunk(layout) + 5
    rng = np.random.default_rng(96)
    x = torch.from_numpy((np.clip(np.round(rng.standard_normal((B, C, L)) * 4), -8, 8) / 4).astype(np.float32))
    sign = rng.choice([-1.0, 1.0], size=C)
    w = torch.from_numpy((sign * np.array([3.0] * 14 + [3.5] * 2)).astype(np.float32))
    bias = torch.tensor([-2.0])
    x[0, :, L - 3] = torch.from_numpy(2 * sign).float()                 # logit 2 * 49 - 2 = +96
    x[1, :, 1] = torch.from_numpy(-2 * sign).float()                    # logit -100
    pm64 = gm.pool_model(x.double(), w.double(), bias.double())
    assert float(pm64["m"].max()) == 96.0 and float(pm64["m"].min()) == -100.0 and float(pm64["p"][0].max()) > 1 - 1e-12
    assert torch.equal(gm.pool_model(x, w, bias)["m"].double(), pm64["m"])                    # exact in float32
    g, mul, dctx = _rand("extreme.g", (B, C, L)), _rand("extreme.mul", (B, C)), _rand("extreme.dctx", (B, C))
    xg, gg = _to_layout(x, layout), _to_layout(g, layout)
    ctx, lse, stat, m = gc_attn.pool_fwd(xg, lay, B, L, w.cuda(), bias.cuda())
    dx, dwpart = gc_attn.bwd_apply(xg, gg, lay, B, L, mul.cuda(), dctx.cuda(), ctx, w.cuda(), m, stat)
    pm32 = gm.pool_model(x, w, bias)
    dx64, dw64 = gm.bwd_apply_model(x, g, mul, dctx, w, bias)
    dx32, dw32 = gm.bwd_apply_model(x, g, mul, dctx, w, bias, dtype=torch.float32)
    assert torch.equal(m.cpu().double(), pm64["m"])
    for name, got, r64, r32, base in (("ctx", ctx, pm64["ctx"], pm32["ctx"], FWD), ("lse", lse, pm64["lse"], pm32["lse"], FWD),
                                      ("dx", _from_layout(dx, layout, B, L), dx64, dx32, BWD), ("dw", dwpart.double().sum(0), dw64, dw32, BWD)):
        assert torch.isfinite(got).all(), name
        bound = max(base, 10.0 * _rel(r32, r64))
        e = _rel(got, r64)
        print("extreme %s %s: rel-L2 %.2e (bound %.2e; the float32 CPU evaluation: %.2e)" % (layout, name, e, bound, _rel(r32, r64)))
        assert e < bound, name


# ---------------------------------------------------------------- the module against the golden
def _module(sp, d, tag):
    m = gm.build_module(sp, tag)
    m.load_state_dict(gm.golden_state_dict(d, tag), strict=True)
    return m.cuda()


def _case(d, tag):
    xs = [torch.from_numpy(d["%s|%s" % (tag, n)]).cuda() for n in gm.input_names(tag)]
    return (xs if len(xs) > 1 else xs[0]), torch.from_numpy(d["%s|g" % tag]).cuda()


def _run(m, x, g, pm=False):
    for p in m.parameters():
        p.grad = None
    many = isinstance(x, list)
    xs = [t.detach().clone().requires_grad_(True) for t in (x if many else [x])]
    if pm:
        B, C = xs[0].shape[:2]
        L = xs[0].numel() // (B * C)
        rows = xs[0].reshape(B, C, L).permute(0, 2, 1).reshape(B * L, C)
        out = m.forward_pm(rows, B, L)
        out = out.reshape(B, L, out.shape[1]).permute(0, 2, 1).reshape(g.shape)
    else:
        out = m(xs if many else xs[0])
    out.backward(g)
    res = {"out": out.detach()}
    for i, t in enumerate(xs):
        res["dx%s" % (i or "")] = t.grad
    for n, p in m.named_parameters():
        res["grad|" + n] = p.grad
    for n, b_ in m.named_buffers():
        res["buf|" + n] = b_.detach().clone()
    return res


def _pm_cases():
    return [(t, pm) for t in gm.CASES for pm in ((False, True) if gm.kind_of(t) in ("gc", "sa2", "d2") else (False,))]


@pytest.mark.parametrize("tag,pm", _pm_cases())
def test_module_golden(sp, d, tag, pm):
    """forward(x) in the public layout and (GC_attn, Self_Attn2, DenseModule2D) forward_pm on point-major rows against the reference's
    float64 run"""
    x, g = _case(d, tag)
    m = _module(sp, d, tag)
    m.train(gm.CASES[tag]["train"])
    res = _run(m, x, g, pm)
    assert sorted(res) == sorted(gm.quantities(d, tag))
    for q in gm.quantities(d, tag):
        if gm.zero_gradient(tag, q) == "exact":
            assert float(res[q].abs().max()) == 0.0, q
            continue
        if q.endswith("num_batches_tracked"):
            assert int(res[q]) == int(d["%s|%s|full" % (tag, q)]), q
            continue
        if q.startswith("buf|"):
            assert torch.allclose(res[q].double().cpu(), gm.golden_f64(d, tag, q), rtol=1e-5, atol=1e-6), q
            continue
        bound = MARGIN * float(d["%s|noise|%s" % (tag, q)])
        e = _rel(res[q], gm.golden_f64(d, tag, q))
        print("%s pm=%d %s: rel-L2 %.2e (bound %.2e)" % (tag, pm, q, e, bound))
        assert e < bound, (tag, q, e, bound)


# ---------------------------------------------------------------- slope 0
def test_multi_dense_relu_edges(sp):
    """MultiDenseMLP (ReLU: the masks take the sign from the activated value, which is 0 on the whole negative side) with, at every
    level, a column whose pre-activations are all negative (bn.bias = -100), one that holds exact zeros (bn.weight = bn.bias = 0: the
    ReLU's derivative there is 0, as torch's) and one with a negative bn.weight, against the float64 model."""
    from spgan import fixture_rng as fr
    mlps, mlps2, shape = [4, 5], [5, 2], (2, 5, 6, 4)
    m = sp.MultiDenseMLP(mlps, mlps2)
    sd = {}
    for n, v in m.state_dict().items():
        sd[n] = fr.uniform("relu_edges." + n, tuple(v.shape), -0.5, 0.5) if v.dtype.is_floating_point and "running" not in n else v.clone()
    for l in range(2):
        w, b_ = sd["dense_modules.%d.1.weight" % l], sd["dense_modules.%d.1.bias" % l]
        w += 1.0
        w[0], b_[0] = 0.1, -100.0
        w[1], b_[1] = 0.0, 0.0
        w[2] = -1.3
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    xs = [fr.normal("relu_edges.x%d" % i, (shape[0], c) + shape[2:]) for i, c in enumerate(mlps2)]
    g = fr.normal("relu_edges.g", (shape[0], mlps[-1]) + shape[2:])
    gm.CASES["relu_edges"] = dict(kind="mdm", shape=shape, mlps=mlps, mlps2=mlps2, train=True, warm=False)
    try:
        ref = gm.run("relu_edges", xs, g, sd)
    finally:
        del gm.CASES["relu_edges"]
    assert all(float(t[..., 0].max()) < 0.0 and float(t[..., 1].abs().max()) == 0.0 for t in ref["pre"])
    res = _run(m, [t.cuda() for t in xs], g.cuda())
    assert float(res["out"][:, :2].abs().max()) == 0.0
    for q in ref:
        if q == "pre" or q.startswith("buf|"):
            continue
        if q.endswith(".0.bias"):
            assert float(res[q].abs().max()) == 0.0, q
            continue
        r = ref[q]
        if float(r.norm()) == 0.0:
            assert float(res[q].abs().max()) == 0.0, q
            continue
        e = _rel(res[q], r)
        print("relu edges %s: rel-L2 %.2e (bound %.0e)" % (q, e, FWD if q == "out" else BWD))
        assert e < (FWD if q == "out" else BWD), q


# ---------------------------------------------------------------- determinism, capture, no-grad, refusals
@pytest.mark.parametrize("tag", ["gc_4d", "sa2_train", "mdm", "da_gc", "da_sa"])
def test_deterministic(sp, d, tag):
    x, g = _case(d, tag)
    m = _module(sp, d, tag)
    for pm in ((False, True) if tag == "gc_4d" else (False,)):
        a, b_ = _run(m, x, g, pm), _run(m, x, g, pm)
        for q in a:
            if not q.startswith("buf|"):                                # the running statistics move with every training step
                assert torch.equal(a[q], b_[q]), (pm, q)


def test_capture(sp, d):
    """One forward + backward inside spgan.CapturedBody, replayed twice, equals the eager result bit for bit."""
    x, cot = _case(d, "gc_att")

    def make():
        m = _module(sp, d, "gc_att")

        def body(x_, cot_):
            for p in m.parameters():
                p.grad = None
            xg = x_.detach().requires_grad_(True)
            out = m(xg)
            (out * cot_).sum().backward()
            return (out.detach(), xg.grad) + tuple(p.grad for p in m.parameters())
        return m, body
    m_e, body_e = make()
    eager = [t.clone() for t in body_e(x, cot)]
    m_c, body_c = make()
    cap = sp.CapturedBody(body_c, modules=(m_c,), warmup=1)
    for call in range(4):                                # one eager warm-up, the capture, two replays
        res = cap(x, cot)
        assert not cap.eager
        for a, b_ in zip(eager, res):
            assert torch.equal(a, b_), call


def test_no_grad_eval_and_refusals(sp, d):
    x, g = _case(d, "gc_att")
    m = _module(sp, d, "gc_att")
    ref = _run(m, x, g)["out"]
    with torch.no_grad():
        out = m(x)
    assert not out.requires_grad and torch.equal(out, ref)
    assert torch.equal(m.eval()(x), ref)                                   # no layer of GC_attn depends on the mode
    empty = sp.GC_attn(16, fusions=[]).cuda()
    assert empty(x) is x
    xr = x.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(m.train()(xr).sum(), xr, create_graph=True)
    with pytest.raises(RuntimeError, match="GPU"):
        m(x.cpu())
    with pytest.raises(TypeError):
        m(x.double())
    with pytest.raises(ValueError):
        m(x[:, :8])
    with pytest.raises(ValueError):
        m(x[:, :, 0])
    with pytest.raises(ValueError):
        m.forward_pm(x, 3, 37)
    from spgan import gc_attn
    with pytest.raises(ValueError, match="C=1025"):
        gc_attn.pool_fwd(torch.zeros((1, 1025, 4), device="cuda"), "cm", 1, 4)
    with pytest.raises(ValueError, match="layout"):
        gc_attn.pool_fwd(torch.zeros((1, 8, 4), device="cuda"), "rows", 1, 4)


def test_gc_attn_partial_gradients(sp, d):
    """frozen parameters, or an input without a gradient: what is still asked for equals the full backward bit for bit"""
    x, g = _case(d, "gc_att")
    m = _module(sp, d, "gc_att")
    full = _run(m, x, g)
    for p in m.parameters():
        p.requires_grad_(False)
        p.grad = None
    xr = x.clone().requires_grad_(True)
    m(xr).backward(g)
    assert torch.equal(xr.grad, full["dx"]) and all(p.grad is None for p in m.parameters())
    for p in m.parameters():
        p.requires_grad_(True)
        p.grad = None
    m.channel_mul_conv[0].weight.requires_grad_(False)
    m(x).backward(g)
    for n, p in m.named_parameters():
        assert (p.grad is None) if n == "channel_mul_conv.0.weight" else torch.equal(p.grad, full["grad|" + n]), n
    for t in (x.double(), x.half()):
        for mod in (sp.Self_Attn2(16).cuda(), sp.DenseModule2D(16, mlps=[16, 8]).cuda(), sp.Dense_Attn_2D(16, mlps=[16, 16]).cuda()):
            with pytest.raises(TypeError):
                mod(t if mod.__class__.__name__ == "Self_Attn2" else t.reshape(3, 16, 37, 1))
    with pytest.raises(ValueError):
        sp.Self_Attn2(16).cuda().forward_pm(x, 3, 37)


@pytest.mark.parametrize("tag", ["sa2_train", "sa2_eval", "d2_eval", "mdm", "da_gc"])
def test_others_no_grad_and_refusals(sp, d, tag):
    x, g = _case(d, tag)
    m = _module(sp, d, tag)
    m.train(gm.CASES[tag]["train"])
    ref = _run(m, x, g)["out"]
    with torch.no_grad():
        out = m(x)
    assert not out.requires_grad and torch.equal(out, ref)
    xs = [t.clone().requires_grad_(True) for t in (x if isinstance(x, list) else [x])]
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(m(xs if isinstance(x, list) else xs[0]).sum(), xs[0], create_graph=True)
    bad = [t[:, :-1] for t in xs] if isinstance(x, list) else xs[0][:, :-1]
    with pytest.raises(ValueError):
        m(bad)


# ---------------------------------------------------------------- memory
def test_memory_contract(sp):
    """GC_attn(128) at [8,128,8192]: over the live x and cotangent, forward + backward peak at <= 2|x| + 8 MiB -- out and dx; the torch
    formulation keeps x * mul as well."""
    torch.manual_seed(0)
    m = sp.GC_attn(128).cuda()
    x = torch.randn((8, 128, 8192), device="cuda").requires_grad_(True)
    g = torch.randn((8, 128, 8192), device="cuda")
    size = x.numel() * 4
    m(x).backward(g)                                                         # warm: the library's own one-off allocations
    x.grad = None
    for p in m.parameters():
        p.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = m(x)
    out.backward(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("GC_attn(128) [8,128,8192]: peak growth %.1f MiB = %.3f |x| (bound 2|x| + 8 MiB = %.1f MiB)" % (peak / MiB, peak / size, (2 * size + 8 * MiB) / MiB))
    assert peak <= 2 * size + 8 * MiB


def test_dense_attn_2d_has_no_map(sp):
    """Dense_Attn_2D(16, mlps=[16,16], atten='sa') at [1,16,512,8], L = 4096: forward + backward grow the allocation by < 32 MiB, where one
    [L,L] attention map alone would be 64 MiB."""
    torch.manual_seed(0)
    m = sp.Dense_Attn_2D(16, mlps=[16, 16], atten="sa").cuda()
    with torch.no_grad():
        m.atten.gamma.fill_(0.5)
    x = torch.randn((1, 16, 512, 8), device="cuda").requires_grad_(True)
    g = torch.randn((1, 16, 512, 8), device="cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = m(x)
    out.backward(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("Dense_Attn_2D(sa) L=4096: peak growth %.1f MiB (bound 32 MiB; one [L,L] map: 64 MiB)" % (peak / MiB))
    assert torch.isfinite(out).all() and torch.isfinite(x.grad).all()
    assert peak < 32 * MiB
