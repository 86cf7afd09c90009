"""GPU: dot-product point attention without a [B,N,N] map (csrc/point_attn.hip behind spgan.point_attn): its launchers against the float64
model of tests/point_attn_model.py, and spgan.Self_Attn / spgan.Attention(materialize=False) against the vectors captured from the
reference (golden point_attn.npz).

Tolerances.  Launchers vs the float64 model on the same float32 operands: rel-L2 3e-6 for O and lse, 5e-6 for dQ, dK, dV -- or 5 x the
rel-L2 distance between a float32 and a float64 CPU evaluation of the model on those operands where that is larger (the yardstick is
the model, never the kernel).  Modules vs golden (the reference's float64 run): 3e-6 for out and dx, 5e-6 for parameter gradients, or
5 x the golden's stored distance of the reference's float32 run from its float64 run where that is larger (the bound of
tests/test_point_transformer_gpu.py::test_module_golden).  The generator lists the quantities that need the fallback: c grad|gamma
(stored 3.0e-06), d dx (3.5e-06), grad|theta.weight (9.1e-05), grad|phi.weight (9.3e-06), e grad|gamma (1.6e-06).
Exact zeros are asserted as exact zeros: b (one point) d theta = d phi = 0, g (theta = 0) d phi = 0, here as in the reference.
query.bias of Self_Attn adds the same number to every score of one softmax column and cancels: its gradient is an exact zero here and
rounding noise in the reference (float64 below 1e-12, float32 stored as `tag|qbias_f32`, asserted below 1e-5); key.bias does not cancel.
Measured on an MI355X: launchers 1.5e-07 .. 1.1e-06 at the regular shapes; case d's operands dQ 5.2e-05 (bound 5.5e-04), dK 1.7e-05 (4.0e-05),
dV 3.5e-06 (1.4e-05); modules at most 1.0e-06 except case d (dx 1.8e-06, grad|theta.weight 1.7e-04 against 4.5e-04, grad|phi.weight
3.0e-06, grad|g.weight 2.4e-06); the materialised route lands in the same places (d: grad|theta.weight 1.1e-04).
The backward launchers read the forward launcher's own lse: P = exp(S - lse) is recomputed from the same bits of S, so the rounding of S
cancels (the modules work the same way).
Memory: Attention(64, materialize=False) at B 2, N 4096, forward + backward, peaks less than 64 MiB above the state before the call; one
[2,4096,4096] float32 map is 128 MiB."""
import numpy as np
import pytest
import torch

import point_attn_model as pm
from helpers import golden, rel_l2

pytestmark = pytest.mark.gpu
TAGS = list(pm.CASES)


@pytest.fixture(scope="module")
def sp():
    import spgan
    from spgan import _lib
    _lib.load()
    return spgan


@pytest.fixture(scope="module")
def d():
    return golden("point_attn.npz")


def _module(sp, d, tag, materialize=False):
    c = pm.CASES[tag]
    m = sp.Attention(c["ch"], materialize=materialize) if c["module"] == "Attention" else sp.Self_Attn(c["ch"])
    m.load_state_dict(pm.golden_state_dict(d, tag), strict=True)
    return m.cuda()


def _case(d, tag):
    x, cot, _ = pm.golden_inputs(d, tag)
    return x.cuda(), cot.cuda()


def _all(m, x, cot):
    """[out, dx, parameter gradients in named_parameters order]"""
    for p in m.parameters():
        p.grad = None
    xg = x.detach().clone().requires_grad_(True)
    out = m(xg)
    (out * cot).sum().backward()
    return [out.detach(), xg.grad] + [p.grad.clone() for p in m.parameters()]


def _check_golden(d, tag, m, res, what):
    names = ["out", "dx"] + ["grad|" + n for n, _ in m.named_parameters()]
    assert tuple(names) == pm.quantities(tag)
    e = {}
    for q, v in zip(names, res):
        if q == "grad|query.bias":
            assert float(v.abs().max()) == 0.0 and float(d[tag + "|qbias_f32"]) <= 1e-5
        elif q in pm.EXACT_ZERO.get(tag, ()):
            assert not np.any(pm.stored(d, tag, q)) and float(v.abs().max()) == 0.0, (tag, q)
        else:
            e[q] = (pm.golden_rel(d, tag, q, v), max(3e-6 if q in ("out", "dx") else 5e-6, 5.0 * pm.noise(d, tag, q)))
    print("%s %s: rel-L2 vs reference float64 (bound) %s" % (tag, what, {k: "%.2e (%.1e)" % v for k, v in e.items()}))
    for q, (err, bound) in e.items():
        assert err <= bound, (tag, what, q, err, bound)


# ---------------------------------------------------------------- launchers against the float64 model
def _operands(d, name):
    """float32 (q, k, v, dO) [b,n,.] built once on the CPU"""
    if name == "case_d":
        x, cot, sd = pm.golden_inputs(d, "d")
        xp = x.transpose(1, 2)
        q, k, v = (xp @ sd[n].squeeze(-1).t() for n in ("theta.weight", "phi.weight", "g.weight"))
        return q.contiguous(), k.contiguous(), v.contiguous(), torch.randn(v.shape, generator=torch.Generator().manual_seed(1))
    if name == "huge":
        b, n, dk, dv, scale = 1, 70, 8, 16, 40.0
    else:
        (b, n, dk, dv), scale = name, None
    g = torch.Generator().manual_seed(100 * n + dk)
    q, k = torch.randn(b, n, dk, generator=g), torch.randn(b, n, dk, generator=g)
    s = scale if scale is not None else 1.5 / dk ** 0.25                      # scores of standard deviation about 2
    return q * s, k * s, torch.randn(b, n, dv, generator=g), torch.randn(b, n, dv, generator=g)


SHAPES = [(1, 1, 4, 4), (3, 31, 4, 12), (1, 33, 8, 32), (2, 65, 16, 128), (1, 257, 80, 320), (1, 100, 128, 512), "case_d", "huge"]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_launchers_against_model(sp, d, shape):
    from spgan import point_attn
    q, k, v, dO = _operands(d, shape)
    b, n, dk = q.shape
    dv = v.shape[2]
    if shape == "huge":
        S = q.double() @ k.double().transpose(1, 2)
        assert float((S.max(-1).values - S.min(-1).values).min()) > 1e4

    def model(dtype):
        a = [t.to(dtype) for t in (q, k, v, dO)]
        O, lse, _ = pm.core_forward(*a[:3])
        dQ, dK, dV = pm.core_backward(*a)
        return dict(O=O, lse=lse, dQ=dQ, dK=dK, dV=dV)
    m64, m32 = model(torch.float64), model(torch.float32)
    g2 = lambda t: t.reshape(b * n, -1).contiguous().cuda()
    gq, gk, gv, gdO = g2(q), g2(k), g2(v), g2(dO)
    O, lse = point_attn.point_attn_fwd(gq, gk, gv, b, n)
    # the backward reads the forward's own statistic, as in the modules: P = exp(S - lse) is recomputed from the same bits of S, so the
    # rounding of S (one ulp of 1e4 is 1e-3 in the last shape) cancels; an lse rounded independently would not share it
    dQ, dK, dV = point_attn.point_attn_bwd(gq, gk, gv, gdO, lse, b, n)
    got = dict(O=O.view(b, n, dv), lse=lse.view(b, n), dQ=dQ.view(b, n, dk), dK=dK.view(b, n, dk), dV=dV.view(b, n, dv))
    e = {}
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), name
        e[name] = (pm.rel(t.cpu(), m64[name]), max(3e-6 if name in ("O", "lse") else 5e-6, 5.0 * pm.rel(m32[name], m64[name])))
    print("%s: launcher rel-L2 vs float64 model (bound) %s" % (shape, {k_: "%.2e (%.1e)" % v_ for k_, v_ in e.items()}))
    for name, (err, bound) in e.items():
        assert err <= bound, (shape, name, err, bound)


def test_launchers_on_column_slices(sp):
    """q, k, v as slices of one projected tensor and the three gradients into slices of one buffer give the bits of contiguous operands."""
    from spgan import point_attn
    b, n, dk, dv = 2, 45, 8, 20
    g = torch.Generator().manual_seed(3)
    cat = torch.randn(b * n, 2 * dk + dv, generator=g).cuda()
    dO = torch.randn(b * n, dv, generator=g).cuda()
    sl = (cat[:, :dk], cat[:, dk:2 * dk], cat[:, 2 * dk:])
    O1, lse1 = point_attn.point_attn_fwd(*sl, b, n)
    O2, lse2 = point_attn.point_attn_fwd(*[t.contiguous() for t in sl], b, n)
    assert torch.equal(O1, O2) and torch.equal(lse1, lse2)
    dcat = torch.full_like(cat, float("nan"))
    point_attn.point_attn_bwd(*sl, dO, lse1, b, n, dq=dcat[:, :dk], dk_out=dcat[:, dk:2 * dk], dv_out=dcat[:, 2 * dk:])
    ref = point_attn.point_attn_bwd(*[t.contiguous() for t in sl], dO, lse1, b, n)
    assert torch.equal(dcat, torch.cat(ref, 1))


# ---------------------------------------------------------------- modules against the reference (golden)
@pytest.mark.parametrize("tag", TAGS)
def test_module_golden(sp, d, tag):
    m = _module(sp, d, tag)
    x, cot = _case(d, tag)
    res = _all(m, x, cot)
    assert tuple(res[0].shape) == tuple(x.shape)
    _check_golden(d, tag, m, res, "fused")


@pytest.mark.parametrize("tag", ["a", "c", "d"])
def test_both_routes_of_attention(sp, d, tag):
    """materialize=True and False each satisfy the golden's bounds; the attribute switches the route of one module."""
    m = _module(sp, d, tag, materialize=True)
    x, cot = _case(d, tag)
    res_t = _all(m, x, cot)
    _check_golden(d, tag, m, res_t, "materialised")
    m.materialize = False
    res_f = _all(m, x, cot)
    _check_golden(d, tag, m, res_f, "fused (attribute)")
    ref_f = _all(_module(sp, d, tag, materialize=False), x, cot)
    for a, b_ in zip(res_f, ref_f):
        assert torch.equal(a, b_)


def test_point_attention_function(sp, d):
    """spgan.point_attn.point_attention: unpadded widths (dk 3, dv 6) against the float64 model's autograd; refusals."""
    from spgan import point_attn
    g = torch.Generator().manual_seed(9)
    q, k, v, dO = (torch.randn(2, 37, w, generator=g) for w in (3, 3, 6, 6))
    leaves = [t.cuda().requires_grad_(True) for t in (q, k, v)]
    out = point_attn.point_attention(*leaves)
    (out * dO.cuda()).sum().backward()

    def model(dtype):
        a = [t.to(dtype) for t in (q, k, v, dO)]
        return (pm.core_forward(*a[:3])[0],) + tuple(pm.core_backward(*a))
    m64, m32 = model(torch.float64), model(torch.float32)
    for nm, t, r64, r32 in zip(("O", "dQ", "dK", "dV"), [out.detach()] + [t.grad for t in leaves], m64, m32):
        assert pm.rel(t.cpu(), r64) <= max(3e-6 if nm == "O" else 5e-6, 5.0 * pm.rel(r32, r64)), nm
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(point_attn.point_attention(*leaves).sum(), leaves[0], create_graph=True)
    with pytest.raises(TypeError, match="float32"):
        point_attn.point_attention(*[t.detach().double() for t in leaves])
    with pytest.raises(ValueError):
        point_attn.point_attention(torch.zeros(1, 4, 132).cuda(), torch.zeros(1, 4, 132).cuda(), torch.zeros(1, 4, 8).cuda())
    big = sp.Attention(1032).cuda()
    big.materialize = False
    with pytest.raises(ValueError, match="ch=1032"):
        big(torch.zeros(1, 1032, 4).cuda())


# ---------------------------------------------------------------- properties of the modules
@pytest.mark.parametrize("tag", ["a", "e"])
def test_fresh_module_is_identity(sp, d, tag):
    """gamma = 0 (a freshly built module): out equals x bit for bit, gamma.grad is non-zero, dx == dy bit for bit and every other parameter
    gradient is an exact zero."""
    m = _module(sp, d, tag)
    with torch.no_grad():
        m.gamma.zero_()
    x, cot = _case(d, tag)
    res = _all(m, x, cot)
    assert torch.equal(res[0], x) and torch.equal(res[1], cot)
    for (n, p), g in zip(m.named_parameters(), res[2:]):
        if n == "gamma":
            assert float(g.abs().max()) > 0.0
        else:
            assert float(g.abs().max()) == 0.0, n


@pytest.mark.parametrize("tag", ["c", "e"])
def test_repeatable(sp, d, tag):
    x, cot = _case(d, tag)
    res = [_all(_module(sp, d, tag), x, cot) for _ in range(2)]
    for a, b_ in zip(*res):
        assert torch.equal(a, b_), tag


def test_peak_memory_without_a_map(sp):
    """Attention(64, materialize=False) at B 2, N 4096: forward + backward peak, minus what was live before, below 64 MiB (one [2,4096,4096]
    float32 map is 128 MiB; x, the projections, o, oo, outputs and gradients at ch 64 total under 25 MiB)."""
    B, N, ch = 2, 4096, 64
    g = torch.Generator().manual_seed(0)
    m = sp.Attention(ch, materialize=False).cuda()
    with torch.no_grad():
        m.gamma.fill_(0.5)
    x = torch.randn(B, ch, N, generator=g).cuda().requires_grad_(True)
    cot = torch.randn(B, ch, N, generator=g).cuda()
    (m(x) * cot).sum().backward()                        # first call: library load, cached transposes
    x.grad = None
    for p in m.parameters():
        p.grad = None
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    (m(x) * cot).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("peak %.1f MiB over the %.1f MiB live before (one [B,N,N] map: %.0f MiB)" % (peak / 2**20, base / 2**20, B * N * N * 4 / 2**20))
    assert peak < 64 * 2**20
    assert bool(torch.isfinite(x.grad).all())


@pytest.mark.parametrize("tag", ["a", "e"])
def test_capture(sp, d, tag):
    """One forward + backward inside spgan.CapturedBody, replayed twice, equals the eager result bit for bit."""
    x, cot = _case(d, tag)

    def make():
        m = _module(sp, d, tag)

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


# ---------------------------------------------------------------- inside the generator
class _Opts:
    np = 256; nk = 20; nz = 128; softmax = True; off = False; attn = True
    use_head = False; eql = False; z_norm = False; small_d = False


ZERO_GRAD_BIASES = ("conv_w.0.bias", "conv_w.3.bias", "conv_x.0.bias", "global_conv.0.bias", "global_conv.3.bias")


def test_generator_with_fused_attention(sp):
    """A small --attn generator (np 256) with G.attn.materialize = False against the same generator on the default route: output and
    every parameter gradient at the rtol of tests/test_parity_gpu.py::test_generator_attn_eql_golden for tag `attn` (1e-4; the biases in
    front of a train-mode BatchNorm have zero gradients and are compared absolutely, as there); then one TrainStep with it."""
    from oracle import spgan_oracle as orc
    from spgan import fixture_rng as fr
    B, N = 4, 256
    params = fr.init_params(orc.generator_shapes(attn=True), salt=30)
    x = fr.sphere_template(N)[None].repeat(B, 1, 1).cuda()
    z = fr.latent(B, N, seed=130).cuda()
    res = []
    for fused in (False, True):
        G = sp.Generator(_Opts)
        sdict = G.state_dict()
        G.load_state_dict({**sdict, **{k: v.detach().clone() for k, v in params.items()}})
        G = G.cuda().train()
        assert G.attn.materialize is True
        if fused:
            G.attn.materialize = False
        out = G(x, z)
        dy = fr.normal("g13.dy.attn", out.shape)
        (out * dy.cuda()).sum().backward()
        res.append((out.detach(), {n: p.grad.clone() for n, p in G.named_parameters()}))
    (out_m, g_m), (out_f, g_f) = res
    e_out = rel_l2(out_f.cpu().numpy(), out_m.cpu().numpy())
    worst = max((rel_l2(g_f[n].cpu().numpy(), g_m[n].cpu().numpy()), n) for n in g_m if not n.endswith(ZERO_GRAD_BIASES))
    print("generator: out rel-L2 %.2e, worst gradient %.2e (%s)" % ((e_out,) + worst))
    assert e_out <= 1e-4
    for n in g_m:
        e = rel_l2(g_f[n].cpu().numpy(), g_m[n].cpu().numpy())
        assert e <= 1e-4 or float((g_f[n] - g_m[n]).abs().max()) <= (2e-3 if n.endswith(ZERO_GRAD_BIASES) else 1e-7), (n, e)
    D = sp.Discriminator(_Opts).cuda().train()
    tr = sp.TrainStep(G, D, gan="ls", use_gp=False)
    info = tr.step(x, fr.synthetic_real(B, N, seed=81).cuda(), z, fr.latent(B, N, seed=83).cuda())
    assert bool(torch.isfinite(info["loss_d"])) and bool(torch.isfinite(info["loss_g"]))
