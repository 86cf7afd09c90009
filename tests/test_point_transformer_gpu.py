"""GPU: spgan.PointTransformerLayer (csrc/pair_attn.hip behind spgan.pair_attn) against the vectors captured from the reference (golden
point_transformer.npz) and its launchers against the float64 model of tests/point_transformer_model.py.

Tolerances.  Module vs golden (the reference's float64 run): rel-L2 3e-6 for out, dx and dpos, 5e-6 for parameter gradients (the bases of
tests/test_deform_xyz_gpu.py) -- or 5 x the golden's stored distance of the reference's float32 run from its float64 run where that is
larger.  The generator lists the quantities whose 5 x distance exceeds the base: case d only (sim spans -35 .. +50): `dx` (stored
1.26e-06), `grad|attn_mlp.0.weight` (8.34e-06), `grad|attn_mlp.0.bias` (1.06e-05), `grad|attn_mlp.2.weight` (9.02e-06); every other
quantity keeps the base bound.
attn_mlp.2.bias cancels in the softmax: its gradient is an exact zero here and rounding noise in the reference's float32 run, at most
1.55e-06 absolute over the six cases (stored as `tag|ba2_f32`); the test asserts the stored value stays below 1e-5.
Case b (one point): dpos and every attention-MLP gradient are exact zeros here and in the reference.  Case f (w_a2 = 0): the gradients of
attn_mlp.0 are exact zeros in both.
Launchers vs the float64 model on the same float32 operands: 3e-6 for the forward's results, P and dS, 5e-6 for the sums of the pair
backward, or 5 x the rel-L2 distance between a float32 and a float64 CPU evaluation of the model on those operands where that is larger.
A shape with 256 < dim <= 512 (two value columns per thread in the forward, three row groups of Wc) is checked against the float64
model's autograd with the same bounds, the yardstick being the model's own float32 evaluation.
Memory: forward + backward at b 1, n 1024, dim 128, H 64, mult 4 stay below ONE [b,n,n,dim] float32 tensor (512 MiB); the reference's
formulation holds more than five of them."""
import numpy as np
import pytest
import torch

import point_transformer_model as pm
from helpers import golden

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
    return golden("point_transformer.npz")


def _module(sp, d, tag):
    c = pm.CASES[tag]
    m = sp.PointTransformerLayer(c["dim"], pos_mlp_hidden_dim=c["H"], attn_mlp_hidden_mult=c["mult"])
    m.load_state_dict(pm.golden_state_dict(d, tag), strict=True)
    return m.cuda()


def _run(m, x, pos, cot):
    xg, pg = x.detach().clone().requires_grad_(True), pos.detach().clone().requires_grad_(True)
    out = m(xg, pg)
    (out * cot).sum().backward()
    return out.detach(), xg.grad, pg.grad


def _case(d, tag):
    return tuple(torch.from_numpy(d["%s|%s" % (tag, k)]).cuda() for k in ("x", "pos", "g"))


def _all(m, x, pos, cot):
    for p in m.parameters():
        p.grad = None
    return list(_run(m, x, pos, cot)) + [p.grad.clone() for p in m.parameters()]


# ---------------------------------------------------------------- module against the reference (golden)
@pytest.mark.parametrize("tag", TAGS)
def test_module_golden(sp, d, tag):
    c = pm.CASES[tag]
    m = _module(sp, d, tag)
    out, dx, dpos = _run(m, *_case(d, tag))
    assert tuple(out.shape) == (c["b"], c["n"], c["dim"])
    got = {"out": out, "dx": dx, "dpos": dpos}
    got.update({"grad|" + n: p.grad for n, p in m.named_parameters()})
    e = {}
    for q, v in got.items():
        if q == "grad|attn_mlp.2.bias":
            assert float(v.abs().max()) == 0.0 and float(d[tag + "|ba2_f32"]) <= 1e-5
            continue
        stored = d["%s|%s|full" % (tag, q)] if "%s|%s|full" % (tag, q) in d else d["%s|%s|samples" % (tag, q)]
        if not np.any(stored):                                               # b: one point; f: w_a2 = 0 -- exact zeros here as there
            assert float(v.abs().max()) == 0.0, (tag, q)
            continue
        e[q] = pm.golden_rel(d, tag, q, v)
    print("%s: rel-L2 vs reference float64 %s" % (tag, {k: "%.2e" % v for k, v in e.items()}))
    for q, v in e.items():
        bound = max(3e-6 if q in ("out", "dx", "dpos") else 5e-6, 5.0 * pm.noise(d, tag, q))
        assert v <= bound, (tag, q, v, bound)
    if tag == "b":
        assert set(e) == {"out", "dx", "grad|to_qkv.weight", "grad|pos_mlp.0.bias", "grad|pos_mlp.2.weight", "grad|pos_mlp.2.bias"}


# ---------------------------------------------------------------- launchers against the float64 model
@pytest.mark.parametrize("tag", ["a", "c", "d", "e"])
def test_launchers_against_model(sp, d, tag):
    """Every launcher on float32 operands built once on the CPU: the saved softmax statistic (lse), P, dS and the partial-reduction
    outputs (Z per row group, the dWc | dw_a2 records) included."""
    from spgan import pair_attn
    c = pm.CASES[tag]
    b, n, D, H, M = c["b"], c["n"], c["dim"], c["H"], c["dim"] * c["mult"]
    x, pos, cot = (t.cpu() for t in _case(d, tag))
    sd = pm.golden_state_dict(d, tag)
    # float32 operands of the pair launchers, from the float32 model
    Wq, Wk, Wv, Wp1, bp1, Wp2, bp2, Wa1, wa2, Wc, cv = pm.derived(sd, torch.float32)
    q, k, v = x @ Wq.t(), x @ Wk.t(), x @ Wv.t()
    QaC, Ka = q @ Wa1.t() + cv, k @ Wa1.t()
    ops32 = dict(pos=pos, Wp1=Wp1, bp1=bp1, QaC=QaC, Ka=Ka, Wc=Wc, wa2=wa2, v=v)

    def model(dtype):
        o = {k_: t.to(dtype) for k_, t in ops32.items()}
        Sv, R, lse = pm.pair_fwd(o["pos"], o["Wp1"], o["bp1"], o["QaC"], o["Ka"], o["Wc"], o["wa2"], o["v"])
        g = cot.to(dtype)
        dR = g @ Wp2.to(dtype)
        P = pm.pair_probs(o["pos"], o["Wp1"], o["bp1"], o["QaC"], o["Ka"], o["Wc"], o["wa2"], lse)
        return dict(Sv=Sv, R=R, lse=lse, P=P, dR=dR)
    m64, m32 = model(torch.float64), model(torch.float32)
    # the backward's inputs are taken from the float64 model rounded once, so that both sides read the same float32 numbers
    P32, dR32 = m64["P"].float(), m64["dR"].float()

    def model_bwd(dtype):
        o = {k_: t.to(dtype) for k_, t in ops32.items()}
        dS = pm.pair_dsim(P32.to(dtype), cot.to(dtype), o["v"], dR32.to(dtype), o["pos"], o["Wp1"], o["bp1"])
        dS_in = dS32.to(dtype) if dS32 is not None else dS
        dQa, dKa, Zq, Zk, dWc, dwa2 = pm.pair_bwd(o["pos"], o["Wp1"], o["bp1"], o["QaC"], o["Ka"], o["Wc"], o["wa2"], P32.to(dtype), dS_in, dR32.to(dtype))
        return dict(dS=dS, dQa=dQa, dKa=dKa, Zq=Zq, Zk=Zk, dWc=dWc, dwa2=dwa2)
    dS32 = None
    dS32 = model_bwd(torch.float64)["dS"].float()
    b64, b32 = model_bwd(torch.float64), model_bwd(torch.float32)

    dev = torch.device("cuda")
    Mp, Hp = pair_attn.padded_sizes(D, H, c["mult"])
    pad = lambda t, w: torch.nn.functional.pad(t, (0, w - t.shape[-1])).contiguous().to(dev)
    Wp1p = pad(torch.cat([Wp1, bp1[:, None]], 1).t(), Hp).t().contiguous()
    Wcp = pad(torch.nn.functional.pad(Wc, (0, 0, 0, Mp - M)), Hp)
    gQ, gK, gw = pad(QaC.reshape(b * n, M), Mp), pad(Ka.reshape(b * n, M), Mp), pad(wa2, Mp)
    gpos, gv = pos.to(dev).contiguous(), v.reshape(b * n, D).to(dev).contiguous()
    Sv, R, lse = pair_attn.pair_attn_fwd(gpos, Wp1p, gQ, gK, Wcp, gw, gv)
    P = pair_attn.pair_attn_probs(gpos, Wp1p, gQ, gK, Wcp, gw, m64["lse"].float().reshape(-1).to(dev))
    gP, gdR = P32.to(dev).contiguous(), pad(dR32.reshape(b * n, H), Hp)
    dS = pair_attn.pair_attn_dsim(gP, cot.reshape(b * n, D).to(dev), gv, gdR, gpos, Wp1p)
    gdS = dS32.to(dev).contiguous()
    WcT = Wcp.t().contiguous()
    dQa, Zq, rec = pair_attn.pair_attn_bwd(0, gpos, Wp1p, gQ, gK, Wcp, WcT, gw, gP, gdS, gdR)
    dKa, Zk, none = pair_attn.pair_attn_bwd(1, gpos, Wp1p, gQ, gK, Wcp, WcT, gw, gP, gdS, gdR)
    assert none is None and tuple(Zq.shape) == (Mp // 128, b * n, Hp) and rec.shape[0] == b * min(n, max(1, 512 // b))
    assert float(R[:, H:].abs().max() if Hp > H else 0.0) == 0.0 and float(dQa[:, M:].abs().max() if Mp > M else 0.0) == 0.0
    rec = rec.double().sum(0)
    got = dict(Sv=Sv.view(b, n, D), R=R[:, :H].reshape(b, n, H), lse=lse.view(b, n), P=P, dS=dS, dQa=dQa[:, :M].reshape(b, n, M),
               dKa=dKa[:, :M].reshape(b, n, M), Zq=Zq.double().sum(0)[:, :H].reshape(b, n, H), Zk=Zk.double().sum(0)[:, :H].reshape(b, n, H),
               dWc=rec[:Mp * Hp].view(Mp, Hp)[:M, :H], dwa2=rec[Mp * Hp:][:M])
    e = {}
    for name, t in got.items():
        ref64, ref32 = (m64, m32) if name in m64 else (b64, b32)
        bound = max(3e-6 if name in ("Sv", "R", "lse", "P", "dS") else 5e-6, 5.0 * pm.rel(ref32[name], ref64[name]))
        e[name] = (pm.rel(t.cpu(), ref64[name]), bound)
    print("%s: launcher rel-L2 vs float64 model (bound) %s" % (tag, {k_: "%.2e (%.1e)" % v_ for k_, v_ in e.items()}))
    for name, (err, bound) in e.items():
        assert err <= bound, (tag, name, err, bound)


def test_wide_dim_against_model(sp):
    """dim 320 (mult 1, H 8), b 2, n 40: threads 0..63 of the forward own a second value column (256 < dim <= 512), waves own no, one or
    two of them, M = 320 pads to three row groups.  Against the float64 model's autograd; bound max(base, 5 x the distance of the
    model's float32 evaluation from its float64 one).  The first seed whose ReLUs keep 2e-6 from their kinks is taken."""
    c = dict(b=2, n=40, dim=320, H=8, mult=1)
    for seed in range(50):
        g = torch.Generator().manual_seed(seed)
        x, pos, cot = (torch.randn(c["b"], c["n"], k, generator=g) for k in (c["dim"], 3, c["dim"]))
        sd = {k: (torch.rand(*shp, generator=g) * 2 - 1) / (shp[1] if len(shp) == 2 else 8) ** 0.5 for k, shp in pm.state_shapes(c).items()}
        if pm.relu_margin(sd, x, pos) >= 2e-6:
            break
    else:
        raise AssertionError("no seed meets the margin condition")
    o64, g64 = pm.autograd_run(sd, x.double(), pos.double(), cot.double())
    o32, g32 = pm.autograd_run(sd, x, pos, cot)
    m = sp.PointTransformerLayer(c["dim"], pos_mlp_hidden_dim=c["H"], attn_mlp_hidden_mult=c["mult"])
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    out, dx, dpos = _run(m, x.cuda(), pos.cuda(), cot.cuda())
    got = {"out": (out, o64, o32), "dx": (dx, g64["dx"], g32["dx"]), "dpos": (dpos, g64["dpos"], g32["dpos"])}
    got.update({n: (p.grad, g64[n], g32[n]) for n, p in m.named_parameters() if n != "attn_mlp.2.bias"})
    assert float(m.attn_mlp[2].bias.grad.abs().max()) == 0.0
    e = {q: (pm.rel(v.cpu(), r64), max(3e-6 if q in ("out", "dx", "dpos") else 5e-6, 5.0 * pm.rel(r32, r64))) for q, (v, r64, r32) in got.items()}
    print("dim 320 (seed %d): rel-L2 vs float64 model (bound) %s" % (seed, {k: "%.2e (%.1e)" % v for k, v in e.items()}))
    for q, (err, bound) in e.items():
        assert err <= bound, (q, err, bound)


# ---------------------------------------------------------------- properties of the module
def test_deterministic(sp, d):
    """Bit equality of the output and all gradients over two runs: case c, and 3 clouds of 100 points (25 query tiles of 4, four key tiles)."""
    g = torch.Generator().manual_seed(5)
    shapes = [("c",) + _case(d, "c"), (None, torch.randn(3, 100, 24, generator=g).cuda(), torch.randn(3, 100, 3, generator=g).cuda(),
                                       torch.randn(3, 100, 24, generator=g).cuda())]
    for tag, x, pos, cot in shapes:
        res = [_all(_module(sp, d, "c"), x, pos, cot) for _ in range(2)]
        for a, b_ in zip(*res):
            assert torch.equal(a, b_), tag


def test_permutation_and_translation(sp, d):
    """Permuting the points of x and pos together permutes out; adding a constant to pos changes nothing -- both within the noise bound
    of the output (3e-6; case c stores 1.17e-07)."""
    m = _module(sp, d, "c")
    x, pos, cot = _case(d, "c")
    with torch.no_grad():
        out = m(x, pos)
        perm = torch.randperm(x.shape[1], generator=torch.Generator().manual_seed(3)).cuda()
        e_perm = pm.rel(m(x[:, perm].contiguous(), pos[:, perm].contiguous()), out[:, perm])
        e_shift = pm.rel(m(x, pos + torch.tensor([0.5, -0.25, 0.125]).cuda()), out)     # exactly representable: the differences keep their bits' scale
    print("permutation %.2e, translation %.2e" % (e_perm, e_shift))
    assert e_perm <= 3e-6 and e_shift <= 3e-6


def test_refusals(sp, d):
    m = _module(sp, d, "a")
    x, pos, cot = _case(d, "a")
    xg = x.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="once differentiable"):
        torch.autograd.grad(m(xg, pos).sum(), xg, create_graph=True)
    with pytest.raises(RuntimeError, match="GPU"):
        m(x.cpu(), pos.cpu())
    with pytest.raises(ValueError, match="pos must be"):
        m(x, pos[:, :-1])
    with pytest.raises(ValueError, match="x must be"):
        m(x[:, :, :-1], pos)
    with pytest.raises(ValueError, match="pos_mlp_hidden_dim=65"):
        sp.PointTransformerLayer(32, pos_mlp_hidden_dim=65)
    with pytest.raises(ValueError, match="dim=600"):
        sp.PointTransformerLayer(600)


def test_capture(sp, d):
    """One forward + backward inside spgan.CapturedBody, replayed, equals the eager result bit for bit (the operand images are rebuilt
    inside the capture; nothing synchronises with the host)."""
    x, pos, cot = _case(d, "c")

    def make():
        m = _module(sp, d, "c")

        def body(x_, pos_, cot_):
            for p in m.parameters():
                p.grad = None
            xg, pg = x_.detach().requires_grad_(True), pos_.detach().requires_grad_(True)
            out = m(xg, pg)
            (out * cot_).sum().backward()
            return (out.detach(), xg.grad, pg.grad) + tuple(p.grad for p in m.parameters())
        return m, body
    m_e, body_e = make()
    eager = [t.clone() for t in body_e(x, pos, cot)]
    m_c, body_c = make()
    cap = sp.CapturedBody(body_c, modules=(m_c,), warmup=1)
    for call in range(4):                                # one eager warm-up, the capture, two replays
        res = cap(x, pos, cot)
        assert not cap.eager
        for a, b_ in zip(eager, res):
            assert torch.equal(a, b_), call


def test_follows_no_operand_mode(sp, d):
    """ops.set_mfma_operands does not reach the layer: the 'f16' mode gives the bits of the default mode."""
    res = []
    for kind in ("f32", "f16"):
        sp.ops.set_mfma_operands(kind)
        try:
            res.append(_all(_module(sp, d, "a"), *_case(d, "a")))
        finally:
            sp.ops.set_mfma_operands("f32")
    for a, b_ in zip(*res):
        assert torch.equal(a, b_)


def test_peak_memory_below_one_pair_tensor(sp):
    """b 1, n 1024, dim 128, H 64, mult 4: forward + backward peak, minus what was live before, below one [b,n,n,dim] float32 tensor."""
    b, n, dim = 1, 1024, 128
    g = torch.Generator().manual_seed(0)
    m = sp.PointTransformerLayer(dim).cuda()
    x = torch.randn(b, n, dim, generator=g).cuda().requires_grad_(True)
    pos = torch.randn(b, n, 3, generator=g).cuda().requires_grad_(True)
    cot = torch.randn(b, n, dim, generator=g).cuda()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    (m(x, pos) * cot).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("peak %.1f MiB over the %.1f MiB live before (one [b,n,n,dim] tensor: 512 MiB)" % (peak / 2**20, base / 2**20))
    assert peak < b * n * n * dim * 4
    assert all(bool(torch.isfinite(t).all()) for t in (x.grad, pos.grad))
