"""A plain torch model of the decomposed PointTransformerLayer (spgan.modules.PointTransformerLayer, csrc/pair_attn.hip; DESIGN.md
section 25) and the case table of golden `point_transformer.npz`.

For x [b,n,dim], pos [b,n,3] (point-major) and q, k, v = the three thirds of x Wqkv^T:

    r_ij   = relu(Wp1 (pos_i - pos_j) + bp1)                    [H]      the position MLP's hidden layer, per pair
    pre_ij = QaC_i - Ka_j + Wc r_ij                             [M]      QaC = q Wa1^T + c, Ka = k Wa1^T, Wc = Wa1 Wp2, c = Wa1 bp2 + ba1
    sim_ij = wa2 . relu(pre_ij)                                          (+ ba2, which the softmax cancels)
    a      = softmax_j(sim);  Sv_i = sum_j a_ij v_j;  R_i = sum_j a_ij r_ij
    out_i  = Sv_i + Wp2 R_i + bp2

which equals the reference's sum_j a_ij (v_j + e_ij), e_ij = Wp2 r_ij + bp2, because the a_ij of a row sum to one.  The model
materialises every pair tensor: it is the yardstick, evaluated in float64 or float32, not the memory behaviour.  Each launcher of
spgan.pair_attn has its contract here (fwd, probs, dsim, bwd) without padding, and layer_backward chains the written-out formulas;
tests/test_point_transformer_cpu.py pins them against autograd."""
import numpy as np
import torch

TILE = 32                       # keys per tile of the pair kernel (and pairs per MFMA tile)
# tag -> sizes (the issue's table; the key tile is 32)
CASES = {
    "a": dict(b=2, n=2 * TILE, dim=32, H=16, mult=4),    # aligned baseline: two full key tiles, dim * mult = 128 (one row group, no padded row)
    "b": dict(b=1, n=1, dim=8, H=8, mult=2),             # one point: a = 1, out = v + bp2
    "c": dict(b=3, n=2 * TILE + 5, dim=24, H=20, mult=3),     # nothing aligned
    "d": dict(b=1, n=3 * TILE + 1, dim=32, H=16, mult=4),     # sim spans +-40, every row's maximum in the last key tile
    "e": dict(b=1, n=16, dim=128, H=64, mult=4),         # the reference's demo sizes: four row groups, two hidden tiles.  Its two weight
                                                         # gradients of more than 8192 elements are stored, and compared, as every 16th
                                                         # flattened value: columns 0, 16, 32, .. of their 128-wide rows (the smaller cases in full)
    "f": dict(b=2, n=37, dim=16, H=8, mult=2),           # wa2 = 0: uniform attention, out_i = mean_j (v_j + e_ij)
}
STATE_KEYS = ("to_qkv.weight", "pos_mlp.0.weight", "pos_mlp.0.bias", "pos_mlp.2.weight", "pos_mlp.2.bias", "attn_mlp.0.weight",
              "attn_mlp.0.bias", "attn_mlp.2.weight", "attn_mlp.2.bias")
ATTN_PARAMS = ("attn_mlp.0.weight", "attn_mlp.0.bias", "attn_mlp.2.weight", "attn_mlp.2.bias")
SAMPLE_MIN, SAMPLE_STRIDE = 8192, 16        # results of more than SAMPLE_MIN elements are stored as every SAMPLE_STRIDE-th value + norm


def state_shapes(c):
    d, H, M = c["dim"], c["H"], c["dim"] * c["mult"]
    return {"to_qkv.weight": (3 * d, d), "pos_mlp.0.weight": (H, 3), "pos_mlp.0.bias": (H,), "pos_mlp.2.weight": (d, H),
            "pos_mlp.2.bias": (d,), "attn_mlp.0.weight": (M, d), "attn_mlp.0.bias": (M,), "attn_mlp.2.weight": (1, M), "attn_mlp.2.bias": (1,)}


def _bf16(t):
    return t.bfloat16().float()


def case_tensors(tag, seed=0):
    """(x, pos, cotangent, state_dict) of a case in float32, from a seeded generator.  Weights of more than 1024 elements are bfloat16-exact
    (the golden stores their upper halves).  Case d and f are shaped as the table says; make_golden asserts d's conditions."""
    c = CASES[tag]
    g = torch.Generator().manual_seed(1000 * seed + ord(tag))
    rn = lambda *s: torch.randn(*s, generator=g)
    x, pos, cot = rn(c["b"], c["n"], c["dim"]), rn(c["b"], c["n"], 3), _bf16(rn(c["b"], c["n"], c["dim"]))
    sd = {}
    for k_, shp in state_shapes(c).items():
        fan = shp[1] if len(shp) == 2 else state_shapes(c)[k_.replace("bias", "weight")][1]
        w = (torch.rand(*shp, generator=g) * 2 - 1) / fan ** 0.5          # nn.Linear's range
        sd[k_] = _bf16(w) if w.numel() > 1024 else w
    if tag == "f":
        sd["attn_mlp.2.weight"].zero_()
    if tag == "d":
        # spread sim to about +-40, then pull the last point's key so far along a direction that raises sim that it wins every row
        sim = sim_of(sd, x.double(), pos.double())
        sd["attn_mlp.2.weight"] *= float(80.0 / (sim.max() - sim.min()))
        D = c["dim"]
        W, Wa1, wa2 = sd["to_qkv.weight"].double(), sd["attn_mlp.0.weight"].double(), sd["attn_mlp.2.weight"].double()[0]
        Wq, Wk = W[:D], W[D:2 * D]
        best, u = -1e30, None
        for _ in range(512):            # as a key the point must win the other rows (-Ka grows), as a query its own key must win its row
            cand = rn(D).double()
            as_key = float(wa2 @ torch.relu(-(Wa1 @ (Wk @ cand))))
            own = float(wa2 @ torch.relu(Wa1 @ ((Wq - Wk) @ cand))) - float(wa2 @ torch.relu(Wa1 @ (Wq @ cand)))
            if min(as_key, own) > best:
                best, u = min(as_key, own), cand
        for t in range(1, 200):
            x[0, -1] = (0.25 * t * u).float()
            sim = sim_of(sd, x.double(), pos.double())
            if bool((sim[:, :, -1] > sim[:, :, :-1].max(-1).values + 0.5).all()):
                break
    return x, pos, cot, sd


# ---------------------------------------------------------------- the decomposed forward
def derived(sd, dtype):
    """(Wq, Wk, Wv, Wp1, bp1, Wp2, bp2, Wa1, wa2, Wc, c) in dtype"""
    p = {k_: v_.to(dtype) for k_, v_ in sd.items()}
    D = p["pos_mlp.2.bias"].numel()
    W = p["to_qkv.weight"]
    Wa1, Wp2, bp2 = p["attn_mlp.0.weight"], p["pos_mlp.2.weight"], p["pos_mlp.2.bias"]
    return (W[:D], W[D:2 * D], W[2 * D:], p["pos_mlp.0.weight"], p["pos_mlp.0.bias"], Wp2, bp2, Wa1, p["attn_mlp.2.weight"][0],
            Wa1 @ Wp2, Wa1 @ bp2 + p["attn_mlp.0.bias"])


def hidden(pos, Wp1, bp1):
    """r [b,n,n,H]"""
    return torch.relu((pos[:, :, None] - pos[:, None, :]) @ Wp1.t() + bp1)


def pre_of(r, QaC, Ka, Wc):
    return QaC[:, :, None] - Ka[:, None, :] + r @ Wc.t()


def sim_of(sd, x, pos):
    Wq, Wk, _, Wp1, bp1, _, _, Wa1, wa2, Wc, c = derived(sd, x.dtype)
    return torch.relu(pre_of(hidden(pos, Wp1, bp1), x @ Wq.t() @ Wa1.t() + c, x @ Wk.t() @ Wa1.t(), Wc)) @ wa2


def relu_margin(sd, x, pos):
    """The smallest |pre-activation| of the two per-pair ReLUs (float64): a unit closer to zero than float32 rounding may switch between
    a float32 and a float64 evaluation, and one switched unit moves a gradient by far more than rounding does."""
    Wq, Wk, _, Wp1, bp1, _, _, Wa1, _, Wc, c = derived(sd, torch.float64)
    x, pos = x.double(), pos.double()
    z = (pos[:, :, None] - pos[:, None, :]) @ Wp1.t() + bp1
    pre = pre_of(torch.relu(z), x @ Wq.t() @ Wa1.t() + c, x @ Wk.t() @ Wa1.t(), Wc)
    return min(float(z.abs().min()), float(pre.abs().min()))


def pair_fwd(pos, Wp1, bp1, QaC, Ka, Wc, wa2, v):
    """spgan.pair_attn.pair_attn_fwd: -> (Sv [b,n,D], R [b,n,H], lse [b,n])"""
    r = hidden(pos, Wp1, bp1)
    sim = torch.relu(pre_of(r, QaC, Ka, Wc)) @ wa2
    a = torch.softmax(sim, -1)
    return a @ v, torch.einsum("bij,bijh->bih", a, r), torch.logsumexp(sim, -1)


def pair_probs(pos, Wp1, bp1, QaC, Ka, Wc, wa2, lse):
    """pair_attn_probs: P [b,n,n] = exp(sim - lse)"""
    return torch.exp(torch.relu(pre_of(hidden(pos, Wp1, bp1), QaC, Ka, Wc)) @ wa2 - lse[:, :, None])


def pair_dsim(P, dout, v, dR, pos, Wp1, bp1):
    """pair_attn_dsim: dS_ij = P_ij (g_ij - delta_i), g_ij = dout_i . v_j + dR_i . r_ij, delta_i = sum_j P_ij g_ij / sum_j P_ij
    (= dout_i . (out_i - bp2) when the row of P sums to one)"""
    g = dout @ v.transpose(1, 2) + torch.einsum("bih,bijh->bij", dR, hidden(pos, Wp1, bp1))
    return P * (g - ((P * g).sum(-1) / P.sum(-1))[:, :, None])


def pair_bwd(pos, Wp1, bp1, QaC, Ka, Wc, wa2, P, dS, dR):
    """Both roles of pair_attn_bwd, written out: -> (dQa, dKa, Zq, Zk, dWc, dwa2)."""
    r = hidden(pos, Wp1, bp1)
    pre = pre_of(r, QaC, Ka, Wc)
    dpre = dS[..., None] * wa2 * (pre > 0)
    dz = (dpre @ Wc + P[..., None] * dR[:, :, None]) * (r > 0)
    return (dpre.sum(2), -dpre.sum(1), dz.sum(2), dz.sum(1), torch.einsum("bijm,bijh->mh", dpre, r),
            torch.einsum("bij,bijm->m", dS, torch.relu(pre)))


def layer_forward(sd, x, pos, keep=False):
    """The layer through the launcher contracts.  keep=True also returns what the backward reads."""
    Wq, Wk, Wv, Wp1, bp1, Wp2, bp2, Wa1, wa2, Wc, c = derived(sd, x.dtype)
    q, k, v = x @ Wq.t(), x @ Wk.t(), x @ Wv.t()
    QaC, Ka = q @ Wa1.t() + c, k @ Wa1.t()
    Sv, R, lse = pair_fwd(pos, Wp1, bp1, QaC, Ka, Wc, wa2, v)
    out = Sv + R @ Wp2.t() + bp2
    return (out, (q, k, v, QaC, Ka, R, lse)) if keep else out


def layer_backward(sd, x, pos, dout):
    """Every gradient of (layer_forward * dout).sum(), by the written-out chain of spgan.pair_attn.PairAttnFn: {name: gradient}."""
    Wq, Wk, Wv, Wp1, bp1, Wp2, bp2, Wa1, wa2, Wc, c = derived(sd, x.dtype)
    out, (q, k, v, QaC, Ka, R, lse) = layer_forward(sd, x, pos, keep=True)
    f2 = lambda t: t.reshape(-1, t.shape[-1])
    dR = dout @ Wp2
    P = pair_probs(pos, Wp1, bp1, QaC, Ka, Wc, wa2, lse)
    dS = pair_dsim(P, dout, v, dR, pos, Wp1, bp1)
    dv = P.transpose(1, 2) @ dout
    dQa, dKa, Zq, Zk, dWc, dwa2 = pair_bwd(pos, Wp1, bp1, QaC, Ka, Wc, wa2, P, dS, dR)
    dq, dk = dQa @ Wa1, dKa @ Wa1
    dc = f2(dQa).sum(0)
    Zd = Zq - Zk
    g = {"dx": dq @ Wq + dk @ Wk + dv @ Wv, "dpos": Zd @ Wp1,
         "to_qkv.weight": torch.cat([f2(dq).t() @ f2(x), f2(dk).t() @ f2(x), f2(dv).t() @ f2(x)]),
         "pos_mlp.0.weight": f2(Zd).t() @ f2(pos), "pos_mlp.0.bias": f2(Zq).sum(0),
         "pos_mlp.2.weight": f2(dout).t() @ f2(R) + Wa1.t() @ dWc, "pos_mlp.2.bias": f2(dout).sum(0) + Wa1.t() @ dc,
         "attn_mlp.0.weight": f2(dQa).t() @ f2(q) + f2(dKa).t() @ f2(k) + dWc @ Wp2.t() + torch.outer(dc, bp2),
         "attn_mlp.0.bias": dc, "attn_mlp.2.weight": dwa2[None], "attn_mlp.2.bias": torch.zeros(1, dtype=x.dtype)}
    return out, g


def autograd_run(sd, x, pos, dout, forward=None):
    """(out, {name: gradient}) of a forward (default: layer_forward) by torch.autograd, in the dtype of x."""
    p = {k_: v_.to(x.dtype).clone().requires_grad_(True) for k_, v_ in sd.items()}
    xr, pr = x.clone().requires_grad_(True), pos.clone().requires_grad_(True)
    out = (forward or layer_forward)(p, xr, pr)
    (out * dout).sum().backward()
    g = {"dx": xr.grad, "dpos": pr.grad}
    g.update({k_: (v_.grad if v_.grad is not None else torch.zeros_like(v_)) for k_, v_ in p.items()})
    return out.detach(), g


# ---------------------------------------------------------------- golden access
def rel(a, b):
    a, b = a.double(), b.double()
    n = float(b.norm())
    return float((a - b).norm()) / n if n > 0 else float((a - b).norm())


def golden_state_dict(d, tag):
    sd = {}
    for k_ in STATE_KEYS:
        if "%s|param16|%s" % (tag, k_) in d:
            sd[k_] = torch.from_numpy((d["%s|param16|%s" % (tag, k_)].astype(np.uint32) << 16).view(np.float32).copy())
        else:
            sd[k_] = torch.from_numpy(d["%s|param|%s" % (tag, k_)].copy())
    return sd


def noise(d, tag, q):
    return float(d[tag + "|noise"][list(d["noise_keys"]).index(q)])


def golden_rel(d, tag, q, got):
    """rel-L2 of `got` against the golden's float64 quantity q (all of it, or its stored samples); an all-zero golden gives the absolute norm."""
    got = got.detach().double().cpu().reshape(-1)
    if "%s|%s|samples" % (tag, q) in d:
        return rel(got[::int(d["%s|%s|stride" % (tag, q)])], torch.from_numpy(d["%s|%s|samples" % (tag, q)]))
    return rel(got, torch.from_numpy(d["%s|%s|full" % (tag, q)]).reshape(-1))
