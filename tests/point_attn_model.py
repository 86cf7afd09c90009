"""A plain torch model of dot-product point self-attention (spgan.point_attn, csrc/point_attn.hip), of the two
modules that run on it -- Attention (Generation/modules.py:534-558) and Self_Attn (Common/utilities.py:210-245) -- and the case table
of golden `point_attn.npz`.

Core, per shape, on point-major rows q, k [b,n,dk], v [b,n,dv]:

    S_ij = q_i . k_j (unscaled),  P = softmax_j(S),  O_i = sum_j P_ij v_j,  lse_i = log sum_j exp(S_ij)
    dP = dO V^T,  D_i = dO_i . O_i,  dS = P (dP - D),  dQ = dS K,  dK = dS^T Q,  dV = P^T dO

Attention:  theta, phi, g = x W^T (no bias);  q = theta, k = phi, v = g;  out = gamma W_o O + x.
Self_Attn:  softmax(query_key, 1) normalises over the FIRST point index and bmm(value, attn) sums over it, so
            out_j = gamma sum_i softmax_i(query_i . key_j) value_i + x_j:  q = key projection, k = query projection, v = value projection.

The model materialises every [b,n,n] map: it is the yardstick, evaluated in float64 or float32, not the memory behaviour."""
import numpy as np
import torch

GAMMA = 0.7
# tag -> module, sizes (the issue's table)
CASES = {
    "a": dict(module="Attention", B=2, N=100, ch=64),      # N not a multiple of 32; dk 8, dv 32
    "b": dict(module="Attention", B=1, N=1, ch=16),        # one point: P = 1; dk 2 is padded to 4; d theta = d phi = 0 exactly
    "c": dict(module="Attention", B=1, N=257, ch=640),     # the generator's widths (dk 80, dv 320); N one past a multiple of every tile size
    "d": dict(module="Attention", B=1, N=160, ch=64),      # scores span +-30 per row, row maximum at j = N - 1, prefix maximum rises at every 32
    "e": dict(module="Self_Attn", B=2, N=96, ch=128),      # non-zero biases; dk 16, dv 128; the swapped roles
    "f": dict(module="Self_Attn", B=3, N=33, ch=24),       # dk 3, padded; dv 24; N = 33
    "g": dict(module="Attention", B=1, N=64, ch=64),       # theta.weight = 0: uniform attention; d phi = 0 exactly
}
SAMPLE_MIN, SAMPLE_STRIDE = 2048, 16        # results of more than SAMPLE_MIN elements are stored as every SAMPLE_STRIDE-th value + norm
BIG, BIG_STRIDE = 32768, 64                 # beyond BIG elements: inputs and weights on a coarse bf16-exact grid, results as every 64th value
STATE_KEYS = {"Attention": ("gamma", "theta.weight", "phi.weight", "g.weight", "o.weight"),
              "Self_Attn": ("gamma", "query.weight", "query.bias", "key.weight", "key.bias", "value.weight", "value.bias")}


def state_shapes(c):
    ch = c["ch"]
    if c["module"] == "Attention":
        return {"gamma": (), "theta.weight": (ch // 8, ch, 1), "phi.weight": (ch // 8, ch, 1), "g.weight": (ch // 2, ch, 1),
                "o.weight": (ch, ch // 2, 1)}
    return {"gamma": (1,), "query.weight": (ch // 8, ch, 1), "query.bias": (ch // 8,), "key.weight": (ch // 8, ch, 1), "key.bias": (ch // 8,),
            "value.weight": (ch, ch, 1), "value.bias": (ch,)}


def _bf16(t):
    return t.bfloat16().float()


def case_tensors(tag):
    """(x [B,ch,N], cotangent [B,ch,N], state_dict) of a case in float32 from a seeded generator.  Weights of more than 1024 elements are
    bfloat16-exact (the golden stores their upper halves), and so are x and the cotangent."""
    c = CASES[tag]
    B, N, ch = c["B"], c["N"], c["ch"]
    g = torch.Generator().manual_seed(7000 + ord(tag))
    rn = lambda *s: torch.randn(*s, generator=g)
    grid = lambda lim, den, *s: torch.randint(-lim, lim + 1, s, generator=g).float() / den      # few distinct bf16-exact values: compresses
    big = B * ch * N > BIG
    x, cot = (grid(3, 2, B, ch, N), grid(2, 2, B, ch, N)) if big else (_bf16(rn(B, ch, N)), _bf16(rn(B, ch, N)))
    sd = {}
    for k_, shp in state_shapes(c).items():
        if k_ == "gamma":
            sd[k_] = torch.full(shp, GAMMA)
            continue
        fan = shp[1] if len(shp) == 3 else ch
        w = (torch.rand(*shp, generator=g) * 2 - 1) / fan ** 0.5            # nn.Conv1d's range
        if w.numel() > BIG:
            w = grid(2, 64, *shp) * (640.0 / fan) ** 0.5                     # +-2/64 at fan-in 640: about nn.Conv1d's range
        sd[k_] = _bf16(w) if w.numel() > 1024 else w
    if tag == "g":
        sd["theta.weight"].zero_()
    if tag == "d":
        # theta_0 = channel 0 of x in [1, 2], phi_0 = channel 1 of x = a ramp over the points from -45 to +45: S_ij = theta_i0 phi_j0 + a
        # small remainder (the other rows of both weights are scaled down), so every row spans more than +-30 and rises with j
        x[:, 0] = 1.0 + torch.rand(B, N, generator=g)
        x[:, 1] = torch.linspace(-45.0, 45.0, N)[None]
        for k_, col in (("theta.weight", 0), ("phi.weight", 1)):
            sd[k_] *= 0.05
            sd[k_][0] = 0.0
            sd[k_][:, :2] = 0.0
            sd[k_][0, col] = 1.0
        x = _bf16(x)
    return x, cot, sd


# ---------------------------------------------------------------- the core
def core_forward(q, k, v):
    """-> (O [b,n,dv], lse [b,n], P [b,n,n])"""
    S = q @ k.transpose(1, 2)
    return torch.softmax(S, -1) @ v, torch.logsumexp(S, -1), torch.softmax(S, -1)


def core_backward(q, k, v, dO):
    """-> (dQ, dK, dV) by the written-out formulas"""
    O, _, P = core_forward(q, k, v)
    dP = dO @ v.transpose(1, 2)
    D = (dO * O).sum(-1, keepdim=True)
    dS = P * (dP - D)
    return dS @ k, dS.transpose(1, 2) @ q, P.transpose(1, 2) @ dO


def scores(tag, sd, x):
    """S [B,N,N] of a case in the core's orientation (row = the point whose softmax it is)"""
    w = lambda n: sd[n].to(x.dtype).squeeze(-1)
    xp = x.transpose(1, 2)
    if CASES[tag]["module"] == "Attention":
        return (xp @ w("theta.weight").t()) @ (xp @ w("phi.weight").t()).transpose(1, 2)
    qy = xp @ w("query.weight").t() + sd["query.bias"].to(x.dtype)
    ky = xp @ w("key.weight").t() + sd["key.bias"].to(x.dtype)
    return ky @ qy.transpose(1, 2)


# ---------------------------------------------------------------- the modules, through the core
def module_forward(kind, sd, x):
    """x [B,ch,N] -> out [B,ch,N] with the parameters of sd (tensors of x's dtype; may require grad)"""
    w = lambda n: sd[n].squeeze(-1)
    xp = x.transpose(1, 2)                                               # [B,N,ch]
    if kind == "Attention":
        O, _, _ = core_forward(xp @ w("theta.weight").t(), xp @ w("phi.weight").t(), xp @ w("g.weight").t())
        return (sd["gamma"] * (O @ w("o.weight").t()) + xp).transpose(1, 2)
    qy = xp @ w("query.weight").t() + sd["query.bias"]
    ky = xp @ w("key.weight").t() + sd["key.bias"]
    vl = xp @ w("value.weight").t() + sd["value.bias"]
    O, _, _ = core_forward(ky, qy, vl)
    return (sd["gamma"] * O + xp).transpose(1, 2)


def module_run(kind, sd, x, cot, dtype):
    """(out, {"dx", "grad|<key>"}) of module_forward by torch.autograd in dtype"""
    p = {k_: v_.to(dtype).clone().requires_grad_(True) for k_, v_ in sd.items()}
    xr = x.to(dtype).clone().requires_grad_(True)
    out = module_forward(kind, p, xr)
    (out * cot.to(dtype)).sum().backward()
    res = {"out": out.detach(), "dx": xr.grad}
    res.update({"grad|" + k_: (v_.grad if v_.grad is not None else torch.zeros_like(v_)) for k_, v_ in p.items()})
    return res


# ---------------------------------------------------------------- golden access
def rel(a, b):
    a, b = a.double(), b.double()
    n = float(b.norm())
    return float((a - b).norm()) / n if n > 0 else float((a - b).norm())


def _get(d, name, shape=None):
    """a stored float32 array, from its upper halves where the generator stored those"""
    head, _, tail = name.partition("|")
    first, _, rest = tail.partition("|")
    k16 = "%s|%s16%s" % (head, first, "|" + rest if rest else "")
    a = (d[k16].astype(np.uint32) << 16).view(np.float32) if k16 in d else np.array(d[name])
    return torch.from_numpy(a.copy()) if shape is None else torch.from_numpy(a.copy()).reshape(shape)


def golden_inputs(d, tag):
    """(x [B,ch,N], cotangent [B,ch,N], state_dict) of a case, float32"""
    c = CASES[tag]
    shp = (c["B"], c["ch"], c["N"])
    return _get(d, tag + "|x", shp), _get(d, tag + "|g", shp), golden_state_dict(d, tag)


def golden_state_dict(d, tag):
    shapes = state_shapes(CASES[tag])
    return {k_: _get(d, "%s|param|%s" % (tag, k_), shapes[k_]) for k_ in STATE_KEYS[CASES[tag]["module"]]}


def quantities(tag):
    return ("out", "dx") + tuple("grad|" + k_ for k_ in STATE_KEYS[CASES[tag]["module"]])


def noise(d, tag, q):
    return float(d[tag + "|noise"][quantities(tag).index(q)])


def stored(d, tag, q):
    return d["%s|%s|full" % (tag, q)] if "%s|%s|full" % (tag, q) in d else d["%s|%s|samples" % (tag, q)]


def golden_rel(d, tag, q, got):
    """rel-L2 of `got` against the golden's float64 quantity q (all of it, or its stored samples); an all-zero golden gives the absolute norm."""
    got = got.detach().double().cpu().reshape(-1)
    if "%s|%s|samples" % (tag, q) in d:
        return rel(got[::int(d["%s|%s|stride" % (tag, q)])], torch.from_numpy(d["%s|%s|samples" % (tag, q)]))
    return rel(got, torch.from_numpy(np.array(d["%s|%s|full" % (tag, q)])).reshape(-1))


EXACT_ZERO = {"b": ("grad|theta.weight", "grad|phi.weight"), "g": ("grad|phi.weight",)}
