"""A plain torch model of the dense family (spgan.DenseEdgeModule, DenseModule1D, Dense_Attn; csrc/edge_dense.hip)
and the case table of golden `dense_edge.npz`.

    e0(i,j) = [x_j - x_i, x_i],   z_l = W_l . cat[e0, y_1 .. y_{l-1}] + b_l,   y_l = lrelu(bn_l(z_l), 0.2),   out_i = max_j y_L(i,j)

The model DOES materialise the edge features and every concatenation: it is the yardstick, evaluated in float64 on the CPU (or wherever
its inputs live), not the algorithm's memory behaviour.  The forward is written from the formulas; the backward is autograd over that
float64 forward (`run`).  `level_model` / `scatter_model` / `bn_apply_model` are the float64 statements of the three launchers."""
import numpy as np
import torch

EPS, MOMENTUM, SLOPE = 1e-5, 0.1, 0.2

# DenseEdgeModule: tag -> B, C, N, k, L, G, train, non-initial running statistics
EDGE_CASES = {
    "a": dict(B=2, C=3, N=64, k=5, L=3, G=16, train=True, warm=False),
    "b": dict(B=2, C=16, N=96, k=20, L=4, G=36, train=True, warm=False),
    "c": dict(B=1, C=7, N=50, k=3, L=2, G=12, train=True, warm=False),
    "d": dict(B=2, C=5, N=40, k=4, L=1, G=24, train=True, warm=False),
    "e": dict(B=2, C=3, N=64, k=5, L=3, G=16, train=False, warm=True),
}
# DenseModule1D: tag -> B, in_dim, N, levels, growth
ROWS_CASES = {
    "rows_train": dict(B=2, C=12, N=70, L=3, G=20, train=True, warm=False),
    "rows_eval": dict(B=2, C=12, N=70, L=3, G=20, train=False, warm=True),
}
# Dense_Attn: tag -> B, in_dim, N
ATTN_CASES = {"attn": dict(B=2, C=16, N=48, train=True, warm=False, gamma=0.6)}
CASES = {**EDGE_CASES, **ROWS_CASES, **ATTN_CASES}


def kind_of(tag):
    return "edge" if tag in EDGE_CASES else ("rows" if tag in ROWS_CASES else "attn")


def _bn_entries(sd, name, p, F, warm, seed):
    from spgan import fixture_rng as fr
    sd[p + ".weight"] = fr.uniform(name + p + ".gamma", (F,), 0.5, 1.5, salt=seed)
    sd[p + ".bias"] = fr.uniform(name + p + ".beta", (F,), -0.2, 0.2, salt=seed)
    if warm:
        sd[p + ".running_mean"] = fr.normal(name + p + ".rm", (F,), 0.1, salt=seed)
        sd[p + ".running_var"] = fr.uniform(name + p + ".rv", (F,), 0.5, 1.5, salt=seed)
        sd[p + ".num_batches_tracked"] = torch.tensor(21, dtype=torch.int64)
    else:
        sd[p + ".running_mean"] = torch.zeros(F)
        sd[p + ".running_var"] = torch.ones(F)
        sd[p + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.int64)


def _conv_entries(sd, name, p, shape, seed):
    from spgan import fixture_rng as fr
    bound = 1.0 / np.sqrt(shape[1])
    sd[p + ".weight"] = fr.uniform(name + p + ".W", shape, -bound, bound, salt=seed)
    sd[p + ".bias"] = fr.uniform(name + p + ".b", (shape[0],), -bound, bound, salt=seed)


def rows_widths(c):
    return [c["G"]] * (c["L"] - 1) + [c["C"]]


def _rows_state(sd, name, prefix, c, seed):
    cin = c["C"]
    for l, w in enumerate(rows_widths(c)):
        _conv_entries(sd, name, "%sdense_modules.%d.0" % (prefix, l), (w, cin, 1), seed)
        _bn_entries(sd, name, "%sdense_modules.%d.1" % (prefix, l), w, c["warm"], seed)
        cin += w


def case_tensors(tag, seed=0, row_salts=None):
    """(x [B,C,N], cotangent, state_dict in the module's own key order) of a case, from spgan.fixture_rng (float32).
    row_salts [G] (DenseEdgeModule cases; the golden's `tag|row_salts`): output channel c of the LAST level's convolution with a
    nonzero entry has its weight row and bias drawn again under that salt -- the channels of z_L are independent of each other, so the
    golden's search for a case without a near-tie in the max repairs one channel at a time instead of redrawing everything."""
    from spgan import fixture_rng as fr
    c = CASES[tag]
    kind = kind_of(tag)
    name = "dense_edge.%s" % tag
    B, C, N = c["B"], c["C"], c["N"]
    x = fr.uniform(name + ".x", (B, C, N), -1.0, 1.0, salt=seed) if C <= 4 else fr.normal(name + ".x", (B, C, N), 1.0, salt=seed)
    sd = {}
    if kind == "edge":
        cin = 2 * C
        for l in range(c["L"]):
            _conv_entries(sd, name, "dense_modules.%d.0" % l, (c["G"], cin, 1, 1), seed)
            _bn_entries(sd, name, "dense_modules.%d.1" % l, c["G"], c["warm"], seed)
            cin += c["G"]
        if row_salts is not None:
            p = "dense_modules.%d.0" % (c["L"] - 1)
            W, b = sd[p + ".weight"], sd[p + ".bias"]
            bound = 1.0 / np.sqrt(W.shape[1])
            for ch, rs in enumerate(row_salts):
                if int(rs):
                    row = fr.uniform("%s%s.row%d" % (name, p, ch), (W.shape[1] + 1,), -bound, bound, salt=seed + 1000003 * int(rs))
                    W[ch, :, 0, 0], b[ch] = row[:-1], row[-1]
        g = fr.normal(name + ".g", (B, c["G"], N), salt=seed)
    elif kind == "rows":
        _rows_state(sd, name, "", c, seed)
        g = fr.normal(name + ".g", (B, C, N), salt=seed)
    else:
        for n, w in (("query", C // 8), ("key", C // 8), ("value", C)):
            _conv_entries(sd, name, "atten." + n, (w, C, 1), seed)
        sd["atten.gamma"] = torch.full((1,), c["gamma"])
        _rows_state(sd, name, "dense.", dict(c, L=3, G=C), seed)
        g = fr.normal(name + ".g", (B, C, N), salt=seed)
    return x, g, sd


def zero_gradient(tag, q):
    """Is quantity q a gradient that is exactly zero in exact arithmetic (rounding noise in the reference, so that no relative measure
    applies)?  "exact": a conv bias in front of a train-mode BatchNorm, which the batch mean absorbs -- the modules return exact zeros.
    "noise": Dense_Attn's atten.query.bias (q_i . k_j gains a term that does not depend on i, the index the softmax normalises over)
    and, in train mode, atten.value.bias (the attention weights sum to one, so it shifts every point of a channel alike and the first
    BatchNorm of `dense` absorbs it): Self_Attn computes them like any other gradient, they come out as rounding noise."""
    if not q.startswith("grad|"):
        return None
    if "dense_modules" in q and q.endswith(".0.bias") and CASES[tag]["train"]:
        return "exact"
    if q == "grad|atten.query.bias" or (q == "grad|atten.value.bias" and CASES[tag]["train"]):
        return "noise"
    return None


def build_module(ns, tag):
    """The module of a case from a namespace that has the three classes (spgan, or the executed reference)."""
    c = CASES[tag]
    kind = kind_of(tag)
    if kind == "edge":
        return ns.DenseEdgeModule(2 * c["C"], c["L"], c["G"], c["k"])
    if kind == "rows":
        return ns.DenseModule1D(c["C"], c["L"], c["G"])
    return ns.Dense_Attn(c["C"])


def golden_state_dict(d, tag):
    pre = "%s|param|" % tag
    return {n[len(pre):]: torch.from_numpy(np.asarray(d[n])) for n in d.files if n.startswith(pre)}


def golden_f64(d, tag, q):
    """The reference's float64 result of quantity q: the golden stores it as its (float32-rounded) distance from the float32 run."""
    return torch.from_numpy(np.asarray(d["%s|%s|full" % (tag, q)])).double() + torch.from_numpy(np.asarray(d["%s|%s|d64|full" % (tag, q)])).double()


def quantities(d, tag):
    pre, suf = "%s|" % tag, "|d64|full"
    return [n[len(pre):-len(suf)] for n in d.files if n.startswith(pre) and n.endswith(suf)]


# ----------------------------------------------------------------------------- forward, from the formulas
def gather_neighbours(P, idx, k):
    """P [B,N,F], idx int64 [B,N,k] / [B,N*k] local -> [B,N,k,F]"""
    B, N, F = P.shape
    return P[torch.arange(B, device=P.device).view(B, 1, 1), idx.reshape(B, N, k)]


def graph_feature(x, idx, k):
    """x [B,C,N] -> [B,2C,N,k] = cat[x_j - x_i, x_i]"""
    B, C, N = x.shape
    xp = x.transpose(1, 2)
    cen = xp.unsqueeze(2).expand(B, N, k, C)
    return torch.cat([gather_neighbours(xp, idx, k) - cen, cen], dim=3).permute(0, 3, 1, 2)


def batch_norm(z, sd, p, training, bufs):
    """z [..., F] over all leading dimensions; writes the buffers after the step into bufs"""
    F = z.shape[-1]
    flat = z.reshape(-1, F)
    n = flat.shape[0]
    rm, rv, nb = sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".num_batches_tracked"]
    if training:
        mean = flat.mean(dim=0)
        var = ((flat - mean) ** 2).mean(dim=0)
        bufs[p + ".running_mean"] = ((1 - MOMENTUM) * rm + MOMENTUM * mean).detach()
        bufs[p + ".running_var"] = ((1 - MOMENTUM) * rv + MOMENTUM * var * n / (n - 1)).detach()
        bufs[p + ".num_batches_tracked"] = nb + 1
    else:
        mean, var = rm, rv
        bufs[p + ".running_mean"], bufs[p + ".running_var"], bufs[p + ".num_batches_tracked"] = rm, rv, nb
    return (z - mean) / torch.sqrt(var + EPS) * sd[p + ".weight"] + sd[p + ".bias"], mean, var


def lrelu(v):
    return torch.where(v > 0, v, SLOPE * v)


def dense_levels(feats, sd, prefix, L, training, bufs):
    """feats [..., K0] -> (y_L [..., w_L], zs): the dense stack over the last dimension"""
    zs = []
    y = None
    for l in range(L):
        W = sd["%sdense_modules.%d.0.weight" % (prefix, l)]
        z = feats @ W.reshape(W.shape[0], W.shape[1]).t() + sd["%sdense_modules.%d.0.bias" % (prefix, l)]
        y = lrelu(batch_norm(z, sd, "%sdense_modules.%d.1" % (prefix, l), training, bufs)[0])
        feats = torch.cat([feats, y], dim=-1)
        zs.append(z)
    return y, zs


def dense_edge_forward(x, idx, k, sd, training):
    """-> dict(out [B,G,N], zs = the pre-norm z_l [B,N,k,G], bufs)"""
    L = len([n for n in sd if n.endswith(".0.weight")])
    bufs = {}
    y, zs = dense_levels(graph_feature(x, idx, k).permute(0, 2, 3, 1), sd, "", L, training, bufs)
    return dict(out=y.max(dim=2)[0].transpose(1, 2), zs=zs, bufs=bufs)


def dense_rows_forward(x, sd, training, prefix=""):
    L = len([n for n in sd if n.startswith(prefix + "dense_modules.") and n.endswith(".0.weight")])
    bufs = {}
    y, zs = dense_levels(x.transpose(1, 2), sd, prefix, L, training, bufs)
    return dict(out=y.transpose(1, 2), zs=zs, bufs=bufs)


def self_attn_forward(x, sd, prefix="atten."):
    """Common/utilities.py:226-245 as a formula: out[:, :, j] = gamma * sum_i softmax_i(q_i . k_j) v_i + x_j"""
    def conv(n):
        W = sd[prefix + n + ".weight"]
        return W.reshape(W.shape[0], W.shape[1]) @ x + sd[prefix + n + ".bias"].view(1, -1, 1)
    q, kk, v = conv("query"), conv("key"), conv("value")
    attn = torch.softmax(q.transpose(1, 2) @ kk, dim=1)
    return sd[prefix + "gamma"] * (v @ attn) + x


def dense_attn_forward(x, sd, training, res=True):
    f = dense_rows_forward(self_attn_forward(x, sd), sd, training, prefix="dense.")
    f["out"] = x + f["out"] if res else f["out"]
    return f


def run(tag, x, g, sd, idx=None, dtype=torch.float64):
    """One model forward + backward: -> dict with the golden's quantities (out, dx, grad|<parameter>, buf|<buffer>) and zs."""
    c = CASES[tag]
    kind = kind_of(tag)
    s = {}
    for n, v in sd.items():
        s[n] = v.to(dtype).clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in n else \
            (v.to(dtype) if v.dtype.is_floating_point else v.clone())
    xr = x.to(dtype).clone().requires_grad_(True)
    if kind == "edge":
        f = dense_edge_forward(xr, idx, c["k"], s, c["train"])
    elif kind == "rows":
        f = dense_rows_forward(xr, s, c["train"])
    else:
        f = dense_attn_forward(xr, s, c["train"])
    (f["out"] * g.to(dtype)).sum().backward()
    res = {"out": f["out"].detach(), "dx": xr.grad, "zs": [z.detach() for z in f["zs"]]}
    for n, v in s.items():
        if v.dtype.is_floating_point and v.requires_grad:
            res["grad|" + n] = v.grad if v.grad is not None else torch.zeros_like(v)
    for n, v in f["bufs"].items():
        res["buf|" + n] = v
    return res


# ----------------------------------------------------------------------------- the launchers, in float64
def level_model(A, W, raw_cols, scale, shift, bias=None, P=None, Q=None, idx=None, slope=SLOPE):
    """A [M,K] (or None), W [N,K], scale / shift [K]; P, Q [M/k, N], idx [M/k, k] -> Y [M,N]; every operand converted to float64"""
    d = lambda t: None if t is None else t.double().cpu()                    # noqa: E731
    A, W, scale, shift, bias, P, Q = d(A), d(W), d(scale), d(shift), d(bias), d(P), d(Q)
    Y = 0.0
    if A is not None:
        act = A * scale + shift
        act = torch.where(act > 0, act, slope * act)
        op = torch.cat([A[:, :raw_cols], act[:, raw_cols:]], dim=1)
        Y = op @ W.t()
    if bias is not None:
        Y = Y + bias
    if P is not None:
        k = idx.shape[1]
        Y = Y + (Q.unsqueeze(1) + P[idx.long().cpu()]).reshape(idx.shape[0] * k, -1)
    return Y


def scatter_model(D, idx):
    """D [M*k, C], idx [M,k] global rows -> [M, 2C] = [dP | dQ]"""
    D = D.double().cpu()
    M, k = idx.shape
    dQ = D.view(M, k, -1).sum(dim=1)
    dP = torch.zeros_like(dQ).index_add_(0, idx.long().cpu().reshape(-1), D)
    return torch.cat([dP, dQ], dim=1)


def bn_apply_model(g, z, mean, invstd, gamma, sums, count):
    g, z, mean, invstd, gamma, sums = (t.double().cpu() for t in (g, z, mean, invstd, gamma, sums))
    C = g.shape[1]
    return gamma * invstd * (g - sums[:C] / count - (z - mean) * invstd * sums[C:] / count)
