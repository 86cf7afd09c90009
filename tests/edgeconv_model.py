"""A plain torch model of the decomposed max-aggregation edge convolution (spgan.modules.edgeConv, csrc/edge_max.hip; DESIGN.md
section 18) and the case table of golden `edgeconv.npz`.

    y(i,j,c) = Q(i,c) + P(n(i,j),c),   P = Wd x,   Q = (Wc - Wd) x + b,   W = [Wc | Wd]
    out(i,c) = relu(a_c (Q + ext_j P_n) + s_c),   ext = max for a_c >= 0, min for a_c < 0,   a = gamma invstd,   s = beta - a mean

The model DOES materialise P over the neighbours ([B,N,k,F]): it is the yardstick, evaluated in float64 on the CPU (or wherever its
inputs live), not the algorithm's memory behaviour.  `backward` is the closed form of the issue, with the selection either the
model's own or one handed in (the kernel's), so that everything behind the discrete choice is compared tightly."""
import numpy as np
import torch

EPS, MOMENTUM = 1e-5, 0.1

# tag -> Fin, Fout, k, B, N, train, number of negative bn.weight entries, non-initial running statistics
CASES = {
    "xyz":   dict(Fin=3, Fout=16, k=8, B=2, N=64, train=True, neg=0, warm=False),
    "feat":  dict(Fin=16, Fout=32, k=10, B=2, N=128, train=True, neg=0, warm=False),
    "eval":  dict(Fin=16, Fout=32, k=10, B=2, N=128, train=False, neg=0, warm=True),
    "neg":   dict(Fin=16, Fout=32, k=10, B=2, N=128, train=True, neg=7, warm=True),
}
PARAMS = ("conv.conv.weight", "conv.conv.bias", "conv.bn.weight", "conv.bn.bias")
BUFFERS = ("conv.bn.running_mean", "conv.bn.running_var", "conv.bn.num_batches_tracked")


def case_tensors(tag, seed=0):
    """(x [B,Fin,N], cotangent [B,Fout,N], state_dict) of a case, from spgan.fixture_rng (float32)."""
    from spgan import fixture_rng as fr
    c = CASES[tag]
    Fin, F = c["Fin"], c["Fout"]
    name = "edgeconv.%s" % tag
    if Fin <= 4:
        x = fr.uniform(name + ".x", (c["B"], Fin, c["N"]), -1.0, 1.0, salt=seed)
    else:
        x = fr.normal(name + ".x", (c["B"], Fin, c["N"]), 0.7, salt=seed)
    g = fr.normal(name + ".g", (c["B"], F, c["N"]), salt=seed)
    bound = 1.0 / np.sqrt(2 * Fin)
    sd = {
        "conv.conv.weight": fr.uniform(name + ".W", (F, 2 * Fin, 1, 1), -bound, bound, salt=seed),
        "conv.conv.bias": fr.uniform(name + ".b", (F,), -bound, bound, salt=seed),
        "conv.bn.weight": fr.uniform(name + ".gamma", (F,), 0.5, 1.5, salt=seed),
        "conv.bn.bias": fr.uniform(name + ".beta", (F,), -0.2, 0.2, salt=seed),
        "conv.bn.running_mean": torch.zeros(F),
        "conv.bn.running_var": torch.ones(F),
        "conv.bn.num_batches_tracked": torch.tensor(0, dtype=torch.int64),
    }
    if c["neg"]:
        which = torch.from_numpy(np.random.default_rng(seed + 5).permutation(F)[:c["neg"]].copy())
        sd["conv.bn.weight"][which] *= -1.0
    if c["warm"]:
        sd["conv.bn.running_mean"] = fr.normal(name + ".rm", (F,), 0.1, salt=seed)
        sd["conv.bn.running_var"] = fr.uniform(name + ".rv", (F,), 0.5, 1.5, salt=seed)
        sd["conv.bn.num_batches_tracked"] = torch.tensor(21, dtype=torch.int64)
    return x, g, sd


def golden_state_dict(d, tag):
    return {n: torch.from_numpy(np.asarray(d["%s|param|%s" % (tag, n)])) for n in PARAMS + BUFFERS}


def golden_f64(d, tag, q):
    """The reference's float64 result of quantity q: the golden stores it as its (float32-rounded) distance from the float32 run."""
    return torch.from_numpy(np.asarray(d["%s|%s|full" % (tag, q)])).double() + torch.from_numpy(np.asarray(d["%s|%s|d64|full" % (tag, q)])).double()


def gather_neighbours(P, idx, k):
    """P [B,N,F], idx int64 [B,N*k] local -> [B,N,k,F]"""
    B, N, F = P.shape
    nb = idx.view(B, N, k)
    return P[torch.arange(B, device=P.device).view(B, 1, 1), nb]


def forward_pq(P, Q, idx, k, gamma, beta, rm, rv, training, eps=EPS, momentum=MOMENTUM):
    """Everything behind the per-point GEMM: P, Q [B,N,F], idx int64 [B,N*k] -> dict (out is [B,N,F] here)."""
    B, N, F = P.shape
    Pn = gather_neighbours(P, idx, k)                        # [B,N,k,F]
    E = B * N * k
    if training:
        y = Q.unsqueeze(2) + Pn
        mean = y.mean(dim=(0, 1, 2))
        var = ((y - mean) ** 2).mean(dim=(0, 1, 2))
        new_rm = (1 - momentum) * rm + momentum * mean
        new_rv = (1 - momentum) * rv + momentum * var * E / (E - 1)
    else:
        mean, var, new_rm, new_rv = rm, rv, rm, rv
    invstd = 1.0 / torch.sqrt(var + eps)
    a = gamma * invstd
    s = beta - a * mean
    pmax, jmax = Pn.max(dim=2)
    pmin, jmin = Pn.min(dim=2)
    up = (a >= 0).view(1, 1, F)
    psel = torch.where(up, pmax, pmin)
    sel = torch.where(up, jmax, jmin)
    out = torch.relu(a * (Q + psel) + s)
    return dict(out_pm=out, sel=sel, P=P, Q=Q, Pn=Pn, psum=Pn.sum(dim=2), pmax=pmax, pmin=pmin, jmax=jmax, jmin=jmin, a=a, s=s,
                mean=mean, var=var, invstd=invstd, running_mean=new_rm, running_var=new_rv, training=training, k=k, idx=idx)


def forward(x, idx, k, W, b, gamma, beta, rm, rv, training, eps=EPS, momentum=MOMENTUM):
    """x [B,Fin,N], idx int64 [B,N*k]; every tensor in the dtype the model is to run in.  -> dict (out is [B,F,N])."""
    B, Fin, N = x.shape
    F = W.shape[0]
    W2 = W.reshape(F, 2 * Fin)
    Wc, Wd = W2[:, :Fin], W2[:, Fin:]
    xp = x.transpose(1, 2)                                   # [B,N,Fin]
    f = forward_pq(xp @ Wd.t(), xp @ (Wc - Wd).t() + b, idx, k, gamma, beta, rm, rv, training, eps, momentum)
    f.update(out=f["out_pm"].transpose(1, 2), x=x, W2=W2)
    return f


def backward_pq(f, g_pm, sel=None, active=None):
    """The closed form behind the GEMMs: cotangent g_pm [B,N,F] -> dict(dP, dQ [B,N,F], dgamma, dbeta, r).
    sel [B,N,F] (ranks) / active [B,N,F] (bool): the selection and the ReLU mask to use instead of the model's own."""
    P, Q, Pn, a, mean, invstd, k, idx = (f[n] for n in ("P", "Q", "Pn", "a", "mean", "invstd", "k", "idx"))
    B, N, F = P.shape
    E = B * N * k
    sel = f["sel"] if sel is None else sel
    active = (f["out_pm"] > 0) if active is None else active
    r = g_pm * active.to(g_pm.dtype)
    psel = torch.gather(Pn, 2, sel.unsqueeze(2)).squeeze(2)
    xhat_sel = (Q + psel - mean) * invstd
    s1 = r.sum(dim=(0, 1))
    s2 = (r * xhat_sel).sum(dim=(0, 1))
    nb = idx.view(B, N, k)
    chosen = torch.gather(nb.unsqueeze(3).expand(B, N, k, F), 2, sel.unsqueeze(2)).squeeze(2)        # [B,N,F]: the selected neighbour
    T1 = torch.zeros_like(P).scatter_add_(1, chosen, r)
    if f["training"]:
        deg = torch.zeros(B, N, dtype=P.dtype, device=P.device).scatter_add_(1, idx, torch.ones(B, N * k, dtype=P.dtype, device=P.device)).unsqueeze(2)
        SQ = torch.zeros_like(P).scatter_add_(1, idx.unsqueeze(2).expand(B, N * k, F), Q.unsqueeze(2).expand(B, N, k, F).reshape(B, N * k, F))
        dQ = a * (r - k * s1 / E - (s2 / E) * invstd * (k * Q + f["psum"] - k * mean))
        dP = a * (T1 - deg * s1 / E - (s2 / E) * invstd * (SQ + deg * (P - mean)))
    else:
        dQ, dP = a * r, a * T1
    return dict(dP=dP, dQ=dQ, dgamma=s2, dbeta=s1, r=r)


def backward(f, g, sel=None, active=None):
    """The whole closed-form backward for cotangent g [B,F,N] -> dict(dx, dW, db, dgamma, dbeta, dP, dQ, r)."""
    x, W2 = f["x"], f["W2"]
    F, Fin = W2.shape[0], x.shape[1]
    o = backward_pq(f, g.transpose(1, 2), sel, active)
    dP, dQ = o["dP"], o["dQ"]
    Wc, Wd = W2[:, :Fin], W2[:, Fin:]
    xp = x.transpose(1, 2)
    dWp = torch.einsum("bnf,bnc->fc", dP, xp)
    dWq = torch.einsum("bnf,bnc->fc", dQ, xp)
    o.update(dx=(dP @ Wd + dQ @ (Wc - Wd)).transpose(1, 2), dW=torch.cat([dWq, dWp - dWq], dim=1).view(F, 2 * Fin, 1, 1), db=dQ.sum(dim=(0, 1)))
    return o


def composition(x, idx, k, W, b, gamma, beta, rm, rv, training, eps=EPS):
    """The materialised route in plain torch (what a user had to write before): edge tensor -> matmul -> batch norm -> relu -> max.
    -> (out [B,F,N], y [B,N,k,F] pre-norm)."""
    B, Fin, N = x.shape
    F = W.shape[0]
    xp = x.transpose(1, 2)
    nbr = gather_neighbours(xp, idx, k)                                           # [B,N,k,Fin]
    cen = xp.unsqueeze(2).expand(B, N, k, Fin)
    ee = torch.cat([cen, nbr - cen], dim=3)
    y = ee @ W.reshape(F, 2 * Fin).t() + b
    if training:
        mean = y.mean(dim=(0, 1, 2))
        var = ((y - mean) ** 2).mean(dim=(0, 1, 2))
    else:
        mean, var = rm, rv
    z = torch.relu((y - mean) / torch.sqrt(var + eps) * gamma + beta)
    return z.max(dim=2)[0].transpose(1, 2), y
