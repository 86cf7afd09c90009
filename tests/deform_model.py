"""A plain torch model of the decomposed full-rank edge convolution (spgan.modules.deform_edgeConv_simple / deform_edgeConv_first,
csrc/edge_rank.hip) and the case table of golden `deform.npz`.

With j = idx[i,r] and W1 = [Wc | Wd] (Generation/modules.py:1394-1466, get_edge_features :683-725: the central half first):

    z(i,r,:) = P[j] + Q[i],   P = x Wd^T,   Q = x (Wc - Wd)^T + b1              inte_conv_hk's Conv2d(2Fin -> F1, 1x1)
    h(i,r,:) = lrelu(scale1 * z + shift1)                                       BatchNorm2d over the E = M*k edges
    y(i,:)   = b2 + sum_r W2[:,:,0,r] h(i,r,:)                                  conv2's Conv2d(F1 -> Fout, [1,k]):  h.flat @ W2i^T
    out      = relu(bn2(y))                                                     statistics over the M points

The model materialises h: it is the yardstick, evaluated in float64 or float32, not the memory behaviour."""
import numpy as np
import torch

EPS, MOMENTUM, SLOPE = 1e-5, 0.1, 0.01

# tag -> class, Fin, Fout, k, B, N, train, every third bn.weight negated, non-initial running statistics
CASES = {
    "simple/xyz":  dict(cls="simple", Fin=3, Fout=16, k=4, B=2, N=48, train=True, neg=False, warm=False),
    "simple/feat": dict(cls="simple", Fin=16, Fout=32, k=10, B=2, N=64, train=True, neg=True, warm=False),
    "simple/eval": dict(cls="simple", Fin=8, Fout=8, k=6, B=3, N=40, train=False, neg=False, warm=True),
    "simple/k1":   dict(cls="simple", Fin=4, Fout=4, k=1, B=2, N=32, train=True, neg=False, warm=False),
    "first/odd":   dict(cls="first", Fin=7, Fout=12, k=5, B=2, N=40, train=True, neg=False, warm=False),
}
STATE_KEYS = ("conv2.conv.weight", "conv2.conv.bias", "conv2.bn.weight", "conv2.bn.bias", "conv2.bn.running_mean", "conv2.bn.running_var",
              "conv2.bn.num_batches_tracked", "inte_conv_hk.0.weight", "inte_conv_hk.0.bias", "inte_conv_hk.1.weight", "inte_conv_hk.1.bias",
              "inte_conv_hk.1.running_mean", "inte_conv_hk.1.running_var", "inte_conv_hk.1.num_batches_tracked")
BUFFERS = tuple(n for n in STATE_KEYS if "running" in n or "num_batches" in n)
ZERO_GRAD_BIASES = ("conv2.conv.bias", "inte_conv_hk.0.bias")      # in front of a train-mode BatchNorm


def widths(c):
    """(F1, Fout) of a case: F1 = Fout for deform_edgeConv_simple, Fin for deform_edgeConv_first."""
    return (c["Fout"] if c["cls"] == "simple" else c["Fin"]), c["Fout"]


def out_shape(c):
    return (c["B"], c["Fout"], c["N"]) if c["cls"] == "simple" else (c["B"], c["Fout"], c["N"], 1, 1)


def case_tensors(tag, seed=0):
    """(x [B,Fin,N], cotangent of the output's shape, state_dict) of a case, from spgan.fixture_rng (float32)."""
    from spgan import fixture_rng as fr
    c = CASES[tag]
    C, k = c["Fin"], c["k"]
    F1, F = widths(c)
    name = "deform.%s" % tag
    if C <= 4:
        x = fr.uniform(name + ".x", (c["B"], C, c["N"]), -1.0, 1.0, salt=seed)
    else:
        x = fr.normal(name + ".x", (c["B"], C, c["N"]), 0.7, salt=seed)
    g = fr.normal(name + ".g", out_shape(c), salt=seed)
    b1, b2 = 1.0 / np.sqrt(2 * C), 1.0 / np.sqrt(F1 * k)
    sd = {
        "conv2.conv.weight": fr.uniform(name + ".W2", (F, F1, 1, k), -b2, b2, salt=seed),
        "conv2.conv.bias": fr.uniform(name + ".b2", (F,), -b2, b2, salt=seed),
        "conv2.bn.weight": fr.uniform(name + ".gamma2", (F,), 0.5, 1.5, salt=seed),
        "conv2.bn.bias": fr.uniform(name + ".beta2", (F,), -0.2, 0.2, salt=seed),
        "conv2.bn.running_mean": torch.zeros(F),
        "conv2.bn.running_var": torch.ones(F),
        "conv2.bn.num_batches_tracked": torch.tensor(0, dtype=torch.int64),
        "inte_conv_hk.0.weight": fr.uniform(name + ".W1", (F1, 2 * C, 1, 1), -b1, b1, salt=seed),
        "inte_conv_hk.0.bias": fr.uniform(name + ".b1", (F1,), -b1, b1, salt=seed),
        "inte_conv_hk.1.weight": fr.uniform(name + ".gamma1", (F1,), 0.5, 1.5, salt=seed),
        "inte_conv_hk.1.bias": fr.uniform(name + ".beta1", (F1,), -0.2, 0.2, salt=seed),
        "inte_conv_hk.1.running_mean": torch.zeros(F1),
        "inte_conv_hk.1.running_var": torch.ones(F1),
        "inte_conv_hk.1.num_batches_tracked": torch.tensor(0, dtype=torch.int64),
    }
    if c["neg"]:
        sd["conv2.bn.weight"][::3] *= -1.0
        sd["inte_conv_hk.1.weight"][::3] *= -1.0
    if c["warm"]:
        sd["conv2.bn.running_mean"] = fr.normal(name + ".rm2", (F,), 0.1, salt=seed)
        sd["conv2.bn.running_var"] = fr.uniform(name + ".rv2", (F,), 0.5, 1.5, salt=seed)
        sd["conv2.bn.num_batches_tracked"] = torch.tensor(21, dtype=torch.int64)
        sd["inte_conv_hk.1.running_mean"] = fr.normal(name + ".rm1", (F1,), 0.1, salt=seed)
        sd["inte_conv_hk.1.running_var"] = fr.uniform(name + ".rv1", (F1,), 0.5, 1.5, salt=seed)
        sd["inte_conv_hk.1.num_batches_tracked"] = torch.tensor(21, dtype=torch.int64)
    return x, g, sd


def golden_state_dict(d, tag):
    return {n: torch.from_numpy(np.asarray(d["%s|param|%s" % (tag, n)])) for n in STATE_KEYS}


def golden_f64(d, tag, q):
    """The reference's float64 result of quantity q: the golden stores it as its (float32-rounded) distance from the float32 run."""
    return torch.from_numpy(np.asarray(d["%s|%s|full" % (tag, q)])).double() + torch.from_numpy(np.asarray(d["%s|%s|d64|full" % (tag, q)])).double()


# --------------------------------------------------------------------------------------------- the launchers (csrc/edge_rank.hip)
def pre_norm(PQ, gidx):
    """PQ [M,2F1] = [P | Q], gidx int64 [M,k] global rows -> z [M,k,F1] = Q_i + P_j"""
    F1 = PQ.shape[1] // 2
    return PQ[:, None, F1:] + PQ[gidx][:, :, :F1]


def lrelu(a):
    return torch.where(a > 0, a, a * SLOPE)


def rank_h(PQ, gidx, scale1, shift1):
    """-> (h [M,k,F1], a = scale1*z + shift1, z)"""
    z = pre_norm(PQ, gidx)
    a = z * scale1 + shift1
    return lrelu(a), a, z


def rank_gemm(PQ, gidx, scale1, shift1, W2i, b2=None):
    """-> y [M,O]; W2i [O, k*F1] tap-major"""
    h = rank_h(PQ, gidx, scale1, shift1)[0]
    y = h.reshape(h.shape[0], -1) @ W2i.t()
    return y if b2 is None else y + b2


def rank_wgrad(PQ, gidx, scale1, shift1, dy):
    """dy [M,O] -> dW2i [O, k*F1]"""
    h = rank_h(PQ, gidx, scale1, shift1)[0]
    return dy.t() @ h.reshape(h.shape[0], -1)


def rank_dgrad(dy, W2i, PQ, gidx, scale1, shift1, mean1, invstd1):
    """-> (da [M,k,F1], sums [2F1] = [sum da | sum da*zhat])"""
    _, a, z = rank_h(PQ, gidx, scale1, shift1)
    M, k, F1 = a.shape
    da = (dy @ W2i).view(M, k, F1) * torch.where(a > 0, torch.ones_like(a), torch.full_like(a, SLOPE))
    zhat = (z - mean1) * invstd1
    return da, torch.cat([da.sum(dim=(0, 1)), (da * zhat).sum(dim=(0, 1))])


def rank_scatter(da, gidx, scale1, PQ=None, mean1=None, invstd1=None, sums=None):
    """-> dPQ [M,2F1] = [dP | dQ]; sums given: train mode (the BatchNorm correction), else eval mode"""
    M, k, F1 = da.shape
    dz = da
    if sums is not None:
        E = M * k
        zhat = (pre_norm(PQ, gidx) - mean1) * invstd1
        dz = da - sums[:F1] / E - zhat * sums[F1:] / E
    dz = dz * scale1
    dP = torch.zeros(M, F1, dtype=da.dtype).index_add(0, gidx.reshape(-1), dz.reshape(M * k, F1))
    return torch.cat([dP, dz.sum(dim=1)], dim=1)


def colstats(Y):
    mean = Y.mean(dim=0)
    var = ((Y - mean) ** 2).mean(dim=0)
    return mean, var


# --------------------------------------------------------------------------------------------- the layer
def images(W1, W2):
    """W1 [F1,2Fin,1,1], W2 [Fout,F1,1,k] -> Wst [2F1,Fin] = [Wd ; Wc - Wd], W2i [Fout, k*F1] (column r*F1 + c)"""
    F1, Fin = W1.shape[0], W1.shape[1] // 2
    Wm = W1.reshape(F1, 2 * Fin)
    Wd = Wm[:, Fin:]
    return torch.cat([Wd, Wm[:, :Fin] - Wd], dim=0), W2[:, :, 0, :].permute(0, 2, 1).reshape(W2.shape[0], -1)


def global_idx(idx, B, N, k):
    return (idx.view(B, N, k) + torch.arange(B, device=idx.device).view(B, 1, 1) * N).view(B * N, k)


def _bn(Y, gamma, beta, rm, rv, training, eps, momentum):
    n = Y.shape[0]
    if training:
        mean, var = colstats(Y)
        new_rm = (1 - momentum) * rm + momentum * mean
        new_rv = (1 - momentum) * rv + momentum * var * n / (n - 1)
    else:
        mean, var, new_rm, new_rv = rm, rv, rm, rv
    invstd = 1.0 / torch.sqrt(var + eps)
    a = gamma * invstd
    return dict(mean=mean, var=var, invstd=invstd, a=a, s=beta - a * mean, running_mean=new_rm, running_var=new_rv)


def forward(x, idx, k, sd, training, eps=EPS, momentum=MOMENTUM):
    """x [B,Fin,N], idx int64 [B,N*k] local, sd = the state_dict in the dtype the model is to run in -> dict (out is [B,Fout,N])."""
    B, C, N = x.shape
    M = B * N
    W1, W2 = sd["inte_conv_hk.0.weight"], sd["conv2.conv.weight"]
    F1, Fout = W1.shape[0], W2.shape[0]
    Wst, W2i = images(W1, W2)
    xp = x.transpose(1, 2).reshape(M, C)
    gidx = global_idx(idx, B, N, k)
    PQ = xp @ Wst.t() + torch.cat([torch.zeros_like(sd["inte_conv_hk.0.bias"]), sd["inte_conv_hk.0.bias"]])
    bn1 = _bn(pre_norm(PQ, gidx).reshape(M * k, F1), sd["inte_conv_hk.1.weight"], sd["inte_conv_hk.1.bias"], sd["inte_conv_hk.1.running_mean"],
              sd["inte_conv_hk.1.running_var"], training, eps, momentum)
    Y = rank_gemm(PQ, gidx, bn1["a"], bn1["s"], W2i, sd["conv2.conv.bias"])
    bn2 = _bn(Y, sd["conv2.bn.weight"], sd["conv2.bn.bias"], sd["conv2.bn.running_mean"], sd["conv2.bn.running_var"], training, eps, momentum)
    out_pm = torch.relu(Y * bn2["a"] + bn2["s"])
    return dict(out=out_pm.view(B, N, Fout).transpose(1, 2), out_pm=out_pm, PQ=PQ, Y=Y, bn1=bn1, bn2=bn2, xp=xp, gidx=gidx, k=k, C=C, B=B, N=N,
                training=training, Wst=Wst, W2i=W2i, W1=W1, W2=W2)


def backward(f, g):
    """The closed-form backward for cotangent g [B,Fout,N] -> dict(dx, grad|<parameter>...)."""
    B, N, C, k = f["B"], f["N"], f["C"], f["k"]
    M = B * N
    Wst, W2i, PQ, gidx, bn1, bn2 = f["Wst"], f["W2i"], f["PQ"], f["gidx"], f["bn1"], f["bn2"]
    Fout, F1 = W2i.shape[0], Wst.shape[0] // 2
    train = f["training"]
    g_pm = g.reshape(B, Fout, N).transpose(1, 2).reshape(M, Fout)
    r = g_pm * (f["out_pm"] > 0).to(g.dtype)
    xh2 = (f["Y"] - bn2["mean"]) * bn2["invstd"]
    s1, s2 = r.sum(dim=0), (r * xh2).sum(dim=0)
    dy = bn2["a"] * (r - s1 / M - xh2 * s2 / M) if train else bn2["a"] * r
    dW2i = rank_wgrad(PQ, gidx, bn1["a"], bn1["s"], dy)
    da, sums1 = rank_dgrad(dy, W2i, PQ, gidx, bn1["a"], bn1["s"], bn1["mean"], bn1["invstd"])
    dPQ = rank_scatter(da, gidx, bn1["a"], PQ, bn1["mean"], bn1["invstd"], sums1 if train else None)
    dWst = dPQ.t() @ f["xp"]
    dW1 = torch.cat([dWst[F1:], dWst[:F1] - dWst[F1:]], dim=1).view(F1, 2 * C, 1, 1)
    dx_pm = dPQ @ Wst
    return {"dx": dx_pm.view(B, N, C).transpose(1, 2), "grad|conv2.conv.weight": dW2i.view(Fout, k, F1).permute(0, 2, 1).unsqueeze(2),
            "grad|conv2.conv.bias": dy.sum(dim=0), "grad|conv2.bn.weight": s2, "grad|conv2.bn.bias": s1, "grad|inte_conv_hk.0.weight": dW1,
            "grad|inte_conv_hk.0.bias": dPQ[:, F1:].sum(dim=0), "grad|inte_conv_hk.1.weight": sums1[F1:], "grad|inte_conv_hk.1.bias": sums1[:F1],
            "dy": dy, "da": da, "dPQ": dPQ}
