"""A plain torch model of the decomposed upsampling edge convolution (spgan.modules.upsample_edgeConv, csrc/edge_window.hip; DESIGN.md
section 19) and the case table of golden `upsample.npz`.

With d(i,j) = x_n(i,j) - x_i, w = k//2 + 1, T = k - w + 1 = k/2 (Generation/modules.py:799-845):

    u(i,t,:) = (sum_r Wc_r) x_i + b1 + sum_{r<w} Wd_r d(i,t+r)                      inte_conv_hk's Conv2d(2C -> 4C, [1,w])
    a(i,t,:) = lrelu(bn1(u))                                                        statistics over the M*T rows
    y(i,:)   = (sum_{j<k} Vc_j) x_i + b2 + sum_{j<k} Vd_j d(i,j) + V2p a(i).flat    conv2's Conv2d(2C -> 2Fout, [1,2k]) on cat(ee, inte)
    out      = relu(bn2(y)),  out[b, f, s*N + n] = y[b, 2f+s, n]

The reference's transpose / view chain between the two convolutions reads, per point, the flat (4C, T) block in order o*T + t as
(2C, k) in order c'*k + j and moves no data; with u stored as rows (i,t) it is the column permutation `images()` applies to conv2's
last k taps.  The model materialises the differences: it is the yardstick, evaluated in float64, not the memory behaviour."""
import numpy as np
import torch

EPS, MOMENTUM, SLOPE = 1e-5, 0.1, 0.01

# tag -> Fin, Fout, k, B, N, train, every third bn.weight negated, non-initial running statistics
CASES = {
    "xyz":  dict(Fin=3, Fout=16, k=4, B=2, N=48, train=True, neg=False, warm=False),
    "feat": dict(Fin=16, Fout=32, k=10, B=2, N=64, train=True, neg=True, warm=False),
    "eval": dict(Fin=8, Fout=8, k=6, B=3, N=40, train=False, neg=False, warm=True),
    "k2":   dict(Fin=4, Fout=4, k=2, B=2, N=32, train=True, neg=False, warm=False),
}
XYZ_CASE = dict(C=8, k=4, B=2, N=48)          # get_edge_features_xyz
PARAMS = ("conv2.conv.weight", "conv2.conv.bias", "conv2.bn.weight", "conv2.bn.bias",
          "inte_conv_hk.0.weight", "inte_conv_hk.0.bias", "inte_conv_hk.1.weight", "inte_conv_hk.1.bias")
BUFFERS = ("conv2.bn.running_mean", "conv2.bn.running_var", "conv2.bn.num_batches_tracked",
           "inte_conv_hk.1.running_mean", "inte_conv_hk.1.running_var", "inte_conv_hk.1.num_batches_tracked")
STATE_KEYS = ("conv2.conv.weight", "conv2.conv.bias", "conv2.bn.weight", "conv2.bn.bias", "conv2.bn.running_mean", "conv2.bn.running_var",
              "conv2.bn.num_batches_tracked", "inte_conv_hk.0.weight", "inte_conv_hk.0.bias", "inte_conv_hk.1.weight", "inte_conv_hk.1.bias",
              "inte_conv_hk.1.running_mean", "inte_conv_hk.1.running_var", "inte_conv_hk.1.num_batches_tracked")
ZERO_GRAD_BIASES = ("conv2.conv.bias", "inte_conv_hk.0.bias")      # in front of a train-mode BatchNorm


def case_tensors(tag, seed=0):
    """(x [B,Fin,N], cotangent [B,Fout,2N], state_dict) of a case, from spgan.fixture_rng (float32)."""
    from spgan import fixture_rng as fr
    c = CASES[tag]
    C, F, k = c["Fin"], c["Fout"], c["k"]
    w = k // 2 + 1
    name = "upsample.%s" % tag
    if C <= 4:
        x = fr.uniform(name + ".x", (c["B"], C, c["N"]), -1.0, 1.0, salt=seed)
    else:
        x = fr.normal(name + ".x", (c["B"], C, c["N"]), 0.7, salt=seed)
    g = fr.normal(name + ".g", (c["B"], F, 2 * c["N"]), salt=seed)
    b1, b2 = 1.0 / np.sqrt(2 * C * w), 1.0 / np.sqrt(2 * C * 2 * k)
    sd = {
        "conv2.conv.weight": fr.uniform(name + ".V", (2 * F, 2 * C, 1, 2 * k), -b2, b2, salt=seed),
        "conv2.conv.bias": fr.uniform(name + ".b2", (2 * F,), -b2, b2, salt=seed),
        "conv2.bn.weight": fr.uniform(name + ".gamma2", (2 * F,), 0.5, 1.5, salt=seed),
        "conv2.bn.bias": fr.uniform(name + ".beta2", (2 * F,), -0.2, 0.2, salt=seed),
        "conv2.bn.running_mean": torch.zeros(2 * F),
        "conv2.bn.running_var": torch.ones(2 * F),
        "conv2.bn.num_batches_tracked": torch.tensor(0, dtype=torch.int64),
        "inte_conv_hk.0.weight": fr.uniform(name + ".W1", (4 * C, 2 * C, 1, w), -b1, b1, salt=seed),
        "inte_conv_hk.0.bias": fr.uniform(name + ".b1", (4 * C,), -b1, b1, salt=seed),
        "inte_conv_hk.1.weight": fr.uniform(name + ".gamma1", (4 * C,), 0.5, 1.5, salt=seed),
        "inte_conv_hk.1.bias": fr.uniform(name + ".beta1", (4 * C,), -0.2, 0.2, salt=seed),
        "inte_conv_hk.1.running_mean": torch.zeros(4 * C),
        "inte_conv_hk.1.running_var": torch.ones(4 * C),
        "inte_conv_hk.1.num_batches_tracked": torch.tensor(0, dtype=torch.int64),
    }
    if c["neg"]:
        sd["conv2.bn.weight"][::3] *= -1.0
        sd["inte_conv_hk.1.weight"][::3] *= -1.0
    if c["warm"]:
        sd["conv2.bn.running_mean"] = fr.normal(name + ".rm2", (2 * F,), 0.1, salt=seed)
        sd["conv2.bn.running_var"] = fr.uniform(name + ".rv2", (2 * F,), 0.5, 1.5, salt=seed)
        sd["conv2.bn.num_batches_tracked"] = torch.tensor(21, dtype=torch.int64)
        sd["inte_conv_hk.1.running_mean"] = fr.normal(name + ".rm1", (4 * C,), 0.1, salt=seed)
        sd["inte_conv_hk.1.running_var"] = fr.uniform(name + ".rv1", (4 * C,), 0.5, 1.5, salt=seed)
        sd["inte_conv_hk.1.num_batches_tracked"] = torch.tensor(21, dtype=torch.int64)
    return x, g, sd


def xyz_tensors(seed=0):
    """(x [B,C,N], pc [B,3,N], cotangents of e_fea and e_xyz) for get_edge_features_xyz."""
    from spgan import fixture_rng as fr
    c = XYZ_CASE
    x = fr.normal("upsample.xyzfn.x", (c["B"], c["C"], c["N"]), 0.7, salt=seed)
    pc = fr.uniform("upsample.xyzfn.pc", (c["B"], 3, c["N"]), -1.0, 1.0, salt=seed)
    gf = fr.normal("upsample.xyzfn.gf", (c["B"], 2 * c["C"], c["N"], c["k"]), salt=seed)
    gx = fr.normal("upsample.xyzfn.gx", (c["B"], 6, c["N"], c["k"]), salt=seed)
    return x, pc, gf, gx


def golden_state_dict(d, tag):
    return {n: torch.from_numpy(np.asarray(d["%s|param|%s" % (tag, n)])) for n in STATE_KEYS}


def golden_f64(d, tag, q):
    """The reference's float64 result of quantity q: the golden stores it as its (float32-rounded) distance from the float32 run."""
    return torch.from_numpy(np.asarray(d["%s|%s|full" % (tag, q)])).double() + torch.from_numpy(np.asarray(d["%s|%s|d64|full" % (tag, q)])).double()


# --------------------------------------------------------------------------------------------- the launchers (csrc/edge_window.hip)
def differences(x_pm, gidx):
    """x_pm [M,C], gidx int64 [M,k] global rows -> d [M,k,C]"""
    return x_pm[gidx] - x_pm[:, None, :]


def windows(D, w):
    """d [M,k,C] -> the A operand [M,T,w*C]: row (i,t) = [d(i,t) | ... | d(i,t+w-1)]"""
    M, k, C = D.shape
    return torch.stack([D[:, t:t + w, :].reshape(M, w * C) for t in range(k - w + 1)], dim=1)


def window_gemm(x_pm, gidx, W, w, rowadd=None, add2=None):
    """-> Y [M*T, O]; W [O, w*C] tap-major"""
    A = windows(differences(x_pm, gidx), w)
    M, T, _ = A.shape
    Y = A @ W.t()
    if rowadd is not None:
        Y = Y + rowadd[:, None, :]
    Y = Y.reshape(M * T, -1)
    return Y if add2 is None else Y + add2


def window_wgrad(x_pm, gidx, G, w):
    """G [M*T, O] -> dW [O, w*C]"""
    A = windows(differences(x_pm, gidx), w)
    M, T, K = A.shape
    return G.t() @ A.reshape(M * T, K)


def window_dgrad(G, W, k, C, w):
    """G [M*T, O], W [O, w*C] -> S [M,k,C] with S(i,j) = sum_{t+r=j} G(i,t) W_r"""
    T = k - w + 1
    M = G.shape[0] // T
    Z = (G @ W).view(M, T, w, C)
    S = torch.zeros(M, k, C, dtype=G.dtype, device=G.device)
    for t in range(T):
        S[:, t:t + w, :] += Z[:, t]
    return S


def window_scatter(S, gidx, add_a=None, add_b=None):
    """-> dx [M,C] = addends - sum_j S(i,j) + sum over the in-edges"""
    M, k, C = S.shape
    dx = -S.sum(dim=1)
    dx = dx.index_add(0, gidx.reshape(-1), S.reshape(M * k, C))
    for a in (add_a, add_b):
        if a is not None:
            dx = dx + a
    return dx


def colstats(Y):
    mean = Y.mean(dim=0)
    var = ((Y - mean) ** 2).mean(dim=0)
    return mean, var


# --------------------------------------------------------------------------------------------- the layer
def images(W1, V, C, k):
    """The operand images of the two conv weights.  W1 [4C,2C,1,w], V [2Fout,2C,1,2k] ->
    Wc1 [4C,C], Wd1 [4C,w*C], Vc [F2,C], Vd [F2,k*C], V2p [F2, T*4C] (column t*4C + o = conv2 column (c',k+j) with c'*k + j = o*T + t)."""
    w = W1.shape[3]
    T = k - w + 1
    F2 = V.shape[0]
    Wc1 = W1[:, :C, 0, :].sum(dim=2)
    Wd1 = W1[:, C:, 0, :].permute(0, 2, 1).reshape(4 * C, w * C)
    Vc = V[:, :C, 0, :k].sum(dim=2)
    Vd = V[:, C:, 0, :k].permute(0, 2, 1).reshape(F2, k * C)
    V2p = V[:, :, 0, k:].reshape(F2, 4 * C, T).permute(0, 2, 1).reshape(F2, T * 4 * C)
    return Wc1, Wd1, Vc, Vd, V2p


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
    """x [B,C,N], idx int64 [B,N*k] local, sd = the state_dict in the dtype the model is to run in -> dict (out is [B,Fout,2N])."""
    B, C, N = x.shape
    M = B * N
    W1, V = sd["inte_conv_hk.0.weight"], sd["conv2.conv.weight"]
    w = W1.shape[3]
    T = k - w + 1
    F2 = V.shape[0]
    Wc1, Wd1, Vc, Vd, V2p = images(W1, V, C, k)
    xp = x.transpose(1, 2).reshape(M, C)
    gidx = global_idx(idx, B, N, k)
    Q1 = xp @ Wc1.t() + sd["inte_conv_hk.0.bias"]
    U = window_gemm(xp, gidx, Wd1, w, rowadd=Q1)                                    # [M*T, 4C]
    bn1 = _bn(U, sd["inte_conv_hk.1.weight"], sd["inte_conv_hk.1.bias"], sd["inte_conv_hk.1.running_mean"], sd["inte_conv_hk.1.running_var"],
              training, eps, momentum)
    Z1 = U * bn1["a"] + bn1["s"]
    A1 = torch.where(Z1 > 0, Z1, Z1 * SLOPE)
    Q2 = xp @ Vc.t() + sd["conv2.conv.bias"]
    Y3 = A1.reshape(M, T * 4 * C) @ V2p.t()
    Y = window_gemm(xp, gidx, Vd, k, rowadd=Q2, add2=Y3)                            # [M, F2]
    bn2 = _bn(Y, sd["conv2.bn.weight"], sd["conv2.bn.bias"], sd["conv2.bn.running_mean"], sd["conv2.bn.running_var"], training, eps, momentum)
    out_pm = torch.relu(Y * bn2["a"] + bn2["s"])
    out = out_pm.view(B, N, F2).transpose(1, 2).reshape(B, F2 // 2, 2 * N)
    return dict(out=out, out_pm=out_pm, U=U, Z1=Z1, A1=A1, Y=Y, bn1=bn1, bn2=bn2, xp=xp, gidx=gidx, k=k, w=w, T=T, C=C, B=B, N=N,
                training=training, img=(Wc1, Wd1, Vc, Vd, V2p), W1=W1, V=V)


def backward(f, g):
    """The closed-form backward for cotangent g [B,Fout,2N] -> dict(dx, grad|<parameter>...)."""
    B, N, C, k, w, T = f["B"], f["N"], f["C"], f["k"], f["w"], f["T"]
    M = B * N
    Wc1, Wd1, Vc, Vd, V2p = f["img"]
    F2 = Vc.shape[0]
    xp, gidx, bn1, bn2 = f["xp"], f["gidx"], f["bn1"], f["bn2"]
    train = f["training"]
    g_pm = g.reshape(B, F2, N).transpose(1, 2).reshape(M, F2)
    r = g_pm * (f["out_pm"] > 0).to(g.dtype)
    xh2 = (f["Y"] - bn2["mean"]) * bn2["invstd"]
    s1, s2 = r.sum(dim=0), (r * xh2).sum(dim=0)
    dy = bn2["a"] * (r - s1 / M - xh2 * s2 / M) if train else bn2["a"] * r
    D = differences(xp, gidx)
    dVc = dy.t() @ xp
    dVd = dy.t() @ D.reshape(M, k * C)
    dV2p = dy.t() @ f["A1"].reshape(M, T * 4 * C)
    gz = (dy @ V2p).reshape(M * T, 4 * C) * torch.where(f["Z1"] > 0, torch.ones_like(f["Z1"]), torch.full_like(f["Z1"], SLOPE))
    xh1 = (f["U"] - bn1["mean"]) * bn1["invstd"]
    t1, t2 = gz.sum(dim=0), (gz * xh1).sum(dim=0)
    E = M * T
    dU = bn1["a"] * (gz - t1 / E - xh1 * t2 / E) if train else bn1["a"] * gz
    dQ1 = dU.view(M, T, 4 * C).sum(dim=1)
    dWc1 = dQ1.t() @ xp
    dWd1 = window_wgrad(xp, gidx, dU, w)
    S = window_dgrad(dU, Wd1, k, C, w) + window_dgrad(dy, Vd, k, C, k)
    dx_pm = window_scatter(S, gidx, dy @ Vc, dQ1 @ Wc1)
    dV = torch.zeros_like(f["V"])
    dV[:, :C, 0, :k] = dVc[:, :, None]
    dV[:, C:, 0, :k] = dVd.view(F2, k, C).permute(0, 2, 1)
    dV[:, :, 0, k:] = dV2p.view(F2, T, 4 * C).permute(0, 2, 1).reshape(F2, 2 * C, k)
    dW1 = torch.zeros_like(f["W1"])
    dW1[:, :C, 0, :] = dWc1[:, :, None]
    dW1[:, C:, 0, :] = dWd1.view(4 * C, w, C).permute(0, 2, 1)
    return {"dx": dx_pm.view(B, N, C).transpose(1, 2), "grad|conv2.conv.weight": dV, "grad|conv2.conv.bias": dy.sum(dim=0),
            "grad|conv2.bn.weight": s2, "grad|conv2.bn.bias": s1, "grad|inte_conv_hk.0.weight": dW1,
            "grad|inte_conv_hk.0.bias": dU.sum(dim=0), "grad|inte_conv_hk.1.weight": t2, "grad|inte_conv_hk.1.bias": t1,
            "dU": dU, "dy": dy, "S": S}


def literal(x, idx, k, sd, training, eps=EPS):
    """The reference's own sequence of operations (edge tensor, conv2d, transpose / view chain, concatenation) in plain torch -> out."""
    import torch.nn.functional as F_
    B, C, N = x.shape
    nb = idx.view(B, N, k)
    xp = x.transpose(1, 2)
    nbr = xp[torch.arange(B).view(B, 1, 1), nb].permute(0, 3, 1, 2)                  # [B,C,N,k]
    cen = x.unsqueeze(3).expand(B, C, N, k)
    ee = torch.cat([cen, nbr - cen], dim=1)
    h = F_.conv2d(ee, sd["inte_conv_hk.0.weight"], sd["inte_conv_hk.0.bias"])
    h = F_.batch_norm(h, sd["inte_conv_hk.1.running_mean"].clone(), sd["inte_conv_hk.1.running_var"].clone(), sd["inte_conv_hk.1.weight"],
                      sd["inte_conv_hk.1.bias"], training, MOMENTUM, eps)
    h = F_.leaky_relu(h, SLOPE)
    h = h.transpose(2, 1).contiguous().view(B, N, 2 * C, 2, k // 2).contiguous().view(B, N, 2 * C, k).permute(0, 2, 1, 3)
    y = F_.conv2d(torch.cat((ee, h), 3), sd["conv2.conv.weight"], sd["conv2.conv.bias"])
    y = F_.batch_norm(y, sd["conv2.bn.running_mean"].clone(), sd["conv2.bn.running_var"].clone(), sd["conv2.bn.weight"], sd["conv2.bn.bias"],
                      training, MOMENTUM, eps)
    y = torch.relu(y)
    return y.contiguous().view(B, -1, 2, N).contiguous().view(B, -1, 2 * N)
