"""A plain torch model of the decomposed weighted full-rank edge convolution (spgan.modules.deform_edgeConv_feat, csrc/edge_rank.hip's
spgan_edge_weight_* launchers) and the case table of golden `deform_feat.npz`.

With j = idx[i,r], e(i,r) = cat[x_i, x_j - x_i] (Generation/modules.py:1543-1599) and the notation of tests/deform_model.py:

    u  = P_h[j] + Q_h[i]                      h  = lrelu(bn_h(u))            inte_conv_hk, as a per-point GEMM PQ_h [M, 2Fin]
    z1 = P_1[j] + Q_1[i]   [16]               a1 = lrelu(bn1(z1))            conv_fea.0, as a per-point GEMM PQ_1 [M, 32]
    z2 = W_m2 a1 + b       [64]               a2 = lrelu(bn2(z2))            conv_fea.3
    z3 = W_m3 a2 + b       [Fin]              a3 = lrelu(bn3(z3))            conv_fea.6
    s  = exp(a3 - wmax) * wrs,  wmax = max_r a3,  wrs = 1 / sum_r exp(a3 - wmax)     (softmax=True; otherwise s = a3)
    y(i,:) = b2 + sum_r W2[:,:,0,r] (h*s)(i,r,:)                             (h*s).flat @ W2i^T
    out    = relu(bn_c(y))

The model materialises h, s and h*s: it is the yardstick, evaluated in float64 or float32, not the memory behaviour.  The layer's backward
is torch.autograd over this forward; the launchers' backward formulas are written out (wdgrad, wwgrad) and pinned against autograd by
tests/test_deform_feat_cpu.py."""
import numpy as np
import torch

import deform_model as dm
from deform_model import EPS, MOMENTUM, SLOPE, colstats, global_idx, lrelu, pre_norm   # noqa: F401

# tag -> sizes, mode and softmax flag (the issue's table); warm: non-initial running statistics
CASES = {
    "a": dict(B=2, N=50, Fin=3, Fout=20, k=5, train=True, softmax=True, warm=False),     # scalar staging, partial point tile, Fout % 16 != 0
    "b": dict(B=2, N=96, Fin=32, Fout=48, k=20, train=True, softmax=True, warm=False),   # the workload's k
    "c": dict(B=1, N=70, Fin=72, Fout=64, k=8, train=True, softmax=False, warm=False),   # two 64-channel staging chunks, the second ragged
    "d": dict(B=2, N=64, Fin=16, Fout=32, k=1, train=True, softmax=True, warm=False),    # softmax over one rank: s == 1
    "e": dict(B=2, N=64, Fin=32, Fout=32, k=32, train=False, softmax=True, warm=True),   # K_MAX, running statistics
}
F_A, F_B = 16, 64                                  # the weight MLP's hidden widths
NORMS = ("conv2.bn", "conv_fea.1", "conv_fea.4", "conv_fea.7", "inte_conv_hk.1")      # state_dict order
CONVS = ("conv2.conv", "conv_fea.0", "conv_fea.3", "conv_fea.6", "inte_conv_hk.0")


def _keys():
    out = []
    for conv, bn in (("conv2.conv", "conv2.bn"), ("conv_fea.0", "conv_fea.1"), ("conv_fea.3", "conv_fea.4"), ("conv_fea.6", "conv_fea.7"),
                     ("inte_conv_hk.0", "inte_conv_hk.1")):
        out += [conv + ".weight", conv + ".bias"] + [bn + "." + n for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    return tuple(out)


STATE_KEYS = _keys()
BUFFERS = tuple(n for n in STATE_KEYS if "running" in n or "num_batches" in n)
ZERO_GRAD_BIASES = tuple(c + ".bias" for c in CONVS)       # every conv bias sits in front of a train-mode BatchNorm


def conv_shapes(c):
    C, F, k = c["Fin"], c["Fout"], c["k"]
    return {"conv2.conv": (F, C, 1, k), "conv_fea.0": (F_A, 2 * C, 1, 1), "conv_fea.3": (F_B, F_A, 1, 1), "conv_fea.6": (C, F_B, 1, 1),
            "inte_conv_hk.0": (C, 2 * C, 1, 1)}


def case_tensors(tag, seed=0):
    """(x [B,Fin,N], cotangent [B,Fout,N], state_dict) of a case, from spgan.fixture_rng (float32)."""
    from spgan import fixture_rng as fr
    c = CASES[tag]
    C = c["Fin"]
    name = "deform_feat.%s" % tag
    if C <= 4:
        x = fr.uniform(name + ".x", (c["B"], C, c["N"]), -1.0, 1.0, salt=seed)
    else:
        x = fr.normal(name + ".x", (c["B"], C, c["N"]), 0.7, salt=seed)
    g = fr.normal(name + ".g", (c["B"], c["Fout"], c["N"]), salt=seed).bfloat16().float()
    sd = {}
    for (conv, shape), bn in zip(conv_shapes(c).items(), NORMS):
        F_ = shape[0]
        b = 1.0 / np.sqrt(shape[1] * shape[3])
        # bfloat16-exact values (held in float32): the stored parameters compress to half their size in the golden file
        sd[conv + ".weight"] = fr.uniform("%s.%s.W" % (name, conv), shape, -b, b, salt=seed).bfloat16().float()
        sd[conv + ".bias"] = fr.uniform("%s.%s.b" % (name, conv), (F_,), -b, b, salt=seed)
        sd[bn + ".weight"] = fr.uniform("%s.%s.gamma" % (name, bn), (F_,), 0.5, 1.5, salt=seed)
        sd[bn + ".bias"] = fr.uniform("%s.%s.beta" % (name, bn), (F_,), -0.2, 0.2, salt=seed)
        if c["warm"]:
            sd[bn + ".running_mean"] = fr.normal("%s.%s.rm" % (name, bn), (F_,), 0.1, salt=seed)
            sd[bn + ".running_var"] = fr.uniform("%s.%s.rv" % (name, bn), (F_,), 0.5, 1.5, salt=seed)
            sd[bn + ".num_batches_tracked"] = torch.tensor(21, dtype=torch.int64)
        else:
            sd[bn + ".running_mean"], sd[bn + ".running_var"] = torch.zeros(F_), torch.ones(F_)
            sd[bn + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.int64)
    return x, g, {n: sd[n] for n in STATE_KEYS}


def golden_state_dict(d, tag):
    return {n: torch.from_numpy(np.asarray(d["%s|param|%s" % (tag, n)])) for n in STATE_KEYS}


# a result with more than SAMPLE_MIN elements is stored as every SAMPLE_STRIDE-th element + its L2 norm; the stride is coprime to every
# k and Fin of the cases, so the samples of conv2's weight gradient [Fout,Fin,1,k] visit every rank and every input channel
SAMPLE_STRIDE, SAMPLE_MIN = 7, 8192


def golden_pair(d, tag, q, value):
    """(the reference's float64 result of quantity q, the matching elements of `value`): the golden stores the float64 run as its
    distance from the float32 run, in full or -- the large conv2 weight gradients -- as strided samples (helpers.check's two forms)."""
    name = "%s|%s" % (tag, q)
    v = torch.as_tensor(value)
    if name + "|full" in d:
        assert tuple(v.shape) == tuple(d[name + "|full"].shape), (name, tuple(v.shape))
        return torch.from_numpy(np.asarray(d[name + "|full"])).double() + torch.from_numpy(np.asarray(d[name + "|d64|full"])).double(), v
    stride = int(d[name + "|stride"])
    ref = torch.from_numpy(np.asarray(d[name + "|samples"])).double() + torch.from_numpy(np.asarray(d[name + "|d64|samples"])).double()
    return ref, v.reshape(-1)[::stride][:ref.numel()]


# --------------------------------------------------------------------------------------------- the launchers (spgan_edge_weight_*)
def mask(a):
    return torch.where(a > 0, torch.ones_like(a), torch.full_like(a, SLOPE))


def gather(PQ, gidx):
    """-> z [M*k, F] = Q_i + P_j"""
    z = pre_norm(PQ, gidx)
    return z.reshape(-1, z.shape[2])


def norm(z3, sc3, sh3):
    """z3 [M,k,F] -> (wmax, wrs) [M,F]"""
    a3 = lrelu(z3 * sc3 + sh3)
    wmax = a3.max(dim=1)[0]
    return wmax, 1.0 / torch.exp(a3 - wmax[:, None]).sum(dim=1)


def weight(z3, sc3, sh3, soft):
    """-> (s [M,k,F], a3pre = sc3*z3 + sh3)"""
    pre = z3 * sc3 + sh3
    a3 = lrelu(pre)
    if not soft:
        return a3, pre
    wmax, wrs = norm(z3, sc3, sh3)
    return torch.exp(a3 - wmax[:, None]) * wrs[:, None], pre


def wgemm(PQ, gidx, sc1, sh1, z3, sc3, sh3, soft, W2i, b2=None):
    """-> y [M,O] = b2 + (h*s).flat @ W2i^T"""
    hs = dm.rank_h(PQ, gidx, sc1, sh1)[0] * weight(z3, sc3, sh3, soft)[0]
    y = hs.reshape(hs.shape[0], -1) @ W2i.t()
    return y if b2 is None else y + b2


def wwgrad(PQ, gidx, sc1, sh1, z3, sc3, sh3, soft, dy):
    """-> dW2i [O, k*F]"""
    hs = dm.rank_h(PQ, gidx, sc1, sh1)[0] * weight(z3, sc3, sh3, soft)[0]
    return dy.t() @ hs.reshape(hs.shape[0], -1)


def wdgrad(dy, W2i, PQ, gidx, sc1, sh1, mean1, invstd1, z3, sc3, sh3, mean3, invstd3, soft):
    """-> (du [M,k,F], sums_u [2F], g3 [M,k,F], sums_3 [2F])"""
    h, ah, u = dm.rank_h(PQ, gidx, sc1, sh1)
    s, pre3 = weight(z3, sc3, sh3, soft)
    M, k, F = h.shape
    dmm = (dy @ W2i).view(M, k, F)
    du = mask(ah) * dmm * s
    ds = dmm * h
    g3 = mask(pre3) * (s * (ds - (ds * s).sum(dim=1, keepdim=True)) if soft else ds)
    uhat, zhat = (u - mean1) * invstd1, (z3 - mean3) * invstd3
    return (du, torch.cat([du.sum(dim=(0, 1)), (du * uhat).sum(dim=(0, 1))]), g3, torch.cat([g3.sum(dim=(0, 1)), (g3 * zhat).sum(dim=(0, 1))]))


# --------------------------------------------------------------------------------------------- the layer
def _stack(W):
    """W [F,2Fin,1,1] -> [2F,Fin] = [Wd ; Wc - Wd]"""
    F_, C = W.shape[0], W.shape[1] // 2
    Wm = W.reshape(F_, 2 * C)
    return torch.cat([Wm[:, C:], Wm[:, :C] - Wm[:, C:]], dim=0)


def _bn(Y, sd, pre, training, eps, momentum):
    return dm._bn(Y, sd[pre + ".weight"], sd[pre + ".bias"], sd[pre + ".running_mean"], sd[pre + ".running_var"], training, eps, momentum)


def forward(x, idx, k, sd, training, softmax, eps=EPS, momentum=MOMENTUM):
    """x [B,Fin,N], idx int64 [B,N*k] local, sd = the state_dict in the dtype the model is to run in -> dict (out [B,Fout,N], the five
    BatchNorm records under their state_dict prefixes).  Differentiable by autograd in x and every floating-point entry of sd."""
    B, C, N = x.shape
    M = B * N
    xp = x.transpose(1, 2).reshape(M, C)
    gidx = global_idx(idx, B, N, k)

    def pq(conv):
        b = sd[conv + ".bias"]
        return xp @ _stack(sd[conv + ".weight"]).t() + torch.cat([torch.zeros_like(b), b])
    PQh, PQ1 = pq("inte_conv_hk.0"), pq("conv_fea.0")
    bn = {"inte_conv_hk.1": _bn(gather(PQh, gidx), sd, "inte_conv_hk.1", training, eps, momentum)}
    z1 = gather(PQ1, gidx)
    bn["conv_fea.1"] = _bn(z1, sd, "conv_fea.1", training, eps, momentum)
    z2 = lrelu(z1 * bn["conv_fea.1"]["a"] + bn["conv_fea.1"]["s"]) @ sd["conv_fea.3.weight"].reshape(F_B, F_A).t() + sd["conv_fea.3.bias"]
    bn["conv_fea.4"] = _bn(z2, sd, "conv_fea.4", training, eps, momentum)
    z3 = lrelu(z2 * bn["conv_fea.4"]["a"] + bn["conv_fea.4"]["s"]) @ sd["conv_fea.6.weight"].reshape(C, F_B).t() + sd["conv_fea.6.bias"]
    bn["conv_fea.7"] = _bn(z3, sd, "conv_fea.7", training, eps, momentum)
    W2 = sd["conv2.conv.weight"]
    W2i = W2[:, :, 0, :].permute(0, 2, 1).reshape(W2.shape[0], -1)
    Y = wgemm(PQh, gidx, bn["inte_conv_hk.1"]["a"], bn["inte_conv_hk.1"]["s"], z3.view(M, k, C), bn["conv_fea.7"]["a"], bn["conv_fea.7"]["s"],
              softmax, W2i, sd["conv2.conv.bias"])
    bn["conv2.bn"] = _bn(Y, sd, "conv2.bn", training, eps, momentum)
    out_pm = torch.relu(Y * bn["conv2.bn"]["a"] + bn["conv2.bn"]["s"])
    return dict(out=out_pm.view(B, N, -1).transpose(1, 2), bn=bn, PQh=PQh, PQ1=PQ1, z1=z1, z2=z2, z3=z3, Y=Y, gidx=gidx, W2i=W2i)


def run(x, idx, g, k, sd, training, softmax):
    """forward + autograd backward in the dtype of x -> {out, dx, grad|<parameter>, buf|<buffer>} (num_batches_tracked left out)"""
    x = x.clone().requires_grad_(True)
    sd = {n: (v.clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in n else v) for n, v in sd.items()}
    f = forward(x, idx, k, sd, training, softmax)
    (f["out"] * g).sum().backward()
    got = {"out": f["out"].detach(), "dx": x.grad}
    for n, v in sd.items():
        if v.requires_grad:
            got["grad|" + n] = v.grad if v.grad is not None else torch.zeros_like(v)
    for pre, rec in f["bn"].items():
        got["buf|%s.running_mean" % pre], got["buf|%s.running_var" % pre] = rec["running_mean"].detach(), rec["running_var"].detach()
    return got
