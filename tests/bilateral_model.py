"""A plain torch model of the decomposed bilateral upsampling edge convolution (spgan.modules.bilateral_upsample_edgeConv, csrc/edge_rank.hip's
spgan_edge_stored_gemm / _wgrad / _dgrad) and the case table of golden `bilateral.npz`.

With j = idx[i,r], e(i,r) = cat[x_i, x_j - x_i], y(i,r) = cat[pc_i, pc_j - pc_i], C = Fin, w = k/2 + 1, T = k/2 (Generation/modules.py:847-925)
and the notation of tests/upsample_model.py and tests/deform_xyz_model.py:

    u(i,t,:)  = inte_conv_hk's Conv2d(2C -> 4C, [1,w]) at window position t          [M*T, 4C]       a1 = lrelu(bn1(u))
    z_f, z_x  = conv_fea / conv_xyz, per-point GEMMs over x / pc                      [M, k, 16]      w0 = a_f * a_x
    z2, z3    = conv_all.0 / conv_all.3 over edge rows                                [M*k, 64], [M*k, 2C]
    s         = softmax over the k ranks of a3 = lrelu(bn3(z3))                       (softmax=False: s = a3)
    inte(i, j, c') = a1(i, t, 2c' + h),  j = h*T + t                                  the reference's transpose / view chain
    y(i,:)    = conv2's taps 0..k-1 over e  +  sum_{j,c'} V[:, c', 0, k+j] inte(i,j,c') s(i,j,c')
    out       = relu(bn2(y)),  out[b, f, s*N + n] = y[b, 2f+s, n]

The layer model works in the reference's own channel and rank order: it is the yardstick of the layer, independent of the order in which
the kernels store things.  The launcher models (stored_*) take the kernels' layout: U and z3 [M,k,F1] with rows (point, rank), the first
BatchNorm's vectors [2*F1] with entry (r & 1)*F1 + c.  Everything is materialised; float64 or float32 by the dtype of the arguments."""
import numpy as np
import torch

import deform_feat_model as fm
import deform_model as dm
import deform_xyz_model as xm
import upsample_model as um
from deform_model import EPS, MOMENTUM, global_idx, lrelu
from deform_feat_model import SAMPLE_MIN, golden_pair, mask                               # noqa: F401
from deform_xyz_model import noise, param                                                 # noqa: F401

# tag -> sizes, mode and softmax flag (the issue's table)
CASES = {
    "a": dict(B=2, N=50, Fin=3, Fout=8, k=4, train=True, softmax=True, warm=False),       # scalar staging (2C = 6), partial point tile, fp64 kNN mode
    "b": dict(B=2, N=96, Fin=32, Fout=32, k=10, train=True, softmax=True, warm=False),    # the workload's k, T = 5
    "c": dict(B=1, N=70, Fin=40, Fout=24, k=8, train=True, softmax=False, warm=False),    # 2C = 80: a full 64-channel staging chunk and a ragged one
    "d": dict(B=2, N=64, Fin=16, Fout=16, k=2, train=True, softmax=True, warm=False),     # T = 1, w = 2: one window position, two ranks
    "e": dict(B=2, N=64, Fin=16, Fout=32, k=28, train=False, softmax=True, warm=True),    # the largest k, warmed running statistics
}
F_A, F_B = 16, 64
# a result with more than SAMPLE_MIN elements is stored as every SAMPLE_STRIDE-th element + its L2 norm (golden_pair reads the stride from the
# file); 29 is coprime to every k, 2k, w and channel count of the cases, so the samples of a weight gradient visit every tap and channel
SAMPLE_STRIDE = 29
LAYERS = (("conv2.conv", "conv2.bn"), ("conv_xyz.0", "conv_xyz.1"), ("conv_fea.0", "conv_fea.1"), ("conv_all.0", "conv_all.1"),
          ("conv_all.3", "conv_all.4"), ("inte_conv_hk.0", "inte_conv_hk.1"))               # state_dict order
CONVS = tuple(c for c, _ in LAYERS)
NORMS = tuple(n for _, n in LAYERS)


def _keys():
    out = []
    for conv, bn in LAYERS:
        out += [conv + ".weight", conv + ".bias"] + [bn + "." + n for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    return tuple(out)


STATE_KEYS = _keys()
BUFFERS = tuple(n for n in STATE_KEYS if "running" in n or "num_batches" in n)
ZERO_GRAD_BIASES = tuple(c + ".bias" for c in CONVS)       # every conv bias sits in front of a train-mode BatchNorm


def conv_shapes(c):
    C, F, k = c["Fin"], c["Fout"], c["k"]
    return {"conv2.conv": (2 * F, 2 * C, 1, 2 * k), "conv_xyz.0": (F_A, 6, 1, 1), "conv_fea.0": (F_A, 2 * C, 1, 1), "conv_all.0": (F_B, F_A, 1, 1),
            "conv_all.3": (2 * C, F_B, 1, 1), "inte_conv_hk.0": (4 * C, 2 * C, 1, k // 2 + 1)}


def norm_width(c, bn):
    C, F = c["Fin"], c["Fout"]
    return {"conv2.bn": 2 * F, "conv_xyz.1": F_A, "conv_fea.1": F_A, "conv_all.1": F_B, "conv_all.4": 2 * C, "inte_conv_hk.1": 4 * C}[bn]


def case_tensors(tag, seed=0):
    """(x [B,Fin,N], pc [B,3,N], cotangent [B,Fout,2N], state_dict) of a case, from spgan.fixture_rng (float32)."""
    from spgan import fixture_rng as fr
    c = CASES[tag]
    C = c["Fin"]
    name = "bilateral.%s" % tag
    if C <= 4:
        x = fr.uniform(name + ".x", (c["B"], C, c["N"]), -1.0, 1.0, salt=seed)
    else:
        x = fr.normal(name + ".x", (c["B"], C, c["N"]), 0.7, salt=seed)
    pc = fr.uniform(name + ".pc", (c["B"], 3, c["N"]), -1.0, 1.0, salt=seed)
    g = fr.normal(name + ".g", (c["B"], c["Fout"], 2 * c["N"]), salt=seed).bfloat16().float()
    sd = {}
    for (conv, shape), bn in zip(conv_shapes(c).items(), NORMS):
        F_ = norm_width(c, bn)
        b = 1.0 / np.sqrt(shape[1] * shape[3])
        # multiples of a power of two near b/2, at most 9 levels: bfloat16-exact values (held in float32), whose 16-bit halves compress
        q = 2.0 ** np.floor(np.log2(b / 2))
        sd[conv + ".weight"] = (torch.round(fr.uniform("%s.%s.W" % (name, conv), shape, -b, b, salt=seed) / q) * q).bfloat16().float()
        sd[conv + ".bias"] = fr.uniform("%s.%s.b" % (name, conv), (shape[0],), -b, b, salt=seed)
        sd[bn + ".weight"] = fr.uniform("%s.%s.gamma" % (name, bn), (F_,), 0.5, 1.5, salt=seed)
        sd[bn + ".bias"] = fr.uniform("%s.%s.beta" % (name, bn), (F_,), -0.2, 0.2, salt=seed)
        if c["warm"]:
            sd[bn + ".running_mean"] = fr.normal("%s.%s.rm" % (name, bn), (F_,), 0.1, salt=seed)
            sd[bn + ".running_var"] = fr.uniform("%s.%s.rv" % (name, bn), (F_,), 0.5, 1.5, salt=seed)
            sd[bn + ".num_batches_tracked"] = torch.tensor(21, dtype=torch.int64)
        else:
            sd[bn + ".running_mean"], sd[bn + ".running_var"] = torch.zeros(F_), torch.ones(F_)
            sd[bn + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.int64)
    return x, pc, g, {n: sd[n] for n in STATE_KEYS}


def golden_state_dict(d, tag):
    return {n: torch.from_numpy(param(d, tag, n)) for n in STATE_KEYS}


# --------------------------------------------------------------------------------------------- the launchers (spgan_edge_stored_*)
def stored_h(U, sc1, sh1):
    """U [M,k,F1], sc1 / sh1 [2*F1] -> (h = lrelu(pre), pre): the affine of rank r is the half (r & 1) of the vectors"""
    k, F1 = U.shape[1], U.shape[2]
    par = torch.arange(k) % 2
    pre = U * sc1.view(2, F1)[par] + sh1.view(2, F1)[par]
    return lrelu(pre), pre


def stored_gemm(U, sc1, sh1, z3, sc3, sh3, soft, W2i, b2=None):
    """-> y [M,O] = b2 + (h*s).flat @ W2i^T"""
    hs = stored_h(U, sc1, sh1)[0] * fm.weight(z3, sc3, sh3, soft)[0]
    y = hs.reshape(hs.shape[0], -1) @ W2i.t()
    return y if b2 is None else y + b2


def stored_wgrad(U, sc1, sh1, z3, sc3, sh3, soft, dy):
    """-> dW2i [O, k*F1]"""
    hs = stored_h(U, sc1, sh1)[0] * fm.weight(z3, sc3, sh3, soft)[0]
    return dy.t() @ hs.reshape(hs.shape[0], -1)


def stored_dgrad(dy, W2i, U, sc1, sh1, mean1, invstd1, z3, sc3, sh3, mean3, invstd3, soft):
    """-> (gU [M,k,F1], sums_u [2*2F1] = [sum gU | sum gU*uhat] per (rank parity, channel), g3 [M,k,F1], sums_3 [2F1])"""
    h, ah = stored_h(U, sc1, sh1)
    s, pre3 = fm.weight(z3, sc3, sh3, soft)
    M, k, F1 = h.shape
    par = torch.arange(k) % 2
    dmm = (dy @ W2i).view(M, k, F1)
    gU = mask(ah) * dmm * s
    ds = dmm * h
    g3 = mask(pre3) * (s * (ds - (ds * s).sum(dim=1, keepdim=True)) if soft else ds)
    uhat, zhat = (U - mean1.view(2, F1)[par]) * invstd1.view(2, F1)[par], (z3 - mean3) * invstd3

    def by_parity(t):
        return t.view(M, k // 2, 2, F1).sum(dim=(0, 1)).reshape(-1)
    return (gU, torch.cat([by_parity(gU), by_parity(gU * uhat)]), g3, torch.cat([g3.sum(dim=(0, 1)), (g3 * zhat).sum(dim=(0, 1))]))


# --------------------------------------------------------------------------------------------- the layer
def _bn(Y, sd, pre, training, eps, momentum):
    return dm._bn(Y, sd[pre + ".weight"], sd[pre + ".bias"], sd[pre + ".running_mean"], sd[pre + ".running_var"], training, eps, momentum)


def forward(x, pc, idx, k, sd, training, softmax, eps=EPS, momentum=MOMENTUM):
    """x [B,C,N], pc [B,3,N], idx int64 [B,N*k] local, sd = the state_dict in the dtype the model is to run in -> dict (out [B,Fout,2N], the
    six BatchNorm records under their state_dict prefixes).  Differentiable by autograd in x, pc and every floating-point entry of sd."""
    B, C, N = x.shape
    M = B * N
    W1, V = sd["inte_conv_hk.0.weight"], sd["conv2.conv.weight"]
    w = W1.shape[3]
    T = k - w + 1
    F2 = V.shape[0]
    Wc1, Wd1, Vc, Vd, _ = um.images(W1, V, C, k)
    xp, pp = x.transpose(1, 2).reshape(M, C), pc.transpose(1, 2).reshape(M, 3)
    gidx = global_idx(idx, B, N, k)
    bn = {}
    # the interpolation, as upsample_edgeConv
    U = um.window_gemm(xp, gidx, Wd1, w, rowadd=xp @ Wc1.t() + sd["inte_conv_hk.0.bias"])               # [M*T, 4C]
    bn["inte_conv_hk.1"] = _bn(U, sd, "inte_conv_hk.1", training, eps, momentum)
    A1 = lrelu(U * bn["inte_conv_hk.1"]["a"] + bn["inte_conv_hk.1"]["s"])
    inte = A1.view(M, T, 2 * C, 2).permute(0, 3, 1, 2).reshape(M, k, 2 * C)                                # (i, j = h*T + t, c') = a1(i, t, 2c'+h)

    # the weight, as deform_edgeConv with 2C output channels
    def pq(rows, conv):
        b = sd[conv + ".bias"]
        return rows @ fm._stack(sd[conv + ".weight"]).t() + torch.cat([torch.zeros_like(b), b])
    PQf, PQx = pq(xp, "conv_fea.0"), pq(pp, "conv_xyz.0")
    for n, PQ in (("conv_fea.1", PQf), ("conv_xyz.1", PQx)):
        bn[n] = _bn(fm.gather(PQ, gidx), sd, n, training, eps, momentum)
    w0 = xm.gather2(PQf, PQx, gidx, bn["conv_fea.1"]["a"], bn["conv_fea.1"]["s"], bn["conv_xyz.1"]["a"], bn["conv_xyz.1"]["s"])
    z2 = w0 @ sd["conv_all.0.weight"].reshape(F_B, F_A).t() + sd["conv_all.0.bias"]
    bn["conv_all.1"] = _bn(z2, sd, "conv_all.1", training, eps, momentum)
    z3 = lrelu(z2 * bn["conv_all.1"]["a"] + bn["conv_all.1"]["s"]) @ sd["conv_all.3.weight"].reshape(2 * C, F_B).t() + sd["conv_all.3.bias"]
    bn["conv_all.4"] = _bn(z3, sd, "conv_all.4", training, eps, momentum)
    s = fm.weight(z3.view(M, k, 2 * C), bn["conv_all.4"]["a"], bn["conv_all.4"]["s"], softmax)[0]
    # conv2 over cat(e, inte * s): taps k..2k-1 read channel c' of rank j
    Y3 = (inte * s).permute(0, 2, 1).reshape(M, 2 * C * k) @ V[:, :, 0, k:].reshape(F2, 2 * C * k).t()
    Y = um.window_gemm(xp, gidx, Vd, k, rowadd=xp @ Vc.t() + sd["conv2.conv.bias"], add2=Y3)
    bn["conv2.bn"] = _bn(Y, sd, "conv2.bn", training, eps, momentum)
    out_pm = torch.relu(Y * bn["conv2.bn"]["a"] + bn["conv2.bn"]["s"])
    out = out_pm.view(B, N, F2).transpose(1, 2).reshape(B, F2 // 2, 2 * N)
    return dict(out=out, bn=bn, U=U, z3=z3, Y=Y, Y3=Y3, gidx=gidx)


def run(x, pc, idx, g, k, sd, training, softmax):
    """forward + autograd backward in the dtype of x -> {out, dx, dpc, grad|<parameter>, buf|<buffer>} (num_batches_tracked left out)"""
    x, pc = x.clone().requires_grad_(True), pc.clone().requires_grad_(True)
    sd = {n: (v.clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in n else v) for n, v in sd.items()}
    f = forward(x, pc, idx, k, sd, training, softmax)
    (f["out"] * g).sum().backward()
    got = {"out": f["out"].detach(), "dx": x.grad, "dpc": pc.grad if pc.grad is not None else torch.zeros_like(pc)}
    for n, v in sd.items():
        if v.requires_grad:
            got["grad|" + n] = v.grad if v.grad is not None else torch.zeros_like(v)
    for pre, rec in f["bn"].items():
        got["buf|%s.running_mean" % pre], got["buf|%s.running_var" % pre] = rec["running_mean"].detach(), rec["running_var"].detach()
    return got
