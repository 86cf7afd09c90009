"""A plain torch model of the decomposed coordinate-guided full-rank edge convolution (spgan.modules.deform_edgeConv, csrc/edge_rank.hip's
spgan_edge_weight_gather2 / spgan_edge_weight_split) and the case table of golden `deform_xyz.npz`.

With j = idx[i,r], e(i,r) = cat[x_i, x_j - x_i], y(i,r) = cat[pc_i, pc_j - pc_i] (Generation/modules.py:1468-1540; one graph, built in the
feature space of x, gathers both) and the notation of tests/deform_feat_model.py:

    u   = P_h[j] + Q_h[i]                     h   = lrelu(bn_h(u))           inte_conv_hk, a per-point GEMM PQ_h [M, 2Fin] over x
    z_f = P_f[j] + Q_f[i]   [16]              a_f = lrelu(bn_f(z_f))         conv_fea,     a per-point GEMM PQ_f [M, 32]   over x
    z_x = P_x[j] + Q_x[i]   [16]              a_x = lrelu(bn_x(z_x))         conv_xyz,     a per-point GEMM PQ_x [M, 32]   over pc
    w0  = a_f * a_x         [16]                                             gather2; no BatchNorm between w0 and conv_all.0
    z2  = W_m2 w0 + b       [64]              a2  = lrelu(bn2(z2))           conv_all.0
    z3  = W_m3 a2 + b       [Fin]             a3  = lrelu(bn3(z3))           conv_all.3
    s   = softmax over the k ranks of a3      (softmax=False: s = a3)
    y(i,:) = b2 + sum_r W2[:,:,0,r] (h*s)(i,r,:)
    out    = lrelu(bn_c(y))                                                  conv2: a plain Sequential, LeakyReLU at its end

The model materialises everything: it is the yardstick, evaluated in float64 or float32, not the memory behaviour.  The layer's backward
is torch.autograd over this forward; the split launcher's backward formulas are written out (split) and pinned against autograd by
tests/test_deform_xyz_cpu.py.  The argument order of gather2 / split follows spgan.edge_weight's wrappers."""
import numpy as np
import torch

import deform_feat_model as fm
import deform_model as dm
from deform_model import EPS, MOMENTUM, SLOPE, colstats, global_idx, lrelu, pre_norm   # noqa: F401
from deform_feat_model import SAMPLE_MIN, SAMPLE_STRIDE, golden_pair, mask                # noqa: F401

# tag -> sizes (Fin == Fout == F: the layer runs with no other pair), mode and softmax flag (the issue's table)
CASES = {
    "a": dict(B=2, N=50, F=3, k=5, train=True, softmax=True, warm=False),      # scalar staging, fp64 kNN mode, partial point tile
    "b": dict(B=2, N=96, F=32, k=20, train=True, softmax=True, warm=False),    # the workload's k
    "c": dict(B=1, N=70, F=72, k=8, train=True, softmax=False, warm=False),    # two 64-channel staging chunks, the second ragged
    "d": dict(B=2, N=64, F=16, k=1, train=True, softmax=True, warm=False),     # softmax over one rank: s == 1
    "e": dict(B=2, N=64, F=32, k=32, train=False, softmax=True, warm=True),    # K_MAX, warmed running statistics
}
F_A, F_B = 16, 64                                  # the branches' width and the weight MLP's hidden width
LAYERS = (("conv2.0", "conv2.1"), ("conv_xyz.0", "conv_xyz.1"), ("conv_fea.0", "conv_fea.1"), ("conv_all.0", "conv_all.1"),
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
# k = 1: the softmax weight is 1, nothing reaches the weight MLP, its two branches or the coordinates
SINGLE_RANK_ZERO = ("conv_fea", "conv_xyz", "conv_all")


def conv_shapes(c):
    F, k = c["F"], c["k"]
    return {"conv2.0": (F, F, 1, k), "conv_xyz.0": (F_A, 6, 1, 1), "conv_fea.0": (F_A, 2 * F, 1, 1), "conv_all.0": (F_B, F_A, 1, 1),
            "conv_all.3": (F, F_B, 1, 1), "inte_conv_hk.0": (F, 2 * F, 1, 1)}


def norm_width(c, bn):
    F = c["F"]
    return {"conv2.1": F, "conv_xyz.1": F_A, "conv_fea.1": F_A, "conv_all.1": F_B, "conv_all.4": F, "inte_conv_hk.1": F}[bn]


def case_tensors(tag, seed=0):
    """(x [B,F,N], pc [B,3,N], cotangent [B,F,N], state_dict) of a case, from spgan.fixture_rng (float32)."""
    from spgan import fixture_rng as fr
    c = CASES[tag]
    C = c["F"]
    name = "deform_xyz.%s" % tag
    if C <= 4:
        x = fr.uniform(name + ".x", (c["B"], C, c["N"]), -1.0, 1.0, salt=seed)
    else:
        x = fr.normal(name + ".x", (c["B"], C, c["N"]), 0.7, salt=seed)
    pc = fr.uniform(name + ".pc", (c["B"], 3, c["N"]), -1.0, 1.0, salt=seed)
    g = fr.normal(name + ".g", (c["B"], C, c["N"]), salt=seed).bfloat16().float()
    sd = {}
    for (conv, shape), bn in zip(conv_shapes(c).items(), NORMS):
        F_ = norm_width(c, bn)
        b = 1.0 / np.sqrt(shape[1] * shape[3])
        # bfloat16-exact values (held in float32): the stored parameters compress to half their size in the golden file
        sd[conv + ".weight"] = fr.uniform("%s.%s.W" % (name, conv), shape, -b, b, salt=seed).bfloat16().float()
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


def param(d, tag, n):
    """A stored parameter or buffer as a numpy array (`tag|param16|n` holds the upper halves of bfloat16-exact float32 values)"""
    if "%s|param16|%s" % (tag, n) in d:
        return (d["%s|param16|%s" % (tag, n)].astype(np.uint32) << 16).view(np.float32)
    return np.asarray(d["%s|param|%s" % (tag, n)])


def golden_state_dict(d, tag):
    return {n: torch.from_numpy(param(d, tag, n)) for n in STATE_KEYS}


def noise(d, tag, q):
    """The reference's own float32-vs-float64 rel-L2 distance of quantity q (out, dx, dpc, grad|<parameter>, buf|<buffer>)"""
    return float(d[tag + "|noise"][[str(n) for n in d["noise_keys"]].index(q)])


# --------------------------------------------------------------------------------------------- the launchers
def branch(PQ, gidx, sc, sh):
    """-> (a [M,k,F] = lrelu(pre), pre = sc*z + sh, z = Q_i + P_j)"""
    z = pre_norm(PQ, gidx)
    pre = z * sc + sh
    return lrelu(pre), pre, z


def gather2(PQa, PQb, gidx, sca, sha, scb, shb):
    """-> w0 [M*k, F] = a_a * a_b"""
    w0 = branch(PQa, gidx, sca, sha)[0] * branch(PQb, gidx, scb, shb)[0]
    return w0.reshape(-1, w0.shape[2])


def split(dw0, PQa, PQb, gidx, sca, sha, mua, inva, scb, shb, mub, invb):
    """dw0 [M*k, F] -> (ga [M,k,F], sums_a [2F] = [sum ga | sum ga*zhat_a], gb [M,k,F], sums_b [2F])"""
    aa, prea, za = branch(PQa, gidx, sca, sha)
    ab, preb, zb = branch(PQb, gidx, scb, shb)
    d = dw0.view(aa.shape)
    ga, gb = mask(prea) * d * ab, mask(preb) * d * aa

    def sums(g, z, mu, inv):
        return torch.cat([g.sum(dim=(0, 1)), (g * ((z - mu) * inv)).sum(dim=(0, 1))])
    return ga, sums(ga, za, mua, inva), gb, sums(gb, zb, mub, invb)


# --------------------------------------------------------------------------------------------- the layer
def _bn(Y, sd, pre, training, eps, momentum):
    return dm._bn(Y, sd[pre + ".weight"], sd[pre + ".bias"], sd[pre + ".running_mean"], sd[pre + ".running_var"], training, eps, momentum)


def forward(x, pc, idx, k, sd, training, softmax, eps=EPS, momentum=MOMENTUM):
    """x [B,F,N], pc [B,3,N], idx int64 [B,N*k] local, sd = the state_dict in the dtype the model is to run in -> dict (out [B,F,N], the six
    BatchNorm records under their state_dict prefixes).  Differentiable by autograd in x, pc and every floating-point entry of sd."""
    B, C, N = x.shape
    M = B * N
    xp, pp = x.transpose(1, 2).reshape(M, C), pc.transpose(1, 2).reshape(M, 3)
    gidx = global_idx(idx, B, N, k)

    def pq(rows, conv):
        b = sd[conv + ".bias"]
        return rows @ fm._stack(sd[conv + ".weight"]).t() + torch.cat([torch.zeros_like(b), b])
    PQh, PQf, PQx = pq(xp, "inte_conv_hk.0"), pq(xp, "conv_fea.0"), pq(pp, "conv_xyz.0")
    bn = {n: _bn(fm.gather(PQ, gidx), sd, n, training, eps, momentum) for n, PQ in (("inte_conv_hk.1", PQh), ("conv_fea.1", PQf), ("conv_xyz.1", PQx))}
    w0 = gather2(PQf, PQx, gidx, bn["conv_fea.1"]["a"], bn["conv_fea.1"]["s"], bn["conv_xyz.1"]["a"], bn["conv_xyz.1"]["s"])
    z2 = w0 @ sd["conv_all.0.weight"].reshape(F_B, F_A).t() + sd["conv_all.0.bias"]
    bn["conv_all.1"] = _bn(z2, sd, "conv_all.1", training, eps, momentum)
    z3 = lrelu(z2 * bn["conv_all.1"]["a"] + bn["conv_all.1"]["s"]) @ sd["conv_all.3.weight"].reshape(C, F_B).t() + sd["conv_all.3.bias"]
    bn["conv_all.4"] = _bn(z3, sd, "conv_all.4", training, eps, momentum)
    W2 = sd["conv2.0.weight"]
    W2i = W2[:, :, 0, :].permute(0, 2, 1).reshape(W2.shape[0], -1)
    Y = fm.wgemm(PQh, gidx, bn["inte_conv_hk.1"]["a"], bn["inte_conv_hk.1"]["s"], z3.view(M, k, C), bn["conv_all.4"]["a"], bn["conv_all.4"]["s"],
                 softmax, W2i, sd["conv2.0.bias"])
    bn["conv2.1"] = _bn(Y, sd, "conv2.1", training, eps, momentum)
    out_pm = lrelu(Y * bn["conv2.1"]["a"] + bn["conv2.1"]["s"])
    return dict(out=out_pm.view(B, N, -1).transpose(1, 2), bn=bn, PQh=PQh, PQf=PQf, PQx=PQx, w0=w0, z2=z2, z3=z3, Y=Y, gidx=gidx, W2i=W2i)


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
