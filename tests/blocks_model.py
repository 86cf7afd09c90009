"""A plain torch model of the bilateral / deform blocks (spgan.modules.bilateral_block ... deform_block_feat; Generation/modules.py:928-1391),
composed from the layer models (upsample_model, bilateral_model, deform_xyz_model, deform_feat_model), float64 models of the four
block-tail launchers (csrc/block_tail.hip), and the case table of golden `blocks.npz`.

With y [B,F,L] the block's edge convolution (L = N or 2N), p = max over the points of x:

    xs    = lrelu(bn(fc.3 lrelu(bn(fc.0 p))))                     [B,Fout]     the BatchNorm1d's run over the B rows
    g     = lrelu(bn(g_fc.0 xs))                                  [B,512]
    x_ec  = lrelu(bn_uc(y))                                        [B,F,L]      BatchNorm1d over B*L values per channel
    x_out = cat[xs broadcast, x_ec]   g_out = cat[g broadcast, x_ec]
    middle blocks: x_out = lrelu(bn(add_cov.0 cat[xs broadcast, x_ec]))        [B,Fout,L]

Everything is materialised; float64 or float32 by the dtype of the arguments."""
import numpy as np
import torch

import bilateral_model as bm
import deform_feat_model as fm
import deform_model as dm
import deform_xyz_model as xm
import upsample_model as um
from deform_model import EPS, MOMENTUM, lrelu
from deform_feat_model import golden_pair, mask                              # noqa: F401
from deform_xyz_model import param                                           # noqa: F401

SLOPE = 0.01
# block -> (layer model, the layer's state_dict prefix, the block BatchNorm's prefix, takes pc, has g_fc, has add_cov, doubles the points)
BLOCKS = {
    "bilateral_block":          ("up", "upsample_cov.0.", "upsample_cov.1", False, False, False, True),
    "bilateral_block_l1":       ("up", "upsample_cov.0.", "upsample_cov.1", False, True, False, True),
    "bilateral_block_l2":       ("bi", "upsample_cov.", "bn_uc", True, True, False, True),
    "bilateral_block_l3":       ("bi", "upsample_cov.", "bn_uc", True, True, False, True),
    "bilateral_block_l4":       ("bi", "upsample_cov.", "bn_uc", True, False, False, True),
    "deform_block_middle":      ("xyz", "deform_cov.", "bn_uc", True, True, True, False),
    "deform_block_tail":        ("xyz", "deform_cov.", "bn_uc", True, False, False, False),
    "deform_block_feat_middle": ("feat", "deform_cov.", "bn_uc", False, False, True, False),
    "deform_block_feat":        ("feat", "deform_cov.", "bn_uc", False, True, True, False),
}
STATE_COUNTS = {"bilateral_block": 33, "bilateral_block_l1": 40, "bilateral_block_l2": 68, "bilateral_block_l3": 68, "bilateral_block_l4": 61,
                "deform_block_middle": 75, "deform_block_tail": 61, "deform_block_feat_middle": 61, "deform_block_feat": 68}


def _case(block, N=24, Fout=16, num_k=4, train=True, warm=False):
    return dict(block=block, B=4, N=N, Fin=8, Fout=Fout, num_k=num_k, train=train, warm=warm)


# B 4 (a BatchNorm1d over two rows only yields +-1), N 24, Fin 8, Fout 16 (8 where the layer needs Fin == Fout), num_k 4
CASES = {
    "bb": _case("bilateral_block"),
    "l1": _case("bilateral_block_l1"),
    "l2": _case("bilateral_block_l2"),
    "l3": _case("bilateral_block_l3"),
    "l4": _case("bilateral_block_l4"),
    "dm": _case("deform_block_middle", Fout=8),
    "dt": _case("deform_block_tail", Fout=8),
    "fm": _case("deform_block_feat_middle"),
    "df": _case("deform_block_feat"),
    "l2e": _case("bilateral_block_l2", train=False, warm=True),               # eval mode, warmed running statistics
    "dfe": _case("deform_block_feat", train=False, warm=True),
    "dm23": _case("deform_block_middle", N=23, Fout=8),                        # rows of 23 floats: not 16-byte aligned
    "df1": _case("deform_block_feat", num_k=1),                                # one neighbour
}
SAMPLE_STRIDE, SAMPLE_MIN = 29, 8192
FILE2 = ("l4", "df", "l2e", "dfe", "dm23", "df1")      # the cases stored in blocks2.npz (each file stays under 1 MiB)


def load_golden():
    """blocks.npz and blocks2.npz as one dict"""
    from helpers import golden
    out = {}
    for name in ("blocks.npz", "blocks2.npz"):
        f = golden(name)
        out.update({k: f[k] for k in f.files})
    for key in [k for k in out if k.endswith("|packed")]:       # the small float32 arrays of a case, stored as one
        flat, at = out.pop(key), 0
        for entry in out.pop(key + "_names"):
            name, dims = str(entry).split(";")
            shape = tuple(int(s_) for s_ in dims.split(",")) if dims else ()
            n = int(np.prod(shape))
            out[name] = flat[at:at + n].reshape(shape)
            at += n
    return out


def layer_k(c):
    return c["num_k"] // 2 if BLOCKS[c["block"]][6] else c["num_k"]


def out_shapes(c):
    """-> (shape of x_out, shape of g_out | None)"""
    _, _, _, _, has_g, add, up = BLOCKS[c["block"]]
    L = 2 * c["N"] if up else c["N"]
    return (c["B"], c["Fout"] if add else 2 * c["Fout"], L), ((c["B"], 512 + c["Fout"], L) if has_g else None)


def make_module(c, spgan):
    cls = getattr(spgan, c["block"])
    if c["block"].startswith("bilateral"):
        return cls(c["Fin"], c["Fout"], c["N"], num_k=c["num_k"])
    return cls(c["Fin"], c["Fout"], num_k=c["num_k"])


def zero_grad_biases(keys):
    """the conv / linear biases in front of a train-mode BatchNorm: every bias that is not a BatchNorm's own"""
    keys = set(keys)
    return tuple(n for n in keys if n.endswith(".bias") and n[:-5] + ".running_mean" not in keys)


def cotangents(tag, seed=0):
    """(cotangent of x_out, cotangent of g_out | None): bfloat16-exact values from spgan.fixture_rng.  The golden stores the seed and the
    tensors' sums instead of the tensors."""
    from spgan import fixture_rng as fr
    sx, sg = out_shapes(CASES[tag])
    name = "blocks.%s" % tag
    return (fr.normal(name + ".gx", sx, salt=seed).bfloat16().float(),
            None if sg is None else fr.normal(name + ".gg", sg, salt=seed).bfloat16().float())


def golden_cotangents(d, tag):
    gx, gg = cotangents(tag, int(d[tag + "|seed"]))
    assert gx.double().sum().item() == d[tag + "|gsum"][0] and (gg is None or gg.double().sum().item() == d[tag + "|gsum"][1]), tag
    return gx, gg


def case_tensors(tag, seed=0):
    """(x [B,Fin,N], pc [B,3,N], cotangent of x_out, cotangent of g_out | None, state_dict) of a case, from spgan.fixture_rng (float32).
    Matrices of more than 1024 elements hold bfloat16-exact values: the golden stores their upper halves."""
    import spgan
    from spgan import fixture_rng as fr
    c = CASES[tag]
    name = "blocks.%s" % tag
    x = fr.normal(name + ".x", (c["B"], c["Fin"], c["N"]), 0.7, salt=seed)
    pc = fr.uniform(name + ".pc", (c["B"], 3, c["N"]), -1.0, 1.0, salt=seed)
    gx, gg = cotangents(tag, seed)
    shapes = {n: tuple(v.shape) for n, v in make_module(c, spgan).state_dict().items()}
    sd = {}
    for n, shape in shapes.items():
        pre, leaf = n.rsplit(".", 1)
        is_bn = pre + ".running_mean" in shapes
        if leaf == "num_batches_tracked":
            sd[n] = torch.tensor(21 if c["warm"] else 0, dtype=torch.int64)
        elif leaf == "running_mean":
            sd[n] = fr.normal("%s.%s" % (name, n), shape, 0.1, salt=seed) if c["warm"] else torch.zeros(shape)
        elif leaf == "running_var":
            sd[n] = fr.uniform("%s.%s" % (name, n), shape, 0.5, 1.5, salt=seed) if c["warm"] else torch.ones(shape)
        elif is_bn:
            sd[n] = fr.uniform("%s.%s" % (name, n), shape, 0.5, 1.5, salt=seed) if leaf == "weight" else fr.uniform("%s.%s" % (name, n), shape, -0.2, 0.2, salt=seed)
        else:
            ws = shapes[pre + ".weight"]
            b = 1.0 / np.sqrt(int(np.prod(ws[1:])))
            v = fr.uniform("%s.%s" % (name, n), shape, -b, b, salt=seed)
            sd[n] = v.bfloat16().float() if leaf == "weight" else v
    return x, pc, gx, gg, sd


def golden_state_dict(d, tag):
    return {str(n): torch.from_numpy(param(d, tag, str(n))) for n in d["state_keys|" + CASES[tag]["block"]]}


def noise(d, tag, q):
    """The reference's own float32-vs-float64 rel-L2 distance of quantity q"""
    return float(d[tag + "|noise"][[str(n) for n in d[tag + "|noise_keys"]].index(q)])


# --------------------------------------------------------------------------------------------- the launchers (spgan_cm_stats, spgan_block_tail_*)
def cm_stats(Y):
    """Y [B,C,L] -> (mean [C], biased var [C]) over the B*L values of a channel"""
    rows = Y.transpose(1, 2).reshape(-1, Y.shape[1])
    return dm.colstats(rows)


def tail_fwd(Y, xs, g, scale, shift):
    """-> (out_x = cat[xs broadcast, a], out_g = cat[g broadcast, a] | None), a = lrelu(scale*Y + shift); xs None: no broadcast channels"""
    B, C, L = Y.shape
    a = lrelu(Y * scale.view(1, C, 1) + shift.view(1, C, 1))
    rep = lambda v: v.view(B, -1, 1).expand(B, v.shape[1], L)
    return (a if xs is None else torch.cat([rep(xs), a], dim=1)), (None if g is None else torch.cat([rep(g), a], dim=1))


def tail_gact(Y, dout_x, dout_g, extra, Cs, Cg, scale, shift):
    C = Y.shape[1]
    tot = torch.zeros_like(Y)
    for t, off in ((dout_x, Cs), (dout_g, Cg), (extra, 0)):
        if t is not None:
            tot = tot + t[:, off:off + C]
    return tot * mask(Y * scale.view(1, C, 1) + shift.view(1, C, 1))


def tail_bwd(Y, dout_x, dout_g, extra, Cs, Cg, scale, shift, mean, invstd, gamma, train):
    """-> (sums [2C] = [sum gact | sum gact*yhat], dxs [B,Cs], dg [B,Cg], dY)"""
    B, C, L = Y.shape
    ga = tail_gact(Y, dout_x, dout_g, extra, Cs, Cg, scale, shift)
    yhat = (Y - mean.view(1, C, 1)) * invstd.view(1, C, 1)
    s0, s1 = ga.sum(dim=(0, 2)), (ga * yhat).sum(dim=(0, 2))
    dxs = torch.zeros(B, Cs, dtype=Y.dtype) if dout_x is None else dout_x[:, :Cs].sum(dim=2)
    dg = torch.zeros(B, Cg, dtype=Y.dtype) if dout_g is None else dout_g[:, :Cg].sum(dim=2)
    if train:
        n = B * L
        dY = (gamma * invstd).view(1, C, 1) * (ga - (s0 / n).view(1, C, 1) - yhat * (s1 / n).view(1, C, 1))
    else:
        dY = scale.view(1, C, 1) * ga
    return torch.cat([s0, s1]), dxs, dg, dY


# --------------------------------------------------------------------------------------------- the blocks
def _bn(Y, sd, pre, training, eps=EPS, momentum=MOMENTUM):
    return dm._bn(Y, sd[pre + ".weight"], sd[pre + ".bias"], sd[pre + ".running_mean"], sd[pre + ".running_var"], training, eps, momentum)


def _layer(kind, x, pc, idx, k, sd, training):
    """-> (y [B,F,L], the layer's BatchNorm records under their prefixes)"""
    if kind == "up":
        f = um.forward(x, idx, k, sd, training)
        return f["out"], {"inte_conv_hk.1": f["bn1"], "conv2.bn": f["bn2"]}
    if kind == "bi":
        f = bm.forward(x, pc, idx, k, sd, training, True)
    elif kind == "xyz":
        f = xm.forward(x, pc, idx, k, sd, training, True)
    else:
        f = fm.forward(x, idx, k, sd, training, True)
    return f["out"], f["bn"]


def forward(block, x, pc, idx, k, sd, training):
    """x [B,Fin,N], pc [B,3,N] | None, idx int64 [B,N*k] local, sd = the block's state_dict in the dtype the model is to run in ->
    dict(x_out, g_out | None, bn = the BatchNorm records under their state_dict prefixes).  Differentiable by autograd."""
    kind, lpre, bnp, _, has_g, add, _ = BLOCKS[block]
    y, recs = _layer(kind, x, pc, idx, k, {n[len(lpre):]: v for n, v in sd.items() if n.startswith(lpre)}, training)
    bn = {lpre + n: r for n, r in recs.items()}
    B, F, L = y.shape
    p = x.max(dim=2)[0]
    h = p @ sd["fc.0.weight"].t() + sd["fc.0.bias"]
    bn["fc.1"] = _bn(h, sd, "fc.1", training)
    h = lrelu(h * bn["fc.1"]["a"] + bn["fc.1"]["s"]) @ sd["fc.3.weight"].t() + sd["fc.3.bias"]
    bn["fc.4"] = _bn(h, sd, "fc.4", training)
    xs = lrelu(h * bn["fc.4"]["a"] + bn["fc.4"]["s"])
    g = None
    if has_g:
        h = xs @ sd["g_fc.0.weight"].t() + sd["g_fc.0.bias"]
        bn["g_fc.1"] = _bn(h, sd, "g_fc.1", training)
        g = lrelu(h * bn["g_fc.1"]["a"] + bn["g_fc.1"]["s"])
    rows = y.transpose(1, 2).reshape(B * L, F)
    bn[bnp] = _bn(rows, sd, bnp, training)
    x_out, g_out = tail_fwd(y, xs, g, bn[bnp]["a"], bn[bnp]["s"])
    if add:
        W = sd["add_cov.0.weight"]
        z = x_out.transpose(1, 2).reshape(B * L, -1) @ W.reshape(W.shape[0], -1).t() + sd["add_cov.0.bias"]
        bn["add_cov.1"] = _bn(z, sd, "add_cov.1", training)
        x_out = lrelu(z * bn["add_cov.1"]["a"] + bn["add_cov.1"]["s"]).view(B, L, -1).transpose(1, 2)
    return dict(x_out=x_out, g_out=g_out, bn=bn)


def run(block, x, pc, idx, gx, gg, k, sd, training):
    """forward + autograd backward in the dtype of x -> {x_out, g_out, dx, dpc, grad|<parameter>, buf|<buffer>} (num_batches_tracked left
    out; g_out / dpc only where the block has them)"""
    x = x.clone().requires_grad_(True)
    pc = pc.clone().requires_grad_(True) if BLOCKS[block][3] else None
    sd = {n: (v.clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in n else v) for n, v in sd.items()}
    f = forward(block, x, pc, idx, k, sd, training)
    loss = (f["x_out"] * gx).sum()
    if f["g_out"] is not None:
        loss = loss + (f["g_out"] * gg).sum()
    loss.backward()
    got = {"x_out": f["x_out"].detach(), "dx": x.grad}
    if f["g_out"] is not None:
        got["g_out"] = f["g_out"].detach()
    if pc is not None:
        got["dpc"] = pc.grad if pc.grad is not None else torch.zeros_like(pc)
    for n, v in sd.items():
        if v.requires_grad:
            got["grad|" + n] = v.grad if v.grad is not None else torch.zeros_like(v)
    for pre, rec in f["bn"].items():
        got["buf|%s.running_mean" % pre], got["buf|%s.running_var" % pre] = rec["running_mean"].detach(), rec["running_var"].detach()
    return got
