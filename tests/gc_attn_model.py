"""A plain torch model of spgan.GC_attn and of every launcher of spgan.gc_attn (csrc/gc_attn.hip), of Self_Attn2,
DenseModule2D, MultiDenseMLP and Dense_Attn_2D (Common/utilities.py), and the case table of golden `utilities_rest.npz`.
GC_attn, per sample b over its L flattened positions, x_n in R^C:

    m_n = w . x_n + b_mask,  p = softmax_n(m)  (average pooling: p_n = 1/L),  ctx = sum_n p_n x_n
    branch(ctx) = W2 relu(LayerNorm(W1 ctx + b1)) + b2,  add = branch_add(ctx),  mul = sigmoid(branch_mul(ctx)),  out_n = x_n * mul + add
    backward (g = dout):  dmul = sum_n g_n * x_n,  dadd = sum_n g_n,  dctx from the two branches,
                          s_n = p_n (dctx . x_n - dctx . ctx),  dx_n = g_n * mul + p_n dctx + s_n w,  dw = sum_{b,n} s_n x_n,  db_mask = 0

The model is the yardstick, evaluated in float64 on the CPU (or in the dtype asked for): the forward and the launcher models are written
from the formulas; the module's backward is autograd over the float64 forward (`run`)."""
import numpy as np
import torch

LN_EPS = 1e-5
EPS, MOMENTUM = 1e-5, 0.1
BOTH = ("channel_add", "channel_mul")

# GC_attn: tag -> input shape, out_dim, pool, fusions
GC_CASES = {
    "gc_att": dict(shape=(3, 16, 37), out_dim=None, pool="att", fusions=BOTH),
    "gc_avg": dict(shape=(3, 16, 37), out_dim=5, pool="avg", fusions=BOTH),
    "gc_add": dict(shape=(3, 16, 37), out_dim=None, pool="att", fusions=("channel_add",)),
    "gc_mul": dict(shape=(3, 16, 37), out_dim=None, pool="att", fusions=("channel_mul",)),
    "gc_4d": dict(shape=(2, 16, 11, 4), out_dim=None, pool="att", fusions=BOTH),
}
# Self_Attn2(16); DenseModule2D(6, mlps=[99,8,5,7]); MultiDenseMLP([8,5,7],[6,3,2]); Dense_Attn_2D(6, mlps=[6,8,16], atten)
OTHER_CASES = {
    "sa2_train": dict(kind="sa2", shape=(3, 16, 37), train=True, warm=False, gamma=0.7),
    "sa2_eval": dict(kind="sa2", shape=(3, 16, 37), train=False, warm=True, gamma=0.7),
    "d2_train": dict(kind="d2", shape=(2, 6, 11, 4), mlps=(99, 8, 5, 7), train=True, warm=False),
    "d2_eval": dict(kind="d2", shape=(2, 6, 11, 4), mlps=(99, 8, 5, 7), train=False, warm=True),
    "mdm": dict(kind="mdm", shape=(2, 6, 11, 4), mlps=(8, 5, 7), mlps2=(6, 3, 2), train=True, warm=False),
    "da_gc": dict(kind="da", shape=(2, 6, 11, 4), mlps=(6, 8, 16), atten="gc", train=True, warm=False),
    "da_sa": dict(kind="da", shape=(2, 6, 11, 4), mlps=(6, 8, 16), atten="sa", train=True, warm=False, gamma=0.6),
}
CASES = {**{t: dict(c, kind="gc", train=True) for t, c in GC_CASES.items()}, **OTHER_CASES}


def kind_of(tag):
    return CASES[tag]["kind"]


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


def _dense2d_state(sd, name, prefix, in_dim, mlps, warm, seed):
    cin = in_dim
    for l, w in enumerate(mlps[1:]):
        _conv_entries(sd, name, "%sdense_modules.%d.0" % (prefix, l), (w, cin, 1, 1), seed)
        _bn_entries(sd, name, "%sdense_modules.%d.1" % (prefix, l), w, warm, seed)
        cin += w


def _conv_entries(sd, name, p, shape, seed):
    from spgan import fixture_rng as fr
    bound = 1.0 / np.sqrt(shape[1])
    sd[p + ".weight"] = fr.uniform(name + p + ".W", shape, -bound, bound, salt=seed)
    sd[p + ".bias"] = fr.uniform(name + p + ".b", (shape[0],), -bound, bound, salt=seed)


def gc_state(sd, name, prefix, C, O, pool, fusions, seed):
    """the entries of one GC_attn in the module's key order"""
    from spgan import fixture_rng as fr
    if pool == "att":
        _conv_entries(sd, name, prefix + "conv_mask", (1, C, 1), seed)
    for br in ("channel_add_conv", "channel_mul_conv"):
        if br[:-5] not in fusions:
            continue
        p = prefix + br
        _conv_entries(sd, name, p + ".0", (O, C, 1), seed)
        sd[p + ".1.weight"] = fr.uniform(name + p + ".lnw", (O, 1), 0.5, 1.5, salt=seed)
        sd[p + ".1.bias"] = fr.uniform(name + p + ".lnb", (O, 1), -0.2, 0.2, salt=seed)
        _conv_entries(sd, name, p + ".3", (C, O, 1), seed)


def out_shape(tag):
    c = CASES[tag]
    s = c["shape"]
    return s if c["kind"] in ("gc", "sa2") else (s[0], c["mlps"][-1]) + tuple(s[2:])


def case_tensors(tag, seed=0):
    """(x, cotangent, state_dict in the module's own key order) of a case, from spgan.fixture_rng (float32).  x is a tensor, or the list
    of MultiDenseMLP's inputs."""
    from spgan import fixture_rng as fr
    c = CASES[tag]
    kind = c["kind"]
    name = "utilities_rest.%s" % tag
    shape = c["shape"]
    x = fr.normal(name + ".x", shape, 1.0, salt=seed)
    g = fr.normal(name + ".g", out_shape(tag), 1.0, salt=seed)
    sd = {}
    C = shape[1]
    if kind == "gc":
        gc_state(sd, name, "", C, c["out_dim"] or C, c["pool"], c["fusions"], seed)
    elif kind == "sa2":
        sd["gamma"] = torch.full((1,), c["gamma"])
        for n, w in (("query", C // 8), ("key", C // 8), ("value", C)):
            _conv_entries(sd, name, n + ".0", (w, C, 1), seed)
            _bn_entries(sd, name, n + ".1", w, c["warm"], seed)
    elif kind == "d2":
        _dense2d_state(sd, name, "", C, c["mlps"], c["warm"], seed)
    elif kind == "mdm":
        x = [x] + [fr.normal(name + ".x%d" % i, (shape[0], w) + tuple(shape[2:]), 1.0, salt=seed) for i, w in enumerate(c["mlps2"]) if i]
        cin = c["mlps2"][0]
        for l, w in enumerate(c["mlps"]):
            _conv_entries(sd, name, "dense_modules.%d.0" % l, (w, cin, 1, 1), seed)
            _bn_entries(sd, name, "dense_modules.%d.1" % l, w, c["warm"], seed)
            if l < len(c["mlps"]) - 1:
                cin += w + c["mlps2"][l + 1]
    else:
        Ca = c["mlps"][-1]
        if c["atten"] == "gc":
            gc_state(sd, name, "atten.", Ca, Ca, "att", BOTH, seed)
        else:
            sd["atten.gamma"] = torch.full((1,), c["gamma"])
            for n, w in (("query", Ca // 8), ("key", Ca // 8), ("value", Ca)):
                _conv_entries(sd, name, "atten." + n, (w, Ca, 1), seed)
        _dense2d_state(sd, name, "dense.", C, c["mlps"], c["warm"], seed)
    return x, g, sd


def zero_gradient(tag, q):
    """Is quantity q a gradient that is exactly zero in exact arithmetic (rounding noise in the reference)?  -> "exact" (the modules
    return exact zeros) or None.  conv_mask.bias shifts every logit of a sample alike, which the softmax cancels; a conv bias in front of
    a train-mode BatchNorm is absorbed by the batch mean; Self_Attn's query.bias adds a term to the scores that does not depend on the
    index the softmax normalises over."""
    if not q.startswith("grad|"):
        return None
    c = CASES[tag]
    if q.endswith("conv_mask.bias") or q == "grad|atten.query.bias":
        return "exact"
    if c["train"] and q.endswith(".0.bias") and ("dense_modules" in q or c["kind"] == "sa2"):
        return "exact"
    return None


def build_module(ns, tag):
    """The module of a case from a namespace that has the classes (spgan, or the executed reference)"""
    c = CASES[tag]
    kind = c["kind"]
    if kind == "gc":
        return ns.GC_attn(c["shape"][1], c["out_dim"], c["pool"], list(c["fusions"]))
    if kind == "sa2":
        return ns.Self_Attn2(c["shape"][1])
    if kind == "d2":
        return ns.DenseModule2D(in_dim=c["shape"][1], mlps=list(c["mlps"]))
    if kind == "mdm":
        return ns.MultiDenseMLP(list(c["mlps"]), list(c["mlps2"]))
    return ns.Dense_Attn_2D(c["shape"][1], mlps=list(c["mlps"]), atten=c["atten"])


INIT_SEED = 1234        # the golden's `tag|init|*`: the reference module's initial values under this torch seed
INIT_TAGS = ("gc_att", "gc_avg", "sa2_train", "d2_train", "mdm", "da_gc")        # one per class; gc_avg: the module without conv_mask


def golden_state_dict(d, tag, what="param"):
    pre = "%s|%s|" % (tag, what)
    return {n[len(pre):]: torch.from_numpy(np.asarray(d[n])) for n in d.files if n.startswith(pre)}


def golden_f64(d, tag, q):
    """The reference's float64 result of quantity q: the golden stores it as its (float32-rounded) distance from the float32 run"""
    return torch.from_numpy(np.asarray(d["%s|%s|full" % (tag, q)])).double() + torch.from_numpy(np.asarray(d["%s|%s|d64|full" % (tag, q)])).double()


def quantities(d, tag):
    pre, suf = "%s|" % tag, "|d64|full"
    return [n[len(pre):-len(suf)] for n in d.files if n.startswith(pre) and n.endswith(suf)]


# ----------------------------------------------------------------------------- forward, from the formulas
def pool_model(x, w=None, bias=None):
    """x [B,C,L] -> dict(ctx [B,C], p [B,L], m [B,L] or None, lse [B]) in x's dtype"""
    B, C, L = x.shape
    if w is None:
        p = torch.full((B, L), 1.0 / L, dtype=x.dtype, device=x.device)
        m, lse = None, torch.full((B,), float(np.log(L)), dtype=x.dtype, device=x.device)
    else:
        m = torch.einsum("c,bcl->bl", w.reshape(-1), x) + (0.0 if bias is None else bias.reshape(()))
        p = torch.softmax(m, dim=1)
        lse = torch.logsumexp(m, dim=1)
    return dict(ctx=torch.einsum("bl,bcl->bc", p, x), p=p, m=m, lse=lse)


def branch_hidden(ctx, prm):
    """ctx [B,C], prm = (W1 [O,C], b1, ln.weight, ln.bias, W2 [C,O], b2) -> (h, xhat, hn): the first convolution's output, its normalised
    form and the LayerNorm's output (the ReLU's pre-activation), each [B,O]"""
    W1, b1, lw, lb = (t.reshape(t.shape[0], -1) if i == 0 else t.reshape(-1) for i, t in enumerate(prm[:4]))
    h = ctx @ W1.t() + b1
    mean = h.mean(dim=1, keepdim=True)
    var = ((h - mean) ** 2).mean(dim=1, keepdim=True)
    xhat = (h - mean) / torch.sqrt(var + LN_EPS)
    return h, xhat, xhat * lw + lb


def branch_model(ctx, prm, sigmoid):
    W2, b2 = prm[4].reshape(prm[4].shape[0], -1), prm[5].reshape(-1)
    t = torch.relu(branch_hidden(ctx, prm)[2]) @ W2.t() + b2
    return torch.sigmoid(t) if sigmoid else t


def branch_params(sd, prefix, name):
    """the six tensors of channel_<name>_conv, or None"""
    p = "%schannel_%s_conv" % (prefix, name)
    if p + ".0.weight" not in sd:
        return None
    return tuple(sd[p + k] for k in (".0.weight", ".0.bias", ".1.weight", ".1.bias", ".3.weight", ".3.bias"))


def gc_forward(x, sd, prefix=""):
    """x [B,C,...] -> dict(out of x's shape, ctx, pre = the ReLU pre-activations of every branch, one tensor [B, O] each)"""
    size = x.shape
    f = x.reshape(size[0], size[1], -1)
    add_p, mul_p = branch_params(sd, prefix, "add"), branch_params(sd, prefix, "mul")
    if add_p is None and mul_p is None:
        return dict(out=x, ctx=None, pre=[])
    w = sd.get(prefix + "conv_mask.weight")
    pool = pool_model(f, w, sd.get(prefix + "conv_mask.bias"))
    out, pre = f, []
    if mul_p is not None:
        out = out * branch_model(pool["ctx"], mul_p, True).unsqueeze(2)
        pre.append(branch_hidden(pool["ctx"], mul_p)[2])
    if add_p is not None:
        out = out + branch_model(pool["ctx"], add_p, False).unsqueeze(2)
        pre.append(branch_hidden(pool["ctx"], add_p)[2])
    return dict(out=out.reshape(size), ctx=pool["ctx"], pre=pre)


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
    return (z - mean) / torch.sqrt(var + EPS) * sd[p + ".weight"] + sd[p + ".bias"]


def lrelu(v, slope):
    return torch.where(v > 0, v, slope * v)


def conv_bn_act(rows, sd, p, training, bufs, pre, slope):
    """rows [..., K] -> act(bn(rows W^T + b)) for the Sequential(conv, bn, act) at prefix p; the pre-activation is appended to pre"""
    W = sd[p + ".0.weight"]
    z = batch_norm(rows @ W.reshape(W.shape[0], W.shape[1]).t() + sd[p + ".0.bias"], sd, p + ".1", training, bufs)
    pre.append(z)
    return lrelu(z, slope)


def _rows(x):
    """[B,C,...] -> [B,L,C]"""
    return x.reshape(x.shape[0], x.shape[1], -1).transpose(1, 2)


def _unrows(r, like):
    return r.transpose(1, 2).reshape((like.shape[0], r.shape[2]) + tuple(like.shape[2:]))


def dense2d_forward(x, sd, training, prefix=""):
    """DenseModule2D: every level reads cat[x, y_1 .. y_{l-1}]"""
    L = len([n for n in sd if n.startswith(prefix + "dense_modules.") and n.endswith(".0.weight")])
    bufs, pre = {}, []
    feats, y = _rows(x), None
    for l in range(L):
        y = conv_bn_act(feats, sd, "%sdense_modules.%d" % (prefix, l), training, bufs, pre, 0.2)
        feats = torch.cat([feats, y], dim=-1)
    return dict(out=_unrows(y, x), bufs=bufs, pre=pre)


def multi_dense_forward(xs, sd, training):
    """MultiDenseMLP: pc = cat[pc, y_i, x[i+1]], ReLU"""
    L = len(xs)
    bufs, pre = {}, []
    pc, y = _rows(xs[0]), None
    for l in range(L):
        y = conv_bn_act(pc, sd, "dense_modules.%d" % l, training, bufs, pre, 0.0)
        if l < L - 1:
            pc = torch.cat([pc, y, _rows(xs[l + 1])], dim=-1)
    return dict(out=_unrows(y, xs[0]), bufs=bufs, pre=pre)


def _attend(q, k, v):
    """q, k [B,L,d], v [B,L,dv] -> out_j = sum_i softmax_i(q_i . k_j) v_i   [B,L,dv]"""
    return torch.softmax(q @ k.transpose(1, 2), dim=1).transpose(1, 2) @ v


def self_attn2_forward(x, sd, training):
    bufs, pre = {}, []
    r = _rows(x)
    q, k, v = (conv_bn_act(r, sd, n, training, bufs, pre, 0.2) for n in ("query", "key", "value"))
    return dict(out=sd["gamma"] * _unrows(_attend(q, k, v), x) + x, bufs=bufs, pre=pre)


def self_attn_forward(x, sd, prefix):
    r = _rows(x)

    def conv(n):
        W = sd[prefix + n + ".weight"]
        return r @ W.reshape(W.shape[0], W.shape[1]).t() + sd[prefix + n + ".bias"]
    return sd[prefix + "gamma"] * _unrows(_attend(conv("query"), conv("key"), conv("value")), x) + x


def dense_attn2d_forward(x, sd, training):
    f = dense2d_forward(x, sd, training, prefix="dense.")
    if "atten.gamma" in sd:
        f["out"] = self_attn_forward(f["out"], sd, "atten.")
    else:
        a = gc_forward(f["out"], sd, "atten.")
        f["out"], f["pre"] = a["out"], f["pre"] + a["pre"]
    return f


def forward(tag, x, sd):
    c = CASES[tag]
    kind = c["kind"]
    if kind == "gc":
        return dict(gc_forward(x, sd), bufs={})
    if kind == "sa2":
        return self_attn2_forward(x, sd, c["train"])
    if kind == "d2":
        return dense2d_forward(x, sd, c["train"])
    if kind == "mdm":
        return multi_dense_forward(x, sd, c["train"])
    return dense_attn2d_forward(x, sd, c["train"])


def input_names(tag):
    return ["x"] + (["x%d" % i for i in range(1, len(CASES[tag]["mlps2"]))] if CASES[tag]["kind"] == "mdm" else [])


def run(tag, x, g, sd, dtype=torch.float64):
    """One model forward + backward: -> dict with the golden's quantities (out, dx [dx1 ..], grad|<parameter>, buf|<buffer>) and pre"""
    s = {}
    for n, v in sd.items():
        s[n] = v.to(dtype).clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in n else \
            (v.to(dtype) if v.dtype.is_floating_point else v.clone())
    xs = [t.to(dtype).clone().requires_grad_(True) for t in (x if isinstance(x, (list, tuple)) else [x])]
    f = forward(tag, xs if isinstance(x, (list, tuple)) else xs[0], s)
    (f["out"] * g.to(dtype)).sum().backward()
    res = {"out": f["out"].detach(), "pre": [t.detach() for t in f["pre"]]}
    for n, t in zip(input_names(tag), xs):
        res["d" + n] = t.grad
    for n, v in s.items():
        if v.dtype.is_floating_point and v.requires_grad:
            res["grad|" + n] = v.grad if v.grad is not None else torch.zeros_like(v)
    for n, v in f["bufs"].items():
        res["buf|" + n] = v
    return res


def kink_margin(pre):
    """the smallest |pre-activation| in front of a ReLU / LeakyReLU relative to its column's largest (a GC branch: to its tensor's
    largest, over all B*O values), over every tensor of `pre`"""
    def one(t):
        if t.dim() == 2:                                        # a GC branch [B,O]
            return float(t.abs().min() / t.abs().max())
        c = t.reshape(-1, t.shape[-1]).abs()
        return float((c.min(dim=0)[0] / c.max(dim=0)[0]).min())
    return min(one(t) for t in pre) if pre else float("inf")


# ----------------------------------------------------------------------------- the launchers (channel-major operands [B,C,L]; a point-major
# launcher's operands are transposed by the caller), every operand converted to `dtype` on the CPU
def _d(t, dtype=torch.float64):
    return None if t is None else t.detach().to(dtype).cpu()


def apply_model(x, mul, add, dtype=torch.float64):
    x, mul, add = _d(x, dtype), _d(mul, dtype), _d(add, dtype)
    out = x if mul is None else x * mul.unsqueeze(2)
    return out if add is None else out + add.unsqueeze(2)


def bwd_reduce_model(x, g, dtype=torch.float64):
    x, g = _d(x, dtype), _d(g, dtype)
    return (g * x).sum(dim=2), g.sum(dim=2)


def bwd_apply_model(x, g, mul, dctx, w=None, bias=None, dtype=torch.float64):
    """-> (dx [B,C,L], dw [C] or None) from the formulas of the head; p is recomputed from x, w, bias"""
    x, g, mul, dctx, w, bias = (_d(t, dtype) for t in (x, g, mul, dctx, w, bias))
    pool = pool_model(x, w, bias)
    p = pool["p"]
    dx = (g if mul is None else g * mul.unsqueeze(2)) + p.unsqueeze(1) * dctx.unsqueeze(2)
    if w is None:
        return dx, None
    s = p * (torch.einsum("bc,bcl->bl", dctx, x) - (dctx * pool["ctx"]).sum(dim=1, keepdim=True))
    return dx + s.unsqueeze(1) * w.reshape(1, -1, 1), torch.einsum("bl,bcl->c", s, x)


def channel_model(ctx, add_p, mul_p, dadd=None, dmul=None, dtype=torch.float64):
    """Both branches forward and, with cotangents of add / mul, backward by autograd over the float64 formulas:
    -> dict(add, mul, dctx, grads = {branch: six tensors})"""
    ctx = _d(ctx, dtype).requires_grad_(True)
    prm = {n: (None if p is None else [_d(t, dtype).requires_grad_(True) for t in p]) for n, p in (("add", add_p), ("mul", mul_p))}
    add = None if prm["add"] is None else branch_model(ctx, prm["add"], False)
    mul = None if prm["mul"] is None else branch_model(ctx, prm["mul"], True)
    out = dict(add=None if add is None else add.detach(), mul=None if mul is None else mul.detach())
    if dadd is None and dmul is None:
        return out
    loss = 0.0
    if add is not None:
        loss = loss + (add * _d(dadd, dtype)).sum()
    if mul is not None:
        loss = loss + (mul * _d(dmul, dtype)).sum()
    loss.backward()
    out["dctx"] = ctx.grad
    out["grads"] = {n: [t.grad for t in p] for n, p in prm.items() if p is not None}
    return out
