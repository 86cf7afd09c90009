"""A torch model of the pointnet2 extension (spgan.pointnet2_utils, spgan.pytorch_utils, spgan.pointnet2_modules),
written from the stated semantics: sequential loops for the ball query and farthest point sampling, a stable sort for the three nearest,
torch.gather for the gathers, plain tensor algebra and autograd for the modules.  Every function works in the dtype of its inputs
(float32: the kernels' rounding order for distances, d2 = (dx*dx + dy*dy) + dz*dz with dx = centre - candidate; float64: the exact
reference of the module tests).  `cuda_stand_in` wraps the ops in the calling convention of the reference's native extension, for
tests/golden/make_golden_pointnet2_ext.py."""
import types

import numpy as np
import torch

BN_EPS, BN_MOMENTUM = 1e-5, 0.1


# ------------------------------------------------------------------------------------------------------------------------ ops
def dist2(query, cloud):
    """query [B,m,3], cloud [B,n,3] -> [B,m,n] in the inputs' dtype, every operation rounded on its own."""
    d = query[:, :, None, :] - cloud[:, None, :, :]
    sq = d * d
    return (sq[..., 0] + sq[..., 1]) + sq[..., 2]


def radius2(radius, dtype):
    r = torch.tensor(float(radius), dtype=dtype)
    return r * r


def ball_query(radius, nsample, xyz, new_xyz):
    """-> int32 [B,m,nsample]: index order, strict d2 < r*r; the first hit fills every slot, later hits overwrite slots 1 ..; the walk
    ends at nsample hits; an empty ball keeps zeros."""
    hits = (dist2(new_xyz, xyz) < radius2(radius, xyz.dtype)).numpy()
    B, m, n = hits.shape
    idx = np.zeros((B, m, nsample), dtype=np.int32)
    for b in range(B):
        for j in range(m):
            cnt = 0
            for k in range(n):
                if hits[b, j, k]:
                    if cnt == 0:
                        idx[b, j, :] = k
                    idx[b, j, cnt] = k
                    cnt += 1
                    if cnt >= nsample:
                        break
    return torch.from_numpy(idx)


def furthest_point_sample(xyz, npoint):
    """-> int32 [B,npoint]: starts at point 0; every later pick is the first maximum of the running minimum distance."""
    B, n, _ = xyz.shape
    out = np.zeros((B, npoint), dtype=np.int32)
    for b in range(B):
        best = torch.full((n,), 1e10, dtype=xyz.dtype)
        last = 0
        for j in range(1, npoint):
            best = torch.minimum(best, dist2(xyz[b:b + 1, last:last + 1], xyz[b:b + 1])[0, 0])
            last = int(torch.argmax(best))
            out[b, j] = last
    return torch.from_numpy(out)


def fps_margin(xyz, npoint):
    """The least gap between the picked maximum and the runner-up over all picks (float64)."""
    x = xyz.double()
    B, n, _ = x.shape
    gap = np.inf
    for b in range(B):
        best = torch.full((n,), 1e10, dtype=torch.float64)
        last = 0
        for j in range(1, npoint):
            best = torch.minimum(best, dist2(x[b:b + 1, last:last + 1], x[b:b + 1])[0, 0])
            top = torch.topk(best, min(2, n))[0]
            if n > 1:
                gap = min(gap, float(top[0] - top[1]))
            last = int(torch.argmax(best))
    return gap


def three_nn_d2(unknown, known):
    """-> (d2 [B,n,3], idx int32 [B,n,3]): ascending (d2, index); with fewer than 3 known the rest is index 0, +inf."""
    d = dist2(unknown, known)
    B, n, m = d.shape
    order = torch.from_numpy(np.argsort(d.numpy(), axis=2, kind="stable"))
    k = min(3, m)
    idx = torch.zeros((B, n, 3), dtype=torch.int64)
    d2 = torch.full((B, n, 3), float("inf"), dtype=d.dtype)
    idx[:, :, :k] = order[:, :, :k]
    d2[:, :, :k] = torch.gather(d, 2, order[:, :, :k])
    return d2, idx.to(torch.int32)


def three_nn(unknown, known):
    """-> (dist = sqrt(d2), idx)."""
    d2, idx = three_nn_d2(unknown, known)
    return torch.sqrt(d2), idx


def gather_operation(features, idx):
    """features [B,C,N], idx [B,npoint] -> [B,C,npoint]."""
    B, C, _ = features.shape
    return torch.gather(features, 2, idx.long().unsqueeze(1).expand(B, C, idx.shape[1]))


def grouping_operation(features, idx):
    """features [B,C,N], idx [B,npoint,nsample] -> [B,C,npoint,nsample]."""
    B, C, _ = features.shape
    _, m, K = idx.shape
    return torch.gather(features, 2, idx.reshape(B, 1, m * K).long().expand(B, C, m * K)).reshape(B, C, m, K)


def three_interpolate(features, idx, weight):
    """features [B,C,M], idx / weight [B,n,3] -> [B,C,n] = (w0*f0 + w1*f1) + w2*f2."""
    B, C, _ = features.shape
    n = idx.shape[1]
    f = torch.gather(features, 2, idx.reshape(B, 1, n * 3).long().expand(B, C, n * 3)).reshape(B, C, n, 3)
    t = f * weight.unsqueeze(1)
    return (t[..., 0] + t[..., 1]) + t[..., 2]


def group_all(use_xyz, xyz, features):
    grouped_xyz = xyz.transpose(1, 2).unsqueeze(2)
    if features is None:
        return grouped_xyz
    return torch.cat([grouped_xyz, features.unsqueeze(2)], dim=1) if use_xyz else features.unsqueeze(2)


def cuda_stand_in():
    """The native extension's entry points (results written into the caller's tensors) over the functions above."""
    m = types.ModuleType("pointnet2_cuda")

    def scatter_add(grad_features, idx_flat, grad_flat):
        grad_features.scatter_add_(2, idx_flat.long().unsqueeze(1).expand_as(grad_flat), grad_flat)

    m.furthest_point_sampling_wrapper = lambda B, N, npoint, xyz, temp, output: output.copy_(furthest_point_sample(xyz, npoint))
    m.gather_points_wrapper = lambda B, C, N, npoint, features, idx, out: out.copy_(gather_operation(features, idx))
    m.gather_points_grad_wrapper = lambda B, C, N, npoint, grad_out, idx, grad_features: scatter_add(grad_features, idx, grad_out)
    m.group_points_wrapper = lambda B, C, N, npoint, nsample, features, idx, out: out.copy_(grouping_operation(features, idx))
    m.group_points_grad_wrapper = lambda B, C, N, npoint, nsample, grad_out, idx, grad_features: scatter_add(
        grad_features, idx.reshape(B, npoint * nsample), grad_out.reshape(B, C, npoint * nsample))
    m.ball_query_wrapper = lambda B, N, npoint, radius, nsample, new_xyz, xyz, idx: idx.copy_(ball_query(radius, nsample, xyz, new_xyz))

    def three_nn_wrapper(B, N, m_, unknown, known, dist2_out, idx):
        d, i = three_nn_d2(unknown, known)
        dist2_out.copy_(d)
        idx.copy_(i)

    def three_interpolate_grad_wrapper(B, c, n, m_, grad_out, idx, weight, grad_features):
        g = (grad_out.unsqueeze(-1) * weight.unsqueeze(1)).reshape(B, c, n * 3)
        scatter_add(grad_features, idx.reshape(B, n * 3), g)

    m.three_nn_wrapper = three_nn_wrapper
    m.three_interpolate_wrapper = lambda B, c, m_, n, features, idx, weight, out: out.copy_(three_interpolate(features, idx, weight))
    m.three_interpolate_grad_wrapper = three_interpolate_grad_wrapper
    return m


# ------------------------------------------------------------------------------------------------------------------------ modules
class Trace:
    """What the capture conditions are computed from: the least distances from a ReLU kink, from a pooling tie and from a ball's surface."""

    def __init__(self):
        self.kink = self.pool = self.ball = self.pick = np.inf

    def margins(self):
        return {"kink": self.kink, "pool": self.pool, "ball": self.ball, "pick": self.pick}


def shared_mlp(x, sd, prefix, nlayers, bn, training, buffers, trace):
    """x [B,C,H,W] through layer0 .. of the SharedMLP whose state_dict entries start with `prefix` -> (normalised pre-activation of the
    last layer, its ReLU)."""
    z = None
    for li in range(nlayers):
        key = "%slayer%d." % (prefix, li)
        W = sd[key + "conv.weight"].to(x.dtype)
        y = torch.einsum("oc,bchw->bohw", W.reshape(W.shape[0], W.shape[1]), x)
        if not bn:
            z = y + sd[key + "conv.bias"].to(x.dtype).view(1, -1, 1, 1)
        else:
            gamma, beta = sd[key + "bn.bn.weight"].to(x.dtype), sd[key + "bn.bn.bias"].to(x.dtype)
            if training:
                mean = y.mean(dim=(0, 2, 3))
                var = ((y - mean.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
                n = y.numel() // y.shape[1]
                rm, rv = buffers[key + "bn.bn.running_mean"], buffers[key + "bn.bn.running_var"]
                buffers[key + "bn.bn.running_mean"] = (1 - BN_MOMENTUM) * rm.to(x.dtype) + BN_MOMENTUM * mean.detach()
                buffers[key + "bn.bn.running_var"] = (1 - BN_MOMENTUM) * rv.to(x.dtype) + BN_MOMENTUM * var.detach() * n / max(n - 1, 1)
                buffers[key + "bn.bn.num_batches_tracked"] = buffers[key + "bn.bn.num_batches_tracked"] + 1
            else:
                mean, var = buffers[key + "bn.bn.running_mean"].to(x.dtype), buffers[key + "bn.bn.running_var"].to(x.dtype)
            z = (y - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + BN_EPS) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
        if trace is not None:
            trace.kink = min(trace.kink, float(z.detach().abs().min()))
        x = torch.relu(z)
    return z, x


def _pool_margin(z, idx, trace):
    """z [B,C,m,K] normalised pre-activations of the last layer: where the maximum is positive, its distance from the largest value at a
    slot that holds ANOTHER point (padded duplicates of the winner carry the same value and the same gradient target)."""
    if trace is None or z.shape[3] < 2:
        return
    zd = z.detach()
    top, arg = zd.max(dim=3, keepdim=True)
    if idx is None:
        other = torch.ones_like(zd, dtype=torch.bool).scatter_(3, arg, False)
    else:
        win = torch.gather(idx.long().unsqueeze(1).expand(zd.shape), 3, arg)
        other = idx.long().unsqueeze(1).expand(zd.shape) != win
    rest = torch.where(other, zd, torch.full_like(zd, -np.inf)).max(dim=3, keepdim=True)[0]
    gap = torch.where(top > 0, top - torch.clamp(rest, min=0.0), torch.full_like(top, np.inf))
    trace.pool = min(trace.pool, float(gap.min()))


def sa_module(cfg, sd, buffers, xyz, features, new_xyz=None, training=True, trace=None):
    """PointnetSAModuleMSG.forward.  cfg: npoint, radii, nsamples, mlps (widths AFTER the constructor's + 3), bn, use_xyz, pool_method.
    -> (new_xyz | None, new_features [B, sum mlp[-1], npoint])."""
    if new_xyz is None and cfg["npoint"] is not None:
        fps = furthest_point_sample(xyz.detach().float(), cfg["npoint"])
        if trace is not None:
            trace.pick = min(trace.pick, fps_margin(xyz.detach(), cfg["npoint"]))
        new_xyz = gather_operation(xyz.transpose(1, 2), fps).transpose(1, 2)
    outs = []
    for i, widths in enumerate(cfg["mlps"]):
        idx = None
        if cfg["npoint"] is None:
            x = group_all(cfg["use_xyz"], xyz, features)
        else:
            # the routing is the float32 kernels': identical to the float64 one when no point is within the asserted margin of a surface
            idx = ball_query(cfg["radii"][i], cfg["nsamples"][i], xyz.detach().float(), new_xyz.detach().float())
            if trace is not None:
                d = dist2(new_xyz.detach().double(), xyz.detach().double())
                trace.ball = min(trace.ball, float((d - float(np.float32(cfg["radii"][i])) ** 2).abs().min()))
            grouped_xyz = grouping_operation(xyz.transpose(1, 2), idx) - new_xyz.transpose(1, 2).unsqueeze(-1)
            if features is None:
                x = grouped_xyz
            else:
                grouped = grouping_operation(features, idx)
                x = torch.cat([grouped_xyz, grouped], dim=1) if cfg["use_xyz"] else grouped
        z, a = shared_mlp(x, sd, "mlps.%d." % i, len(widths) - 1, cfg["bn"], training, buffers, trace)
        if cfg["pool_method"] == "max_pool":
            _pool_margin(z, idx, trace)
            outs.append(a.max(dim=3)[0])
        else:
            outs.append(a.mean(dim=3))
    return new_xyz, torch.cat(outs, dim=1)


def fp_module(cfg, sd, buffers, unknown, known, unknow_feats, known_feats, training=True, trace=None):
    """PointnetFPModule.forward.  cfg: mlp (widths), bn."""
    if known is not None:
        _, idx = three_nn(unknown.detach().float(), known.detach().float())
        d = dist2(unknown.detach(), known.detach())
        d2 = torch.gather(d, 2, idx.long()[:, :, :min(3, known.shape[1])])
        if known.shape[1] < 3:
            d2 = torch.cat([d2, torch.full(d2.shape[:2] + (3 - known.shape[1],), float("inf"), dtype=d2.dtype)], dim=2)
        if trace is not None and known.shape[1] > 3:
            s = dist2(unknown.detach().double(), known.detach().double()).sort(dim=2)[0]
            trace.pick = min(trace.pick, float((s[:, :, 1:4] - s[:, :, 0:3]).min()))
        dist_recip = 1.0 / (torch.sqrt(d2) + 1e-8)
        weight = dist_recip / dist_recip.sum(dim=2, keepdim=True)
        interpolated = three_interpolate(known_feats, idx, weight)
    else:
        interpolated = known_feats.expand(known_feats.shape[0], known_feats.shape[1], unknown.shape[1])
    x = interpolated if unknow_feats is None else torch.cat([interpolated, unknow_feats], dim=1)
    _, a = shared_mlp(x.unsqueeze(-1), sd, "mlp.", len(cfg["mlp"]) - 1, cfg["bn"], training, buffers, trace)
    return a.squeeze(-1)


# ------------------------------------------------------------------------------------------------------------------------ cases
def _sa(B, N, C, **kw):
    cfg = dict(kind="sa", B=B, N=N, C=C, bn=True, use_xyz=True, pool_method="max_pool", training=True, given=False)
    cfg.update(kw)
    return cfg


def _fp(m, C1, C2=6, n=65, known=True, **kw):
    cfg = dict(kind="fp", B=2, n=n, m=m, C1=C1, C2=C2, bn=True, training=True, known=known, mlp=[C2 + C1, 8, 7])
    cfg.update(kw)
    return cfg


# mlps: the widths as the CALLER passes them (the constructor adds 3 to the first with use_xyz)
CASES = {
    "msg": _sa(2, 203, 5, npoint=37, radii=[0.2, 0.45], nsamples=[5, 12], mlps=[[5, 7, 9], [5, 6, 11]]),
    "xyz1": _sa(2, 65, 0, npoint=1, radii=[0.3], nsamples=[1], mlps=[[0, 6, 8]], single=True),
    "nobn": _sa(2, 65, 5, npoint=19, radii=[0.35], nsamples=[6], mlps=[[5, 7, 9]], bn=False, single=True),
    "avg": _sa(2, 65, 5, npoint=19, radii=[0.35], nsamples=[6], mlps=[[5, 8, 6]], pool_method="avg_pool", single=True),
    "all": _sa(2, 65, 5, npoint=None, radii=[None], nsamples=[None], mlps=[[5, 8, 10]], single=True),
    "eval": _sa(2, 65, 5, npoint=11, radii=[0.25, 0.5], nsamples=[4, 8], mlps=[[5, 6, 7], [5, 8, 9]], training=False),
    "given": _sa(2, 65, 5, npoint=13, radii=[0.4], nsamples=[7], mlps=[[5, 7, 9]], given=True, single=True),
    "fp1": _fp(1, 4), "fp2": _fp(2, 4), "fp40": _fp(40, 4), "fp40n": _fp(40, 0), "fpx": _fp(1, 4, known=False),
}
# the multi-tile case of the GPU test (against this model only): more than one tile of every new kernel in every tiled dimension, ending
# mid-tile -- 74 centres (tiles of 8), 203 points (steps of 64), 67 first-layer channels on the scalar path (passes of 64) and 8 on the
# vector path, 12 and 70 slots per centre (row slots of 4 and 128).  The grouped tensor the hoisted route avoids has 3 + 29 columns.
MULTI_TILE = _sa(2, 203, 29, npoint=37, radii=[0.3, 0.6], nsamples=[12, 70], mlps=[[29, 67, 6], [29, 8, 12]])
# GroupAll with more rows per group than spgan_group_max walks (128): the pooling hands over to the row-parallel kernel
GROUP_ALL_LONG = _sa(2, 203, 5, npoint=None, radii=[None], nsamples=[None], mlps=[[5, 8, 10]], single=True)
MARGINS = {"kink": 1e-4, "pool": 1e-4, "ball": 1e-6, "pick": 1e-6}
MULTI_TILE_MARGIN = 1e-5


def module_cfg(cfg):
    """The constructor's view: mlps with the + 3."""
    add = 3 if cfg["use_xyz"] else 0
    out = dict(cfg)
    out["mlps"] = [[w[0] + add] + list(w[1:]) for w in cfg["mlps"]]
    return out


def build(mod, cfg):
    """The module of package `mod` (spgan.pointnet2_modules or the reference's) for a case."""
    if cfg["kind"] == "fp":
        return mod.PointnetFPModule(mlp=list(cfg["mlp"]), bn=cfg["bn"])
    if cfg.get("single"):
        return mod.PointnetSAModule(mlp=list(cfg["mlps"][0]), npoint=cfg["npoint"], radius=cfg["radii"][0], nsample=cfg["nsamples"][0], bn=cfg["bn"],
                                    use_xyz=cfg["use_xyz"], pool_method=cfg["pool_method"])
    return mod.PointnetSAModuleMSG(npoint=cfg["npoint"], radii=list(cfg["radii"]), nsamples=list(cfg["nsamples"]),
                                   mlps=[list(w) for w in cfg["mlps"]], bn=cfg["bn"], use_xyz=cfg["use_xyz"], pool_method=cfg["pool_method"])


def state_dict_for(keys_shapes, seed, initial_buffers):
    """Random parameters (and, unless initial_buffers, random running statistics) for the given (key, shape) list."""
    g = torch.Generator().manual_seed(1000 + seed)
    sd = {}
    for k, shape in keys_shapes:
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(0 if initial_buffers else 3, dtype=torch.int64)
        elif k.endswith("running_mean"):
            sd[k] = torch.zeros(shape) if initial_buffers else torch.randn(shape, generator=g) * 0.2
        elif k.endswith("running_var"):
            sd[k] = torch.ones(shape) if initial_buffers else torch.rand(shape, generator=g) + 0.5
        elif k.endswith("bn.weight"):
            sd[k] = torch.rand(shape, generator=g) + 0.5
        elif k.endswith("bias"):
            sd[k] = torch.randn(shape, generator=g) * 0.3
        else:
            fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else 1
            sd[k] = torch.randn(shape, generator=g) / np.sqrt(max(fan_in, 1))
    return sd


def case_inputs(cfg, seed):
    """-> (names, tensors float32, cotangent-free): the forward's positional inputs (None where absent)."""
    g = torch.Generator().manual_seed(seed)
    B = cfg["B"]
    if cfg["kind"] == "fp":
        unknown = torch.rand(B, cfg["n"], 3, generator=g)
        known = torch.rand(B, cfg["m"], 3, generator=g) if cfg["known"] else None
        uf = torch.randn(B, cfg["C1"], cfg["n"], generator=g) if cfg["C1"] else None
        kf = torch.randn(B, cfg["C2"], cfg["m"], generator=g)
        return ["unknown", "known", "unknow_feats", "known_feats"], [unknown, known, uf, kf]
    xyz = torch.rand(B, cfg["N"], 3, generator=g)
    feats = torch.randn(B, cfg["C"], cfg["N"], generator=g) if cfg["C"] else None
    new_xyz = (torch.rand(B, cfg["npoint"], 3, generator=g) * 0.8 + 0.1) if cfg["given"] else None
    return ["xyz", "features", "new_xyz"], [xyz, feats, new_xyz]


GRAD_INPUTS = {"xyz", "features", "new_xyz", "unknow_feats", "known_feats"}


def run_model(cfg, sd, inputs, dtype, gouts=None, trace=None):
    """One forward (+ backward when gouts is given) of the model -> dict: out<i>, gin|<name>, grad|<param>, buf|<buffer>."""
    mc = module_cfg(cfg) if cfg["kind"] == "sa" else cfg
    names, tensors = inputs
    args = [None if t is None else t.to(dtype).clone().requires_grad_(n in GRAD_INPUTS) for n, t in zip(names, tensors)]
    params = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running_" not in k}
    buffers = {k: v.clone() for k, v in sd.items() if k not in params}
    full = dict(params)
    if cfg["kind"] == "fp":
        outs = (fp_module(mc, full, buffers, *args, training=cfg["training"], trace=trace),)
    else:
        outs = sa_module(mc, full, buffers, args[0], args[1], args[2], training=cfg["training"], trace=trace)
    res = {}
    outs = [o for o in outs if o is not None]
    for i, o in enumerate(outs):
        res["out%d" % i] = o.detach()
    if gouts is not None:
        sum((o * g.to(dtype)).sum() for o, g in zip(outs, gouts)).backward()
        for n, a in zip(names, args):
            if a is not None and a.requires_grad:
                res["gin|" + n] = a.grad if a.grad is not None else torch.zeros_like(a)
        for k, p in params.items():
            res["grad|" + k] = p.grad if p.grad is not None else torch.zeros_like(p)
    for k, v in buffers.items():
        res["buf|" + k] = v.detach() if isinstance(v, torch.Tensor) else torch.tensor(v)
    return res


def cotangents(outs, seed):
    g = torch.Generator().manual_seed(77 + seed)
    return [torch.randn(o.shape, generator=g) for o in outs]


def find_seed(cfg, margins, keys_shapes, seeds=400):
    """The first seed whose float64 run keeps every margin; -> (seed, inputs, sd, gouts, margins found)."""
    for seed in range(seeds):
        inputs = case_inputs(cfg, seed)
        sd = state_dict_for(keys_shapes, seed, initial_buffers=cfg["training"])
        tr = Trace()
        r = run_model(cfg, sd, inputs, torch.float64, None, tr)
        got = tr.margins()
        if all(got[k] > margins[k] for k in margins):
            outs = [r[k] for k in sorted(r) if k.startswith("out")]
            return seed, inputs, sd, cotangents(outs, seed), got
    raise SystemExit("no seed meets the conditions for %r" % (cfg,))
