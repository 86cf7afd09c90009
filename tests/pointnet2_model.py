"""Plain-PyTorch model of the PointNet++ surface of spgan.pointnet_util (set abstraction, multi-scale set abstraction, feature
propagation, three_nn / three_interpolate), written for the tests: functional (parameters and BatchNorm buffers come in as a
state_dict, the updated buffers go out), any float dtype, CPU.  It is the checker behind tests/test_pointnet2_cpu.py (against the
vectors captured from the reference, golden G22) and the oracle of the odd-shape kernel tests in tests/test_pointnet2_gpu.py.
TEST INFRASTRUCTURE: the product never imports this."""
import torch

EPS, MOMENTUM = 1e-5, 0.1


def sqdist(a, b):
    """[B,N,3], [B,M,3] -> [B,N,M] in the expanded form (-2ab + |a|^2) + |b|^2."""
    return (-2.0 * (a @ b.transpose(1, 2)) + (a * a).sum(-1, keepdim=True)) + (b * b).sum(-1).unsqueeze(1)


def gather(points, idx):
    """points [B,N,C], idx [B,...] -> [B,...,C]."""
    B = points.shape[0]
    flat = idx.reshape(B, -1)
    out = torch.gather(points, 1, flat.unsqueeze(-1).expand(-1, -1, points.shape[2]))
    return out.reshape(tuple(idx.shape) + (points.shape[2],))


def fps(xyz, npoint, start):
    B, N, _ = xyz.shape
    out = torch.zeros(B, npoint, dtype=torch.long)
    dist = torch.full((B, N), 1e10, dtype=xyz.dtype)
    far = start.clone()
    ar = torch.arange(B)
    for i in range(npoint):
        out[:, i] = far
        d = ((xyz - xyz[ar, far].unsqueeze(1)) ** 2).sum(-1)
        dist = torch.minimum(dist, d)
        far = dist.argmax(-1)
    return out


def ball_query(radius, nsample, xyz, new_xyz):
    """First nsample indices (ascending) within the radius, padded with the first one."""
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    idx = torch.arange(N).view(1, 1, N).repeat(B, S, 1)
    idx[sqdist(new_xyz, xyz) > radius ** 2] = N
    idx = idx.sort(dim=-1)[0][:, :, :nsample]
    first = idx[:, :, :1].expand(-1, -1, nsample)
    return torch.where(idx == N, first, idx)


def three_nn(xyz1, xyz2):
    """-> (idx [B,N,k], weight [B,N,k], sorted distances [B,N,min(S,4)]), k = min(3,S); ascending (distance, index)."""
    d = sqdist(xyz1, xyz2)
    ds, order = d.sort(dim=-1, stable=True)
    k = min(3, xyz2.shape[1])
    r = 1.0 / (ds[..., :k] + 1e-8)
    return order[..., :k], r / r.sum(-1, keepdim=True), ds[..., :4]


def three_interpolate(points2, idx, weight):
    """points2 [B,S,D] -> [B,N,D]."""
    return (gather(points2, idx) * weight.unsqueeze(-1)).sum(2)


def shared_mlp(rows, K, sd, names, training, new_bufs):
    """rows [Q*K, Cin] -> [Q, Cout]: (linear -> BatchNorm -> ReLU) per (conv, bn) name pair, max over each K consecutive rows."""
    M = rows.shape[0]
    a = rows
    for conv, bn in names:
        W = sd[conv + ".weight"]
        y = a @ W.reshape(W.shape[0], W.shape[1]).t() + sd[conv + ".bias"]
        rm, rv = sd[bn + ".running_mean"], sd[bn + ".running_var"]
        if training:
            mean, var = y.mean(0), y.var(0, unbiased=False)
            new_bufs[bn + ".running_mean"] = ((1 - MOMENTUM) * rm + MOMENTUM * mean).detach()
            new_bufs[bn + ".running_var"] = ((1 - MOMENTUM) * rv + MOMENTUM * var * M / max(M - 1, 1)).detach()
            new_bufs[bn + ".num_batches_tracked"] = sd[bn + ".num_batches_tracked"] + 1
        else:
            mean, var = rm, rv
        a = torch.relu((y - mean) / torch.sqrt(var + EPS) * sd[bn + ".weight"] + sd[bn + ".bias"])
    return a.reshape(M // K, K, -1).max(1)[0]


def _names(sd, convs, bns):
    n = len([k for k in sd if k.startswith(convs + ".") and k.endswith(".weight")])
    return [("%s.%d" % (convs, i), "%s.%d" % (bns, i)) for i in range(n)]


def set_abstraction(sd, xyz_cm, points_cm, npoint, radius, nsample, group_all, start=None, training=True, idx=None):
    """-> (new_xyz [B,3,S], new_points [B,C,S], new buffers, (fps_idx, ball idx))."""
    xyz = xyz_cm.transpose(1, 2)
    pts = None if points_cm is None else points_cm.transpose(1, 2)
    B, N, _ = xyz.shape
    bufs = {}
    if group_all:
        new_xyz = torch.zeros(B, 1, 3, dtype=xyz.dtype)
        grouped = xyz.unsqueeze(1)
        feats = None if pts is None else pts.unsqueeze(1)
        used = (None, None)
    else:
        fi = fps(xyz.detach(), npoint, start) if idx is None else idx[0]
        new_xyz = gather(xyz, fi)
        gi = ball_query(radius, nsample, xyz.detach(), new_xyz.detach()) if idx is None else idx[1]
        grouped = gather(xyz, gi) - new_xyz.unsqueeze(2)
        feats = None if pts is None else gather(pts, gi)
        used = (fi, gi)
    rows = grouped if feats is None else torch.cat([grouped, feats], -1)
    S, K = rows.shape[1], rows.shape[2]
    out = shared_mlp(rows.reshape(B * S * K, -1), K, sd, _names(sd, "mlp_convs", "mlp_bns"), training, bufs)
    return new_xyz.transpose(1, 2), out.reshape(B, S, -1).transpose(1, 2), bufs, used


def set_abstraction_msg(sd, xyz_cm, points_cm, npoint, radius_list, nsample_list, start=None, training=True, idx=None):
    xyz = xyz_cm.transpose(1, 2)
    pts = None if points_cm is None else points_cm.transpose(1, 2)
    B = xyz.shape[0]
    bufs = {}
    fi = fps(xyz.detach(), npoint, start) if idx is None else idx[0]
    new_xyz = gather(xyz, fi)
    outs, balls = [], []
    for i, (radius, K) in enumerate(zip(radius_list, nsample_list)):
        gi = ball_query(radius, K, xyz.detach(), new_xyz.detach()) if idx is None else idx[1][i]
        balls.append(gi)
        grouped = gather(xyz, gi) - new_xyz.unsqueeze(2)
        rows = grouped if pts is None else torch.cat([gather(pts, gi), grouped], -1)          # features first in the multi-scale module
        out = shared_mlp(rows.reshape(B * npoint * K, -1), K, sd, _names(sd, "conv_blocks.%d" % i, "bn_blocks.%d" % i), training, bufs)
        outs.append(out.reshape(B, npoint, -1).transpose(1, 2))
    return new_xyz.transpose(1, 2), torch.cat(outs, 1), bufs, (fi, balls)


def feature_propagation(sd, xyz1_cm, xyz2_cm, points1_cm, points2_cm, training=True):
    """-> ([B,C,N], new buffers).  The weights are constants (no gradient to the coordinates)."""
    xyz1, xyz2 = xyz1_cm.transpose(1, 2).detach(), xyz2_cm.transpose(1, 2).detach()
    p2 = points2_cm.transpose(1, 2)
    B, N, _ = xyz1.shape
    if xyz2.shape[1] == 1:
        interp = p2.expand(B, N, p2.shape[2])
    else:
        idx, w, _ = three_nn(xyz1, xyz2)
        interp = three_interpolate(p2, idx, w)
    rows = interp if points1_cm is None else torch.cat([points1_cm.transpose(1, 2), interp], -1)
    bufs = {}
    out = shared_mlp(rows.reshape(B * N, -1), 1, sd, _names(sd, "mlp_convs", "mlp_bns"), training, bufs)
    return out.reshape(B, N, -1).transpose(1, 2), bufs


# ---------------------------------------------------------------- the cases of golden G22 (tests/golden/make_golden_pointnet2.py)
# tag -> (module class name, constructor arguments, forward argument names in order)
CASES = {
    "sa": ("PointNetSetAbstraction", (64, 0.2, 16, 9, [32, 32, 64], False), ("xyz", "points")),
    "sa_all": ("PointNetSetAbstraction", (None, None, None, 9, [32, 64], True), ("xyz", "points")),
    "msg": ("PointNetSetAbstractionMsg", (64, [0.12, 0.2], [8, 16], 6, [[16, 32], [32, 64]]), ("xyz", "points")),
    "fp": ("PointNetFeaturePropagation", (22, [32, 16]), ("xyz_nograd1", "xyz_nograd2", "points1", "points2")),
    "fp1": ("PointNetFeaturePropagation", (22, [16]), ("xyz_nograd1", "xyz_nograd2", "points1", "points2")),
}
INPUTS_OF = {"msg": "sa"}          # cases that share another case's stored inputs


def case_state_dict(d, tag, dtype=torch.float32):
    pre = tag + "|sd|"
    out = {}
    for k in d.files:
        if k.startswith(pre):
            t = torch.from_numpy(d[k])
            out[k[len(pre):]] = t.to(dtype) if t.is_floating_point() else t
    return out


def case_inputs(d, tag):
    src = INPUTS_OF.get(tag, tag)
    return [torch.from_numpy(d["%s|in|%s" % (src, n)]) for n in CASES[tag][2]]


def run_model(d, tag, sd, args, training=True):
    """The model on case `tag` -> (outputs tuple, new buffers, used indices | None)."""
    kind, cargs, _ = CASES[tag]
    start = torch.from_numpy(d[tag + "|start"])
    if kind == "PointNetSetAbstraction":
        nx, npts, bufs, used = set_abstraction(sd, args[0], args[1], cargs[0], cargs[1], cargs[2], cargs[5], start, training)
        return (nx, npts), bufs, used
    if kind == "PointNetSetAbstractionMsg":
        nx, npts, bufs, used = set_abstraction_msg(sd, args[0], args[1], cargs[0], cargs[1], cargs[2], start, training)
        return (nx, npts), bufs, used
    out, bufs = feature_propagation(sd, args[0], args[1], args[2], args[3], training)
    return (out,), bufs, None
