"""Plain-PyTorch model of spgan.pointconv_util (kernel density, density-aware grouping, DensityNet / WeightNet, the two PointConv set
abstraction modules) and of the kernels of csrc/pointconv.hip, written for the tests: functional (parameters and BatchNorm buffers
come in as a state_dict, the updated buffers go out), any float dtype, CPU.  It is the checker behind tests/test_pointconv_cpu.py
(against the vectors captured from the reference, golden G24) and the oracle of the kernel tests in tests/test_pointconv_gpu.py.
TEST INFRASTRUCTURE: the product never imports this."""
import torch

from pointnet2_model import _names, fps, gather, shared_mlp, sqdist

WIDTH = 16


def compute_density(xyz, bandwidth):
    """[B,N,3] -> [B,N]: mean_j exp(-d_ij / (2 h^2)) / (2.5 h), d in the expanded form."""
    return (torch.exp(-sqdist(xyz, xyz) / (2.0 * bandwidth * bandwidth)) / (2.5 * bandwidth)).mean(-1)


def knn(nsample, xyz, new_xyz):
    """Ascending (distance, index): the product's order; the reference's is unspecified."""
    return sqdist(new_xyz, xyz).sort(dim=-1, stable=True)[1][..., :nsample]


def density_scale(inv, idx):
    """inv [B,N], idx [B,S,K] -> [B,S,K]: the gathered inverse density over its group's maximum."""
    v = gather(inv.unsqueeze(-1), idx).squeeze(-1)
    return v / v.max(dim=2, keepdim=True)[0]


def aggregate(F, Wt, dens, K):
    """F [Q*K,C], Wt [Q*K,16], dens [Q*K,1] | None -> E [Q, 16*C], column c*16 + w."""
    Q = F.shape[0] // K
    f = F if dens is None else F * dens
    return torch.einsum("qkc,qkw->qcw", f.reshape(Q, K, -1), Wt.reshape(Q, K, -1)).reshape(Q, -1)


def pointconv(sd, xyz_cm, points_cm, npoint, nsample, group_all, bandwidth=None, training=True, idx=None):
    """bandwidth None: PointConvSetAbstraction, else PointConvDensitySetAbstraction.
    -> (new_xyz [B,3,S], new_points [B,C,S], new buffers, (fps idx, knn idx))."""
    xyz = xyz_cm.transpose(1, 2)
    pts = None if points_cm is None else points_cm.transpose(1, 2)
    B, N, _ = xyz.shape
    bufs = {}
    inv = None if bandwidth is None else 1.0 / compute_density(xyz, bandwidth)
    if group_all:
        new_xyz = xyz.mean(dim=1, keepdim=True)
        gi = torch.arange(N).view(1, 1, N).expand(B, 1, N)
        grouped = xyz.unsqueeze(1) - new_xyz.unsqueeze(2)
        feats = None if pts is None else pts.unsqueeze(1)
        used = (None, None)
    else:
        fi = fps(xyz.detach(), npoint, torch.zeros(B, dtype=torch.long)) if idx is None else idx[0]
        new_xyz = gather(xyz, fi)
        gi = knn(nsample, xyz.detach(), new_xyz.detach()) if idx is None else idx[1]
        grouped = gather(xyz, gi) - new_xyz.unsqueeze(2)
        feats = None if pts is None else gather(pts, gi)
        used = (fi, gi)
    rows = grouped if feats is None else torch.cat([grouped, feats], -1)
    S, K = rows.shape[1], rows.shape[2]
    M = B * S * K
    F = shared_mlp(rows.reshape(M, -1), 1, sd, _names(sd, "mlp_convs", "mlp_bns"), training, bufs)
    dens = None
    if inv is not None:
        dens = shared_mlp(density_scale(inv, gi).reshape(M, 1), 1, sd, _names(sd, "densitynet.mlp_convs", "densitynet.mlp_bns"), training, bufs)
    Wt = shared_mlp(grouped.reshape(M, 3), 1, sd, _names(sd, "weightnet.mlp_convs", "weightnet.mlp_bns"), training, bufs)
    E = aggregate(F, Wt, dens, K)
    out = shared_mlp(E, 1, sd, [("linear", "bn_linear")], training, bufs)
    return new_xyz.transpose(1, 2), out.reshape(B, S, -1).transpose(1, 2), bufs, used


# ---------------------------------------------------------------- the cases of golden G24 (tests/golden/make_golden_pointconv.py)
# tag -> (module class name, constructor arguments, forward argument names in order (None: that argument is None))
CASES = {
    "dsa": ("PointConvDensitySetAbstraction", (64, 16, 9, [32, 24], 0.1, False), ("xyz", "points")),
    "dsa_nopts": ("PointConvDensitySetAbstraction", (64, 16, 3, [16, 16], 0.1, False), ("xyz", None)),
    "sa": ("PointConvSetAbstraction", (64, 16, 9, [32, 16], 0.1, False), ("xyz", "points")),
    "dsa_all": ("PointConvDensitySetAbstraction", (1, None, 6, [16, 16], 0.1, True), ("xyz", "points")),
}
INPUTS_OF = {"dsa_nopts": "dsa", "sa": "dsa"}          # cases that share another case's stored inputs
BANDWIDTH = 0.1


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
    return [None if n is None else torch.from_numpy(d["%s|in|%s" % (src, n)]) for n in CASES[tag][2]]


def case_indices(d, tag):
    if tag + "|fps0" not in d.files:
        return None
    return torch.from_numpy(d[tag + "|fps0"].astype("int64")), torch.from_numpy(d[tag + "|knn0"].astype("int64"))


def run_model(d, tag, sd, args, training=True, idx=None):
    kind, cargs, _ = CASES[tag]
    bw = cargs[4] if kind == "PointConvDensitySetAbstraction" else None
    nx, npts, bufs, used = pointconv(sd, args[0], args[1], cargs[0], cargs[1], cargs[5], bw, training, idx)
    return (nx, npts), bufs, used
