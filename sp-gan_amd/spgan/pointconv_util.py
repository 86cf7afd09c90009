"""Drop-in for the reference's Common/pointconv_util.py: same names, argument order and return shapes / dtypes; HIP kernels underneath
(libspgan_hip.so), GPU float32 tensors only.  The helper half (lines 18-197 there) is spgan.pointnet_util's; this module adds the
density half (lines 120-172 and 199-383):

    farthest_point_sample(xyz, npoint)                                -> int64 [B,npoint]; starts at index 0 for every shape (:74)
    sample_and_group(npoint, nsample, xyz, points, density_scale=None)
        -> (new_xyz [B,S,3], new_points [B,S,K,3+D], grouped_xyz_norm [B,S,K,3], idx int64 [B,S,K]) (+ grouped_density [B,S,K,1])
    sample_and_group_all(xyz, points, density_scale=None)             one group of all N points around the cloud's MEAN
        -> (new_xyz [B,1,3], new_points [B,1,N,3+D], grouped_xyz [B,1,N,3]) (+ grouped_density [B,1,N,1])
    compute_density(xyz [B,N,3], bandwidth)                           -> [B,N] Gaussian kernel density, differentiable in xyz
    DensityNet(hidden_unit=[16, 8]), WeightNet(in_channel, out_channel, hidden_unit=[8, 8])        on [B,C,K,S] inputs
    PointConvSetAbstraction(npoint, nsample, in_channel, mlp, bandwidth=0.0, group_all=False)
    PointConvDensitySetAbstraction(npoint, nsample, in_channel, mlp, bandwidth, group_all)
        forward(xyz [B,3,N], points [B,D,N] | None) -> (new_xyz [B,3,S], new_points [B,mlp[-1],S])

The nn.Conv2d / nn.BatchNorm2d / nn.Linear / nn.BatchNorm1d children are parameter containers created in the reference's order with
the reference's attribute names, so the same seed gives the same initial parameters and a reference state_dict loads with
strict=True; their forward is never called.  The arithmetic: spgan_kde_density -> FPS / kNN / spgan_group_concat -> three per-row
MLPs on the generic GEMM + BatchNorm path (pointnet_util._shared_mlp with K = 1) -> spgan_group_density_scale ->
spgan_pointconv_aggregate -> linear + BatchNorm1d + ReLU on the same generic path.

Reference behaviour that is kept: DensityNet applies BatchNorm + ReLU behind EVERY layer (its sigmoid branch is dead code, :229);
PointConvSetAbstraction ignores `bandwidth`; both modules reshape with `.view(B, self.npoint, -1)`, so group_all=True goes with
npoint=1; knn_point's neighbour order is unspecified in the reference (topk(sorted=False)) and ascending here -- the module output
sums over the neighbours.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._lib import check
from . import ops
from . import pointnet_util as _pu
from .ops import _f32, _p, _s
from .pointnet_util import group, index_points, knn_point, query_ball_point, square_distance  # noqa: F401  (re-exported unchanged)

Tensor = torch.Tensor
WEIGHT_WIDTH = 16          # WeightNet(3, 16): the only width the reference uses (:281, :334)


def farthest_point_sample(xyz: Tensor, npoint: int) -> Tensor:
    """pointconv_util.py:60-83: every shape starts at its point 0."""
    _f32(xyz, "xyz", 3)
    return _pu.farthest_point_sample(xyz, npoint, start=torch.zeros(xyz.shape[0], dtype=torch.long, device=xyz.device))


# ---------------------------------------------------------------------------------------------- kernel density
class _KdeFn(torch.autograd.Function):
    """xyz [B,N,3] -> (density [B,N], 1/density [B,N]); the backward folds both incoming gradients into one N x N pass."""

    @staticmethod
    def forward(ctx, xyz, bandwidth):
        B, N, _ = xyz.shape
        dens = torch.empty((B, N), dtype=torch.float32, device=xyz.device)
        inv = torch.empty((B, N), dtype=torch.float32, device=xyz.device)
        check(_lib.load().spgan_kde_density(_p(xyz), B, N, float(bandwidth), _p(dens), _p(inv), _s()), "kde_density", B=B, N=N, bandwidth=bandwidth)
        ctx.save_for_backward(xyz, inv)
        ctx.set_materialize_grads(False)          # an unused output arrives as None, not as a tensor of zeros
        ctx.bandwidth = float(bandwidth)
        return dens, inv

    @staticmethod
    def backward(ctx, g, ginv):
        xyz, inv = ctx.saved_tensors
        B, N, _ = xyz.shape
        if g is None and ginv is None:
            return None, None
        g = None if g is None else g.contiguous()
        ginv = None if ginv is None else ginv.contiguous()
        dxyz = torch.empty_like(xyz)
        check(_lib.load().spgan_kde_density_bwd(_p(xyz), _p(g), _p(ginv), _p(inv), B, N, ctx.bandwidth, _p(dxyz), _s()), "kde_density_bwd", B=B, N=N)
        return dxyz, None


def _kde(xyz: Tensor, bandwidth: float):
    xyz = _pu._xyz(xyz, "xyz")
    if xyz.shape[2] != 3:
        raise ValueError("compute_density expects xyz [B,N,3]")
    if not bandwidth > 0:
        raise ValueError("compute_density needs a positive bandwidth, got %r" % (bandwidth,))
    return _KdeFn.apply(xyz, bandwidth)


def compute_density(xyz: Tensor, bandwidth: float) -> Tensor:
    """mean_j exp(-d_ij / (2 h^2)) / (2.5 h) over the point's own cloud (pointconv_util.py:199-209), differentiable in xyz."""
    return _kde(xyz, bandwidth)[0]


class _DensityScaleFn(torch.autograd.Function):
    """inv_density [B,N], idx int64 [B,S,K] -> rows [B*S*K, 1]: the gathered inverse density over its group's maximum (:147, :370-371)."""

    @staticmethod
    def forward(ctx, inv, idx):
        B, N = inv.shape
        S, K = idx.shape[1], idx.shape[2]
        out = torch.empty((B * S * K, 1), dtype=torch.float32, device=inv.device)
        bad = ops.index_check_flag(inv.device)
        check(_lib.load().spgan_group_density_scale(_p(inv), _p(idx), B, N, S, K, _p(out), None if bad is None else _p(bad), _s()),
              "group_density_scale", B=B, N=N, S=S, K=K)
        ops.index_check_raise(bad, "group_density_scale: an index lies outside [0, %d)" % N)
        ctx.save_for_backward(inv, idx)
        return out

    @staticmethod
    def backward(ctx, g):
        inv, idx = ctx.saved_tensors
        B, N = inv.shape
        S, K = idx.shape[1], idx.shape[2]
        dslot = torch.empty((B * S * K, 1), dtype=torch.float32, device=inv.device)
        check(_lib.load().spgan_group_density_scale_bwd(_p(g.contiguous()), _p(inv), _p(idx), B, N, S, K, _p(dslot), _s()),
              "group_density_scale_bwd", B=B, N=N, S=S, K=K)
        rowptr, src = _pu.gather_csr(idx.view(B, S * K), N)
        return _pu._scatter_slots(dslot, 0, 1, rowptr, src, (B, N)), None


def _density_scale(inv: Tensor, idx: Tensor) -> Tensor:
    return _DensityScaleFn.apply(inv.contiguous(), idx.contiguous())


# ---------------------------------------------------------------------------------------------- grouping
def _idx_all(B: int, N: int, device) -> Tensor:
    return torch.arange(N, dtype=torch.int64, device=device).view(1, 1, N).expand(B, 1, N).contiguous()


def _density_arg(density_scale: Tensor, B: int, N: int) -> Tensor:
    _f32(density_scale, "density_scale", 3)
    if tuple(density_scale.shape) != (B, N, 1):
        raise ValueError("density_scale must be [B,N,1], got %s" % (tuple(density_scale.shape),))
    return density_scale.contiguous()


def sample_and_group(npoint: int, nsample: int, xyz: Tensor, points: Optional[Tensor], density_scale: Optional[Tensor] = None):
    """FPS from index 0 + kNN + centred grouping (pointconv_util.py:120-148)."""
    xyz = _pu._xyz(xyz, "xyz")
    B, N, C = xyz.shape
    fps_idx = farthest_point_sample(xyz.detach(), npoint)
    new_xyz = index_points(xyz, fps_idx)
    idx = knn_point(nsample, xyz.detach(), new_xyz.detach())
    new_points = _pu._group_concat(xyz, new_xyz, None if points is None else _pu._xyz(points, "points"), idx)
    grouped_xyz_norm = new_points[..., :C].contiguous() if points is not None else new_points
    if density_scale is None:
        return new_xyz, new_points, grouped_xyz_norm, idx
    return new_xyz, new_points, grouped_xyz_norm, idx, index_points(_density_arg(density_scale, B, N), idx)


def sample_and_group_all(xyz: Tensor, points: Optional[Tensor], density_scale: Optional[Tensor] = None):
    """One group of all N points around the mean of the cloud (pointconv_util.py:150-172); the mean carries a gradient to xyz."""
    xyz = _pu._xyz(xyz, "xyz")
    B, N, C = xyz.shape
    new_xyz = xyz.mean(dim=1, keepdim=True)
    new_points = _pu._group_concat(xyz, new_xyz, None if points is None else _pu._xyz(points, "points"), _idx_all(B, N, xyz.device))
    grouped_xyz = new_points[..., :C].contiguous() if points is not None else new_points
    if density_scale is None:
        return new_xyz, new_points, grouped_xyz
    return new_xyz, new_points, grouped_xyz, _density_arg(density_scale, B, N).view(B, 1, N, 1)


# ---------------------------------------------------------------------------------------------- the PointConv product
class _AggregateFn(torch.autograd.Function):
    """E[q, c*16 + w] = sum_k F[q*K+k, c] * dens[q*K+k] * Wt[q*K+k, w]   (the reference's matmul(...).view(B, npoint, -1), :377)."""

    @staticmethod
    def forward(ctx, F, Wt, dens, K):
        M, C = F.shape
        Q = M // K
        E = torch.empty((Q, C * WEIGHT_WIDTH), dtype=torch.float32, device=F.device)
        check(_lib.load().spgan_pointconv_aggregate(_p(F), _p(Wt), _p(dens), Q, K, C, WEIGHT_WIDTH, _p(E), _s()), "pointconv_aggregate", Q=Q, K=K, C=C)
        ctx.save_for_backward(F, Wt, dens)
        ctx.K = K
        return E

    @staticmethod
    def backward(ctx, dE):
        F, Wt, dens = ctx.saved_tensors
        M, C = F.shape
        K = ctx.K
        dF, dWt = torch.empty_like(F), torch.empty_like(Wt)
        ddens = None if dens is None else torch.empty_like(dens)
        check(_lib.load().spgan_pointconv_aggregate_bwd(_p(dE.contiguous()), _p(F), _p(Wt), _p(dens), M // K, K, C, WEIGHT_WIDTH, _p(dF), _p(dWt),
                                                        _p(ddens), _s()), "pointconv_aggregate_bwd", Q=M // K, K=K, C=C)
        return dF, dWt, ddens, None


def pointconv_aggregate(F: Tensor, Wt: Tensor, dens: Optional[Tensor], K: int) -> Tensor:
    """F [Q*K,C] feature rows, Wt [Q*K,16] WeightNet rows, dens [Q*K,1] | None DensityNet rows -> E [Q, 16*C] (c-major, w-minor)."""
    _f32(F, "F", 2); _f32(Wt, "Wt", 2)
    if K <= 0 or F.shape[0] % K or Wt.shape[0] != F.shape[0] or Wt.shape[1] != WEIGHT_WIDTH:
        raise ValueError("pointconv_aggregate expects F [Q*K,C] and Wt [Q*K,%d], got %s and %s with K=%d" % (WEIGHT_WIDTH, tuple(F.shape), tuple(Wt.shape), K))
    if dens is not None:
        _f32(dens, "dens", 2)
        if tuple(dens.shape) != (F.shape[0], 1):
            raise ValueError("dens must be [Q*K,1], got %s" % (tuple(dens.shape),))
        dens = dens.contiguous()
    return _AggregateFn.apply(F.contiguous(), Wt.contiguous(), dens, K)


# ---------------------------------------------------------------------------------------------- modules
def _rows_of(x: Tensor, name: str) -> Tensor:
    """[B,C,K,S] (the reference's conv layout) -> rows [B*S*K, C]."""
    _f32(x, name, 4)
    B, C, K, S = x.shape
    return x.permute(0, 3, 2, 1).contiguous().view(B * S * K, C)


def _rows_back(rows: Tensor, B: int, K: int, S: int) -> Tensor:
    return rows.view(B, S, K, -1).permute(0, 3, 2, 1)


class DensityNet(torch.nn.Module):
    """pointconv_util.py:211-234.  BatchNorm + ReLU behind every layer, the last one included (the reference's sigmoid is dead code)."""

    def __init__(self, hidden_unit=[16, 8]):
        super().__init__()
        self.mlp_convs = torch.nn.ModuleList()
        self.mlp_bns = torch.nn.ModuleList()
        self.mlp_convs.append(torch.nn.Conv2d(1, hidden_unit[0], 1))
        self.mlp_bns.append(torch.nn.BatchNorm2d(hidden_unit[0]))
        for i in range(1, len(hidden_unit)):
            self.mlp_convs.append(torch.nn.Conv2d(hidden_unit[i - 1], hidden_unit[i], 1))
            self.mlp_bns.append(torch.nn.BatchNorm2d(hidden_unit[i]))
        self.mlp_convs.append(torch.nn.Conv2d(hidden_unit[-1], 1, 1))
        self.mlp_bns.append(torch.nn.BatchNorm2d(1))

    def _rows(self, rows: Tensor) -> Tensor:
        return _pu._shared_mlp(rows, 1, self.mlp_convs, self.mlp_bns, self.training)

    def forward(self, density_scale: Tensor) -> Tensor:
        B, _, K, S = density_scale.shape
        return _rows_back(self._rows(_rows_of(density_scale, "density_scale")), B, K, S)


class WeightNet(torch.nn.Module):
    """pointconv_util.py:236-263."""

    def __init__(self, in_channel, out_channel, hidden_unit=[8, 8]):
        super().__init__()
        self.mlp_convs = torch.nn.ModuleList()
        self.mlp_bns = torch.nn.ModuleList()
        if hidden_unit is None or len(hidden_unit) == 0:
            self.mlp_convs.append(torch.nn.Conv2d(in_channel, out_channel, 1))
            self.mlp_bns.append(torch.nn.BatchNorm2d(out_channel))
        else:
            self.mlp_convs.append(torch.nn.Conv2d(in_channel, hidden_unit[0], 1))
            self.mlp_bns.append(torch.nn.BatchNorm2d(hidden_unit[0]))
            for i in range(1, len(hidden_unit)):
                self.mlp_convs.append(torch.nn.Conv2d(hidden_unit[i - 1], hidden_unit[i], 1))
                self.mlp_bns.append(torch.nn.BatchNorm2d(hidden_unit[i]))
            self.mlp_convs.append(torch.nn.Conv2d(hidden_unit[-1], out_channel, 1))
            self.mlp_bns.append(torch.nn.BatchNorm2d(out_channel))

    def _rows(self, rows: Tensor) -> Tensor:
        return _pu._shared_mlp(rows, 1, self.mlp_convs, self.mlp_bns, self.training)

    def forward(self, localized_xyz: Tensor) -> Tensor:
        B, _, K, S = localized_xyz.shape
        return _rows_back(self._rows(_rows_of(localized_xyz, "localized_xyz")), B, K, S)


class _PointConvBase(torch.nn.Module):
    def _build(self, npoint, nsample, in_channel, mlp, group_all):
        self.npoint = npoint
        self.nsample = nsample
        self.mlp_convs = torch.nn.ModuleList()
        self.mlp_bns = torch.nn.ModuleList()
        last_channel = in_channel
        for out_channel in mlp:
            self.mlp_convs.append(torch.nn.Conv2d(last_channel, out_channel, 1))
            self.mlp_bns.append(torch.nn.BatchNorm2d(out_channel))
            last_channel = out_channel
        self.weightnet = WeightNet(3, WEIGHT_WIDTH)
        self.linear = torch.nn.Linear(WEIGHT_WIDTH * mlp[-1], mlp[-1])
        self.bn_linear = torch.nn.BatchNorm1d(mlp[-1])
        self.group_all = group_all

    def _run(self, xyz: Tensor, points: Optional[Tensor], bandwidth: Optional[float]):
        xyz_pm = _pu._CmToRowsFn.apply(_pu._cm(xyz, "xyz"))
        pts_pm = None if points is None else _pu._CmToRowsFn.apply(_pu._cm(points, "points"))
        B, N, _ = xyz_pm.shape
        inv = None if bandwidth is None else _kde(xyz_pm, bandwidth)[1]
        if self.group_all:
            new_xyz, new_points, gxyz = sample_and_group_all(xyz_pm, pts_pm)
            idx = _idx_all(B, N, xyz_pm.device) if inv is not None else None
        else:
            new_xyz, new_points, gxyz, idx = sample_and_group(self.npoint, self.nsample, xyz_pm, pts_pm)
        _, S, K, Cin = new_points.shape
        if S != self.npoint:
            raise ValueError("the module reshapes to [B, npoint, -1] (pointconv_util.py:313, 377): %d groups but npoint=%r"
                             " (group_all=True goes with npoint=1)" % (S, self.npoint))
        M = B * S * K
        feat = _pu._shared_mlp(new_points.view(M, Cin), 1, self.mlp_convs, self.mlp_bns, self.training)
        dens = None if inv is None else self.densitynet._rows(_density_scale(inv, idx))
        wts = self.weightnet._rows(gxyz.view(M, 3))
        E = pointconv_aggregate(feat, wts, dens, K)
        out = _pu._shared_mlp(E, 1, [self.linear], [self.bn_linear], self.training)
        return _pu._RowsToCmFn.apply(new_xyz), _pu._RowsToCmFn.apply(out.view(B, S, -1))


class PointConvSetAbstraction(_PointConvBase):
    """pointconv_util.py:268-319.  `bandwidth` is accepted and ignored, as there."""

    def __init__(self, npoint, nsample, in_channel, mlp, bandwidth=0.0, group_all=False):
        super().__init__()
        self._build(npoint, nsample, in_channel, mlp, group_all)

    def forward(self, xyz: Tensor, points: Optional[Tensor] = None):
        return self._run(xyz, points, None)


class PointConvDensitySetAbstraction(_PointConvBase):
    """pointconv_util.py:321-383: the feature rows are scaled by DensityNet(inverse density / its group maximum) before the product."""

    def __init__(self, npoint, nsample, in_channel, mlp, bandwidth, group_all):
        super().__init__()
        self._build(npoint, nsample, in_channel, mlp, group_all)
        self.densitynet = DensityNet()
        self.bandwidth = bandwidth

    def forward(self, xyz: Tensor, points: Optional[Tensor] = None):
        return self._run(xyz, points, self.bandwidth)
