"""The pointops extension: metrics/pointops/pointops_util.py (= functions/pointops.py) over the HIP kernels of csrc/pointops.hip.

Names, argument order, shapes and dtypes are the reference's; every index tensor is int32 (`torch.cuda.IntTensor` there).

    from spgan import pointops                      # or, with the reference's own import lines: spgan.compat.install()
    idx = pointops.knnquery(nsample, xyz, new_xyz)                 # int32 [B,m,nsample], ascending (d2, index), nsample <= 200
    idx = pointops.ballquery(radius, nsample, xyz, new_xyz)        # first nsample with d2 < r*r, padded with the first hit
    new_features = pointops.QueryAndGroup(radius, nsample)(xyz, new_xyz, features)        # [B, 3+C, m, nsample]

Every squared distance is d2 = (dx*dx + dy*dy) + dz*dz in float32 with dx = query - candidate, each operation rounded on its own.
Gradients reach `features`, `xyz` and `new_xyz` through the grouping ops and modules; the index ops carry none.  Backward sums run
over per-point slot lists in ascending slot order: no float atomics, results repeat bit for bit.  There is no CPU path.
Differences from the reference: INTEGRATION 22.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib, ops
from .ops import _f32, _p, _s, check
from .pointnet_util import farthest_point_sample, gather_csr, square_distance

Tensor = torch.Tensor

MAX_NSAMPLE = 200            # the reference's array size (knnquery_cuda_kernel.cu)

# The modules group through spgan_pointops_group_cm ("fused": one launch per slice into one buffer) or through the launchers that existed
# before it ("composed": spgan_gather_points_cm per slice, the subtraction, torch.cat).  Both give the same bits; profiles/pointops_bench.json
# holds the measurement behind the default.
GROUP_ROUTE = "fused"


def _cloud(t: Tensor, name: str) -> Tensor:
    _f32(t, name, 3)
    if t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("%s must be [B, n, 3] with B, n >= 1, got %s" % (name, tuple(t.shape)))
    return t.contiguous()


def _feat(t: Tensor, name: str) -> Tensor:
    _f32(t, name, 3)
    if min(t.shape) < 1:
        raise ValueError("%s must be a non-empty [B, C, n], got %s" % (name, tuple(t.shape)))
    return t.contiguous()


def _index(t: Tensor, name: str, dims: int, B: int) -> Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU (spgan has no CPU path); got device %s" % (name, t.device))
    if t.dtype != torch.int32:
        raise TypeError("%s must be int32, got %s" % (name, t.dtype))
    if t.dim() != dims or t.shape[0] != B or min(t.shape) < 1:
        raise ValueError("%s must be a non-empty %d-D tensor with B = %d, got %s" % (name, dims, B, tuple(t.shape)))
    return t.contiguous()


def _pair(xyz: Tensor, new_xyz: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    xyz = _cloud(xyz, "xyz")
    new_xyz = xyz if new_xyz is None else _cloud(new_xyz, "new_xyz")
    if new_xyz.shape[0] != xyz.shape[0]:
        raise ValueError("xyz and new_xyz differ in B: %s, %s" % (tuple(xyz.shape), tuple(new_xyz.shape)))
    return xyz, new_xyz


def _nsample(nsample: int) -> int:
    nsample = int(nsample)
    if not 1 <= nsample <= MAX_NSAMPLE:
        raise ValueError("nsample must lie in [1, %d], got %d" % (MAX_NSAMPLE, nsample))
    return nsample


def _label(label_stat: Tensor, B: int, n: int) -> Tensor:
    label_stat = _index(label_stat, "label_stat", 3, B)
    if label_stat.shape[1] != n:
        raise ValueError("label_stat must be [B, n = %d, nclass], got %s" % (n, tuple(label_stat.shape)))
    return label_stat


# ----------------------------------------------------------------------------------------------------------------------------------
# index ops (no gradient)
# ----------------------------------------------------------------------------------------------------------------------------------
class FurthestSampling(Function):
    @staticmethod
    def forward(ctx, xyz, m):
        """xyz [B,n,3], m -> idx int32 [B,m]; the first pick is point 0 (sampling_cuda_kernel.cu:72-74)."""
        xyz = _cloud(xyz, "xyz")
        start = torch.zeros((xyz.shape[0],), dtype=torch.long, device=xyz.device)
        idx = farthest_point_sample(xyz.detach(), int(m), start).to(torch.int32)
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, a=None):
        return None, None


furthestsampling = FurthestSampling.apply


def knn_with_dist2(nsample: int, xyz: Tensor, new_xyz: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """-> (idx int32 [B,m,nsample], dist2 float32 [B,m,nsample]): what knnquery_cuda computes; `knnquery` returns idx alone."""
    nsample = _nsample(nsample)
    xyz, new_xyz = _pair(xyz.detach(), None if new_xyz is None else new_xyz.detach())
    B, n, _ = xyz.shape
    m = new_xyz.shape[1]
    idx = torch.empty((B, m, nsample), dtype=torch.int32, device=xyz.device)
    dist2 = torch.empty((B, m, nsample), dtype=torch.float32, device=xyz.device)
    check(_lib.load().spgan_pointops_knnquery(_p(xyz), _p(new_xyz), B, n, m, nsample, _p(idx), _p(dist2), _s()), "pointops_knnquery",
          B=B, n=n, m=m, nsample=nsample)
    return idx, dist2


class KNNQuery(Function):
    @staticmethod
    def forward(ctx, nsample, xyz, new_xyz=None):
        """nsample <= 200, xyz [B,n,3], new_xyz [B,m,3] (None: xyz) -> idx int32 [B,m,nsample], ascending (d2, index)."""
        idx, _ = knn_with_dist2(nsample, xyz, new_xyz)
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, a=None):
        return None, None, None


knnquery = KNNQuery.apply


class KNNQueryNaive(Function):
    """The reference sorts a [B,m,n] distance matrix; here it is the kNN kernel, whose tie order (lower index first) is one of the orders
    torch.sort may give."""

    @staticmethod
    def forward(ctx, nsample, xyz, new_xyz=None):
        idx, _ = knn_with_dist2(nsample, xyz, new_xyz)
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, a=None):
        return None, None, None


knnquery_naive = KNNQueryNaive.apply


class KNNQueryExclude(Function):
    """Ranks 1 .. nsample of the kNN order (rank 0 is the query itself when it is a cloud point); nsample <= 199."""

    @staticmethod
    def forward(ctx, nsample, xyz, new_xyz=None):
        idx, _ = knn_with_dist2(int(nsample) + 1, xyz, new_xyz)
        idx = idx[:, :, 1:].contiguous()
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, a=None):
        return None, None, None


knnquery_exclude = KNNQueryExclude.apply


class NearestNeighbor(Function):
    @staticmethod
    def forward(ctx, unknown, known):
        """unknown [B,n,3], known [B,m,3] -> (dist [B,n,3] = sqrt(d2), idx int32 [B,n,3]) of the three nearest known, ascending (d2, index);
        with m < 3 the missing slots hold index 0 and +inf."""
        unknown, known = _cloud(unknown.detach(), "unknown"), _cloud(known.detach(), "known")
        if known.shape[0] != unknown.shape[0]:
            raise ValueError("unknown and known differ in B")
        B, n, _ = unknown.shape
        m = known.shape[1]
        dist2 = torch.empty((B, n, 3), dtype=torch.float32, device=unknown.device)
        idx = torch.empty((B, n, 3), dtype=torch.int32, device=unknown.device)
        check(_lib.load().spgan_pointops_nearestneighbor(_p(unknown), _p(known), B, n, m, _p(dist2), _p(idx), _s()), "pointops_nearestneighbor",
              B=B, n=n, m=m)
        dist = torch.sqrt(dist2)
        ctx.mark_non_differentiable(dist, idx)
        return dist, idx

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None


nearestneighbor = NearestNeighbor.apply


class BallQuery(Function):
    @staticmethod
    def forward(ctx, radius, nsample, xyz, new_xyz):
        """-> idx int32 [B,m,nsample]: the first nsample indices with d2 < radius*radius (strict), padded with the first hit; zeros for an
        empty ball."""
        xyz, new_xyz = _pair(xyz.detach(), new_xyz.detach())
        nsample = int(nsample)
        if nsample < 1:
            raise ValueError("nsample must be >= 1, got %d" % nsample)
        B, n, _ = xyz.shape
        m = new_xyz.shape[1]
        idx = torch.empty((B, m, nsample), dtype=torch.int32, device=xyz.device)
        check(_lib.load().spgan_pointops_ballquery(float(radius), nsample, _p(xyz), _p(new_xyz), B, n, m, _p(idx), _s()), "pointops_ballquery",
              B=B, n=n, m=m, nsample=nsample)
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, a=None):
        return None, None, None, None


ballquery = BallQuery.apply


class FeatureDistribute(Function):
    @staticmethod
    def forward(ctx, max_xyz, xyz):
        """max_xyz [B,n,3], xyz [B,m,3] -> distribute_idx int32 [B,m]: the nearest max_xyz (lowest index among equals), -1 when no squared
        distance is below 100000."""
        max_xyz, xyz = _cloud(max_xyz.detach(), "max_xyz"), _cloud(xyz.detach(), "xyz")
        if max_xyz.shape[0] != xyz.shape[0]:
            raise ValueError("max_xyz and xyz differ in B")
        B, n, _ = max_xyz.shape
        m = xyz.shape[1]
        out = torch.empty((B, m), dtype=torch.int32, device=xyz.device)
        check(_lib.load().spgan_pointops_featuredistribute(_p(max_xyz), _p(xyz), B, n, m, _p(out), _s()), "pointops_featuredistribute",
              B=B, n=n, m=m)
        ctx.mark_non_differentiable(out)
        return out

    @staticmethod
    def backward(ctx, a=None):
        return None, None


featuredistribute = FeatureDistribute.apply


class LabelStatBallRange(Function):
    @staticmethod
    def forward(ctx, radius, xyz, new_xyz, label_stat):
        """label_stat int32 [B,n,nclass] -> int32 [B,m,nclass]: summed over ALL points with d2 < radius*radius."""
        xyz, new_xyz = _pair(xyz.detach(), new_xyz.detach())
        B, n, _ = xyz.shape
        m = new_xyz.shape[1]
        label_stat = _label(label_stat, B, n)
        nclass = label_stat.shape[2]
        out = torch.empty((B, m, nclass), dtype=torch.int32, device=xyz.device)
        check(_lib.load().spgan_pointops_labelstat_ballrange(float(radius), _p(xyz), _p(new_xyz), _p(label_stat), B, n, m, nclass, _p(out), _s()),
              "pointops_labelstat_ballrange", B=B, n=n, m=m, nclass=nclass)
        ctx.mark_non_differentiable(out)
        return out

    @staticmethod
    def backward(ctx, a=None):
        return None, None, None, None


labelstat_ballrange = LabelStatBallRange.apply


class LabelStatIdx(Function):
    @staticmethod
    def forward(ctx, nsample, label_stat, idx):
        """label_stat int32 [B,n,nclass], idx int32 [B,m,nsample] -> int32 [B,m,nclass]: the sum of the rows idx names."""
        if not isinstance(label_stat, torch.Tensor) or label_stat.dim() != 3:
            raise ValueError("label_stat must be int32 [B, n, nclass]")
        B, n, nclass = label_stat.shape
        label_stat = _label(label_stat, B, n)
        idx = _index(idx, "idx", 3, B)
        if idx.shape[2] != int(nsample):
            raise ValueError("idx must be [B, m, nsample = %d], got %s" % (int(nsample), tuple(idx.shape)))
        m = idx.shape[1]
        out = torch.empty((B, m, nclass), dtype=torch.int32, device=idx.device)
        bad = ops.index_check_flag(idx.device)
        check(_lib.load().spgan_pointops_labelstat_idx(_p(label_stat), _p(idx), B, n, m, int(nsample), nclass, _p(out), _p(bad), _s()),
              "pointops_labelstat_idx", B=B, n=n, m=m, nsample=int(nsample), nclass=nclass)
        ops.index_check_raise(bad, "labelstat_idx: an index lies outside [0, %d)" % n)
        ctx.mark_non_differentiable(out)
        return out

    @staticmethod
    def backward(ctx, a=None):
        return None, None, None


labelstat_idx = LabelStatIdx.apply


class LabelStatAndBallQuery(Function):
    @staticmethod
    def forward(ctx, radius, nsample, xyz, new_xyz, label_stat):
        """-> (new_label_stat int32 [B,m,nclass], idx int32 [B,m,nsample]): the ball query, and the label sums over the hits it returns
        only -- the scan ends at nsample hits (labelstat_ballrange sums the whole ball)."""
        xyz, new_xyz = _pair(xyz.detach(), new_xyz.detach())
        nsample = int(nsample)
        if nsample < 1:
            raise ValueError("nsample must be >= 1, got %d" % nsample)
        B, n, _ = xyz.shape
        m = new_xyz.shape[1]
        label_stat = _label(label_stat, B, n)
        nclass = label_stat.shape[2]
        out = torch.empty((B, m, nclass), dtype=torch.int32, device=xyz.device)
        idx = torch.empty((B, m, nsample), dtype=torch.int32, device=xyz.device)
        check(_lib.load().spgan_pointops_labelstat_and_ballquery(float(radius), nsample, _p(xyz), _p(new_xyz), _p(label_stat), B, n, m, nclass,
                                                                 _p(idx), _p(out), _s()),
              "pointops_labelstat_and_ballquery", B=B, n=n, m=m, nsample=nsample, nclass=nclass)
        ctx.mark_non_differentiable(out, idx)
        return out, idx

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None, None, None, None


labelstat_and_ballquery = LabelStatAndBallQuery.apply


def pairwise_distances(x: Tensor, y: Optional[Tensor] = None) -> Tensor:
    """x [N,d], y [M,d] (None: x) -> [N,M] squared distances |x|^2 + |y|^2 - 2<x,y>, clamped at 0 (spgan_square_distance)."""
    _f32(x, "x", 2)
    y = x if y is None else _f32(y, "y", 2)
    return torch.clamp(square_distance(x.unsqueeze(0), y.unsqueeze(0))[0], 0.0, np.inf)


# ----------------------------------------------------------------------------------------------------------------------------------
# gathers with a gradient
# ----------------------------------------------------------------------------------------------------------------------------------
def _gather_cm(features: Tensor, idx: Tensor, what: str, always_check: bool) -> Tensor:
    B, C, n = features.shape
    m = idx.shape[1]
    out = torch.empty((B, C, m), dtype=torch.float32, device=features.device)
    if always_check and not ops.capturing():
        bad = torch.zeros(1, dtype=torch.int32, device=features.device)
    else:
        bad = ops.index_check_flag(features.device)
    check(_lib.load().spgan_gather_points_cm(_p(features), _p(idx), B, C, n, m, _p(out), _p(bad), _s()), "gather_points_cm", B=B, C=C, N=n, m=m)
    ops.index_check_raise(bad, "%s: an index lies outside [0, %d)" % (what, n))
    return out


def _gather_cm_bwd(dout: Tensor, idx: Tensor, C: int, n: int) -> Tensor:
    B, m = idx.shape
    dout = dout.contiguous()
    rowptr, src = gather_csr(idx.to(torch.int64), n)
    dfeat = torch.empty((B, C, n), dtype=torch.float32, device=dout.device)
    check(_lib.load().spgan_gather_points_cm_bwd(_p(dout), _p(rowptr), _p(src), B, C, n, m, _p(dfeat), _s()), "gather_points_cm_bwd",
          B=B, C=C, N=n, m=m)
    return dfeat


class Gathering(Function):
    @staticmethod
    def forward(ctx, features, idx):
        """features [B,C,n], idx int32 [B,m] -> [B,C,m]."""
        features = _feat(features, "features")
        idx = _index(idx, "idx", 2, features.shape[0])
        ctx.save_for_backward(idx)
        ctx.cn = (features.shape[1], features.shape[2])
        return _gather_cm(features, idx, "gathering", False)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        return _gather_cm_bwd(grad_out, idx, *ctx.cn), None


gathering = Gathering.apply


class FeatureGather(Function):
    @staticmethod
    def forward(ctx, max_feature, distribute_idx):
        """max_feature [B,C,n], distribute_idx int32 [B,m] -> [B,C,m].  The index is always checked (one host synchronisation):
        featuredistribute's -1 raises IndexError here."""
        max_feature = _feat(max_feature, "max_feature")
        distribute_idx = _index(distribute_idx, "distribute_idx", 2, max_feature.shape[0])
        ctx.save_for_backward(distribute_idx)
        ctx.cn = (max_feature.shape[1], max_feature.shape[2])
        return _gather_cm(max_feature, distribute_idx, "featuregather", True)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_distribute_feature):
        (idx,) = ctx.saved_tensors
        return _gather_cm_bwd(grad_distribute_feature, idx, *ctx.cn), None


featuregather = FeatureGather.apply


class Interpolation(Function):
    @staticmethod
    def forward(ctx, features, idx, weight):
        """features [B,C,m], idx int32 [B,n,3], weight [B,n,3] -> [B,C,n] = (w0*f0 + w1*f1) + w2*f2; differentiable in features only."""
        features = _feat(features, "features")
        B, C, m = features.shape
        idx = _index(idx, "idx", 3, B)
        weight = _f32(weight, "weight", 3).detach().contiguous()
        if idx.shape[2] != 3 or weight.shape != idx.shape:
            raise ValueError("idx and weight must be [B, n, 3], got %s and %s" % (tuple(idx.shape), tuple(weight.shape)))
        n = idx.shape[1]
        out = torch.empty((B, C, n), dtype=torch.float32, device=features.device)
        bad = ops.index_check_flag(features.device)
        check(_lib.load().spgan_pointops_interpolate_cm(_p(features), _p(idx), _p(weight), B, C, m, n, _p(out), _p(bad), _s()),
              "pointops_interpolate_cm", B=B, C=C, m=m, n=n)
        ops.index_check_raise(bad, "interpolation: an index lies outside [0, %d)" % m)
        ctx.save_for_backward(idx, weight)
        ctx.cm = (C, m)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        idx, weight = ctx.saved_tensors
        C, m = ctx.cm
        B, n, _ = idx.shape
        grad_out = grad_out.contiguous()
        rowptr, src = gather_csr(idx.view(B, n * 3).to(torch.int64), m)
        dfeat = torch.empty((B, C, m), dtype=torch.float32, device=grad_out.device)
        check(_lib.load().spgan_pointops_interpolate_cm_bwd(_p(grad_out), _p(weight), _p(rowptr), _p(src), B, C, m, n, _p(dfeat), _s()),
              "pointops_interpolate_cm_bwd", B=B, C=C, m=m, n=n)
        return dfeat, None, None


interpolation = Interpolation.apply


class GroupingInt(Function):
    @staticmethod
    def forward(ctx, features, idx):
        """features int64 [B,C,n], idx int32 [B,m,nsample] -> int64 [B,C,m,nsample]."""
        if not isinstance(features, torch.Tensor) or not features.is_cuda:
            raise RuntimeError("features must live on the GPU (spgan has no CPU path)")
        if features.dtype != torch.int64 or features.dim() != 3 or min(features.shape) < 1:
            raise TypeError("features must be a non-empty int64 [B, C, n], got %s %s" % (features.dtype, tuple(features.shape)))
        features = features.contiguous()
        B, C, n = features.shape
        idx = _index(idx, "idx", 3, B)
        m, K = idx.shape[1], idx.shape[2]
        out = torch.empty((B, C, m, K), dtype=torch.int64, device=features.device)
        bad = ops.index_check_flag(features.device)
        check(_lib.load().spgan_pointops_group_int(_p(features), _p(idx), B, C, n, m, K, _p(out), _p(bad), _s()), "pointops_group_int",
              B=B, C=C, n=n, m=m, K=K)
        ops.index_check_raise(bad, "grouping_int: an index lies outside [0, %d)" % n)
        ctx.mark_non_differentiable(out)
        return out

    @staticmethod
    def backward(ctx, a=None):
        return None, None


grouping_int = GroupingInt.apply


class _GroupSlices(Function):
    """out [B, (3) + (C), m, K] = [ xyz[b, idx] (- new_xyz[b,j]) | features[b, :, idx] ]: one spgan_pointops_group_cm launch per slice into
    one buffer.  xyz [B,n,3] is read point-major (no transposed copy), the centre is subtracted in the launch (no in-place -=), the
    slices share the buffer (no torch.cat).  Any of xyz / new_xyz / features may be None (new_xyz only with xyz)."""

    @staticmethod
    def forward(ctx, xyz, new_xyz, features, idx):
        B, m, K = idx.shape
        c3 = 0 if xyz is None else 3
        C = 0 if features is None else features.shape[1]
        n = xyz.shape[1] if xyz is not None else features.shape[2]
        lib = _lib.load()
        out = torch.empty((B, c3 + C, m, K), dtype=torch.float32, device=idx.device)
        bad = ops.index_check_flag(idx.device)
        if xyz is not None:
            check(lib.spgan_pointops_group_cm(_p(xyz), 1, _p(new_xyz), _p(idx), B, 3, n, m, K, 0, c3 + C, _p(out), _p(bad), _s()),
                  "pointops_group_cm", B=B, C=3, n=n, m=m, K=K)
        if features is not None:
            check(lib.spgan_pointops_group_cm(_p(features), 0, None, _p(idx), B, C, n, m, K, c3, c3 + C, _p(out), _p(bad), _s()),
                  "pointops_group_cm", B=B, C=C, n=n, m=m, K=K, c0=c3)
        ops.index_check_raise(bad, "grouping: an index lies outside [0, %d)" % n)
        ctx.save_for_backward(idx)
        ctx.dims = (c3, C, n, new_xyz is not None)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        c3, C, n, has_center = ctx.dims
        B, m, K = idx.shape
        need_xyz, need_ctr, need_feat = ctx.needs_input_grad[0] and c3, ctx.needs_input_grad[1] and has_center, ctx.needs_input_grad[2] and C
        dout = dout.contiguous()
        lib = _lib.load()
        rowptr = src = None
        if need_xyz or need_feat:
            rowptr, src = gather_csr(idx.view(B, m * K).to(torch.int64), n)
        dxyz = torch.empty((B, n, 3), dtype=torch.float32, device=dout.device) if need_xyz else None
        dctr = torch.empty((B, m, 3), dtype=torch.float32, device=dout.device) if need_ctr else None
        dfeat = torch.empty((B, C, n), dtype=torch.float32, device=dout.device) if need_feat else None
        if need_xyz or need_ctr:
            check(lib.spgan_pointops_group_cm_bwd(_p(dout), _p(rowptr), _p(src), B, 3, n, m, K, 0, c3 + C, 1, _p(dxyz), _p(dctr), _s()),
                  "pointops_group_cm_bwd", B=B, C=3, n=n, m=m, K=K)
        if need_feat:
            check(lib.spgan_pointops_group_cm_bwd(_p(dout), _p(rowptr), _p(src), B, C, n, m, K, c3, c3 + C, 0, _p(dfeat), None, _s()),
                  "pointops_group_cm_bwd", B=B, C=C, n=n, m=m, K=K, c0=c3)
        return dxyz, dctr, dfeat, None


class Grouping(Function):
    @staticmethod
    def forward(ctx, features, idx):
        """features [B,C,n], idx int32 [B,m,nsample] -> [B,C,m,nsample]."""
        features = _feat(features, "features")
        idx = _index(idx, "idx", 3, features.shape[0])
        B, C, n = features.shape
        m, K = idx.shape[1], idx.shape[2]
        out = torch.empty((B, C, m, K), dtype=torch.float32, device=features.device)
        bad = ops.index_check_flag(features.device)
        check(_lib.load().spgan_pointops_group_cm(_p(features), 0, None, _p(idx), B, C, n, m, K, 0, C, _p(out), _p(bad), _s()),
              "pointops_group_cm", B=B, C=C, n=n, m=m, K=K)
        ops.index_check_raise(bad, "grouping: an index lies outside [0, %d)" % n)
        ctx.save_for_backward(idx)
        ctx.cn = (C, n)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        C, n = ctx.cn
        B, m, K = idx.shape
        grad_out = grad_out.contiguous()
        rowptr, src = gather_csr(idx.view(B, m * K).to(torch.int64), n)
        dfeat = torch.empty((B, C, n), dtype=torch.float32, device=grad_out.device)
        check(_lib.load().spgan_pointops_group_cm_bwd(_p(grad_out), _p(rowptr), _p(src), B, C, n, m, K, 0, C, 0, _p(dfeat), None, _s()),
              "pointops_group_cm_bwd", B=B, C=C, n=n, m=m, K=K)
        return dfeat, None


grouping = Grouping.apply


def _group_composed(xyz: Optional[Tensor], new_xyz: Optional[Tensor], features: Optional[Tensor], idx: Tensor) -> Tensor:
    """_GroupSlices from the launchers that existed before spgan_pointops_group_cm: spgan_gather_points_cm per slice on a transposed copy
    of xyz, the subtraction and torch.cat.  The same bits; kept for the measurement and as the other value of GROUP_ROUTE."""
    B, m, K = idx.shape
    flat = idx.view(B, m * K)
    parts = []
    if xyz is not None:
        g = Gathering.apply(xyz.transpose(1, 2).contiguous(), flat).view(B, 3, m, K)
        if new_xyz is not None:
            g = g - new_xyz.transpose(1, 2).unsqueeze(-1)
        parts.append(g)
    if features is not None:
        parts.append(Gathering.apply(features, flat).view(B, features.shape[1], m, K))
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)


def _group(xyz: Optional[Tensor], new_xyz: Optional[Tensor], features: Optional[Tensor], idx: Tensor) -> Tensor:
    if GROUP_ROUTE == "fused":
        return _GroupSlices.apply(xyz, new_xyz, features, idx)
    if GROUP_ROUTE == "composed":
        return _group_composed(xyz, new_xyz, features, idx)
    raise ValueError("GROUP_ROUTE must be 'fused' or 'composed', got %r" % (GROUP_ROUTE,))


# ----------------------------------------------------------------------------------------------------------------------------------
# modules
# ----------------------------------------------------------------------------------------------------------------------------------
class _QueryBase(nn.Module):
    """radius given: ball query; radius None: kNN.  `factor` times nsample neighbours are asked for (QueryAndGroup_Dilate: 2)."""

    def __init__(self, radius=None, nsample=32, use_xyz=True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def _inputs(self, xyz, new_xyz, features, idx, factor=1):
        xyz, new_xyz = _pair(xyz, new_xyz)
        B, n, _ = xyz.shape
        if features is not None:
            features = _feat(features, "features")
            if features.shape[0] != B or features.shape[2] != n:
                raise ValueError("features must be [B = %d, C, n = %d], got %s" % (B, n, tuple(features.shape)))
        if idx is None:
            if self.radius is not None:
                idx = ballquery(self.radius, factor * self.nsample, xyz, new_xyz)
            else:
                idx = knnquery(factor * self.nsample, xyz, new_xyz)
        else:
            idx = _index(idx, "idx", 3, B)
            if idx.shape[1] != new_xyz.shape[1]:
                raise ValueError("idx must be [B, m = %d, nsample], got %s" % (new_xyz.shape[1], tuple(idx.shape)))
        return xyz, new_xyz, features, idx

    def _new_features(self, xyz, new_xyz, features, idx):
        """[grouped_xyz - new_xyz | grouped features] as QueryAndGroup.forward composes them."""
        if features is not None:
            return _group(xyz if self.use_xyz else None, new_xyz if self.use_xyz else None, features, idx)
        assert self.use_xyz, "Cannot have not features and not use xyz as a feature!"
        return _group(xyz, new_xyz, None, idx)


class QueryAndGroup(_QueryBase):
    """forward(xyz [B,n,3], new_xyz [B,m,3] = None, features [B,C,n] = None, idx = None) -> [B, 3+C, m, nsample] (C alone without use_xyz,
    3 alone without features)."""

    def forward(self, xyz: Tensor, new_xyz: Tensor = None, features: Tensor = None, idx: Tensor = None) -> Tensor:
        return self._new_features(*self._inputs(xyz, new_xyz, features, idx))


class QueryAndGroup_Dilate(_QueryBase):
    """Queries 2*nsample neighbours and keeps nsample columns drawn by np.random.shuffle on the host, as the reference does: the same numpy
    seed picks the same columns.  An injected idx has 2*nsample columns."""

    def forward(self, xyz: Tensor, new_xyz: Tensor = None, features: Tensor = None, idx: Tensor = None) -> Tensor:
        xyz, new_xyz, features, idx = self._inputs(xyz, new_xyz, features, idx, factor=2)
        if idx.shape[2] != 2 * self.nsample:
            raise ValueError("idx must have 2*nsample = %d columns, got %s" % (2 * self.nsample, tuple(idx.shape)))
        idx2 = np.array([i for i in range(2 * self.nsample)])
        np.random.shuffle(idx2)
        idx2 = idx2[:self.nsample]
        idx = idx[:, :, torch.from_numpy(idx2).to(idx.device)].contiguous()
        return self._new_features(xyz, new_xyz, features, idx)


class Le_QueryAndGroup(_QueryBase):
    """-> (grouped_xyz - new_xyz [B,3,m,nsample], new_features): the grouped features [B,C,m,nsample], or grouped_xyz without features."""

    def forward(self, xyz: Tensor, new_xyz: Tensor = None, features: Tensor = None, idx: Tensor = None):
        xyz, new_xyz, features, idx = self._inputs(xyz, new_xyz, features, idx)
        grouped_xyz = _group(xyz, new_xyz, None, idx)
        if features is not None:
            return grouped_xyz, _group(None, None, features, idx)
        assert self.use_xyz, "Cannot have not features and not use xyz as a feature!"
        return grouped_xyz, grouped_xyz


class Le_QueryAndGroup_SameSize(Le_QueryAndGroup):
    """Le_QueryAndGroup with new_xyz of xyz's shape; new_xyz = None means xyz (the reference dereferences None before its own default)."""

    def forward(self, xyz: Tensor, new_xyz: Tensor = None, features: Tensor = None, idx: Tensor = None):
        if new_xyz is None:
            new_xyz = xyz
        assert xyz.size() == new_xyz.size()
        return super().forward(xyz, new_xyz, features, idx)


class Le_QueryAndGroup_OnlyFeature(_QueryBase):
    """-> the grouped features [B,C,m,nsample].  features = None raises ValueError (the reference dies on an undefined name)."""

    def forward(self, xyz: Tensor, new_xyz: Tensor = None, features: Tensor = None, idx: Tensor = None) -> Tensor:
        if features is None:
            raise ValueError("Le_QueryAndGroup_OnlyFeature needs features")
        xyz, new_xyz, features, idx = self._inputs(xyz, new_xyz, features, idx)
        return _group(None, None, features, idx)


class Gen_QueryAndGroupXYZ(_QueryBase):
    """forward(xyz, new_xyz = None) -> grouped_xyz [B,3,m,nsample], the centre NOT subtracted."""

    def forward(self, xyz: Tensor, new_xyz: Tensor = None) -> Tensor:
        xyz, new_xyz, _, idx = self._inputs(xyz, new_xyz, None, None)
        return _group(xyz, None, None, idx)


class GroupAll(nn.Module):
    """-> [B, 3+C, 1, n]: views and one concatenation, as in the reference (there is no gather to run)."""

    def __init__(self, use_xyz: bool = True):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz: Tensor, new_xyz: Tensor, features: Tensor = None) -> Tensor:
        _f32(xyz, "xyz", 3)
        grouped_xyz = xyz.transpose(1, 2).unsqueeze(2)
        if features is not None:
            grouped_features = _f32(features, "features", 3).unsqueeze(2)
            if self.use_xyz:
                return torch.cat([grouped_xyz, grouped_features], dim=1)
            return grouped_features
        return grouped_xyz
