"""The pointnet2 extension's ops: metrics/pointnet2/pointnet2_utils.py (= metrics/pointnet2_utils.py) of the reference over HIP kernels.

Names, argument names, layouts and dtypes are the reference's: coordinates [B,N,3], features [B,C,N], every index tensor int32.

    from spgan import pointnet2_utils                 # or, with the reference's own import lines: spgan.compat.install()
    idx = pointnet2_utils.furthest_point_sample(xyz, npoint)              # int32 [B,npoint], the first pick is point 0
    new_xyz = pointnet2_utils.gather_operation(xyz.transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()
    idx = pointnet2_utils.ball_query(radius, nsample, xyz, new_xyz)       # int32 [B,npoint,nsample]
    new_features = pointnet2_utils.QueryAndGroup(radius, nsample)(xyz, new_xyz, features)      # [B, 3+C, npoint, nsample]

Every op has the semantics of a pointops one (INTEGRATION 23 lists them kernel by kernel), so each calls that launcher; the one kernel
that is new for this extension, the multi-radius ball query `ball_query_multi`, lives in csrc/sa_group.hip.  Squared distances are
d2 = (dx*dx + dy*dy) + dz*dz in float32 with dx = centre - candidate, each operation rounded on its own.  Backward sums run over per-point
slot lists in ascending slot order (no float atomics).  A CPU tensor or a wrong shape raises ValueError; there is no CPU path.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib, ops, pointops
from .ops import _p, _s, check

Tensor = torch.Tensor

MAX_SCALES = _lib.SA_MAX_SCALES      # radii per ball_query_multi launch


def _gpu(t, name: str, dtype, dims: int) -> Tensor:
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
    if not t.is_cuda:
        raise ValueError("%s must live on the GPU (spgan has no CPU path); got device %s" % (name, t.device))
    if t.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if t.dim() != dims or min(t.shape) < 1:
        raise ValueError("%s must be a non-empty %d-D tensor, got shape %s" % (name, dims, tuple(t.shape)))
    return t.contiguous()


def _cloud(t, name: str) -> Tensor:
    t = _gpu(t, name, torch.float32, 3)
    if t.shape[2] != 3:
        raise ValueError("%s must be [B, N, 3], got %s" % (name, tuple(t.shape)))
    return t


def _same_batch(a: Tensor, b: Tensor, na: str, nb: str) -> None:
    if a.shape[0] != b.shape[0]:
        raise ValueError("%s and %s differ in B: %s, %s" % (na, nb, tuple(a.shape), tuple(b.shape)))


def _count(v, name: str) -> int:
    v = int(v)
    if v < 1:
        raise ValueError("%s must be >= 1, got %d" % (name, v))
    return v


class RandomDropout(nn.Module):
    """Drops whole feature channels with a probability drawn from U(0, p) per call, without rescaling the kept ones (the reference names
    a helper, feature_dropout_no_scaling, that its pytorch_utils.py does not define; this is that helper's stated meaning)."""

    def __init__(self, p=0.5, inplace=False):
        super().__init__()
        self.p = p
        self.inplace = inplace

    def forward(self, X):
        theta = float(torch.Tensor(1).uniform_(0, self.p)[0])
        if not self.training or theta <= 0.0:
            return X
        keep = (torch.rand(X.shape[:2], device=X.device) >= theta).to(X.dtype)
        keep = keep.view(tuple(X.shape[:2]) + (1,) * (X.dim() - 2))
        return X.mul_(keep) if self.inplace else X * keep


class FurthestPointSampling(Function):
    @staticmethod
    def forward(ctx, xyz: Tensor, npoint: int) -> Tensor:
        """xyz [B,N,3] -> int32 [B,npoint]; the first pick is point 0 and no point is skipped for its magnitude."""
        xyz = _cloud(xyz, "xyz")
        idx = pointops.furthestsampling(xyz, _count(npoint, "npoint"))
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(xyz, a=None):
        return None, None


furthest_point_sample = FurthestPointSampling.apply


class GatherOperation(Function):
    @staticmethod
    def forward(ctx, features: Tensor, idx: Tensor) -> Tensor:
        """features [B,C,N], idx int32 [B,npoint] -> [B,C,npoint]."""
        features = _gpu(features, "features", torch.float32, 3)
        idx = _gpu(idx, "idx", torch.int32, 2)
        _same_batch(features, idx, "features", "idx")
        ctx.save_for_backward(idx)
        ctx.cn = (features.shape[1], features.shape[2])
        return pointops._gather_cm(features, idx, "gather_operation", False)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        return pointops._gather_cm_bwd(grad_out, idx, *ctx.cn), None


gather_operation = GatherOperation.apply


class ThreeNN(Function):
    @staticmethod
    def forward(ctx, unknown: Tensor, known: Tensor) -> Tuple[Tensor, Tensor]:
        """unknown [B,N,3], known [B,M,3] -> (dist [B,N,3] = sqrt(d2), idx int32 [B,N,3]) of the three nearest known, ascending (d2, index);
        with M < 3 the missing slots hold index 0 and +inf."""
        unknown, known = _cloud(unknown, "unknown"), _cloud(known, "known")
        _same_batch(unknown, known, "unknown", "known")
        dist, idx = pointops.nearestneighbor(unknown, known)
        ctx.mark_non_differentiable(dist, idx)
        return dist, idx

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None


three_nn = ThreeNN.apply


class ThreeInterpolate(Function):
    @staticmethod
    def forward(ctx, features: Tensor, idx: Tensor, weight: Tensor) -> Tensor:
        """features [B,C,M], idx int32 [B,n,3], weight [B,n,3] -> [B,C,n] = (w0*f0 + w1*f1) + w2*f2; differentiable in features only."""
        features = _gpu(features, "features", torch.float32, 3)
        idx = _gpu(idx, "idx", torch.int32, 3)
        weight = _gpu(weight, "weight", torch.float32, 3).detach()
        _same_batch(features, idx, "features", "idx")
        if idx.shape[2] != 3 or weight.shape != idx.shape:
            raise ValueError("idx and weight must be [B, n, 3], got %s and %s" % (tuple(idx.shape), tuple(weight.shape)))
        B, C, m = features.shape
        n = idx.shape[1]
        out = torch.empty((B, C, n), dtype=torch.float32, device=features.device)
        bad = ops.index_check_flag(features.device)
        check(_lib.load().spgan_pointops_interpolate_cm(_p(features), _p(idx), _p(weight), B, C, m, n, _p(out), _p(bad), _s()),
              "pointops_interpolate_cm", B=B, C=C, m=m, n=n)
        ops.index_check_raise(bad, "three_interpolate: an index lies outside [0, %d)" % m)
        ctx.save_for_backward(idx, weight)
        ctx.cm = (C, m)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor):
        idx, weight = ctx.saved_tensors
        C, m = ctx.cm
        B, n, _ = idx.shape
        grad_out = grad_out.contiguous()
        rowptr, src = pointops.gather_csr(idx.view(B, n * 3).to(torch.int64), m)
        dfeat = torch.empty((B, C, m), dtype=torch.float32, device=grad_out.device)
        check(_lib.load().spgan_pointops_interpolate_cm_bwd(_p(grad_out), _p(weight), _p(rowptr), _p(src), B, C, m, n, _p(dfeat), _s()),
              "pointops_interpolate_cm_bwd", B=B, C=C, m=m, n=n)
        return dfeat, None, None


three_interpolate = ThreeInterpolate.apply


class GroupingOperation(Function):
    @staticmethod
    def forward(ctx, features: Tensor, idx: Tensor) -> Tensor:
        """features [B,C,N], idx int32 [B,npoint,nsample] -> [B,C,npoint,nsample]."""
        features = _gpu(features, "features", torch.float32, 3)
        idx = _gpu(idx, "idx", torch.int32, 3)
        _same_batch(features, idx, "features", "idx")
        B, C, n = features.shape
        m, K = idx.shape[1], idx.shape[2]
        out = torch.empty((B, C, m, K), dtype=torch.float32, device=features.device)
        bad = ops.index_check_flag(features.device)
        check(_lib.load().spgan_pointops_group_cm(_p(features), 0, None, _p(idx), B, C, n, m, K, 0, C, _p(out), _p(bad), _s()),
              "pointops_group_cm", B=B, C=C, n=n, m=m, K=K)
        ops.index_check_raise(bad, "grouping_operation: an index lies outside [0, %d)" % n)
        ctx.save_for_backward(idx)
        ctx.cn = (C, n)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor):
        (idx,) = ctx.saved_tensors
        C, n = ctx.cn
        B, m, K = idx.shape
        grad_out = grad_out.contiguous()
        rowptr, src = pointops.gather_csr(idx.view(B, m * K).to(torch.int64), n)
        dfeat = torch.empty((B, C, n), dtype=torch.float32, device=grad_out.device)
        check(_lib.load().spgan_pointops_group_cm_bwd(_p(grad_out), _p(rowptr), _p(src), B, C, n, m, K, 0, C, 0, _p(dfeat), None, _s()),
              "pointops_group_cm_bwd", B=B, C=C, n=n, m=m, K=K)
        return dfeat, None


grouping_operation = GroupingOperation.apply


class BallQuery(Function):
    @staticmethod
    def forward(ctx, radius: float, nsample: int, xyz: Tensor, new_xyz: Tensor) -> Tensor:
        """-> idx int32 [B,npoint,nsample]: the cloud is walked in index order; the first point with d2 < radius*radius (strict) fills
        every slot, later hits overwrite slots 1, 2, ... and the walk ends at nsample hits; an empty ball keeps index 0 in every slot."""
        xyz, new_xyz = _cloud(xyz, "xyz"), _cloud(new_xyz, "new_xyz")
        _same_batch(xyz, new_xyz, "xyz", "new_xyz")
        idx = pointops.ballquery(float(radius), _count(nsample, "nsample"), xyz, new_xyz)
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, a=None):
        return None, None, None, None


ball_query = BallQuery.apply


def ball_query_multi(radii: Sequence[float], nsamples: Sequence[int], xyz: Tensor, new_xyz: Tensor) -> List[Tensor]:
    """The ball queries of up to MAX_SCALES radii around the same centres in ONE walk of the cloud (spgan_sa_ballquery_multi):
    -> [idx int32 [B,npoint,nsamples[s]] per scale], each equal to ball_query(radii[s], nsamples[s], xyz, new_xyz) bit for bit.  More
    radii than MAX_SCALES go in several launches."""
    xyz, new_xyz = _cloud(xyz.detach(), "xyz"), _cloud(new_xyz.detach(), "new_xyz")
    _same_batch(xyz, new_xyz, "xyz", "new_xyz")
    if len(radii) != len(nsamples) or len(radii) < 1:
        raise ValueError("radii and nsamples must be non-empty lists of one length, got %d and %d" % (len(radii), len(nsamples)))
    B, n, _ = xyz.shape
    m = new_xyz.shape[1]
    outs = [torch.empty((B, m, _count(k, "nsample")), dtype=torch.int32, device=xyz.device) for k in nsamples]
    lib = _lib.load()
    for s0 in range(0, len(outs), MAX_SCALES):
        a = _lib.SaQueryArgs()
        part = outs[s0:s0 + MAX_SCALES]
        a.count = len(part)
        for i, t in enumerate(part):
            a.radius[i], a.nsample[i], a.idx[i] = float(radii[s0 + i]), t.shape[2], t.data_ptr()
        check(lib.spgan_sa_ballquery_multi(a, _p(xyz), _p(new_xyz), B, n, m, _s()), "sa_ballquery_multi", B=B, n=n, m=m, scales=a.count)
    return outs


class QueryAndGroup(nn.Module):
    """forward(xyz [B,N,3], new_xyz [B,npoint,3], features [B,C,N] = None) -> [B, 3+C, npoint, nsample] = [grouped_xyz - new_xyz | grouped
    features] (C alone without use_xyz, 3 alone without features).  The centre is subtracted inside the grouping launch: no tensor the
    caller can see is changed in place."""

    def __init__(self, radius: float, nsample: int, use_xyz: bool = True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz: Tensor, new_xyz: Tensor, features: Tensor = None) -> Tensor:
        xyz, new_xyz = _cloud(xyz, "xyz"), _cloud(new_xyz, "new_xyz")
        _same_batch(xyz, new_xyz, "xyz", "new_xyz")
        idx = ball_query(self.radius, self.nsample, xyz, new_xyz)
        return group_around(xyz, new_xyz, features, idx, self.use_xyz)


def group_around(xyz: Tensor, new_xyz: Tensor, features, idx: Tensor, use_xyz: bool) -> Tensor:
    """QueryAndGroup's composition for a given index list (spgan_pointops_group_cm per slice into one buffer)."""
    if features is not None:
        features = _gpu(features, "features", torch.float32, 3)
        if features.shape[0] != xyz.shape[0] or features.shape[2] != xyz.shape[1]:
            raise ValueError("features must be [B = %d, C, N = %d], got %s" % (xyz.shape[0], xyz.shape[1], tuple(features.shape)))
        if use_xyz:
            return pointops._GroupSlices.apply(xyz, new_xyz, features, idx)
        return pointops._GroupSlices.apply(None, None, features, idx)
    assert use_xyz, "Cannot have not features and not use xyz as a feature!"
    return pointops._GroupSlices.apply(xyz, new_xyz, None, idx)


class GroupAll(nn.Module):
    """forward(xyz [B,N,3], new_xyz (ignored), features [B,C,N] = None) -> [B, 3+C, 1, N]: views and one concatenation, nothing is gathered."""

    def __init__(self, use_xyz: bool = True):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz: Tensor, new_xyz: Tensor, features: Tensor = None) -> Tensor:
        xyz = _cloud(xyz, "xyz")
        grouped_xyz = xyz.transpose(1, 2).unsqueeze(2)
        if features is not None:
            grouped_features = _gpu(features, "features", torch.float32, 3).unsqueeze(2)
            if self.use_xyz:
                return torch.cat([grouped_xyz, grouped_features], dim=1)
            return grouped_features
        return grouped_xyz
