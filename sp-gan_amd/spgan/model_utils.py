"""The point-distribution losses of Common/model_utils.py over the HIP kernels of csrc/point_losses.hip.

    from spgan.model_utils import get_repulsion_loss, get_repulsion_loss4, get_perulsion_loss, get_uniform_loss_knn
    from spgan.model_utils import get_cd_loss, get_cd_loss2, get_hausdorff_loss, get_emd_loss, group_nearest

The reference file is TensorFlow 1 over custom ops that are not part of its tree; the signatures here are its own, the semantics of the
missing ops are those of this project's ball query and kNN.  pred / gt are [B,N,3] float32 device tensors; every loss is
a 0-dim float32 tensor, once differentiable, and nothing here synchronises with the host, so each loss runs inside spgan.CapturedBody.

Every repulsion loss groups each point's neighbours (ball: the first `nsample` indices with d2 < radius*radius, padded with the first
hit; kNN: the `nsample` nearest, ties to the lower index), measures the slots (`sq` d2, `l1` |dx|+|dy|+|dz|, `root` sqrt(d2 + 1e-12)),
takes the five smallest by (value, slot), drops the first and averages a tail over the other four.  One wave per point does that from
one scan of the cloud: no [B,N,nsample] index tensor and no [B,N,nsample,3] grouped tensor exists in ball mode, and only [B,N,5] values,
indices and tail derivatives are kept for the backward pass, whose sums have a fixed order (no float atomics).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from .approxmatch import match_cost
from .metrics import nn_distance
from .ops import _f32, _p, _s, check

Tensor = torch.Tensor

METRICS = {"sq": 0, "l1": 1, "root": 2}
TAIL_NONE, TAIL_HINGE, TAIL_REP4 = 0, 1, 2
MIN_NSAMPLE, MAX_NSAMPLE_BALL, MAX_NSAMPLE_KNN, MAX_KEEP = 5, 256, 200, 8
# how the backward pass finds the slots that selected a point: "csr" goes through spgan_gather_csr's per-point slot lists (three
# launches), "table" walks the cloud's [N,keep] index table (one launch; the route that lost, profiles/point_losses_bench.json).  Clouds
# beyond spgan_gather_csr's limit take the table walk.
BACKWARD_ROUTE = "csr"
CSR_MAX_POINTS = 16384


def _validate(pred: Tensor, nsample: int, radius: Optional[float], knn: bool, metric: str, keep: int) -> Tensor:
    """Shapes and sizes first (ValueError, on any device), then the device and dtype (as elsewhere in the package)."""
    if not isinstance(pred, torch.Tensor):
        raise TypeError("pred must be a torch.Tensor")
    if pred.dim() != 3 or pred.shape[2] != 3 or pred.shape[0] < 1 or pred.shape[1] < 1:
        raise ValueError("pred must be [B, N, 3] with B, N >= 1, got %s" % (tuple(pred.shape),))
    if metric not in METRICS:
        raise ValueError("metric must be one of %s, got %r" % (sorted(METRICS), metric))
    nsample, keep = int(nsample), int(keep)
    top = MAX_NSAMPLE_KNN if knn else MAX_NSAMPLE_BALL
    if not MIN_NSAMPLE <= nsample <= top:
        raise ValueError("nsample must lie in [%d, %d] in %s mode, got %d" % (MIN_NSAMPLE, top, "kNN" if knn else "ball", nsample))
    if not 2 <= keep <= min(MAX_KEEP, nsample):
        raise ValueError("keep must lie in [2, min(%d, nsample)], got %d" % (MAX_KEEP, keep))
    if knn:
        if pred.shape[1] < nsample:
            raise ValueError("kNN mode needs N >= nsample, got N = %d, nsample = %d" % (pred.shape[1], nsample))
    else:
        r = float(radius)
        if not r > 0.0 or math.isinf(r):
            raise ValueError("radius must be a positive finite number in ball mode, got %r" % (radius,))
    return _f32(pred, "pred", 3).contiguous()


def _forward(pred: Tensor, nsample: int, radius: Optional[float], knn: bool, metric: str, keep: int, tail: int, h: float, rterm: float):
    """-> (val, idx, coef, loss); coef and loss are None without a tail."""
    B, N, _ = pred.shape
    dev = pred.device
    lib = _lib.load()
    knn_idx = None
    if knn:
        knn_idx = torch.empty((B, N, nsample), dtype=torch.int32, device=dev)
        d2 = torch.empty((B, N, nsample), dtype=torch.float32, device=dev)
        check(lib.spgan_pointops_knnquery(_p(pred), _p(pred), B, N, N, nsample, _p(knn_idx), _p(d2), _s()), "pointops_knnquery",
              B=B, n=N, nsample=nsample)
    val = torch.empty((B, N, keep), dtype=torch.float32, device=dev)
    idx = torch.empty((B, N, keep), dtype=torch.int32, device=dev)
    coef = partial = loss = None
    if tail != TAIL_NONE:
        coef = torch.empty((B, N, keep), dtype=torch.float32, device=dev)
        partial = torch.empty((lib.spgan_point_losses_partials(B, N),), dtype=torch.float64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
    st = lib.spgan_point_losses_fwd(_p(pred), _p(knn_idx), B, N, nsample, 0.0 if knn else float(radius), METRICS[metric], keep, tail,
                                    float(h), float(rterm), _p(val), _p(idx), _p(coef), _p(partial), _p(loss), _s())
    if st == -22:
        raise ValueError("point_losses_fwd refused its sizes: B=%d N=%d nsample=%d radius=%r keep=%d" % (B, N, nsample, radius, keep))
    check(st, "point_losses_fwd", B=B, N=N, nsample=nsample, keep=keep)
    return val, idx, coef, loss


def _backward(pred: Tensor, idx: Tensor, coef: Tensor, gscale: Optional[Tensor], scale: float, metric: str) -> Tensor:
    B, N, keep = idx.shape
    lib = _lib.load()
    rowptr = slots = None
    if BACKWARD_ROUTE == "csr" and N <= CSR_MAX_POINTS:
        rowptr = torch.empty((B * N, 2), dtype=torch.int32, device=pred.device)
        slots = torch.empty((B * N * keep,), dtype=torch.int32, device=pred.device)
        idx64 = idx.reshape(B, N * keep).to(torch.int64)
        check(lib.spgan_gather_csr(_p(idx64), B, N * keep, N, _p(rowptr), _p(slots), None, _s()), "gather_csr", B=B, S=N * keep, N=N)
    dpred = torch.empty_like(pred)
    check(lib.spgan_point_losses_bwd(_p(pred), _p(idx), _p(coef), _p(gscale), float(scale), B, N, keep, METRICS[metric], _p(rowptr), _p(slots),
                                     _p(dpred), _s()), "point_losses_bwd", B=B, N=N, keep=keep)
    return dpred


class _GroupNearest(Function):
    @staticmethod
    def forward(ctx, pred, nsample, radius, knn, metric, keep):
        val, idx, _, _ = _forward(pred, nsample, radius, knn, metric, keep, TAIL_NONE, 0.0, 0.0)
        ctx.save_for_backward(pred, idx)
        ctx.metric = metric
        ctx.mark_non_differentiable(idx)
        return val, idx

    @staticmethod
    @once_differentiable
    def backward(ctx, gval, _gidx):
        pred, idx = ctx.saved_tensors
        gval = _f32(gval, "grad_val", 3).contiguous()
        return _backward(pred, idx, gval, None, 1.0, ctx.metric), None, None, None, None, None


class _PointLoss(Function):
    @staticmethod
    def forward(ctx, pred, nsample, radius, knn, metric, tail, h, rterm):
        _, idx, coef, loss = _forward(pred, nsample, radius, knn, metric, 5, tail, h, rterm)
        ctx.save_for_backward(pred, idx, coef)
        ctx.metric = metric
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        pred, idx, coef = ctx.saved_tensors
        B, N, keep = idx.shape
        gout = _f32(gout, "grad_loss").contiguous()
        return _backward(pred, idx, coef, gout, 1.0 / (B * N * (keep - 1)), ctx.metric), None, None, None, None, None, None, None


def group_nearest(pred: Tensor, nsample: int, radius: Optional[float] = None, metric: str = "sq", keep: int = 5) -> Tuple[Tensor, Tensor]:
    """-> (val [B,N,keep] float32, idx [B,N,keep] int32): the `keep` smallest slots of every point's group by (value, slot), ascending --
    the ball of `radius`, or with radius=None the `nsample` nearest neighbours (self included).  Differentiable in val."""
    knn = radius is None
    pred = _validate(pred, nsample, radius, knn, metric, keep)
    return _GroupNearest.apply(pred, int(nsample), radius, knn, metric, int(keep))


def get_repulsion_loss(pred: Tensor, nsample: int = 20, radius: float = 0.07, knn: bool = False, use_l1: bool = False, h: float = 0.001) -> Tensor:
    """model_utils.py:141-185: mean of max(0, h_eff - v) over the 2nd..5th smallest slot values; v = d2 and h_eff = h, or with use_l1
    v = |dx|+|dy|+|dz| and h_eff = 2*sqrt(h)."""
    metric = "l1" if use_l1 else "sq"
    pred = _validate(pred, nsample, radius, bool(knn), metric, 5)
    h_eff = math.sqrt(h) * 2 if use_l1 else float(h)
    return _PointLoss.apply(pred, int(nsample), radius, bool(knn), metric, TAIL_HINGE, h_eff, 0.0)


def get_repulsion_loss4(pred: Tensor, nsample: int = 20, radius: float = 0.07) -> Tensor:
    """model_utils.py:189-206: mean of radius - sqrt(w) * exp(-w / 0.03**2), w = max(1e-12, d2), over the 2nd..5th smallest d2 of the ball."""
    pred = _validate(pred, nsample, radius, False, "sq", 5)
    return _PointLoss.apply(pred, int(nsample), radius, False, "sq", TAIL_REP4, 0.03, float(radius))


def get_perulsion_loss(pred: Tensor, nsample: int = 15, radius: float = 0.07, knn: bool = False, numpoint: int = 512, use_l1: bool = False) -> Tensor:
    """model_utils.py:209-236: the hinge with h_eff = 0.01 on d2, or with use_l1 h_eff = 2*sqrt(0.001) on sqrt(d2 + 1e-12).  `numpoint`
    only shapes a summary constant in the reference and is ignored."""
    metric = "root" if use_l1 else "sq"
    pred = _validate(pred, nsample, radius, bool(knn), metric, 5)
    h_eff = math.sqrt(0.001) * 2 if use_l1 else 0.01
    return _PointLoss.apply(pred, int(nsample), radius, bool(knn), metric, TAIL_HINGE, h_eff, 0.0)


def get_uniform_loss_knn(pred: Tensor) -> Tensor:
    """model_utils.py:314-322: sum_b var_n(mean_k val) + sum_{b,n} var_k(val) over the six nearest squared distances (self included),
    population variances."""
    val, _ = group_nearest(pred, 6, None, "sq", 6)
    return val.mean(dim=2).var(dim=1, unbiased=False).sum() + val.var(dim=2, unbiased=False).sum()


def _nn(pred: Tensor, gt: Tensor):
    """dists_forward [B,Ngt] (gt -> pred), dists_backward [B,Npred]: the reference's nn_distance(gt, pred)."""
    return nn_distance(gt, pred)


def get_cd_loss(pred: Tensor, gt: Tensor, radius: float):
    """model_utils.py:303-312 -> (loss, None): mean_b of mean(0.8 * forward + 0.2 * backward) / radius; the two means are taken apart,
    which is the reference's value at equal point counts and also defined at unequal ones."""
    f, b = _nn(pred, gt)
    cd = (0.8 * f.mean(dim=1) + 0.2 * b.mean(dim=1)) / radius
    return cd.mean(), None


def get_cd_loss2(pred: Tensor, gt: Tensor, radius: float, forward_weight: float = 1.0, threshold: Optional[float] = 100) -> Tensor:
    """model_utils.py:238-258: distances at or above threshold * (their cloud's mean) count as 0; `radius` is unused, as there."""
    f, b = _nn(pred, gt)
    if threshold is not None:
        f = torch.where(f < f.mean(dim=1, keepdim=True) * threshold, f, torch.zeros_like(f))
        b = torch.where(b < b.mean(dim=1, keepdim=True) * threshold, b, torch.zeros_like(b))
    return (forward_weight * f.mean(dim=1) + b.mean(dim=1)).mean()


def get_hausdorff_loss(pred: Tensor, gt: Tensor, radius: float, forward_weight: float = 1.0, threshold: Optional[float] = None):
    """model_utils.py:261-279 -> (loss, None): max_b of (forward_weight * max forward + max backward) / radius; distances at or above
    `threshold` count as 0."""
    f, b = _nn(pred, gt)
    if threshold is not None:
        f = torch.where(f < threshold, f, torch.zeros_like(f))
        b = torch.where(b < threshold, b, torch.zeros_like(b))
    cd = (forward_weight * f.amax(dim=1) + b.amax(dim=1)) / radius
    return cd.amax(), None


def get_emd_loss(pcd1: Tensor, pcd2: Tensor, radius) -> Tensor:
    """model_utils.py:281-287: mean_b of match_cost(pcd1, pcd2) / radius / N, the approxmatch EMD of tf_approxmatch (spgan.approxmatch:
    fused, the [B,N,N] plan that the reference's approx_match returns is never formed).  `radius` is a float or a [B] tensor; the two
    clouds must have the same point count.  The reference's `_get_emd_loss` (:290-301) unpacks two results from an op that returns one
    and cannot run there; it is not provided."""
    if pcd1.dim() != 3 or pcd2.dim() != 3 or pcd1.shape[1] != pcd2.shape[1]:
        raise ValueError("pcd1 and pcd2 must be [B, N, 3] with the same N, got %s and %s" % (tuple(pcd1.shape), tuple(pcd2.shape)))
    cost = match_cost(pcd1, pcd2) / radius
    return (cost / float(pcd1.shape[1])).mean()
