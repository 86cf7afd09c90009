"""Local-shape Chamfer: the "shape-preserving loss" of Common/loss_utils.py:196-259 (get_local_pair, K = 20) and the evaluation
distance of Common/GAN_metrics.py:596-656 (local_CD / pairwise_local_CD, K = 8), over the HIP kernels of csrc/local_cd.hip.

  knn_moments(query, cloud, k)     the k nearest cloud points of every query (pointops knnquery order) -> idx, mu, cov
                                   (cov in the 6-entry form [xx, xy, xz, yy, yz, zz]); autograd through `cloud` only, as pointops'
                                   index carries no gradient
  ChamferLoss                      the reference class: sum_i min_j + sum_j min_i over the whole batch, D = 3 or 9
  local_CD(pt1, pt2)               [B,N,3] clouds -> (mean term, covariance term), K = 8
  get_local_pair(pt1, pt2)         [B,3,M] clouds -> (like_mu12, like_var12), K = 20; re-exported by spgan.losses
  pairwise_local_cd(sample, ref)   [S,N,3] x [R,M,3] -> [S,R,2], all pairs in one call

The covariance Chamfer runs on the 6-entry storage with the off-diagonal squared differences weighted by 2, which equals the
reference's distance between the flattened 3x3 matrices.  Distances are exact differences, not the |x|^2 + |y|^2 - 2<x,y> expansion
the reference evaluates, so values differ from it at the level of that expansion's float32 cancellation.
"""
from __future__ import annotations

from typing import Tuple

import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib
from .ops import _f32, _p, _s, check
from .pointnet_util import _scatter_slots, gather_csr

Tensor = torch.Tensor

SYM6 = 6        # spgan_nn_dim's D for the 6-entry symmetric storage


def _cloud(t: Tensor, name: str) -> Tensor:
    _f32(t, name, 3)
    if t.shape[2] != 3:
        raise ValueError("%s must be [B, N, 3], got %s" % (name, tuple(t.shape)))
    return t.contiguous()


def _moments(query: Tensor, cloud: Tensor, k: int, want_idx: bool = True):
    B, M, _ = query.shape
    N = cloud.shape[1]
    dev = query.device
    idx = torch.empty((B, M, k), dtype=torch.int64, device=dev) if want_idx else None
    mu = torch.empty((B, M, 3), dtype=torch.float32, device=dev)
    cov = torch.empty((B, M, 6), dtype=torch.float32, device=dev)
    check(_lib.load().spgan_knn_moments(_p(query), _p(cloud), B, M, N, int(k), _p(idx), _p(mu), _p(cov), _s()), "knn_moments",
          B=B, M=M, N=N, k=k)
    return idx, mu, cov


class _KnnMomentsFn(Function):
    @staticmethod
    def forward(ctx, query, cloud, k):
        idx, mu, cov = _moments(query, cloud, k)
        ctx.save_for_backward(idx, cloud, mu)
        ctx.k = k
        ctx.mark_non_differentiable(idx)
        return idx, mu, cov

    @staticmethod
    def backward(ctx, _gidx, gmu, gcov):
        idx, cloud, mu = ctx.saved_tensors
        B, M, K = idx.shape
        N = cloud.shape[1]
        gmu = torch.zeros_like(mu) if gmu is None else gmu.contiguous()
        gcov = torch.zeros((B, M, 6), dtype=torch.float32, device=mu.device) if gcov is None else gcov.contiguous()
        gslot = torch.empty((B * M * K, 3), dtype=torch.float32, device=mu.device)
        check(_lib.load().spgan_moments_bwd(_p(idx), _p(cloud), _p(mu), _p(gmu), _p(gcov), B, M, N, K, _p(gslot), _s()), "moments_bwd",
              B=B, M=M, N=N, K=K)
        rowptr, src = gather_csr(idx.view(B, M * K), N)
        return None, _scatter_slots(gslot, 0, 3, rowptr, src, (B, N, 3)), None


def knn_moments(query: Tensor, cloud: Tensor, k: int) -> Tuple[Tensor, Tensor, Tensor]:
    """query [B,M,3], cloud [B,N,3] -> (idx int64 [B,M,k], mu [B,M,3], cov [B,M,6]): the k nearest cloud points of every query
    (ascending squared distance, the lower index first on ties, the query itself included when it is a cloud point), their mean
    and their biased covariance (compute_mean_covariance, loss_utils.py:196-205).  Differentiable in `cloud`."""
    q, c = _cloud(query, "query"), _cloud(cloud, "cloud")
    if q.shape[0] != c.shape[0]:
        raise ValueError("batch sizes differ: %d and %d" % (q.shape[0], c.shape[0]))
    if not 1 <= int(k) <= min(32, c.shape[1]):
        raise ValueError("k must lie in [1, min(32, N)], got %d (N = %d)" % (k, c.shape[1]))
    return _KnnMomentsFn.apply(q, c, int(k))


def _nn_dim(a: Tensor, b: Tensor, D: int):
    B, Na, _ = a.shape
    Nb = b.shape[1]
    dev = a.device
    da, db = torch.empty((B, Na), device=dev), torch.empty((B, Nb), device=dev)
    ia = torch.empty((B, Na), dtype=torch.int32, device=dev)
    ib = torch.empty((B, Nb), dtype=torch.int32, device=dev)
    check(_lib.load().spgan_nn_dim(_p(a), _p(b), B, Na, Nb, D, _p(da), _p(ia), _p(db), _p(ib), _s()), "nn_dim", B=B, Na=Na, Nb=Nb, D=D)
    return da, ia, db, ib


class _ChamferSumFn(Function):
    """a [B,Na,D], b [B,Nb,D] -> sum_{b,i} min_j d(a_i, b_j) + sum_{b,j} min_i d(a_i, b_j) (a 0-d tensor)."""

    @staticmethod
    def forward(ctx, a, b, D):
        da, ia, db, ib = _nn_dim(a, b, D)
        out = torch.empty((1,), dtype=torch.float32, device=a.device)
        check(_lib.load().spgan_pair_sum(_p(da), da.numel(), _p(db), db.numel(), 1, 1.0, _p(out), 1, _s()), "pair_sum")
        ctx.save_for_backward(a, b, ia, ib)
        ctx.D = D
        return out[0]

    @staticmethod
    def backward(ctx, g):
        a, b, ia, ib = ctx.saved_tensors
        B, Na, _ = a.shape
        Nb = b.shape[1]
        g = g.reshape(1).contiguous()
        ga, gb = torch.empty_like(a), torch.empty_like(b)
        lib = _lib.load()
        check(lib.spgan_chamfer_dim_bwd(_p(a), _p(b), B, Na, Nb, ctx.D, _p(ia), _p(ib), _p(g), _p(ga), _s()), "chamfer_dim_bwd")
        check(lib.spgan_chamfer_dim_bwd(_p(b), _p(a), B, Nb, Na, ctx.D, _p(ib), _p(ia), _p(g), _p(gb), _s()), "chamfer_dim_bwd")
        return ga, gb, None


def chamfer_sum(a: Tensor, b: Tensor, sym6: bool = False) -> Tensor:
    """Chamfer sum of two batches of D-dimensional point sets (D = 3 or 9; sym6: [.,.,6] symmetric-matrix storage, weighted)."""
    _f32(a, "a", 3)
    _f32(b, "b", 3)
    D = a.shape[2]
    if a.shape[0] != b.shape[0] or b.shape[2] != D:
        raise ValueError("expected [B,Na,D] and [B,Nb,D], got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    if (sym6 and D != 6) or (not sym6 and D not in (3, 9)):
        raise ValueError("D must be 3 or 9 (6 with sym6=True), got %d" % D)
    return _ChamferSumFn.apply(a.contiguous(), b.contiguous(), SYM6 if sym6 else D)


class ChamferLoss(nn.Module):
    """Common/loss_utils.py:94-118 (= GAN_metrics.py:23-47): forward(preds [B,N,D], gts [B,M,D]) -> sum of every point's squared
    distance to its nearest point in the other set, over both directions and the whole batch.  D = 3 or 9; differentiable in both."""

    def forward(self, preds: Tensor, gts: Tensor) -> Tensor:
        return chamfer_sum(preds, gts)


def _local_pair(q: Tensor, c2: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    _, mu1, cov1 = knn_moments(q, q, k)
    _, mu2, cov2 = knn_moments(q, c2, k)
    n = float(q.shape[1])
    return chamfer_sum(mu1, mu2) / n, chamfer_sum(cov1, cov2, sym6=True) / n


def local_CD(pt1: Tensor, pt2: Tensor, k: int = 8) -> Tuple[Tensor, Tensor]:
    """GAN_metrics.py:596-626: pt1 [B,N,3], pt2 [B,M,3] -> (Chamfer of the k-neighbourhood means, Chamfer of the covariances), each
    summed over the batch and divided by N; the neighbourhoods are those of pt1's points, in pt1 and in pt2."""
    q, c = _cloud(pt1, "pt1"), _cloud(pt2, "pt2")
    if q.shape[0] != c.shape[0]:
        raise ValueError("batch sizes differ: %d and %d" % (q.shape[0], c.shape[0]))
    return _local_pair(q, c, k)


def get_local_pair(pt1: Tensor, pt2: Tensor, k: int = 20) -> Tuple[Tensor, Tensor]:
    """Common/loss_utils.py:208-257, the shape-preserving loss: pt1 [B,3,M], pt2 [B,3,N] -> (like_mu12, like_var12).  The
    neighbourhoods are those of pt1's points (K = 20) in pt1 and in pt2; both clouds receive gradients."""
    _f32(pt1, "pt1", 3)
    _f32(pt2, "pt2", 3)
    if pt1.shape[1] != 3 or pt2.shape[1] != 3 or pt1.shape[0] != pt2.shape[0]:
        raise ValueError("expected pt1 [B,3,M] and pt2 [B,3,N], got %s and %s" % (tuple(pt1.shape), tuple(pt2.shape)))
    return _local_pair(pt1.transpose(1, 2).contiguous(), pt2.transpose(1, 2).contiguous(), k)


def pairwise_local_cd(sample: Tensor, ref: Tensor, k: int = 8) -> Tensor:
    """sample [S,N,3], ref [R,M,3] -> [S,R,2]: local_CD(sample[s:s+1], ref[r:r+1]) for every pair, equal to that loop bit for bit.
    Each sample's own neighbourhood moments are computed once; the queries always come from the sample (the entry is not
    symmetric).  No gradient."""
    a, b = _cloud(sample, "sample"), _cloud(ref, "ref")
    S, N, _ = a.shape
    R, M, _ = b.shape
    if not 1 <= int(k) <= min(32, N, M):
        raise ValueError("k must lie in [1, min(32, N, M)], got %d" % k)
    lib = _lib.load()
    wsb = lib.spgan_pairwise_local_cd_ws_bytes(S, R, N, M)
    ws = torch.empty((wsb // 4 + 1,), dtype=torch.float32, device=a.device)
    out = torch.empty((S, R, 2), dtype=torch.float32, device=a.device)
    check(lib.spgan_pairwise_local_cd(_p(a), _p(b), S, R, N, M, int(k), _p(out), _p(ws), wsb, _s()), "pairwise_local_cd",
          S=S, R=R, N=N, M=M, k=k)
    return out
