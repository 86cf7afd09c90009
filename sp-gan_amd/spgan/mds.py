"""Minimum-density sampling and the channel-major gather that goes with it: metrics/MDS/MDS_module.py over csrc/expansion.hip.

  minimum_density_sample(xyz [B,N,3], npoint, mean_mst_length [B], split=8192) -> int32 [B,npoint]
      The first pick is point 0.  A running density T starts at 0 (1e9 once selected); every further step adds
      w_k * exp(-d_k / (5 L^2)) for the squared distance d_k to the last pick (L = mean_mst_length[b], the expansion penalty's
      third output; w_k = 1 for k < split, else 2 -- the reference hard-codes 8192) and selects the point of least density, the
      LOWEST index among exact ties.  The reference breaks ties by thread id, which depends on its block size; in float32 ties are
      real (all densities that underflowed to 0), so the rule is fixed here.  No gradient.
  gather_operation(features [B,C,N], idx int32 [B,m]) -> [B,C,m]
      out[b,c,j] = features[b,c,idx[b,j]].  The backward is a deterministic scatter-add that sums duplicate indices (the reference's
      plain `+=` keeps one of them); the two agree on sampled index sets, which are distinct.  N <= 16384 in the backward.
"""
from __future__ import annotations

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib, ops
from .ops import _f32, _i32, _p, _s, check
from .pointnet_util import gather_csr

Tensor = torch.Tensor


def minimum_density_sample(xyz: Tensor, npoint: int, mean_mst_length: Tensor, split: int = 8192) -> Tensor:
    _f32(xyz, "xyz", 3)
    _f32(mean_mst_length, "mean_mst_length", 1)
    B, N, c = xyz.shape
    if c != 3 or B < 1 or N < 1:
        raise ValueError("xyz must be [B, N, 3] with B, N >= 1, got %s" % (tuple(xyz.shape),))
    if mean_mst_length.shape[0] != B:
        raise ValueError("mean_mst_length must have B = %d entries, got %d" % (B, mean_mst_length.shape[0]))
    npoint = int(npoint)
    if not 1 <= npoint <= N:
        raise ValueError("npoint must lie in [1, N = %d], got %d" % (N, npoint))
    xyz = xyz.detach().contiguous()
    L = mean_mst_length.detach().contiguous()
    lib = _lib.load()
    out = torch.empty((B, npoint), dtype=torch.int32, device=xyz.device)
    ws = torch.empty((B, N), dtype=torch.float32, device=xyz.device) if lib.spgan_minimum_density_sample_needs_ws(N) else None
    check(lib.spgan_minimum_density_sample(_p(xyz), B, N, npoint, _p(L), int(split), _p(out), _p(ws), _s()), "minimum_density_sample",
          B=B, N=N, npoint=npoint)
    return out


class _GatherOperationFn(Function):
    @staticmethod
    def forward(ctx, features, idx):
        B, C, N = features.shape
        m = idx.shape[1]
        out = torch.empty((B, C, m), dtype=torch.float32, device=features.device)
        bad = ops.index_check_flag(features.device)
        check(_lib.load().spgan_gather_points_cm(_p(features), _p(idx), B, C, N, m, _p(out), _p(bad), _s()), "gather_points_cm",
              B=B, C=C, N=N, m=m)
        ops.index_check_raise(bad, "gather_operation: an index lies outside [0, %d)" % N)
        ctx.save_for_backward(idx)
        ctx.shape = (B, C, N)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        B, C, N = ctx.shape
        m = idx.shape[1]
        dout = dout.contiguous()
        rowptr, src = gather_csr(idx.to(torch.int64), N)
        dfeat = torch.empty((B, C, N), dtype=torch.float32, device=dout.device)
        check(_lib.load().spgan_gather_points_cm_bwd(_p(dout), _p(rowptr), _p(src), B, C, N, m, _p(dfeat), _s()), "gather_points_cm_bwd",
              B=B, C=C, N=N, m=m)
        return dfeat, None


def gather_operation(features: Tensor, idx: Tensor) -> Tensor:
    _f32(features, "features", 3)
    if not isinstance(idx, torch.Tensor) or not idx.is_cuda:
        raise RuntimeError("idx must be a tensor on the GPU (spgan has no CPU path)")
    if idx.dtype != torch.int32 or idx.dim() != 2 or idx.shape[0] != features.shape[0]:
        raise ValueError("idx must be int32 [B, m] with B = %d, got %s %s" % (features.shape[0], idx.dtype, tuple(idx.shape)))
    if min(features.shape) < 1 or idx.shape[1] < 1:
        raise ValueError("empty features %s or idx %s" % (tuple(features.shape), tuple(idx.shape)))
    return _GatherOperationFn.apply(features.contiguous(), _i32(idx.contiguous(), "idx"))
