"""MST expansion penalty: metrics/expansion_penalty/expansion_penalty_module.py over the HIP kernels of csrc/expansion.hip.

    from spgan.expansion_penalty import expansionPenaltyModule
    dist, assignment, mean_mst_length = expansionPenaltyModule()(xyz, primitive_size, alpha)

xyz [B,n,3]; every run of `primitive_size` consecutive points is one surface element.  Per element a minimum spanning tree is built
(Prim from the element's first point), every tree edge is assigned to one of its endpoints, and an edge longer than alpha times the
element's mean edge length is penalised: dist[b,j] is its length and assignment[b,j] the other endpoint (an index into the cloud) at
the owning endpoint j; every other point has dist 0 and assignment -1.  mean_mst_length [B] is the cloud's mean of the element means.

Once differentiable: grad_xyz[b,j] = 2 * grad_dist[b,j] * (xyz[b,j] - xyz[b,assignment[b,j]]) at the owning endpoints, 0 elsewhere --
only the owner receives a gradient and the factor is that of a squared length, both as in the reference.  No [B, n*512] adjacency
workspace is allocated (the reference holds two), results repeat bit for bit.  Differences from the reference: INTEGRATION 21.
"""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from .ops import _f32, _p, _s, check

Tensor = torch.Tensor

MAX_PRIMITIVE_SIZE = 512


def _check_sizes(xyz: Tensor, primitive_size: int) -> None:
    if not isinstance(xyz, torch.Tensor):
        raise TypeError("input must be a torch.Tensor")
    if xyz.dim() != 3 or xyz.shape[2] != 3 or xyz.shape[0] < 1 or xyz.shape[1] < 1:
        raise ValueError("input must be [B, n, 3] with B, n >= 1, got %s" % (tuple(xyz.shape),))
    p = int(primitive_size)
    if not 2 <= p <= MAX_PRIMITIVE_SIZE:
        raise ValueError("primitive_size must lie in [2, %d], got %d" % (MAX_PRIMITIVE_SIZE, p))
    if xyz.shape[1] % p != 0:
        raise ValueError("n = %d is not a multiple of primitive_size = %d" % (xyz.shape[1], p))
    _f32(xyz, "input", 3)


class expansionPenaltyFunction(Function):
    @staticmethod
    def forward(ctx, xyz, primitive_size, alpha):
        _check_sizes(xyz, primitive_size)
        xyz = xyz.contiguous()
        B, n, _ = xyz.shape
        p = int(primitive_size)
        dev = xyz.device
        dist = torch.empty((B, n), dtype=torch.float32, device=dev)
        assignment = torch.empty((B, n), dtype=torch.int32, device=dev)
        mean_mst_length = torch.empty((B,), dtype=torch.float32, device=dev)
        prim_mean = torch.empty((B * (n // p),), dtype=torch.float32, device=dev)
        check(_lib.load().spgan_expansion_penalty_fwd(_p(xyz), B, n, p, float(alpha), _p(dist), _p(assignment), _p(mean_mst_length),
                                                      _p(prim_mean), _s()), "expansion_penalty_fwd", B=B, n=n, primitive_size=p)
        ctx.save_for_backward(xyz, assignment)
        ctx.mark_non_differentiable(assignment, mean_mst_length)
        return dist, assignment, mean_mst_length

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_dist, _grad_idx, _grad_mml):
        xyz, assignment = ctx.saved_tensors
        B, n, _ = xyz.shape
        grad_dist = _f32(grad_dist, "grad_dist", 2).contiguous()
        grad_xyz = torch.empty_like(xyz)
        check(_lib.load().spgan_expansion_penalty_bwd(_p(xyz), _p(grad_dist), _p(assignment), B, n, _p(grad_xyz), _s()),
              "expansion_penalty_bwd", B=B, n=n)
        return grad_xyz, None, None


class expansionPenaltyModule(nn.Module):
    """forward(input [B,n,3], primitive_size, alpha) -> (dist [B,n] float32, assignment [B,n] int32, mean_mst_length [B])."""

    def forward(self, input: Tensor, primitive_size: int, alpha: float):
        return expansionPenaltyFunction.apply(input, primitive_size, alpha)
