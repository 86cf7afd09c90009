"""The approxmatch earth mover's distance over the HIP kernels of csrc/approxmatch.hip: the soft multi-level transport plan of Fan, Su
and Guibas that PointFlow's `StructuralLosses.match_cost` and PU-Net's `tf_approxmatch` compute, and on which the published MMD-EMD /
COV-EMD / 1-NNA-EMD tables rest.  Neither extension is part of the reference tree; the algorithm is stated in include/spgan_hip.h.

    from spgan.approxmatch import match_cost, approx_match, match_cost_dense, emd_approx_match, MatchCostFunction

    match_cost(seta [B,n,3], setb [B,m,3]) -> [B]           StructuralLosses.match_cost's signature; differentiable in both clouds
    approx_match(xyz1, xyz2) -> match [B,m,n]               tf_approxmatch.approx_match: the dense plan, entry [b,l,k]; opt-in
    match_cost_dense(xyz1, xyz2, match) -> [B]              tf_approxmatch.match_cost: the cost of a caller's dense plan
    emd_approx_match(sample, ref) -> [B]                    evaluation_metrics.py:26-35: match_cost / N

match_cost never forms the [n,m] plan: the forward keeps ten per-point ratios per cloud (10 (n + m) floats per pair) and the backward
recomputes the plan's entries from them.  The plan is a constant in the backward pass, as in both original extensions: the gradients
are those of sum match * |xyz1 - xyz2| with match fixed, not finite differences of the cost.  Once differentiable.  Nothing here
synchronises with the host, so forward and backward run inside spgan.CapturedBody; results repeat bit for bit.  Distances and exp
are float32; what is left of every point's mass, the ratios of the level in flight and all sums are float64.

The larger of n, m must be a multiple of the smaller (the originals compute the ratio in integer arithmetic).  An `xyz1` whose batch
stride is 0 (`cloud[None].expand(B, n, 3)`) is read in place: one sample against B references without a copy.

Importing this module does not load the shared library or touch the GPU.
"""
from __future__ import annotations

from typing import Tuple

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib

Tensor = torch.Tensor
LEVELS = 10                  # j = 7 .. -2 (spgan_approxmatch_levels)
MAX_BATCH = 65535            # pairs per launch sequence; the drivers chunk above it
# waves that share a block's 64 stationary points: 4 (the default) or 1 (the alternative that lost, profiles/approxmatch_bench.json)
SWEEP_WAVES = 4


def _p(t):
    return None if t is None else t.data_ptr()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _cloud(t, name: str) -> Tensor:
    """Shape and dtype (on any device); the device is checked last, by _pair."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("%s must be [B, N, 3] with B, N >= 1, got %s" % (name, tuple(t.shape)))
    if t.dtype != torch.float32:
        raise ValueError("%s must be float32, got %s" % (name, t.dtype))
    return t


def _batch_stride(a: Tensor) -> int:
    """xyz1's batch stride in floats as the kernels take it: 0 for one cloud expanded over the batch, else n * 3 (after .contiguous())."""
    n = a.shape[1]
    if a.shape[0] > 1 and a.stride(0) == 0 and a.stride(2) == 1 and (n == 1 or a.stride(1) == 3):
        return 0
    return n * 3


def _pair(xyz1, xyz2) -> Tuple[Tensor, Tensor, int]:
    """Validated (xyz1, xyz2, stride1): xyz2 contiguous; xyz1 contiguous, or left in place with a batch stride of 0."""
    a, b = _cloud(xyz1, "xyz1"), _cloud(xyz2, "xyz2")
    if a.shape[0] != b.shape[0]:
        raise ValueError("batch sizes differ: %d and %d" % (a.shape[0], b.shape[0]))
    n, m = a.shape[1], b.shape[1]
    if max(n, m) % min(n, m) != 0:
        raise ValueError("the larger point count must be a multiple of the smaller, got n = %d, m = %d" % (n, m))
    if a.shape[0] > MAX_BATCH:
        raise ValueError("at most %d pairs per call, got %d" % (MAX_BATCH, a.shape[0]))
    for t, name in ((a, "xyz1"), (b, "xyz2")):
        if not t.is_cuda:
            raise ValueError("%s must live on the GPU (spgan has no CPU path); got device %s" % (name, t.device))
    if a.device != b.device:
        raise ValueError("the two clouds live on different devices: %s and %s" % (a.device, b.device))
    stride1 = _batch_stride(a)
    return (a if stride1 == 0 else a.contiguous()), b.contiguous(), stride1


def _status(st: int, what: str, **shapes):
    if st == -22:
        raise ValueError("%s refused its sizes: %s" % (what, ", ".join("%s=%s" % kv for kv in shapes.items())))
    _lib.check(st, what, **shapes)


def _forward(a: Tensor, b: Tensor, stride1: int):
    """-> (cost [B], ratioL [B,10,n], ratioR [B,10,m])."""
    B, n, _ = a.shape
    m = b.shape[1]
    lib = _lib.load()
    cost = torch.empty((B,), dtype=torch.float32, device=b.device)
    ratio_l = torch.empty((B, LEVELS, n), dtype=torch.float32, device=b.device)
    ratio_r = torch.empty((B, LEVELS, m), dtype=torch.float32, device=b.device)
    wsb = lib.spgan_approxmatch_ws_bytes(B, n, m)
    ws = torch.empty((wsb // 8,), dtype=torch.float64, device=b.device)
    _status(lib.spgan_approxmatch_fwd(_p(a), stride1, _p(b), B, n, m, SWEEP_WAVES, _p(cost), _p(ratio_l), _p(ratio_r), _p(ws), wsb, _s()),
            "approxmatch_fwd", B=B, n=n, m=m)
    return cost, ratio_l, ratio_r


class MatchCostFunction(Function):
    """forward(xyz1 [B,n,3], xyz2 [B,m,3]) -> cost [B]; backward -> (grad_xyz1, grad_xyz2) with the plan held constant."""

    @staticmethod
    def forward(ctx, xyz1, xyz2):
        a, b, stride1 = _pair(xyz1, xyz2)
        cost, ratio_l, ratio_r = _forward(a, b, stride1)
        ctx.save_for_backward(a, b, ratio_l, ratio_r)
        ctx.stride1 = stride1
        return cost

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_cost):
        a, b, ratio_l, ratio_r = ctx.saved_tensors
        B, n, _ = a.shape
        m = b.shape[1]
        g = grad_cost.to(torch.float32).contiguous()
        g1 = torch.empty((B, n, 3), dtype=torch.float32, device=b.device) if ctx.needs_input_grad[0] else None
        g2 = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        if g1 is not None or g2 is not None:
            _status(_lib.load().spgan_approxmatch_bwd(_p(a), ctx.stride1, _p(b), B, n, m, _p(ratio_l), _p(ratio_r), _p(g), _p(g1), _p(g2), _s()),
                    "approxmatch_bwd", B=B, n=n, m=m)
        return g1, g2


def match_cost(seta: Tensor, setb: Tensor) -> Tensor:
    """[B]: sum over the plan of match(k,l) * |seta[k] - setb[l]| (StructuralLosses.match_cost); fused, differentiable in both clouds."""
    return MatchCostFunction.apply(seta, setb)


def approx_match_records(xyz1: Tensor, xyz2: Tensor):
    """-> (cost [B], ratioL [B,10,n], ratioR [B,10,m]): what the fused forward keeps (no gradient)."""
    a, b, stride1 = _pair(xyz1, xyz2)
    with torch.no_grad():
        return _forward(a.detach(), b.detach(), stride1)


def approx_match(xyz1: Tensor, xyz2: Tensor) -> Tensor:
    """match [B,m,n], entry [b,l,k] = the mass moved from xyz1[b,k] to xyz2[b,l] (tf_approxmatch.approx_match's layout).  Not
    differentiable, as there.  This is the route that pays for the plan's memory: 4 n m bytes per pair."""
    a, b, stride1 = _pair(xyz1, xyz2)
    a, b = a.detach(), b.detach()
    B, n, _ = a.shape
    m = b.shape[1]
    if m > 65535:
        raise ValueError("approx_match writes plans of at most 65535 columns, got m = %d" % m)
    _, ratio_l, ratio_r = _forward(a, b, stride1)
    match = torch.empty((B, m, n), dtype=torch.float32, device=b.device)
    _status(_lib.load().spgan_approxmatch_plan(_p(a), stride1, _p(b), B, n, m, _p(ratio_l), _p(ratio_r), _p(match), _s()),
            "approxmatch_plan", B=B, n=n, m=m)
    return match


class _MatchCostDense(Function):
    @staticmethod
    def forward(ctx, xyz1, xyz2, match):
        a, b, _ = _pair(xyz1, xyz2)
        a = a.contiguous()
        B, n, _ = a.shape
        m = b.shape[1]
        if not isinstance(match, torch.Tensor) or tuple(match.shape) != (B, m, n):
            raise ValueError("match must be [B, m, n] = %s, got %s" % ((B, m, n), tuple(getattr(match, "shape", ()))))
        if match.dtype != torch.float32 or match.device != b.device:
            raise ValueError("match must be float32 on the clouds' device, got %s on %s" % (match.dtype, match.device))
        match = match.detach().contiguous()
        lib = _lib.load()
        cost = torch.empty((B,), dtype=torch.float32, device=b.device)
        ws = torch.empty((B * m,), dtype=torch.float64, device=b.device)
        _status(lib.spgan_match_cost_dense_fwd(_p(a), _p(b), _p(match), B, n, m, _p(cost), _p(ws), B * m * 8, _s()), "match_cost_dense_fwd",
                B=B, n=n, m=m)
        ctx.save_for_backward(a, b, match)
        return cost

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_cost):
        a, b, match = ctx.saved_tensors
        B, n, _ = a.shape
        m = b.shape[1]
        g = grad_cost.to(torch.float32).contiguous()
        g1 = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        g2 = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        if g1 is not None or g2 is not None:
            _status(_lib.load().spgan_match_cost_dense_bwd(_p(a), _p(b), _p(match), B, n, m, _p(g), _p(g1), _p(g2), _s()),
                    "match_cost_dense_bwd", B=B, n=n, m=m)
        return g1, g2, None


def match_cost_dense(xyz1: Tensor, xyz2: Tensor, match: Tensor) -> Tensor:
    """[B]: sum match[b,l,k] * |xyz1[b,k] - xyz2[b,l]| for a caller's dense plan (tf_approxmatch.match_cost); differentiable in the two
    clouds, not in the plan."""
    return _MatchCostDense.apply(xyz1, xyz2, match)


def emd_approx_match(sample: Tensor, ref: Tensor) -> Tensor:
    """evaluation_metrics.py:26-35: match_cost(sample, ref) / N, [B]; the two clouds must have the same point count."""
    _cloud(sample, "sample"), _cloud(ref, "ref")
    if sample.shape[1] != ref.shape[1]:
        raise ValueError("emd_approx is defined for equal point counts only, got %d and %d" % (sample.shape[1], ref.shape[1]))
    return match_cost(sample, ref) / float(sample.shape[1])


__all__ = ["MatchCostFunction", "match_cost", "approx_match", "approx_match_records", "match_cost_dense", "emd_approx_match"]
