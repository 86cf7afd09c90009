"""Drop-in for the ball-query / grouping helpers of the reference
(Common/pointnet_util.py:19-143, Common/pointconv_util.py:60-197): same names, argument order and return
shapes/dtypes; HIP kernels underneath (libspgan_hip.so), GPU tensors only.  The index-producing ops carry no gradient (as in the
reference); the gathers -- index_points, group, sample_and_group -- are differentiable in `points` / `xyz` like the reference's torch
indexing (pointnet_util.py:43-60, pointconv_util.py:174-197), with a deterministic adjoint (per-point slot lists, no float atomics).

    square_distance(src, dst)                          [B,N,C],[B,M,C] -> [B,N,M]
    index_points(points, idx)                          [B,N,C],[B,S(,K)] -> [B,S(,K),C]
    farthest_point_sample(xyz, npoint, start=None)     -> int64 [B,npoint]   (start=None: random, like pointnet_util;
                                                          start=0-tensor: pointconv_util's variant)
    query_ball_point(radius, nsample, xyz, new_xyz)    -> int64 [B,S,nsample]
    knn_point(nsample, xyz, new_xyz)                   -> int64 [B,S,nsample]  (ascending; the reference's order is unspecified)
    group(nsample, xyz, points)                        -> (new_points [B,N,K,C+D], grouped_xyz_norm [B,N,K,C])
    sample_and_group(npoint, radius, nsample, xyz, points, returnfps=False, start=None)

PointNet++ modules (Common/pointnet_util.py:146-320; inputs / outputs channel-major [B,C,N] as there):

    sample_and_group_all(xyz, points)                  -> (zeros [B,1,3], [B,1,N,3+D])
    three_nn(xyz1, xyz2)                               -> (idx int64 [B,N,k], weight [B,N,k]), k = min(3,S); no gradient
    three_interpolate(points2, idx, weight)            [B,S,D] -> [B,N,D]; gradient to points2 only
    PointNetSetAbstraction(npoint, radius, nsample, in_channel, mlp, group_all)
    PointNetSetAbstractionMsg(npoint, radius_list, nsample_list, in_channel, mlp_list)
    PointNetFeaturePropagation(in_channel, mlp)
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib
from ._lib import check
from . import ops
from .ops import _f32, _p, _s

Tensor = torch.Tensor


def _xyz(t: Tensor, name: str) -> Tensor:
    _f32(t, name, 3)
    return t.contiguous()


def square_distance(src: Tensor, dst: Tensor) -> Tensor:
    src, dst = _xyz(src, "src"), _xyz(dst, "dst")
    B, N, C = src.shape
    M = dst.shape[1]
    out = torch.empty((B, N, M), dtype=torch.float32, device=src.device)
    check(_lib.load().spgan_square_distance(_p(src), _p(dst), B, N, M, C, _p(out), _s()), "square_distance", B=B, N=N, M=M, C=C)
    return out


def gather_csr(idx: Tensor, N: int):
    """Per point of each shape, the gather slots that read it: idx int64 [B, ...] (local indices) -> (rowptr int32 [B*N,2], src int32 [B*S])."""
    B = idx.shape[0]
    S = idx.numel() // B
    rowptr = torch.empty((B * N, 2), dtype=torch.int32, device=idx.device)
    src = torch.empty((B * S,), dtype=torch.int32, device=idx.device)
    bad = ops.index_check_flag(idx.device)
    check(_lib.load().spgan_gather_csr(_p(idx), B, S, N, _p(rowptr), _p(src), None if bad is None else _p(bad), _s()), "gather_csr", B=B, S=S, N=N)
    ops.index_check_raise(bad, "gather_csr: an index lies outside [0, %d)" % N)
    return rowptr, src


def _scatter_slots(dout2d: Tensor, col0: int, C: int, rowptr: Tensor, src: Tensor, shape) -> Tensor:
    out = torch.empty(shape, dtype=torch.float32, device=dout2d.device)
    check(_lib.load().spgan_scatter_slots(_p(dout2d), dout2d.shape[1], col0, C, _p(rowptr), _p(src), rowptr.shape[0], _p(out), _s()),
          "scatter_slots", ld=dout2d.shape[1], col0=col0, C=C)
    return out


def _index_points_raw(points: Tensor, idx: Tensor) -> Tensor:
    B, N, C = points.shape
    S = idx.numel() // B
    out = torch.empty(tuple(idx.shape) + (C,), dtype=torch.float32, device=points.device)
    check(_lib.load().spgan_index_points(_p(points), _p(idx), B, N, C, S, _p(out), _s()), "index_points", B=B, N=N, C=C, S=S)
    return out


class _IndexPointsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, idx):
        ctx.save_for_backward(idx)
        ctx.shape = tuple(points.shape)
        return _index_points_raw(points, idx)

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        B, N, C = ctx.shape
        rowptr, src = gather_csr(idx, N)
        return _scatter_slots(dout.contiguous().view(-1, C), 0, C, rowptr, src, ctx.shape), None


def index_points(points: Tensor, idx: Tensor) -> Tensor:
    points = _xyz(points, "points")
    if idx.dtype != torch.int64 or not idx.is_cuda:
        raise TypeError("idx must be an int64 GPU tensor")
    idx = idx.contiguous()
    if points.requires_grad and torch.is_grad_enabled():
        return _IndexPointsFn.apply(points, idx)
    return _index_points_raw(points, idx)


def farthest_point_sample(xyz: Tensor, npoint: int, start: Optional[Tensor] = None) -> Tensor:
    xyz = _xyz(xyz, "xyz")
    B, N, C = xyz.shape
    if C != 3:
        raise ValueError("farthest_point_sample expects xyz [B,N,3]")
    if start is None:
        start = torch.randint(0, N, (B,), dtype=torch.long, device=xyz.device)        # pointnet_util.py:75
    start = start.to(device=xyz.device, dtype=torch.long).contiguous()
    out = torch.empty((B, npoint), dtype=torch.int64, device=xyz.device)
    ws = torch.empty((B, N), dtype=torch.float32, device=xyz.device)
    check(_lib.load().spgan_farthest_point_sample(_p(xyz), B, N, npoint, _p(start), _p(out), _p(ws), _s()), "farthest_point_sample", B=B, N=N)
    return out


def ball_threshold(radius: float) -> float:
    """The float32 `thr` for which `d > thr` equals the reference's `sqrdists > radius ** 2` for every float32 d: torch casts the Python
    double radius ** 2 to the tensor's float32 (round to nearest) and compares there.  Formed from the double, never from a float32 radius."""
    return ctypes.c_float(float(radius) ** 2).value


def query_ball_point(radius: float, nsample: int, xyz: Tensor, new_xyz: Tensor) -> Tensor:
    """The first `nsample` points (ascending index) the reference's mask `sqrdists > radius ** 2` leaves in, padded with the first of them;
    an empty ball gives N in every slot (pointnet_util.py:87-107).  A point exactly on the threshold is inside.  nsample > N (where the
    reference raises an IndexError): still nsample columns, padded the same way."""
    xyz, new_xyz = _xyz(xyz, "xyz"), _xyz(new_xyz, "new_xyz")
    B, N, C = xyz.shape
    S = new_xyz.shape[1]
    out = torch.empty((B, S, nsample), dtype=torch.int64, device=xyz.device)
    check(_lib.load().spgan_query_ball_point(ball_threshold(radius), nsample, _p(xyz), _p(new_xyz), B, N, S, C, _p(out), _s()), "query_ball_point",
          B=B, N=N, S=S, C=C)
    return out


def knn_point(nsample: int, xyz: Tensor, new_xyz: Tensor) -> Tensor:
    xyz, new_xyz = _xyz(xyz, "xyz"), _xyz(new_xyz, "new_xyz")
    B, N, C = xyz.shape
    S = new_xyz.shape[1]
    out = torch.empty((B, S, nsample), dtype=torch.int64, device=xyz.device)
    check(_lib.load().spgan_knn_point(nsample, _p(xyz), _p(new_xyz), B, N, S, C, _p(out), _s()), "knn_point", B=B, N=N, S=S, C=C)
    return out


def _group_concat_raw(xyz: Tensor, center: Tensor, feat: Optional[Tensor], idx: Tensor) -> Tensor:
    B, N, C = xyz.shape
    S, K = idx.shape[1], idx.shape[2]
    D = 0 if feat is None else feat.shape[2]
    out = torch.empty((B, S, K, C + D), dtype=torch.float32, device=xyz.device)
    check(_lib.load().spgan_group_concat(_p(xyz), _p(center.contiguous()), _p(None if feat is None else feat.contiguous()), _p(idx.contiguous()),
                                         B, N, S, K, C, D, _p(out), _s()), "group_concat", B=B, N=N, S=S, K=K)
    return out


class _GroupConcatFn(torch.autograd.Function):
    """out[b,s,j,:] = [xyz[b,idx] - center[b,s] | feat[b,idx]] with gradients for xyz, center and feat."""

    @staticmethod
    def forward(ctx, xyz, center, feat, idx):
        ctx.save_for_backward(idx)
        ctx.shapes = (tuple(xyz.shape), tuple(center.shape), None if feat is None else tuple(feat.shape))
        return _group_concat_raw(xyz, center, feat, idx)

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        sx, sc, sf = ctx.shapes
        B, N, C = sx
        S, K = idx.shape[1], idx.shape[2]
        W = C + (0 if sf is None else sf[2])
        d2 = dout.contiguous().view(-1, W)
        dxyz = dcen = dfeat = None
        if ctx.needs_input_grad[0] or (sf is not None and ctx.needs_input_grad[2]):
            rowptr, src = gather_csr(idx, N)
            if ctx.needs_input_grad[0]:
                dxyz = _scatter_slots(d2, 0, C, rowptr, src, sx)
            if sf is not None and ctx.needs_input_grad[2]:
                dfeat = _scatter_slots(d2, C, sf[2], rowptr, src, sf)
        if ctx.needs_input_grad[1]:
            dcen = torch.empty(sc, dtype=torch.float32, device=dout.device)
            check(_lib.load().spgan_group_center_bwd(_p(d2), W, B * S, K, C, _p(dcen), _s()), "group_center_bwd", Q=B * S, K=K, C=C)
        return dxyz, dcen, dfeat, None


def _group_concat(xyz: Tensor, center: Tensor, feat: Optional[Tensor], idx: Tensor) -> Tensor:
    if torch.is_grad_enabled() and (xyz.requires_grad or center.requires_grad or (feat is not None and feat.requires_grad)):
        return _GroupConcatFn.apply(xyz, center.contiguous(), None if feat is None else feat.contiguous(), idx.contiguous())
    return _group_concat_raw(xyz, center, feat, idx)


def group(nsample: int, xyz: Tensor, points: Optional[Tensor]):
    """kNN-group every point around itself (pointconv_util.py:174-197)."""
    xyz = _xyz(xyz, "xyz")
    idx = knn_point(nsample, xyz.detach(), xyz.detach())
    C = xyz.shape[2]
    new_points = _group_concat(xyz, xyz, None if points is None else _xyz(points, "points"), idx)
    grouped_xyz_norm = new_points[..., :C].contiguous() if points is not None else new_points
    return new_points, grouped_xyz_norm


def sample_and_group(npoint: int, radius: float, nsample: int, xyz: Tensor, points: Optional[Tensor], returnfps: bool = False,
                     start: Optional[Tensor] = None):
    """FPS centres + ball query + centred grouping (pointnet_util.py:110-143)."""
    xyz = _xyz(xyz, "xyz")
    fps_idx = farthest_point_sample(xyz.detach(), npoint, start)
    new_xyz = index_points(xyz, fps_idx)
    idx = query_ball_point(radius, nsample, xyz.detach(), new_xyz.detach())
    new_points = _group_concat(xyz, new_xyz, None if points is None else _xyz(points, "points"), idx)
    if returnfps:
        return new_xyz, new_points, index_points(xyz, idx), fps_idx
    return new_xyz, new_points


# =============================================================================================
# PointNet++ set abstraction / feature propagation (Common/pointnet_util.py:146-320)
# =============================================================================================
# The modules below are the reference's: same constructor arguments, attribute names (mlp_convs / mlp_bns, conv_blocks.i.j / bn_blocks.i.j)
# and creation order, so the same seed gives the same initial parameters and a reference state_dict loads with strict=True.  The
# nn.Conv / nn.BatchNorm children are parameter containers only -- their forward is never called; the arithmetic is HIP:
#   rows [B*S*K, 3+D] (spgan_group_concat) -> per layer one GEMM whose epilogue yields the BatchNorm batch statistics, the previous
#   layer's BatchNorm + ReLU applied on the operand load (ops.gemm_nt, slope 0) -> spgan_group_max (BatchNorm + ReLU + max over K).
#   Backward: spgan_group_max_bwd -> ops.bn_bwd_apply / ops.gemm_tn / ops.gemm_nt_bnbwd per layer, as the Discriminator's generic path.
RELU = 0.0     # slope of the (leaky-)ReLU operand modes: F.relu (pointnet_util.py:203, 261, 319)
GROUP_MAX_K = 128     # spgan_group_max walks the K rows of a centre in one thread; longer groups (group_all: K = N) use ops.maxpool's row-parallel kernel


def sample_and_group_all(xyz: Tensor, points: Optional[Tensor]):
    """One group of all N points around the origin (pointnet_util.py:146-163): -> (new_xyz zeros [B,1,3], new_points [B,1,N,3+D])."""
    xyz = _xyz(xyz, "xyz")
    B, N, C = xyz.shape
    new_xyz = torch.zeros((B, 1, C), dtype=torch.float32, device=xyz.device)
    idx = torch.arange(N, dtype=torch.int64, device=xyz.device).view(1, 1, N).expand(B, 1, N).contiguous()
    return new_xyz, _group_concat(xyz, new_xyz, None if points is None else _xyz(points, "points"), idx)


def three_nn(xyz1: Tensor, xyz2: Tensor):
    """The k = min(3, S) nearest centres xyz2 [B,S,3] of every point xyz1 [B,N,3] (ascending) and their normalised inverse-distance
    weights (pointnet_util.py:301-307) -> (idx int64 [B,N,k], weight float32 [B,N,k]).  No gradient (three_nn of metrics/pointnet2_ops)."""
    xyz1, xyz2 = _xyz(xyz1.detach(), "xyz1"), _xyz(xyz2.detach(), "xyz2")
    B, N, C = xyz1.shape
    S = xyz2.shape[1]
    if C != 3 or xyz2.shape[2] != 3 or xyz2.shape[0] != B:
        raise ValueError("three_nn expects xyz1 [B,N,3] and xyz2 [B,S,3]")
    k = min(3, S)
    idx = torch.empty((B, N, k), dtype=torch.int64, device=xyz1.device)
    weight = torch.empty((B, N, k), dtype=torch.float32, device=xyz1.device)
    check(_lib.load().spgan_three_nn(_p(xyz1), _p(xyz2), B, N, S, _p(idx), _p(weight), _s()), "three_nn", B=B, N=N, S=S)
    return idx, weight


def _three_interpolate_into(points2: Tensor, idx: Tensor, weight: Tensor, out2d: Tensor, col0: int) -> None:
    """out2d[b*N+n, col0:col0+D] = sum_j weight[b,n,j] * points2[b, idx[b,n,j]]  (points2 [B,S,D] contiguous)."""
    B, S, D = points2.shape
    N, k = idx.shape[1], idx.shape[2]
    bad = ops.index_check_flag(points2.device)
    check(_lib.load().spgan_three_interpolate(_p(points2), _p(idx), _p(weight), B, N, S, D, k, _p(out2d), out2d.shape[1], col0,
                                              None if bad is None else _p(bad), _s()), "three_interpolate", B=B, N=N, S=S, D=D, k=k)
    ops.index_check_raise(bad, "three_interpolate: an index lies outside [0, %d)" % S)


def _three_interpolate_bwd(dout2d: Tensor, col0: int, D: int, idx: Tensor, weight: Tensor, S: int) -> Tensor:
    """-> dpoints2 [B,S,D]: per-centre slot lists (gather_csr), weighted, summed in slot order -- no float atomics."""
    B, N, k = idx.shape
    rowptr, src = gather_csr(idx.view(B, N * k), S)
    out = torch.empty((B, S, D), dtype=torch.float32, device=dout2d.device)
    check(_lib.load().spgan_three_interpolate_bwd(_p(dout2d), dout2d.shape[1], col0, D, _p(weight), k, _p(rowptr), _p(src), B * S, _p(out), _s()),
          "three_interpolate_bwd", B=B, N=N, S=S, D=D)
    return out


def _idx_weight(idx: Tensor, weight: Tensor):
    if idx.dtype != torch.int64 or not idx.is_cuda or idx.dim() != 3:
        raise TypeError("idx must be an int64 GPU tensor [B,N,k]")
    _f32(weight, "weight", 3)
    if weight.shape != idx.shape or idx.shape[2] > 3:
        raise ValueError("weight must match idx [B,N,k], k <= 3")
    return idx.contiguous(), weight.detach().contiguous()


class _ThreeInterpolateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points2, idx, weight):
        B, S, D = points2.shape
        ctx.save_for_backward(idx, weight)
        ctx.S = S
        out = torch.empty((B * idx.shape[1], D), dtype=torch.float32, device=points2.device)
        _three_interpolate_into(points2, idx, weight, out, 0)
        return out.view(B, idx.shape[1], D)

    @staticmethod
    def backward(ctx, dout):
        idx, weight = ctx.saved_tensors
        D = dout.shape[2]
        return _three_interpolate_bwd(dout.contiguous().view(-1, D), 0, D, idx, weight, ctx.S), None, None


def three_interpolate(points2: Tensor, idx: Tensor, weight: Tensor) -> Tensor:
    """[B,N,D] = sum_j weight[..., j] * points2[b, idx[..., j]] (pointnet_util.py:308); differentiable in points2 only."""
    points2 = _xyz(points2, "points2")
    idx, weight = _idx_weight(idx, weight)
    return _ThreeInterpolateFn.apply(points2, idx, weight)


def _cm_to_rows(x_cm: Tensor, rows: Tensor, col0: int) -> None:
    B, C, N = x_cm.shape
    check(_lib.load().spgan_cm_to_rows(_p(x_cm), B, C, N, _p(rows), rows.shape[1], col0, _s()), "cm_to_rows", B=B, C=C, N=N)


def _rows_to_cm(rows: Tensor, col0: int, B: int, C: int, N: int) -> Tensor:
    out = torch.empty((B, C, N), dtype=torch.float32, device=rows.device)
    check(_lib.load().spgan_rows_to_cm(_p(rows), rows.shape[1], col0, B, C, N, _p(out), _s()), "rows_to_cm", B=B, C=C, N=N)
    return out


class _CmToRowsFn(torch.autograd.Function):
    """[B,C,N] -> [B,N,C] (the reference's permute(0, 2, 1), materialised point-major for the kernels)."""

    @staticmethod
    def forward(ctx, x_cm):
        B, C, N = x_cm.shape
        rows = torch.empty((B * N, C), dtype=torch.float32, device=x_cm.device)
        _cm_to_rows(x_cm, rows, 0)
        return rows.view(B, N, C)

    @staticmethod
    def backward(ctx, g):
        B, N, C = g.shape
        return _rows_to_cm(g.contiguous().view(B * N, C), 0, B, C, N)


class _RowsToCmFn(torch.autograd.Function):
    """[B,N,C] -> [B,C,N]."""

    @staticmethod
    def forward(ctx, rows):
        B, N, C = rows.shape
        return _rows_to_cm(rows.contiguous().view(B * N, C), 0, B, C, N)

    @staticmethod
    def backward(ctx, g):
        B, C, N = g.shape
        rows = torch.empty((B * N, C), dtype=torch.float32, device=g.device)
        _cm_to_rows(g.contiguous(), rows, 0)
        return rows.view(B, N, C)


def _cm(t: Tensor, name: str) -> Tensor:
    _f32(t, name, 3)
    return t.contiguous()


def _group_max(y: Tensor, Q: int, K: int, scale: Tensor, shift: Tensor, slope: float):
    if K > GROUP_MAX_K:
        return ops.maxpool(y, Q, K, scale, shift, slope)
    Cn = y.shape[1]
    pooled = torch.empty((Q, Cn), dtype=torch.float32, device=y.device)
    arg = torch.empty((Q, Cn), dtype=torch.int32, device=y.device)
    check(_lib.load().spgan_group_max(_p(y), ops._ld(y), Q, K, Cn, _p(scale), _p(shift), float(slope), _p(pooled), _p(arg), _s()),
          "group_max", Q=Q, K=K, C=Cn)
    return pooled, arg


def _group_max_bwd(gpool: Tensor, pooled: Tensor, argmax: Optional[Tensor], y: Tensor, mean: Tensor, invstd: Tensor, slope: float, K: int):
    """-> (g [Q*K,C] dense gradient w.r.t. the BatchNorm output, sums [2C] = (sum g | sum g*xhat))."""
    Q, Cn = gpool.shape
    g = torch.empty((Q * K, Cn), dtype=torch.float32, device=gpool.device)
    gstat = torch.empty((Q, 2 * Cn), dtype=torch.float32, device=gpool.device)
    check(_lib.load().spgan_group_max_bwd(_p(gpool), _p(pooled), _p(argmax), _p(y), ops._ld(y), _p(mean), _p(invstd), float(slope), Q, K, Cn,
                                          _p(g), _p(gstat), _s()), "group_max_bwd", Q=Q, K=K, C=Cn)
    return g, ops.colsum(gstat)[0]


class _Holder:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class _SharedMLPFn(torch.autograd.Function):
    """rows a0 [Q*K, Cin] -> [Q, Cout]: (1x1 conv -> BatchNorm -> ReLU) per layer, then max over the K consecutive rows of a group
    (K = 1: the per-row activations).  inputs: holder(K, training, bns = the nn.BatchNorm modules[, slope: LeakyReLU(slope) instead of
    the ReLU][, keep_out=False (K = 1 only): the result is not saved but formed again in backward from the last pre-norm product, for a
    caller whose result would otherwise live only through this node]), a0, then (weight, bias, gamma, beta) per layer."""

    @staticmethod
    def forward(ctx, holder, a0, *params):
        K, training = holder.K, holder.training
        slope = float(getattr(holder, "slope", RELU))
        M = a0.shape[0]
        Q = M // K
        ys, bns = [], []
        a, pro = a0, None
        for li, bn in enumerate(holder.bns):
            W, b, gamma, beta = params[4 * li:4 * li + 4]
            W2 = W.view(W.shape[0], W.shape[1])
            if training:
                y, st = ops.gemm_nt(a, W2, b, bn=(gamma, beta, bn.running_mean, bn.running_var), pro=pro)
                bn.num_batches_tracked += 1
            else:
                y = ops.gemm_nt(a, W2, b, pro=pro)
                st = ops.bn_prepare(None, None, gamma, beta, M, False, bn.running_mean, bn.running_var)
            ys.append(y); bns.append(st)
            a, pro = y, (st[0], st[1], slope)
        sc, sh = bns[-1][0], bns[-1][1]
        if K == 1:
            out, arg = ops.affine_act(ys[-1], sc, sh, slope), None
        else:
            out, arg = _group_max(ys[-1], Q, K, sc, sh, slope)
        ctx.K, ctx.training, ctx.slope, ctx.L = K, training, slope, len(ys)
        keep_out = K > 1 or getattr(holder, "keep_out", True)
        # the pre-norm products and the statistics are saved tensors, not attributes: autograd drops them with this node's backward
        ctx.save_for_backward(a0, out if keep_out else None, arg, *params, *ys, *[t for st in bns for t in st])
        return out

    @staticmethod
    def backward(ctx, dout):
        a0, out, arg, *rest = ctx.saved_tensors
        K, slope, L = ctx.K, ctx.slope, ctx.L
        params, ys, flat = rest[:4 * L], rest[4 * L:5 * L], rest[5 * L:]
        bns = [flat[4 * li:4 * li + 4] for li in range(L)]
        M = a0.shape[0]
        grads = [None] * len(params)
        if out is None:
            out = ops.affine_act(ys[-1], bns[-1][0], bns[-1][1], slope)
        g, sums = _group_max_bwd(dout.contiguous(), out, arg, ys[-1], bns[-1][3], bns[-1][2], slope, K)
        da0 = None
        for li in range(L - 1, -1, -1):
            W, b, gamma, beta = [p.detach() for p in params[4 * li:4 * li + 4]]
            W2 = W.view(W.shape[0], W.shape[1])
            Cn = W2.shape[0]
            sc, sh, inv, mu = bns[li]
            grads[4 * li + 2], grads[4 * li + 3] = sums[Cn:].clone(), sums[:Cn].clone()
            if ctx.training:
                dy = ops.bn_bwd_apply(g, ys[li], mu, inv, gamma, sums, M)
                grads[4 * li + 1] = torch.zeros_like(b)            # a bias in front of a train-mode BatchNorm: exactly zero gradient
            else:
                dy = ops.bn_bwd_apply(g, ys[li], mu, inv, gamma, torch.zeros_like(sums), M)
                grads[4 * li + 1] = ops.colsum(dy)[0]
            if li > 0:
                psc, psh, pinv, pmu = bns[li - 1]
                grads[4 * li] = ops.gemm_tn(dy, ys[li - 1], pro=(psc, psh, slope)).view_as(W)
                g, s0, s1 = ops.gemm_nt_bnbwd(dy, W2.t().contiguous(), ys[li - 1], psc, psh, pmu, pinv, slope)
                sums = torch.cat([s0, s1])
            else:
                grads[0] = ops.gemm_tn(dy, a0).view_as(W)
                if ctx.training and W2.shape[1] == 1:
                    grads[0] = _one_column_wgrad(grads[0], W, gamma, sums[Cn:], inv)
                if ctx.needs_input_grad[1]:
                    da0 = ops.gemm_nt(dy, W2.t().contiguous())
        return (None, da0) + tuple(g_ if need else None for g_, need in zip(grads, ctx.needs_input_grad[2:]))


def _one_column_wgrad(plain: Tensor, W: Tensor, gamma: Tensor, s1: Tensor, invstd: Tensor) -> Tensor:
    """Weight gradient of a layer with ONE input column in front of a train-mode BatchNorm (PointConv's DensityNet).  y = w*s + b is
    normalised, so the output does not depend on |w| and sum_r dy_r*s_r cancels down to a residue of order eps: with
    dy = gamma*invstd*(g - mean g - xhat*mean(g*xhat)) and s - mean s = (y - mean y)/w,
        dW = (gamma/w) * S1 * (1 - var*invstd^2) = gamma * S1 * eps * invstd^2 / w,      S1 = sum_r g_r*xhat_r (the BatchNorm weight's gradient).
    The product form has no cancellation; the row sum (`plain`) is kept where w == 0, where the identity does not apply."""
    w = W.view(-1)
    closed = gamma * s1 * (ops.BN_EPS * invstd * invstd) / torch.where(w != 0, w, torch.ones_like(w))
    return torch.where(w != 0, closed, plain.view(-1)).view_as(W)


def _mlp_params(convs, bns):
    out = []
    for conv, bn in zip(convs, bns):
        out += [conv.weight, conv.bias, bn.weight, bn.bias]
    return out


def _shared_mlp(rows: Tensor, K: int, convs, bns, training: bool, first_weight: Optional[Tensor] = None) -> Tensor:
    params = _mlp_params(convs, bns)
    if first_weight is not None:
        params[0] = first_weight
    return _SharedMLPFn.apply(_Holder(K=K, training=training, bns=list(bns)), rows, *params)


class PointNetSetAbstraction(torch.nn.Module):
    """pointnet_util.py:166-207.  forward(xyz [B,3,N], points [B,D,N] | None, start=None) -> (new_xyz [B,3,S], new_points [B,mlp[-1],S]);
    start = the FPS start indices [B] (the reference draws them with torch.randint; None does the same)."""

    def __init__(self, npoint, radius, nsample, in_channel, mlp, group_all):
        super().__init__()
        self.npoint, self.radius, self.nsample = npoint, radius, nsample
        self.mlp_convs = torch.nn.ModuleList()
        self.mlp_bns = torch.nn.ModuleList()
        last_channel = in_channel
        for out_channel in mlp:
            self.mlp_convs.append(torch.nn.Conv2d(last_channel, out_channel, 1))
            self.mlp_bns.append(torch.nn.BatchNorm2d(out_channel))
            last_channel = out_channel
        self.group_all = group_all

    def forward(self, xyz: Tensor, points: Optional[Tensor], start: Optional[Tensor] = None):
        xyz_pm = _CmToRowsFn.apply(_cm(xyz, "xyz"))
        pts_pm = None if points is None else _CmToRowsFn.apply(_cm(points, "points"))
        if self.group_all:
            new_xyz, new_points = sample_and_group_all(xyz_pm, pts_pm)
        else:
            new_xyz, new_points = sample_and_group(self.npoint, self.radius, self.nsample, xyz_pm, pts_pm, start=start)
        B, S, K, Cin = new_points.shape
        out = _shared_mlp(new_points.view(B * S * K, Cin), K, self.mlp_convs, self.mlp_bns, self.training)
        return _RowsToCmFn.apply(new_xyz), _RowsToCmFn.apply(out.view(B, S, -1))


class PointNetSetAbstractionMsg(torch.nn.Module):
    """pointnet_util.py:210-267 (multi-scale grouping: one shared MLP per radius, outputs concatenated over channels)."""

    def __init__(self, npoint, radius_list, nsample_list, in_channel, mlp_list):
        super().__init__()
        self.npoint, self.radius_list, self.nsample_list = npoint, radius_list, nsample_list
        self.conv_blocks = torch.nn.ModuleList()
        self.bn_blocks = torch.nn.ModuleList()
        for i in range(len(mlp_list)):
            convs = torch.nn.ModuleList()
            bns = torch.nn.ModuleList()
            last_channel = in_channel + 3
            for out_channel in mlp_list[i]:
                convs.append(torch.nn.Conv2d(last_channel, out_channel, 1))
                bns.append(torch.nn.BatchNorm2d(out_channel))
                last_channel = out_channel
            self.conv_blocks.append(convs)
            self.bn_blocks.append(bns)

    def forward(self, xyz: Tensor, points: Optional[Tensor], start: Optional[Tensor] = None):
        xyz_pm = _CmToRowsFn.apply(_cm(xyz, "xyz"))
        pts_pm = None if points is None else _CmToRowsFn.apply(_cm(points, "points"))
        B, N, C = xyz_pm.shape
        S = self.npoint
        fps_idx = farthest_point_sample(xyz_pm.detach(), S, start)
        new_xyz = index_points(xyz_pm, fps_idx)
        outs = []
        for i, radius in enumerate(self.radius_list):
            K = self.nsample_list[i]
            idx = query_ball_point(radius, K, xyz_pm.detach(), new_xyz.detach())
            rows = _group_concat(xyz_pm, new_xyz, pts_pm, idx).view(B * S * K, -1)        # [xyz - centre | features]
            w0 = self.conv_blocks[i][0].weight
            if pts_pm is not None:
                # the reference concatenates [features | xyz - centre] (:253): the same product with the weight's input columns rotated
                D = pts_pm.shape[2]
                w0 = torch.cat([w0[:, D:], w0[:, :D]], dim=1)
            out = _shared_mlp(rows, K, self.conv_blocks[i], self.bn_blocks[i], self.training, first_weight=w0)
            outs.append(_RowsToCmFn.apply(out.view(B, S, -1)))
        return _RowsToCmFn.apply(new_xyz), torch.cat(outs, dim=1)


class _PropagateInputFn(torch.autograd.Function):
    """rows [B*N, D1+D2] = [points1 | three_interpolate(points2)] (pointnet_util.py:298-314) written into ONE buffer (no torch.cat)."""

    @staticmethod
    def forward(ctx, points1, points2, idx, weight):
        B, D2, S = points2.shape
        N = idx.shape[1]
        D1 = 0 if points1 is None else points1.shape[1]
        rows = torch.empty((B * N, D1 + D2), dtype=torch.float32, device=points2.device)
        if points1 is not None:
            _cm_to_rows(points1, rows, 0)
        p2 = torch.empty((B * S, D2), dtype=torch.float32, device=points2.device)
        _cm_to_rows(points2, p2, 0)
        _three_interpolate_into(p2.view(B, S, D2), idx, weight, rows, D1)
        ctx.save_for_backward(idx, weight)
        ctx.dims = (B, N, S, D1, D2)
        return rows

    @staticmethod
    def backward(ctx, drows):
        idx, weight = ctx.saved_tensors
        B, N, S, D1, D2 = ctx.dims
        drows = drows.contiguous()
        d1 = d2 = None
        if D1 and ctx.needs_input_grad[0]:
            d1 = _rows_to_cm(drows, 0, B, D1, N)
        if ctx.needs_input_grad[1]:
            dp2 = _three_interpolate_bwd(drows, D1, D2, idx, weight, S)
            d2 = _rows_to_cm(dp2.view(B * S, D2), 0, B, D2, S)
        return d1, d2, None, None


class PointNetFeaturePropagation(torch.nn.Module):
    """pointnet_util.py:270-320.  forward(xyz1 [B,3,N], xyz2 [B,3,S], points1 [B,D1,N] | None, points2 [B,D2,S]) -> [B,mlp[-1],N].
    The interpolation weights carry no gradient to xyz1 / xyz2 (three_nn is not differentiable in metrics/pointnet2_ops either)."""

    def __init__(self, in_channel, mlp):
        super().__init__()
        self.mlp_convs = torch.nn.ModuleList()
        self.mlp_bns = torch.nn.ModuleList()
        last_channel = in_channel
        for out_channel in mlp:
            self.mlp_convs.append(torch.nn.Conv1d(last_channel, out_channel, 1))
            self.mlp_bns.append(torch.nn.BatchNorm1d(out_channel))
            last_channel = out_channel

    def forward(self, xyz1: Tensor, xyz2: Tensor, points1: Optional[Tensor], points2: Tensor) -> Tensor:
        if torch.is_grad_enabled() and (xyz1.requires_grad or xyz2.requires_grad):
            raise NotImplementedError(
                "PointNetFeaturePropagation: no gradient to xyz1 / xyz2.  The interpolation weights are produced by three_nn, which is "
                "non-differentiable (as in metrics/pointnet2_ops); the pure-torch reference differentiates them with a 1/(d+1e-8)^2 "
                "factor that is ~1e16 on coincident points.  Pass xyz1.detach() / xyz2.detach().")
        xyz1, xyz2, points2 = _cm(xyz1, "xyz1"), _cm(xyz2, "xyz2"), _cm(points2, "points2")
        if points1 is not None:
            points1 = _cm(points1, "points1")
        B, _, N = xyz1.shape
        S = xyz2.shape[2]
        if S == 1:
            # the reference's repeat branch (:298-299): every point takes the single centre's features
            idx = torch.zeros((B, N, 1), dtype=torch.int64, device=xyz1.device)
            weight = torch.ones((B, N, 1), dtype=torch.float32, device=xyz1.device)
        else:
            idx, weight = three_nn(_CmToRowsFn.apply(xyz1), _CmToRowsFn.apply(xyz2))
        rows = _PropagateInputFn.apply(points1, points2, idx, weight)
        out = _shared_mlp(rows, 1, self.mlp_convs, self.mlp_bns, self.training)
        return _RowsToCmFn.apply(out.view(B, N, -1))
