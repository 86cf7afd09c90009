"""Tensor-level wrappers of the weighted full-rank edge convolution's launchers (csrc/edge_rank.hip; include/spgan_hip.h): the passes behind
`spgan.deform_edgeConv_feat` (functions.WeightedRankEdgeConvFn).  PQ, idx, scale1 / shift1 and W2i as in spgan.edge_rank; the per-edge weight
s(i,r,c) is the softmax over the k ranks of a3 = lrelu(scale3*z3 + shift3) with z3 [M*k, F1] the stored pre-norm output of the weight MLP
and norm = (wmax, wrs) [M,F1] x 2 its per-(point, channel) normaliser (edge_weight_norm); norm=None: s = a3 (softmax=False).
h, s and h*s exist only inside the kernels.  Exact fp32 MFMA products, as spgan.edge_rank."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import check
from .edge_rank import K_MAX, SLOPE, _graph, tile_points
from .ops import _f32, _i32, _ld, _p, _rowmajor2d, _s, _vec

Tensor = torch.Tensor
Norm = Optional[Tuple[Tensor, Tensor]]


def _mod(z3: Tensor, M_: int, k: int, F1: int, scale3: Tensor, shift3: Tensor, norm: Norm):
    """-> the five modulation pointers (z3, scale3, shift3, wmax | None, wrs | None), validated against [M,k,F1]"""
    _f32(z3, "z3")
    if not z3.is_contiguous() or z3.numel() != M_ * k * F1:
        raise ValueError("z3 must be contiguous [M*k, F1] = [%d, %d], got %s" % (M_ * k, F1, tuple(z3.shape)))
    wmax = wrs = None
    if norm is not None:
        wmax, wrs = norm
        for t, n in ((wmax, "wmax"), (wrs, "wrs")):
            _f32(t, n, 2)
            if tuple(t.shape) != (M_, F1) or not t.is_contiguous():
                raise ValueError("%s must be contiguous [M,F1] = [%d, %d], got %s" % (n, M_, F1, tuple(t.shape)))
    return _p(z3), _p(_vec(scale3, F1, "scale3")), _p(_vec(shift3, F1, "shift3")), _p(wmax), _p(wrs)


def edge_weight_gather(PQ: Tensor, idx: Tensor) -> Tensor:
    """z [M*k, F] = Q_i + P_idx[i,r], row i*k + r: the pre-norm rows of a narrow edge layer (the weight MLP's first, F = 16)"""
    M_, k, F_ = _graph(PQ, idx)
    z = torch.empty((M_ * k, F_), dtype=torch.float32, device=PQ.device)
    check(_lib.load().spgan_edge_weight_gather(_p(PQ), 2 * F_, _p(idx), M_, k, F_, _p(z), _s()), "edge_weight_gather", M=M_, k=k, F=F_)
    return z


def edge_weight_norm(z3: Tensor, k: int, scale3: Tensor, shift3: Tensor, slope: float = SLOPE) -> Tuple[Tensor, Tensor]:
    """z3 [M*k, F1] -> (wmax, wrs) [M,F1]: max over the k ranks of a3 and 1 / sum_r exp(a3 - wmax)"""
    _f32(z3, "z3", 2)
    if not 1 <= k <= K_MAX or z3.shape[0] % k or not z3.is_contiguous() or z3.shape[0] < k:
        raise ValueError("edge_weight_norm: z3 must be contiguous [M*k, F1] with 1 <= k <= %d, got %s and k=%d" % (K_MAX, tuple(z3.shape), k))
    M_, F1 = z3.shape[0] // k, z3.shape[1]
    out = torch.empty((2, M_, F1), dtype=torch.float32, device=z3.device)
    check(_lib.load().spgan_edge_weight_norm(_p(z3), M_, k, F1, _p(_vec(scale3, F1, "scale3")), _p(_vec(shift3, F1, "shift3")), float(slope),
                                             _p(out[0]), _p(out[1]), _s()), "edge_weight_norm", M=M_, k=k, F1=F1)
    return out[0], out[1]


def edge_weight_gemm(PQ: Tensor, idx: Tensor, scale1: Tensor, shift1: Tensor, z3: Tensor, scale3: Tensor, shift3: Tensor, norm: Norm, W2i: Tensor,
                     b2: Optional[Tensor] = None, stats: bool = False, slope: float = SLOPE):
    """y [M,O] = b2 + (h*s).flat @ W2i^T   (-> (y, partials, tile_rows) with stats=True, as edge_rank.edge_rank_gemm)"""
    M_, k, F1 = _graph(PQ, idx)
    _rowmajor2d(W2i, "W2i")
    if W2i.shape[1] != k * F1 or W2i.shape[0] < 1:
        raise ValueError("W2i must be [O, k*F1] = [O, %d] (k=%d, F1=%d), got %s" % (k * F1, k, F1, tuple(W2i.shape)))
    O = W2i.shape[0]
    md = _mod(z3, M_, k, F1, scale3, shift3, norm)
    y = torch.empty((M_, O), dtype=torch.float32, device=PQ.device)
    part, tp = None, 0
    if stats:
        tp = tile_points(k)
        part = torch.empty(((M_ + tp - 1) // tp, O, 2), dtype=torch.float32, device=PQ.device)
    check(_lib.load().spgan_edge_weight_gemm(_p(PQ), 2 * F1, _p(idx), M_, k, F1, _p(_vec(scale1, F1, "scale1")), _p(_vec(shift1, F1, "shift1")),
                                             float(slope), *md, _p(W2i), _ld(W2i), _p(_vec(b2, O, "b2")), O, _p(y), O, _p(part), _s()),
          "edge_weight_gemm", M=M_, k=k, F1=F1, O=O)
    return (y, part, tp) if stats else y


def edge_weight_wgrad(PQ: Tensor, idx: Tensor, scale1: Tensor, shift1: Tensor, z3: Tensor, scale3: Tensor, shift3: Tensor, norm: Norm, dy: Tensor,
                      slope: float = SLOPE) -> Tensor:
    """dW2i [O, k*F1] = dy^T @ (h*s).flat"""
    M_, k, F1 = _graph(PQ, idx)
    _rowmajor2d(dy, "dy")
    if dy.shape[0] != M_:
        raise ValueError("dy must have M = %d rows" % M_)
    O = dy.shape[1]
    md = _mod(z3, M_, k, F1, scale3, shift3, norm)
    lib = _lib.load()
    wsb = lib.spgan_edge_rank_wgrad_ws_bytes(M_, k, F1, O)
    if wsb == 0:
        raise ValueError("edge_weight_wgrad: unsupported sizes M=%d k=%d F1=%d O=%d" % (M_, k, F1, O))
    ws = torch.empty((wsb // 4,), dtype=torch.float32, device=PQ.device)
    dW = torch.empty((O, k * F1), dtype=torch.float32, device=PQ.device)
    check(lib.spgan_edge_weight_wgrad(_p(PQ), 2 * F1, _p(idx), M_, k, F1, _p(_vec(scale1, F1, "scale1")), _p(_vec(shift1, F1, "shift1")), float(slope),
                                      *md, _p(dy), _ld(dy), O, _p(dW), k * F1, _p(ws), wsb, _s()), "edge_weight_wgrad", M=M_, k=k, F1=F1, O=O)
    return dW


def edge_weight_dgrad(dy: Tensor, W2t: Tensor, PQ: Tensor, idx: Tensor, scale1: Tensor, shift1: Tensor, mean1: Tensor, invstd1: Tensor, z3: Tensor,
                      scale3: Tensor, shift3: Tensor, mean3: Tensor, invstd3: Tensor, norm: Norm, slope: float = SLOPE):
    """-> (du [M,k,F1], sums_u [2*F1] = [sum du | sum du*uhat], g3 [M*k, F1], sums_3 [2*F1] = [sum g3 | sum g3*z3hat]): the gradients
    reaching the pre-activation BatchNorm outputs of the h branch and of the weight MLP's last layer -- the two per-edge buffers of the
    backward.  W2t [k*F1, O] = W2i transposed."""
    M_, k, F1 = _graph(PQ, idx)
    _rowmajor2d(dy, "dy"); _rowmajor2d(W2t, "W2t")
    O = dy.shape[1]
    if dy.shape[0] != M_ or tuple(W2t.shape) != (k * F1, O):
        raise ValueError("dy must be [M,O] and W2t [k*F1, O] = [%d, %d], got %s and %s" % (k * F1, O, tuple(dy.shape), tuple(W2t.shape)))
    md = _mod(z3, M_, k, F1, scale3, shift3, norm)
    lib = _lib.load()
    tp = tile_points(k)
    tiles = (M_ + tp - 1) // tp
    du = torch.empty((M_, k, F1), dtype=torch.float32, device=PQ.device)
    g3 = torch.empty((M_ * k, F1), dtype=torch.float32, device=PQ.device)
    part = torch.empty((2, tiles, F1, 2), dtype=torch.float32, device=PQ.device)
    check(lib.spgan_edge_weight_dgrad(_p(dy), _ld(dy), _p(W2t), _ld(W2t), _p(PQ), 2 * F1, _p(idx), M_, k, F1, O, _p(_vec(scale1, F1, "scale1")),
                                      _p(_vec(shift1, F1, "shift1")), _p(_vec(mean1, F1, "mean1")), _p(_vec(invstd1, F1, "invstd1")), float(slope),
                                      md[0], md[1], md[2], _p(_vec(mean3, F1, "mean3")), _p(_vec(invstd3, F1, "invstd3")), md[3], md[4],
                                      _p(du), _p(g3), _p(part[0]), _p(part[1]), _s()), "edge_weight_dgrad", M=M_, k=k, F1=F1, O=O)
    sums = torch.empty((2, 2, F1), dtype=torch.float32, device=PQ.device)
    for j in range(2):
        check(lib.spgan_colstats_finalize(_p(part[j]), 1, tiles, F1, M_, 1, tp, _p(sums[j, 0]), _p(sums[j, 1]), _s()), "colstats_finalize")
    return du, sums[0].view(-1), g3, sums[1].view(-1)
