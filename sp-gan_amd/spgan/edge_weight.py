"""Tensor-level wrappers of the weighted full-rank edge convolution's launchers (csrc/edge_rank.hip; include/spgan_hip.h): the passes behind
`spgan.deform_edgeConv_feat` (edge_conv.WeightedRankEdgeConvFn) and, with the two-branch passes at the end, `spgan.deform_edgeConv`
(edge_conv.CoordRankEdgeConvFn); the stored-operand forms at the end serve `spgan.bilateral_upsample_edgeConv`
(edge_conv.BilateralUpsampleEdgeConvFn).  PQ, idx, scale1 / shift1 and W2i as in spgan.edge_rank; the per-edge weight
s(i,r,c) is the softmax over the k ranks of a3 = lrelu(scale3*z3 + shift3) with z3 [M*k, F1] the stored pre-norm output of the weight MLP
and norm = (wmax, wrs) [M,F1] x 2 its per-(point, channel) normaliser (edge_weight_norm); norm=None: s = a3 (softmax=False).
h, s and h*s exist only inside the kernels.  Exact fp32 MFMA products, as spgan.edge_rank."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import check
from .edge_max import tile_sums
from .edge_rank import K_MAX, SLOPE, Norm, _dgrad_sizes, _graph, _mod, edge_rank_gemm, edge_rank_wgrad, tile_points
from .ops import _f32, _ld, _p, _rowmajor2d, _s, _vec

Tensor = torch.Tensor


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
    return edge_rank_gemm(PQ, idx, scale1, shift1, W2i, b2, stats, slope, mod=(z3, scale3, shift3, norm))


def edge_weight_wgrad(PQ: Tensor, idx: Tensor, scale1: Tensor, shift1: Tensor, z3: Tensor, scale3: Tensor, shift3: Tensor, norm: Norm, dy: Tensor,
                      slope: float = SLOPE) -> Tensor:
    """dW2i [O, k*F1] = dy^T @ (h*s).flat"""
    return edge_rank_wgrad(PQ, idx, scale1, shift1, dy, slope, mod=(z3, scale3, shift3, norm))


def edge_weight_dgrad(dy: Tensor, W2t: Tensor, PQ: Tensor, idx: Tensor, scale1: Tensor, shift1: Tensor, mean1: Tensor, invstd1: Tensor, z3: Tensor,
                      scale3: Tensor, shift3: Tensor, mean3: Tensor, invstd3: Tensor, norm: Norm, slope: float = SLOPE):
    """-> (du [M,k,F1], sums_u [2*F1] = [sum du | sum du*uhat], g3 [M*k, F1], sums_3 [2*F1] = [sum g3 | sum g3*z3hat]): the gradients
    reaching the pre-activation BatchNorm outputs of the h branch and of the weight MLP's last layer -- the two per-edge buffers of the
    backward.  W2t [k*F1, O] = W2i transposed."""
    M_, k, F1, O, tp, tiles = _dgrad_sizes(dy, W2t, PQ, idx)
    md = _mod((z3, scale3, shift3, norm), M_, k, F1)
    du = torch.empty((M_, k, F1), dtype=torch.float32, device=PQ.device)
    g3 = torch.empty((M_ * k, F1), dtype=torch.float32, device=PQ.device)
    part = torch.empty((2, tiles, F1, 2), dtype=torch.float32, device=PQ.device)
    check(_lib.load().spgan_edge_weight_dgrad(_p(dy), _ld(dy), _p(W2t), _ld(W2t), _p(PQ), 2 * F1, _p(idx), M_, k, F1, O, _p(_vec(scale1, F1, "scale1")),
                                              _p(_vec(shift1, F1, "shift1")), _p(_vec(mean1, F1, "mean1")), _p(_vec(invstd1, F1, "invstd1")),
                                              float(slope), md[0], md[1], md[2], _p(_vec(mean3, F1, "mean3")), _p(_vec(invstd3, F1, "invstd3")),
                                              md[3], md[4], _p(du), _p(g3), _p(part[0]), _p(part[1]), _s()), "edge_weight_dgrad", M=M_, k=k, F1=F1, O=O)
    return du, tile_sums(part[0], M_, tp), g3, tile_sums(part[1], M_, tp)


def _graph2(PQa: Tensor, PQb: Tensor, idx: Tensor):
    M_, k, F_ = _graph(PQa, idx)
    if _graph(PQb, idx) != (M_, k, F_):
        raise ValueError("PQa and PQb must both be [M, 2*F] = [%d, %d], got %s and %s" % (M_, 2 * F_, tuple(PQa.shape), tuple(PQb.shape)))
    return M_, k, F_


def edge_weight_gather2(PQa: Tensor, PQb: Tensor, idx: Tensor, scale_a: Tensor, shift_a: Tensor, scale_b: Tensor, shift_b: Tensor,
                        slope: float = SLOPE) -> Tensor:
    """w0 [M*k, F] = a_a * a_b, a_x = lrelu(scale_x * (Qx_i + Px_idx[i,r]) + shift_x), row i*k + r: the product of two activated narrow edge
    branches over one graph (deform_edgeConv's feature and coordinate branch, F = 16); neither branch is stored."""
    M_, k, F_ = _graph2(PQa, PQb, idx)
    w0 = torch.empty((M_ * k, F_), dtype=torch.float32, device=PQa.device)
    check(_lib.load().spgan_edge_weight_gather2(_p(PQa), 2 * F_, _p(PQb), 2 * F_, _p(idx), M_, k, F_, _p(_vec(scale_a, F_, "scale_a")),
                                                _p(_vec(shift_a, F_, "shift_a")), _p(_vec(scale_b, F_, "scale_b")), _p(_vec(shift_b, F_, "shift_b")),
                                                float(slope), _p(w0), _s()), "edge_weight_gather2", M=M_, k=k, F=F_)
    return w0


def edge_weight_split(dw0: Tensor, PQa: Tensor, PQb: Tensor, idx: Tensor, scale_a: Tensor, shift_a: Tensor, mean_a: Tensor, invstd_a: Tensor,
                      scale_b: Tensor, shift_b: Tensor, mean_b: Tensor, invstd_b: Tensor, slope: float = SLOPE):
    """dw0 [M*k, F], the gradient of edge_weight_gather2's product -> (ga [M,k,F] = lrelu'(pre_a) * dw0 * a_b, sums_a [2F] = [sum ga |
    sum ga*zhat_a], gb [M,k,F] = lrelu'(pre_b) * dw0 * a_a, sums_b [2F]): the gradients reaching the two branches' BatchNorm outputs, in
    the form edge_rank.edge_rank_scatter takes."""
    M_, k, F_ = _graph2(PQa, PQb, idx)
    _f32(dw0, "dw0")
    if not dw0.is_contiguous() or dw0.numel() != M_ * k * F_:
        raise ValueError("dw0 must be contiguous [M*k, F] = [%d, %d], got %s" % (M_ * k, F_, tuple(dw0.shape)))
    tp = tile_points(k)
    ga = torch.empty((M_, k, F_), dtype=torch.float32, device=PQa.device)
    gb = torch.empty_like(ga)
    part = torch.empty((2, (M_ + tp - 1) // tp, F_, 2), dtype=torch.float32, device=PQa.device)
    v = lambda t, n: _p(_vec(t, F_, n))
    check(_lib.load().spgan_edge_weight_split(_p(dw0), _p(PQa), 2 * F_, _p(PQb), 2 * F_, _p(idx), M_, k, F_, v(scale_a, "scale_a"), v(shift_a, "shift_a"),
                                              v(mean_a, "mean_a"), v(invstd_a, "invstd_a"), v(scale_b, "scale_b"), v(shift_b, "shift_b"),
                                              v(mean_b, "mean_b"), v(invstd_b, "invstd_b"), float(slope), _p(ga), _p(gb), _p(part[0]), _p(part[1]),
                                              _s()), "edge_weight_split", M=M_, k=k, F=F_)
    return ga, tile_sums(part[0], M_, tp), gb, tile_sums(part[1], M_, tp)


# ----------------------------------------------------------------------------- the stored-operand forms (bilateral_upsample_edgeConv)
STORED_K_MAX = 28


def _stored(U: Tensor, z3: Tensor, k: int):
    """U and z3 hold [M,k,F1] values each, contiguous, in any view of that memory (U is upsample_edgeConv's [M*k/2, 2*F1]) -> (M, F1)"""
    _f32(U, "U"); _f32(z3, "z3", 2)
    if k % 2 or not 2 <= k <= STORED_K_MAX:
        raise ValueError("edge_stored: k must be even and lie in 2..%d, got k=%d" % (STORED_K_MAX, k))
    if not z3.is_contiguous() or z3.shape[0] % k or z3.shape[0] < k or not U.is_contiguous() or U.numel() != z3.numel():
        raise ValueError("edge_stored: z3 must be contiguous [M*k, F1] and U hold as many contiguous values, got %s and %s (k=%d)"
                         % (tuple(z3.shape), tuple(U.shape), k))
    return z3.shape[0] // k, z3.shape[1]


def edge_stored_gemm(U: Tensor, k: int, scale1: Tensor, shift1: Tensor, z3: Tensor, scale3: Tensor, shift3: Tensor, norm: Norm, W2i: Tensor,
                     b2: Optional[Tensor] = None, stats: bool = False, slope: float = SLOPE):
    """y [M,O] = b2 + (h*s).flat @ W2i^T with h(i,r,c) = lrelu(scale1[(r&1)*F1 + c] * U[i,r,c] + shift1[(r&1)*F1 + c]): edge_weight_gemm
    whose modulated operand is the stored pre-norm tensor U [M,k,F1]; scale1, shift1 [2*F1]; W2i [O, k*F1], column r*F1 + c.
    (-> (y, partials, tile_rows) with stats=True)"""
    M_, F1 = _stored(U, z3, k)
    _rowmajor2d(W2i, "W2i")
    if W2i.shape[1] != k * F1 or W2i.shape[0] < 1:
        raise ValueError("W2i must be [O, k*F1] = [O, %d] (k=%d, F1=%d), got %s" % (k * F1, k, F1, tuple(W2i.shape)))
    O = W2i.shape[0]
    md = _mod((z3, scale3, shift3, norm), M_, k, F1)
    y = torch.empty((M_, O), dtype=torch.float32, device=U.device)
    part, tp = None, 0
    if stats:
        tp = tile_points(k)
        part = torch.empty(((M_ + tp - 1) // tp, O, 2), dtype=torch.float32, device=U.device)
    check(_lib.load().spgan_edge_stored_gemm(_p(U), M_, k, F1, _p(_vec(scale1, 2 * F1, "scale1")), _p(_vec(shift1, 2 * F1, "shift1")), float(slope), *md,
                                             _p(W2i), _ld(W2i), _p(_vec(b2, O, "b2")), O, _p(y), O, _p(part), _s()), "edge_stored_gemm",
          M=M_, k=k, F1=F1, O=O)
    return (y, part, tp) if stats else y


def edge_stored_wgrad(U: Tensor, k: int, scale1: Tensor, shift1: Tensor, z3: Tensor, scale3: Tensor, shift3: Tensor, norm: Norm, dy: Tensor,
                      slope: float = SLOPE) -> Tensor:
    """dW2i [O, k*F1] = dy^T @ (h*s).flat over the stored h (edge_stored_gemm)"""
    M_, F1 = _stored(U, z3, k)
    _rowmajor2d(dy, "dy")
    if dy.shape[0] != M_:
        raise ValueError("dy must have M = %d rows" % M_)
    O = dy.shape[1]
    md = _mod((z3, scale3, shift3, norm), M_, k, F1)
    lib = _lib.load()
    wsb = lib.spgan_edge_rank_wgrad_ws_bytes(M_, k, F1, O)
    if wsb == 0:
        raise ValueError("edge_stored_wgrad: unsupported sizes M=%d k=%d F1=%d O=%d" % (M_, k, F1, O))
    ws = torch.empty((wsb // 4,), dtype=torch.float32, device=U.device)
    dW = torch.empty((O, k * F1), dtype=torch.float32, device=U.device)
    check(lib.spgan_edge_stored_wgrad(_p(U), M_, k, F1, _p(_vec(scale1, 2 * F1, "scale1")), _p(_vec(shift1, 2 * F1, "shift1")), float(slope), *md,
                                      _p(dy), _ld(dy), O, _p(dW), k * F1, _p(ws), wsb, _s()), "edge_stored_wgrad", M=M_, k=k, F1=F1, O=O)
    return dW


def edge_stored_dgrad(dy: Tensor, W2t: Tensor, U: Tensor, k: int, scale1: Tensor, shift1: Tensor, mean1: Tensor, invstd1: Tensor, z3: Tensor,
                      scale3: Tensor, shift3: Tensor, mean3: Tensor, invstd3: Tensor, norm: Norm, slope: float = SLOPE):
    """-> (gU [M,k,F1], sums_u [2*2F1] = [sum gU | sum gU*uhat], one entry per (rank parity, channel) as scale1 is laid out, g3 [M*k, F1],
    sums_3 [2*F1]): edge_weight_dgrad over the stored h.  W2t [k*F1, O] = W2i transposed; scale1, shift1, mean1, invstd1 [2*F1]."""
    M_, F1 = _stored(U, z3, k)
    _rowmajor2d(dy, "dy"); _rowmajor2d(W2t, "W2t")
    O = dy.shape[1]
    if dy.shape[0] != M_ or tuple(W2t.shape) != (k * F1, O):
        raise ValueError("dy must be [M,O] and W2t [k*F1, O] = [%d, %d], got %s and %s" % (k * F1, O, tuple(dy.shape), tuple(W2t.shape)))
    tp = tile_points(k)
    tiles = (M_ + tp - 1) // tp
    md = _mod((z3, scale3, shift3, norm), M_, k, F1)
    gU = torch.empty((M_, k, F1), dtype=torch.float32, device=U.device)
    g3 = torch.empty((M_ * k, F1), dtype=torch.float32, device=U.device)
    part_u = torch.empty((tiles, 2 * F1, 2), dtype=torch.float32, device=U.device)
    part_3 = torch.empty((tiles, F1, 2), dtype=torch.float32, device=U.device)
    v1 = lambda t, n: _p(_vec(t, 2 * F1, n))
    check(_lib.load().spgan_edge_stored_dgrad(_p(dy), _ld(dy), _p(W2t), _ld(W2t), _p(U), M_, k, F1, O, v1(scale1, "scale1"), v1(shift1, "shift1"),
                                              v1(mean1, "mean1"), v1(invstd1, "invstd1"), float(slope), md[0], md[1], md[2],
                                              _p(_vec(mean3, F1, "mean3")), _p(_vec(invstd3, F1, "invstd3")), md[3], md[4], _p(gU), _p(g3),
                                              _p(part_u), _p(part_3), _s()), "edge_stored_dgrad", M=M_, k=k, F1=F1, O=O)
    return gU, tile_sums(part_u, M_, tp), g3, tile_sums(part_3, M_, tp)
