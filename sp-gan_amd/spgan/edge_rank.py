"""Tensor-level wrappers of the full-rank edge convolution's launchers (csrc/edge_rank.hip; include/spgan_hip.h): the passes behind
`spgan.deform_edgeConv_simple` / `spgan.deform_edgeConv_first` (edge_conv.RankEdgeConvFn).  PQ [M,2F1] = [P | Q] is the per-point GEMM's
result, idx int32 [M,k] global rows, scale1 / shift1 [F1] the affine of the first BatchNorm, W2i [O, k*F1] the [1,k] conv weight, tap-major
(column r*F1 + c); h(i,r,c) = lrelu(scale1*(Q_i + P_idx[i,r]) + shift1) exists only inside the kernels.
This layer does not follow `ops.set_mfma_operands`: its products are always exact fp32 MFMA with fp32 accumulation.
Same conventions as spgan.ops: arguments validated, outputs from PyTorch's caching allocator, launches on the current stream."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import check
from .edge_max import tile_sums
from .ops import _f32, _i32, _ld, _p, _rowmajor2d, _s, _vec

Tensor = torch.Tensor
Norm = Optional[Tuple[Tensor, Tensor]]
Mod = Optional[Tuple[Tensor, Tensor, Tensor, Norm]]       # (z3, scale3, shift3, norm): the per-edge weight of spgan.edge_weight
K_MAX = 32
SLOPE = 0.01


def _graph(PQ: Tensor, idx: Tensor):
    _f32(PQ, "PQ", 2); _i32(idx, "idx")
    if not PQ.is_contiguous() or PQ.shape[1] % 2 or PQ.shape[1] < 2:
        raise ValueError("PQ must be contiguous [M, 2*F1], got %s" % (tuple(PQ.shape),))
    if idx.dim() != 2 or idx.shape[0] != PQ.shape[0] or not idx.is_contiguous():
        raise ValueError("idx must be contiguous int32 [M,k] with one row per row of PQ")
    M_, k, F1 = PQ.shape[0], idx.shape[1], PQ.shape[1] // 2
    if not 1 <= k <= K_MAX or M_ < 1:
        raise ValueError("edge_rank: unsupported sizes M=%d k=%d F1=%d (1 <= k <= %d, M >= 1)" % (M_, k, F1, K_MAX))
    return M_, k, F1


def tile_points(k: int) -> int:
    tp = _lib.load().spgan_edge_rank_tile_points(k)
    if tp <= 0:
        raise ValueError("edge_rank: unsupported k=%d (1 <= k <= %d)" % (k, K_MAX))
    return tp


def _mod(mod: Mod, M_: int, k: int, F1: int):
    """-> the five modulation pointers (z3, scale3, shift3, wmax | None, wrs | None), validated against [M,k,F1]"""
    z3, scale3, shift3, norm = mod
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


def _dgrad_sizes(dy: Tensor, W2t: Tensor, PQ: Tensor, idx: Tensor):
    """The dgrad launchers' common checks -> (M, k, F1, O, tile_points, tiles)"""
    M_, k, F1 = _graph(PQ, idx)
    _rowmajor2d(dy, "dy"); _rowmajor2d(W2t, "W2t")
    O = dy.shape[1]
    if dy.shape[0] != M_ or tuple(W2t.shape) != (k * F1, O):
        raise ValueError("dy must be [M,O] and W2t [k*F1, O] = [%d, %d], got %s and %s" % (k * F1, O, tuple(dy.shape), tuple(W2t.shape)))
    tp = tile_points(k)
    return M_, k, F1, O, tp, (M_ + tp - 1) // tp


def edge_rank_gemm(PQ: Tensor, idx: Tensor, scale1: Tensor, shift1: Tensor, W2i: Tensor, b2: Optional[Tensor] = None, stats: bool = False,
                   slope: float = SLOPE, mod: Mod = None):
    """y [M,O] = b2 + h.flat @ W2i^T   (-> (y, partials, tile_rows) with stats=True: the (sum, centred M2) column records of y for
    spgan_colstats_finalize_bn / edge_max.edge_max_bn).  mod: h is multiplied by the per-edge weight (edge_weight.edge_weight_gemm)."""
    M_, k, F1 = _graph(PQ, idx)
    _rowmajor2d(W2i, "W2i")
    if W2i.shape[1] != k * F1 or W2i.shape[0] < 1:
        raise ValueError("W2i must be [O, k*F1] = [O, %d] (k=%d, F1=%d), got %s" % (k * F1, k, F1, tuple(W2i.shape)))
    O = W2i.shape[0]
    lib = _lib.load()
    fn, name, md = (lib.spgan_edge_rank_gemm, "edge_rank_gemm", ()) if mod is None else (lib.spgan_edge_weight_gemm, "edge_weight_gemm", _mod(mod, M_, k, F1))
    y = torch.empty((M_, O), dtype=torch.float32, device=PQ.device)
    part, tp = None, 0
    if stats:
        tp = tile_points(k)
        part = torch.empty(((M_ + tp - 1) // tp, O, 2), dtype=torch.float32, device=PQ.device)
    check(fn(_p(PQ), 2 * F1, _p(idx), M_, k, F1, _p(_vec(scale1, F1, "scale1")), _p(_vec(shift1, F1, "shift1")), float(slope), *md,
             _p(W2i), _ld(W2i), _p(_vec(b2, O, "b2")), O, _p(y), O, _p(part), _s()), name, M=M_, k=k, F1=F1, O=O)
    return (y, part, tp) if stats else y


def edge_rank_wgrad(PQ: Tensor, idx: Tensor, scale1: Tensor, shift1: Tensor, dy: Tensor, slope: float = SLOPE, mod: Mod = None) -> Tensor:
    """dW2i [O, k*F1] = dy^T @ h.flat   (mod: as edge_rank_gemm)"""
    M_, k, F1 = _graph(PQ, idx)
    _rowmajor2d(dy, "dy")
    if dy.shape[0] != M_:
        raise ValueError("dy must have M = %d rows" % M_)
    O = dy.shape[1]
    lib = _lib.load()
    fn, name, md = (lib.spgan_edge_rank_wgrad, "edge_rank_wgrad", ()) if mod is None else (lib.spgan_edge_weight_wgrad, "edge_weight_wgrad", _mod(mod, M_, k, F1))
    wsb = lib.spgan_edge_rank_wgrad_ws_bytes(M_, k, F1, O)
    if wsb == 0:
        raise ValueError("%s: unsupported sizes M=%d k=%d F1=%d O=%d" % (name, M_, k, F1, O))
    ws = torch.empty((wsb // 4,), dtype=torch.float32, device=PQ.device)
    dW = torch.empty((O, k * F1), dtype=torch.float32, device=PQ.device)
    check(fn(_p(PQ), 2 * F1, _p(idx), M_, k, F1, _p(_vec(scale1, F1, "scale1")), _p(_vec(shift1, F1, "shift1")), float(slope), *md,
             _p(dy), _ld(dy), O, _p(dW), k * F1, _p(ws), wsb, _s()), name, M=M_, k=k, F1=F1, O=O)
    return dW


def edge_rank_dgrad(dy: Tensor, W2t: Tensor, PQ: Tensor, idx: Tensor, scale1: Tensor, shift1: Tensor, mean1: Tensor, invstd1: Tensor,
                    slope: float = SLOPE):
    """-> (da [M,k,F1] = lrelu'(a) * (dy @ W2i) -- the one per-edge buffer of the layer, backward only --, sums [2*F1] = [sum da | sum da*zhat]
    over the M*k edges).  W2t [k*F1, O] = W2i transposed."""
    M_, k, F1, O, tp, tiles = _dgrad_sizes(dy, W2t, PQ, idx)
    da = torch.empty((M_, k, F1), dtype=torch.float32, device=PQ.device)
    part = torch.empty((tiles, F1, 2), dtype=torch.float32, device=PQ.device)
    check(_lib.load().spgan_edge_rank_dgrad(_p(dy), _ld(dy), _p(W2t), _ld(W2t), _p(PQ), 2 * F1, _p(idx), M_, k, F1, O, _p(_vec(scale1, F1, "scale1")),
                                            _p(_vec(shift1, F1, "shift1")), _p(_vec(mean1, F1, "mean1")), _p(_vec(invstd1, F1, "invstd1")),
                                            float(slope), _p(da), _p(part), _s()), "edge_rank_dgrad", M=M_, k=k, F1=F1, O=O)
    return da, tile_sums(part, M_, tp)


def edge_rank_scatter(da: Tensor, rowptr: Tensor, src: Tensor, scale1: Tensor, PQ: Optional[Tensor] = None, idx: Optional[Tensor] = None,
                      mean1: Optional[Tensor] = None, invstd1: Optional[Tensor] = None, sums: Optional[Tensor] = None) -> Tensor:
    """-> dPQ [M,2F1] = [dP | dQ] over the in-edge lists of ops.csr_build.  sums (with PQ, idx, mean1, invstd1): train mode, the
    BatchNorm correction terms are applied per edge; without: eval mode (dz = scale1 * da)."""
    if da.dim() != 3 or not da.is_contiguous() or da.dtype != torch.float32 or not da.is_cuda:
        raise ValueError("da must be contiguous float32 [M,k,F1] on the GPU")
    M_, k, F1 = da.shape
    if not 1 <= k <= K_MAX:
        raise ValueError("edge_rank_scatter: unsupported k=%d" % k)
    _i32(rowptr, "rowptr"); _i32(src, "src")
    if rowptr.numel() != M_ + 1 or src.numel() != M_ * k:
        raise ValueError("rowptr [M+1] / src [M*k] do not fit da [M,k,F1]")
    train = sums is not None
    if train:
        if PQ is None or idx is None or mean1 is None or invstd1 is None:
            raise ValueError("edge_rank_scatter: train mode needs PQ, idx, mean1 and invstd1 with sums")
        if _graph(PQ, idx) != (M_, k, F1):
            raise ValueError("PQ / idx do not fit da [M,k,F1]")
    dPQ = torch.empty((M_, 2 * F1), dtype=torch.float32, device=da.device)
    check(_lib.load().spgan_edge_rank_scatter(_p(da), _p(rowptr), _p(src), _p(PQ) if train else None, 2 * F1, _p(idx) if train else None, M_, k, F1,
                                              _p(_vec(scale1, F1, "scale1")), _p(_vec(mean1, F1, "mean1")) if train else None,
                                              _p(_vec(invstd1, F1, "invstd1")) if train else None, _p(_vec(sums, 2 * F1, "sums")) if train else None,
                                              _p(dPQ), 2 * F1, _s()), "edge_rank_scatter", M=M_, k=k, F1=F1)
    return dPQ
