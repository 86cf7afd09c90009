"""Tensor-level wrappers of the max-aggregation edge convolution's launchers (csrc/edge_max.hip; include/spgan_hip.h): the passes
behind `spgan.edgeConv` (edge_conv.EdgeMaxConvFn).  PQ [M,2F] = [P | Q] is the per-point GEMM's result, idx int32 [M,k] global rows.
Same conventions as spgan.ops: arguments validated, outputs from PyTorch's caching allocator, launches on the current stream."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._lib import check
from .ops import BN_EPS, BN_MOMENTUM, _f32, _i32, _p, _s, _vec

Tensor = torch.Tensor


def _pq(PQ: Tensor, F_: int) -> Tensor:
    _f32(PQ, "PQ", 2)
    if not PQ.is_contiguous() or PQ.shape[1] != 2 * F_:
        raise ValueError("PQ must be contiguous [M, 2F]")
    return PQ


def tile_sums(part: Tensor, M_: int, tile_points: int, out: Optional[Tensor] = None) -> Tensor:
    """A backward pass's per-tile records, partials [tiles,F,2] over M points in tiles of tile_points -> sums [2F] = [sum | sum * xhat]
    (into out [2,F] when given)"""
    tiles, F_ = part.shape[0], part.shape[1]
    sums = torch.empty((2, F_), dtype=torch.float32, device=part.device) if out is None else out
    check(_lib.load().spgan_colstats_finalize(_p(part), 1, tiles, F_, M_, 1, tile_points, _p(sums[0]), _p(sums[1]), _s()), "colstats_finalize")
    return sums.view(-1)


def edge_max_gather(PQ: Tensor, idx: Tensor):
    """Train-mode gather pass over PQ [M,2F] = [P | Q]: -> (pmax, pmin [M,F], rmax, rmin uint8 [M,F], partials, tile_rows):
    max / min of P over each point's k neighbours with the ranks of the extremes, and the (sum, centred M2) records of the M*k edge
    values Q_i + P_n (finalize mode 0 with tile_rows)."""
    F_ = PQ.shape[1] // 2
    _pq(PQ, F_); _i32(idx, "idx")
    M_, k = idx.shape
    lib = _lib.load()
    tp = lib.spgan_edge_max_tile_points()
    f = torch.empty((2, M_, F_), dtype=torch.float32, device=PQ.device)
    rk = torch.empty((2, M_, F_), dtype=torch.uint8, device=PQ.device)
    part = torch.empty(((M_ + tp - 1) // tp, F_, 2), dtype=torch.float32, device=PQ.device)
    check(lib.spgan_edge_max_gather(_p(PQ), 2 * F_, _p(idx), M_, k, F_, _p(f[0]), _p(f[1]), _p(rk[0]), _p(rk[1]), _p(part), None, None,
                                    None, None, _s()), "edge_max_gather", M=M_, k=k, F=F_)
    return f[0], f[1], rk[0], rk[1], part, tp * k


def edge_max_bn(part: Tensor, tile_rows: int, E: int, gamma: Tensor, beta: Tensor, running_mean: Optional[Tensor], running_var: Optional[Tensor],
                momentum: float = BN_MOMENTUM, eps: float = BN_EPS):
    """edge_max_gather's records -> the train-mode BatchNorm2d bookkeeping over the E = M*k edges: (scale, shift, invstd, mean) [4,F]; the
    running statistics are updated in place (unbiased variance), as nn.BatchNorm2d does."""
    F_ = part.shape[1]
    st = torch.empty((4, F_), dtype=torch.float32, device=part.device)
    check(_lib.load().spgan_colstats_finalize_bn(_p(part), part.shape[0], F_, E, tile_rows, _p(_vec(gamma, F_, "gamma")), _p(_vec(beta, F_, "beta")),
                                                 float(eps), float(momentum), _p(running_mean), _p(running_var), _p(st[0]), _p(st[1]), _p(st[2]),
                                                 _p(st[3]), _s()), "colstats_finalize_bn", C=F_, G=E)
    return st


def edge_max_finish(PQ: Tensor, pmax: Tensor, pmin: Tensor, rmax: Tensor, rmin: Tensor, scale: Tensor, shift: Tensor):
    """-> (out [M,F] = relu(scale*(Q + (scale >= 0 ? pmax : pmin)) + shift), sel uint8 [M,F] = chosen rank | 0x80 where the ReLU clipped)."""
    M_, F_ = pmax.shape
    _pq(PQ, F_)
    out = torch.empty((M_, F_), dtype=torch.float32, device=PQ.device)
    sel = torch.empty((M_, F_), dtype=torch.uint8, device=PQ.device)
    check(_lib.load().spgan_edge_max_finish(_p(PQ), 2 * F_, _p(pmax), _p(pmin), _p(rmax), _p(rmin), _p(_vec(scale, F_, "scale")),
                                            _p(_vec(shift, F_, "shift")), M_, F_, _p(out), _p(sel), _s()), "edge_max_finish", M=M_, F=F_)
    return out, sel


def edge_max_eval(PQ: Tensor, idx: Tensor, scale: Tensor, shift: Tensor):
    """Gather and finish in one pass (the affine is known: eval mode) -> (out, sel)."""
    F_ = PQ.shape[1] // 2
    _pq(PQ, F_); _i32(idx, "idx")
    M_, k = idx.shape
    out = torch.empty((M_, F_), dtype=torch.float32, device=PQ.device)
    sel = torch.empty((M_, F_), dtype=torch.uint8, device=PQ.device)
    check(_lib.load().spgan_edge_max_gather(_p(PQ), 2 * F_, _p(idx), M_, k, F_, None, None, None, None, None, _p(_vec(scale, F_, "scale")),
                                            _p(_vec(shift, F_, "shift")), _p(out), _p(sel), _s()), "edge_max_gather", M=M_, k=k, F=F_)
    return out, sel


def edge_max_bwd_point(g: Tensor, sel: Tensor, PQ: Tensor, idx: Tensor, mean: Tensor, invstd: Tensor) -> Tensor:
    """g [M,F] becomes r = g * 1[out > 0] IN PLACE; -> sums [2F] = [sum r | sum r * xhat_sel] (the gradients of BatchNorm's bias | weight)."""
    M_, F_ = g.shape
    _pq(PQ, F_); _i32(idx, "idx"); _f32(g, "g", 2)
    if not g.is_contiguous() or sel.dtype != torch.uint8 or not sel.is_contiguous() or sel.shape != g.shape:
        raise ValueError("g must be contiguous [M,F] and sel uint8 of the same shape")
    lib = _lib.load()
    tp = lib.spgan_edge_max_tile_points()
    part = torch.empty(((M_ + tp - 1) // tp, F_, 2), dtype=torch.float32, device=g.device)
    check(lib.spgan_edge_max_bwd_point(_p(g), _p(sel), _p(PQ), 2 * F_, _p(idx), M_, idx.shape[1], F_, _p(_vec(mean, F_, "mean")),
                                       _p(_vec(invstd, F_, "invstd")), _p(part), _s()), "edge_max_bwd_point", M=M_, F=F_)
    return tile_sums(part, M_, tp)


def edge_max_bwd_graph(r: Tensor, sel: Tensor, PQ: Tensor, k: int, rowptr: Tensor, src: Tensor, scale: Tensor, idx: Optional[Tensor] = None,
                       mean: Optional[Tensor] = None, invstd: Optional[Tensor] = None, sums: Optional[Tensor] = None) -> Tensor:
    """-> dPQ [M,2F] = [dP | dQ].  sums (with idx, mean, invstd): train mode; without: eval mode (the statistics are constants)."""
    M_, F_ = r.shape
    _pq(PQ, F_); _i32(rowptr, "rowptr"); _i32(src, "src")
    if rowptr.numel() != M_ + 1 or src.numel() != M_ * k:
        raise ValueError("rowptr [M+1] / src [M*k] do not fit r [M,F]")
    dPQ = torch.empty((M_, 2 * F_), dtype=torch.float32, device=r.device)
    check(_lib.load().spgan_edge_max_bwd_graph(_p(r), _p(sel), _p(PQ), 2 * F_, _p(rowptr), _p(src), _p(idx), M_, k, F_, _p(_vec(scale, F_, "scale")),
                                               _p(_vec(mean, F_, "mean")), _p(_vec(invstd, F_, "invstd")), _p(_vec(sums, 2 * F_, "sums")), _p(dPQ),
                                               2 * F_, _s()), "edge_max_bwd_graph", M=M_, k=k, F=F_)
    return dPQ


def _vpq(VPQ: Tensor, PQ: Tensor) -> Tensor:
    _f32(VPQ, "VPQ", 2)
    if not VPQ.is_contiguous() or VPQ.shape != PQ.shape:
        raise ValueError("VPQ must be contiguous [M, 2F] like PQ")
    return VPQ


def _r_sel(r: Tensor, sel: Tensor) -> None:
    _f32(r, "r", 2)
    if not r.is_contiguous() or sel.dtype != torch.uint8 or not sel.is_contiguous() or sel.shape != r.shape:
        raise ValueError("r must be contiguous [M,F] and sel uint8 of the same shape")


def edge_max_dbl_point(r: Tensor, sel: Tensor, PQ: Tensor, VPQ: Tensor, idx: Tensor, mean: Optional[Tensor] = None,
                       invstd: Optional[Tensor] = None) -> Tensor:
    """The direction's sums for the second derivative through dx: VPQ [M,2F] = [VP | VQ] = v Wst^T, t(i,j) = VQ_i + VP_n(i,j).
    With mean, invstd (train mode) -> dsums [3F] = [T1 | T2 | S] = [sum_e t_e | sum_e t_e * xhat_e | sum_i r_i * t(i, sel)];
    without (eval mode) -> [F] = S."""
    M_, F_ = r.shape
    _pq(PQ, F_); _vpq(VPQ, PQ); _i32(idx, "idx"); _r_sel(r, sel)
    train = mean is not None
    lib = _lib.load()
    tp = lib.spgan_edge_max_tile_points()
    part = torch.empty((2 if train else 1, (M_ + tp - 1) // tp, F_, 2), dtype=torch.float32, device=r.device)
    check(lib.spgan_edge_max_dbl_point(_p(r), _p(sel), _p(PQ), 2 * F_, _p(VPQ), 2 * F_, _p(idx), M_, idx.shape[1], F_, _p(_vec(mean, F_, "mean")),
                                       _p(_vec(invstd, F_, "invstd")), _p(part[0]) if train else None, _p(part[-1]), _s()),
          "edge_max_dbl_point", M=M_, F=F_)
    dsums = torch.empty((4 if train else 2, F_), dtype=torch.float32, device=r.device)
    if train:
        tile_sums(part[0], M_, tp, out=dsums[:2])
    tile_sums(part[-1], M_, tp, out=dsums[-2:])
    return dsums.view(-1)[:3 * F_] if train else dsums[0]


def edge_max_dbl_graph(r: Tensor, sel: Tensor, PQ: Tensor, VPQ: Tensor, idx: Tensor, scale: Tensor, k: Optional[int] = None,
                       rowptr: Optional[Tensor] = None, src: Optional[Tensor] = None, mean: Optional[Tensor] = None,
                       invstd: Optional[Tensor] = None, sums: Optional[Tensor] = None, dsums: Optional[Tensor] = None):
    """-> (ghat [M,F], PQbar [M,2F] | None): the cotangents of the incoming cotangent g and of PQ.  sums, dsums (with rowptr, src, mean,
    invstd): train mode; without: eval mode (the statistics are constants: ghat = 1[out > 0] * scale * t(i, sel), no PQbar)."""
    M_, F_ = r.shape
    _pq(PQ, F_); _vpq(VPQ, PQ); _i32(idx, "idx"); _r_sel(r, sel)
    k = idx.shape[1] if k is None else k
    if idx.shape != (M_, k):
        raise ValueError("idx [M,k] does not fit r [M,F]")
    train = sums is not None
    ghat = torch.empty((M_, F_), dtype=torch.float32, device=r.device)
    PQbar = None
    if train:
        _i32(rowptr, "rowptr"); _i32(src, "src")
        if rowptr.numel() != M_ + 1 or src.numel() != M_ * k:
            raise ValueError("rowptr [M+1] / src [M*k] do not fit r [M,F]")
        PQbar = torch.empty((M_, 2 * F_), dtype=torch.float32, device=r.device)
    check(_lib.load().spgan_edge_max_dbl_graph(_p(r), _p(sel), _p(PQ), 2 * F_, _p(VPQ), 2 * F_, _p(rowptr) if train else None,
                                               _p(src) if train else None, _p(idx), M_, k, F_, _p(_vec(scale, F_, "scale")),
                                               _p(_vec(mean, F_, "mean")) if train else None, _p(_vec(invstd, F_, "invstd")) if train else None,
                                               _p(_vec(sums, 2 * F_, "sums")), _p(_vec(dsums, 3 * F_, "dsums")), _p(ghat), _p(PQbar), 2 * F_, _s()),
          "edge_max_dbl_graph", M=M_, k=k, F=F_)
    return ghat, PQbar
