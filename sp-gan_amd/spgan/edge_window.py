"""Tensor-level wrappers of the rank-window edge convolution's launchers (csrc/edge_window.hip; include/spgan_hip.h): the passes behind
`spgan.upsample_edgeConv` (edge_conv.UpsampleEdgeConvFn).  x [M,C] point-major, idx int32 [M,k] global rows, W [O, w*C] the difference
half of a [1,w] conv weight, tap-major; T = k - w + 1 window positions per point, output rows (i,t).
Same conventions as spgan.ops: arguments validated, outputs from PyTorch's caching allocator, launches on the current stream."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._lib import check
from .ops import _i32, _ld, _p, _rowmajor2d, _s

Tensor = torch.Tensor


def _graph(x: Tensor, idx: Tensor):
    _rowmajor2d(x, "x"); _i32(idx, "idx")
    if idx.dim() != 2 or idx.shape[0] != x.shape[0] or not idx.is_contiguous():
        raise ValueError("idx must be contiguous int32 [M,k] with one row per row of x")
    return x.shape[0], idx.shape[1], x.shape[1]


def _taps(W: Tensor, C: int, k: int, name: str) -> int:
    _rowmajor2d(W, name)
    w = W.shape[1] // C
    if w * C != W.shape[1] or not 1 <= w <= k:
        raise ValueError("%s must be [O, w*C] with 1 <= w <= k (C=%d, k=%d), got %s" % (name, C, k, tuple(W.shape)))
    return w


def tile_points(k: int, T: int) -> int:
    tp = _lib.load().spgan_edge_window_tile_points(k, T)
    if tp <= 0:
        raise ValueError("edge_window: unsupported k=%d, T=%d" % (k, T))
    return tp


def edge_window_gemm(x: Tensor, idx: Tensor, W: Tensor, rowadd: Optional[Tensor] = None, add2: Optional[Tensor] = None, stats: bool = False):
    """Y [M*T, O] = windows(d) @ W^T + rowadd[i] + add2   (-> (Y, partials, tile_rows) with stats=True: the (sum, centred M2) column
    records of Y for spgan_colstats_finalize_bn)."""
    M_, k, Cn = _graph(x, idx)
    w = _taps(W, Cn, k, "W")
    O, T = W.shape[0], k - w + 1
    lib = _lib.load()
    if rowadd is not None and (tuple(_rowmajor2d(rowadd, "rowadd").shape) != (M_, O)):
        raise ValueError("rowadd must be [M,O]")
    if add2 is not None and (tuple(_rowmajor2d(add2, "add2").shape) != (M_ * T, O)):
        raise ValueError("add2 must be [M*T,O]")
    Y = torch.empty((M_ * T, O), dtype=torch.float32, device=x.device)
    part, tp = None, 0
    if stats:
        tp = tile_points(k, T)
        part = torch.empty(((M_ + tp - 1) // tp, O, 2), dtype=torch.float32, device=x.device)
    check(lib.spgan_edge_window_gemm(_p(x), _ld(x), _p(idx), M_, k, Cn, _p(W), _ld(W), O, w, _p(rowadd), _ld(rowadd) if rowadd is not None else 0,
                                     _p(add2), _ld(add2) if add2 is not None else 0, _p(Y), O, _p(part), _s()), "edge_window_gemm", M=M_, k=k, C=Cn,
          O=O, w=w)
    return (Y, part, tp * T) if stats else Y


def edge_window_wgrad(x: Tensor, idx: Tensor, G: Tensor, w: int) -> Tensor:
    """dW [O, w*C] = sum over the rows (i,t) of G[(i,t), :]^T windows(d)[(i,t), :]"""
    M_, k, Cn = _graph(x, idx)
    _rowmajor2d(G, "G")
    T = k - w + 1
    if not 1 <= w <= k or G.shape[0] != M_ * T:
        raise ValueError("G must have M*T = %d rows" % (M_ * T))
    O = G.shape[1]
    lib = _lib.load()
    wsb = lib.spgan_edge_window_wgrad_ws_bytes(M_, k, Cn, O, w)
    if wsb == 0:
        raise ValueError("edge_window_wgrad: unsupported sizes M=%d k=%d C=%d O=%d w=%d" % (M_, k, Cn, O, w))
    ws = torch.empty((wsb // 4,), dtype=torch.float32, device=x.device)
    dW = torch.empty((O, w * Cn), dtype=torch.float32, device=x.device)
    check(lib.spgan_edge_window_wgrad(_p(x), _ld(x), _p(idx), M_, k, Cn, _p(G), _ld(G), O, w, _p(dW), w * Cn, _p(ws), wsb, _s()), "edge_window_wgrad",
          M=M_, k=k, C=Cn, O=O, w=w)
    return dW


def edge_window_dgrad(G: Tensor, Wt: Tensor, k: int, Cn: int, out: Optional[Tensor] = None) -> Tensor:
    """S [M,k,C] (+)= sum_{t+r=j} G(i,t,:) W_r, Wt [w*C, O] = the weight image transposed.  out: accumulate into it."""
    _rowmajor2d(G, "G"); _rowmajor2d(Wt, "Wt")
    w = Wt.shape[0] // Cn
    T = k - w + 1
    O = G.shape[1]
    if w * Cn != Wt.shape[0] or not 1 <= w <= k or Wt.shape[1] != O or G.shape[0] % T:
        raise ValueError("Wt must be [w*C, O] and G [M*T, O]")
    M_ = G.shape[0] // T
    acc = out is not None
    if acc:
        if tuple(out.shape) != (M_, k, Cn) or not out.is_contiguous() or out.dtype != torch.float32:
            raise ValueError("out must be contiguous float32 [M,k,C]")
    else:
        out = torch.empty((M_, k, Cn), dtype=torch.float32, device=G.device)
    check(_lib.load().spgan_edge_window_dgrad(_p(G), _ld(G), _p(Wt), _ld(Wt), M_, k, Cn, O, w, _p(out), 1 if acc else 0, _s()), "edge_window_dgrad",
          M=M_, k=k, C=Cn, O=O, w=w)
    return out


def edge_window_scatter(S: Tensor, rowptr: Tensor, src: Tensor, add_a: Optional[Tensor] = None, add_b: Optional[Tensor] = None) -> Tensor:
    """dx [M,C] = add_a + add_b - sum_j S[m,j] + sum over the in-edge lists (ops.csr_build) of S[e]"""
    if S.dim() != 3 or not S.is_contiguous() or S.dtype != torch.float32:
        raise ValueError("S must be contiguous float32 [M,k,C]")
    M_, k, Cn = S.shape
    _i32(rowptr, "rowptr"); _i32(src, "src")
    if rowptr.numel() != M_ + 1 or src.numel() != M_ * k:
        raise ValueError("rowptr [M+1] / src [M*k] do not fit S [M,k,C]")
    for a in (add_a, add_b):
        if a is not None and tuple(_rowmajor2d(a, "addend").shape) != (M_, Cn):
            raise ValueError("an addend must be [M,C]")
    dx = torch.empty((M_, Cn), dtype=torch.float32, device=S.device)
    check(_lib.load().spgan_edge_window_scatter(_p(S), _p(rowptr), _p(src), M_, k, Cn, _p(add_a), _ld(add_a) if add_a is not None else 0, _p(add_b),
                                                _ld(add_b) if add_b is not None else 0, _p(dx), Cn, _s()), "edge_window_scatter", M=M_, k=k, C=Cn)
    return dx
