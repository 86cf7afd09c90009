"""Tensor-level wrappers of the block tail's launchers (csrc/block_tail.hip; include/spgan_hip.h): the passes behind the bilateral / deform
blocks of spgan.modules (edge_conv.BlockTailFn).  Y [B,C,L] is the pre-norm, channel-major output of the block's edge convolution, xs [B,Cs]
and g [B,Cg] the global vectors that are broadcast in front of it, scale / shift [C] the affine of the block's BatchNorm1d;
a = lrelu(scale*Y + shift) is written once, into both outputs, and its masked cotangent exists only inside the kernels.
Same conventions as spgan.ops: arguments validated, outputs from PyTorch's caching allocator, launches on the current stream."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import check
from .edge_max import tile_sums
from .ops import _f32, _p, _s, _vec

Tensor = torch.Tensor
SLOPE = 0.01


def _cm3(t: Tensor, name: str) -> Tuple[int, int, int]:
    _f32(t, name, 3)
    if not t.is_contiguous() or t.numel() == 0:
        raise ValueError("%s must be a non-empty contiguous [B,C,L] tensor, got %s with strides %s" % (name, tuple(t.shape), t.stride()))
    return tuple(t.shape)


def _rows(t: Optional[Tensor], B: int, name: str) -> int:
    """a global vector [B,Cn] (None: no such channels) -> Cn"""
    if t is None:
        return 0
    _f32(t, name, 2)
    if t.shape[0] != B or not t.is_contiguous():
        raise ValueError("%s must be contiguous [B,*] = [%d,*], got %s" % (name, B, tuple(t.shape)))
    return t.shape[1]


def _cot(t: Optional[Tensor], B: int, Ctot: int, L: int, name: str) -> Optional[Tensor]:
    if t is None:
        return None
    if _cm3(t, name) != (B, Ctot, L):
        raise ValueError("%s must be [%d,%d,%d], got %s" % (name, B, Ctot, L, tuple(t.shape)))
    return t


def cm_stats(Y: Tensor):
    """-> (partials [B,C,2], tile_rows = L): the (sum, centred M2) records of Y's rows, one per (b, c): what edge_conv.bn_stats takes as
    `records` with count = B*L."""
    B, C, L = _cm3(Y, "Y")
    part = torch.empty((B, C, 2), dtype=torch.float32, device=Y.device)
    check(_lib.load().spgan_cm_stats(_p(Y), B, C, L, _p(part), _s()), "cm_stats", B=B, C=C, L=L)
    return part, L


def block_tail_fwd(Y: Tensor, xs: Optional[Tensor], g: Optional[Tensor], scale: Tensor, shift: Tensor, slope: float = SLOPE,
                   want_x: bool = True, want_g: bool = True):
    """-> (out_x [B,Cs+C,L] = cat[xs broadcast, a] | None, out_g [B,Cg+C,L] = cat[g broadcast, a] | None), a = lrelu(scale*Y + shift)"""
    B, C, L = _cm3(Y, "Y")
    if not (want_x or want_g):
        raise ValueError("block_tail_fwd: at least one output must be wanted")
    Cs, Cg = _rows(xs, B, "xs") if want_x else 0, _rows(g, B, "g") if want_g else 0
    out_x = torch.empty((B, Cs + C, L), dtype=torch.float32, device=Y.device) if want_x else None
    out_g = torch.empty((B, Cg + C, L), dtype=torch.float32, device=Y.device) if want_g else None
    check(_lib.load().spgan_block_tail_fwd(_p(Y), _p(xs) if Cs else None, _p(g) if Cg else None, B, C, L, Cs, Cg, _p(_vec(scale, C, "scale")),
                                           _p(_vec(shift, C, "shift")), float(slope), _p(out_x), _p(out_g), _s()),
          "block_tail_fwd", B=B, C=C, L=L, Cs=Cs, Cg=Cg)
    return out_x, out_g


def _cots(Y: Tensor, dout_x, dout_g, extra, Cs: int, Cg: int):
    B, C, L = _cm3(Y, "Y")
    return B, C, L, _cot(dout_x, B, Cs + C, L, "dout_x"), _cot(dout_g, B, Cg + C, L, "dout_g"), _cot(extra, B, C, L, "extra")


def block_tail_bwd_reduce(Y: Tensor, dout_x: Optional[Tensor], dout_g: Optional[Tensor], extra: Optional[Tensor], Cs: int, Cg: int, scale: Tensor,
                          shift: Tensor, mean: Tensor, invstd: Tensor, slope: float = SLOPE, want_dxs: bool = True, want_dg: bool = True):
    """-> (sums [2C] = [sum gact | sum gact*yhat] over all B*L values of a channel, dxs [B,Cs] | None, dg [B,Cg] | None): gact = (dout_x's +
    dout_g's data channels + extra) * lrelu'; each of the three cotangents may be None.  dxs / dg are the row sums of the broadcast
    channels' cotangents (None where there are no such channels or the sums are not wanted: their rows are then not read; zeros where
    the cotangent is absent)."""
    B, C, L, dout_x, dout_g, extra = _cots(Y, dout_x, dout_g, extra, Cs, Cg)
    part = torch.empty((B, C, 2), dtype=torch.float32, device=Y.device)
    dxs = torch.empty((B, Cs), dtype=torch.float32, device=Y.device) if Cs and want_dxs else None
    dg = torch.empty((B, Cg), dtype=torch.float32, device=Y.device) if Cg and want_dg else None
    check(_lib.load().spgan_block_tail_bwd_reduce(_p(Y), _p(dout_x), _p(dout_g), _p(extra), B, C, L, Cs, Cg, _p(_vec(scale, C, "scale")),
                                                  _p(_vec(shift, C, "shift")), float(slope), _p(_vec(mean, C, "mean")),
                                                  _p(_vec(invstd, C, "invstd")), _p(part), _p(dxs), _p(dg), _s()),
          "block_tail_bwd_reduce", B=B, C=C, L=L, Cs=Cs, Cg=Cg)
    return tile_sums(part, B * L, L), dxs, dg


def block_tail_bwd_apply(Y: Tensor, dout_x: Optional[Tensor], dout_g: Optional[Tensor], extra: Optional[Tensor], Cs: int, Cg: int, scale: Tensor,
                         shift: Tensor, mean: Tensor, invstd: Tensor, gamma: Optional[Tensor], sums: Optional[Tensor], slope: float = SLOPE) -> Tensor:
    """-> dY [B,C,L].  sums [2C] (block_tail_bwd_reduce's): train mode, dY = gamma*invstd*(gact - sum/count - yhat*sum_yhat/count) with
    count = B*L; sums None: eval mode, dY = scale*gact."""
    B, C, L, dout_x, dout_g, extra = _cots(Y, dout_x, dout_g, extra, Cs, Cg)
    dY = torch.empty_like(Y)
    check(_lib.load().spgan_block_tail_bwd_apply(_p(Y), _p(dout_x), _p(dout_g), _p(extra), B, C, L, Cs, Cg, _p(_vec(scale, C, "scale")),
                                                 _p(_vec(shift, C, "shift")), float(slope), _p(_vec(mean, C, "mean")),
                                                 _p(_vec(invstd, C, "invstd")), _p(_vec(gamma, C, "gamma")),
                                                 _p(_vec(sums, 2 * C, "sums")), float(B * L), _p(dY), _s()),
          "block_tail_bwd_apply", B=B, C=C, L=L, Cs=Cs, Cg=Cg)
    return dY
