"""EdgeConv2's dT = dout . WoT formed inside its attention backward (csrc/edge_dt.hip).

The chain  dT = gemm_nt(dout, WoT) -> edge_attend_bwd(dT, ...)  writes the [M, k*F] tensor dT and reads it back once.  The fused launch
keeps dT in its MFMA accumulators.  Its bits are the chain's wherever the chain's product runs the 256 x 256-tile kernel (the k-order of
every accumulator, the per-element expressions and the records' summation order are the chain's); everywhere else -- EdgeConv1's F = 64,
the 16-bit and split-bf16 operand modes, CPU tensors, tile_hint 1, SPGAN_NT_WIDE=0 -- `usable` is False and nets.edgeblock_backward keeps
the chain.

The launchers bind the C entries directly (as adain_epi.py does) and are also reachable as ops.edge_attend_bwd_dt /
ops.edge_attend_bwd_dt_selected.  They are not defined in ops.py: every function of ops.py has a CPU model in tests/kernel_model.py, and
this launch has none -- its reference is the chain itself.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, ops
from ._lib import check
from .ops import _f32, _finalize, _i32, _ld, _p, _pqr, _rowmajor2d, _s, _vec

Tensor = torch.Tensor

# Module-level switch: False sends nets.edgeblock_backward back to the two-launch chain (tests and A/B runs compare the two routes).
ENABLED = [True]
# Fused launches issued through `backward` since import (tests assert the route through it, not through timing).
LAUNCHES = [0]


class route:
    """with edge_dt.route(False): ...   -- the chain instead of the fused launch inside the block."""

    def __init__(self, on: bool):
        self.on = bool(on)

    def __enter__(self):
        self.prev = ENABLED[0]
        ENABLED[0] = self.on

    def __exit__(self, *exc):
        ENABLED[0] = self.prev


def edge_attend_bwd_dt_selected(dout: Tensor, WoT: Tensor, k: int, F_: int) -> bool:
    """Would gemm_nt(dout, WoT) run the 256 x 256-tile kernel right now (operand mode, tile hint, sizes, alignment)?  Only then does
    edge_attend_bwd_dt give the bits of the chain gemm_nt -> edge_attend_bwd."""
    if not (dout.is_cuda and WoT.is_cuda) or dout.dtype != torch.float32 or WoT.dtype != torch.float32 or ops._MFMA_F16[0] != 0:
        return False
    if dout.dim() != 2 or WoT.dim() != 2 or dout.stride(1) != 1 or WoT.stride(1) != 1 or dout.shape[1] != F_ or tuple(WoT.shape) != (k * F_, F_):
        return False
    return bool(_lib.load().spgan_edge_attend_bwd_dt_selected(_p(dout), _ld(dout), _p(WoT), _ld(WoT), dout.shape[0], k, F_, ops._NT_TILE_HINT[0]))


def edge_attend_bwd_dt(dout: Tensor, WoT: Tensor, h2pre: Tensor, sc2, sh2, mean2, inv2, PQR: Tensor, idx: Tensor, bx, scx, shx, meanx, invx,
                       slope: float, _part_out: Optional[list] = None):
    """ops.edge_attend_bwd(ops.gemm_nt(dout, WoT), ...) in one launch: dT [M, k*F] stays in the kernel's accumulators.
    k = 10, F = 128, fp32 GPU tensors; the caller checks edge_attend_bwd_dt_selected for bit equality with the chain.
    -> (g2 [E,F], gy [E,F], sums2 [2F], sumsy [2F]); _part_out (a list) receives the raw per-tile records."""
    F_ = bx.numel()
    H = PQR.shape[1] - 2 * F_
    _pqr(PQR, H, F_); _i32(idx, "idx")
    M_, k = idx.shape
    _rowmajor2d(dout, "dout"); _rowmajor2d(WoT, "WoT"); _f32(h2pre, "h2pre", 2)
    if dout.shape != (M_, F_) or WoT.shape != (k * F_, F_) or not h2pre.is_contiguous() or h2pre.numel() != M_ * k * F_:
        raise ValueError("dout [M,F], WoT [k*F,F] and a contiguous h2pre with M*k*F elements expected")
    lib = _lib.load()
    tp = lib.spgan_edge_attend_bwd_tile_points()
    tiles = (M_ + tp - 1) // tp
    g2 = torch.empty((M_ * k, F_), dtype=torch.float32, device=PQR.device)
    gy = torch.empty((M_ * k, F_), dtype=torch.float32, device=PQR.device)
    part = torch.empty((tiles, 2 * F_, 2), dtype=torch.float32, device=PQR.device)
    v = lambda t, n: _p(_vec(t, F_, n))
    check(lib.spgan_edge_attend_bwd_dt(_p(dout), _ld(dout), _p(WoT), _ld(WoT), _p(h2pre), v(sc2, "sc2"), v(sh2, "sh2"), v(mean2, "mean2"),
                                       v(inv2, "inv2"), _p(PQR), PQR.shape[1], H, F_, _p(idx), M_, k, v(bx, "bx"), v(scx, "scx"), v(shx, "shx"),
                                       v(meanx, "meanx"), v(invx, "invx"), float(slope), _p(g2), _p(gy), _p(part), _s()),
          "edge_attend_bwd_dt", M=M_, k=k, F=F_)
    if _part_out is not None:
        _part_out.append(part)
    s0, s1 = _finalize(part, 1, tiles, 2 * F_, tiles * tp, 1, tp)
    return g2, gy, s0[0], s1[0]


ops.edge_attend_bwd_dt = edge_attend_bwd_dt
ops.edge_attend_bwd_dt_selected = edge_attend_bwd_dt_selected


def usable(dout: Tensor, WoT: Tensor, T: Tensor, h2pre: Tensor, PQR: Tensor, k: int, F_: int) -> bool:
    """Does the fused launch take this block's backward?  GPU fp32 tensors in the fp32 operand mode, k = 10, F = 128, and the chain's
    gemm_nt(dout, WoT) would run the 256 x 256-tile kernel (edge_attend_bwd_dt_selected: sizes, alignment, tile hint, SPGAN_NT_WIDE)."""
    if not ENABLED[0] or k != 10 or F_ != 128:
        return False
    for t in (dout, WoT, T, h2pre, PQR):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
            return False
    if not (h2pre.is_contiguous() and PQR.is_contiguous()):
        return False
    return edge_attend_bwd_dt_selected(dout, WoT, k, F_)


def backward(dout: Tensor, WoT: Tensor, h2pre: Tensor, sc2, sh2, mean2, inv2, PQR: Tensor, idx: Tensor, bx, scx, shx, meanx, invx, slope: float):
    """-> (g2, gy, sums2, sumsy): what ops.edge_attend_bwd(ops.gemm_nt(dout, WoT), ...) returns, bit for bit."""
    LAUNCHES[0] += 1
    return edge_attend_bwd_dt(dout, WoT, h2pre, sc2, sh2, mean2, inv2, PQR, idx, bx, scx, shx, meanx, invx, slope)
