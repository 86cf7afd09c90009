"""AdaptivePointNorm inside the epilogue of its style GEMM (SPGAN_EPI_ADAIN of spgan_gemm_nt; csrc/adain_epi.hpp).

The chain  gb = gemm_nt(style, Ws, bs) -> colstats(x) -> adain_fwd(x, gb)  writes the per-point [M,2C] tensor [gamma|beta] and reads it back
for one fmaf per element.  Here the GEMM's epilogue applies the normalisation to its accumulators: [M,2C] never reaches memory, gamma is
stored only for the rows whose backward needs it, and the per-tile (max, arg-max) records of the output replace a max-pool pass over it.
The bits are those of the chain: the k-order of every accumulator and the epilogue's expressions are the chain's.

The launchers bind the C entries directly (as edge_conv.py / pair_attn.py do); GPU tensors only -- on CPU tensors (the host-composition
tests) `usable` is False and the callers in nets.py keep the chain.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib, ops
from ._lib import GemmNTArgs, check
from .ops import BN_EPS, EPI_LINEAR, ROW_TILE, _ld, _p, _s

Tensor = torch.Tensor
EPI_ADAIN = 4
assert EPI_ADAIN not in (EPI_LINEAR, ops.EPI_MASK_OUT, ops.EPI_BNBWD, ops.EPI_EDGE_BNBWD)

# Module-level switch: False sends every caller back to the three-launch chain (tests compare the two routes).
ENABLED = [True]


class route:
    """with adain_epi.route(False): ...   -- the chain instead of the fused launch inside the block."""

    def __init__(self, on: bool):
        self.on = bool(on)

    def __enter__(self):
        self.prev = ENABLED[0]
        ENABLED[0] = self.on

    def __exit__(self, *exc):
        ENABLED[0] = self.prev


def _al16(t: Tensor) -> bool:
    return t.data_ptr() % 16 == 0


def usable(x: Tensor, style: Tensor, Ws: Tensor, N: int) -> bool:
    """Does the fused launch take this layer?  fp32 operand mode, GPU tensors, C % 32 == 0, 16-byte aligned rows with K % 4 == 0, more
    than 64 rows.  x is [M,C] or the one [N,C] block every shape shares."""
    if not ENABLED[0] or not (x.is_cuda and style.is_cuda and Ws.is_cuda) or ops._MFMA_F16[0] != 0:
        return False
    if x.dim() != 2 or style.dim() != 2 or Ws.dim() != 2 or x.dtype != torch.float32 or style.dtype != torch.float32 or Ws.dtype != torch.float32:
        return False
    M, K = style.shape
    Cn = x.shape[1]
    if Ws.shape != (2 * Cn, K) or Cn % 32 or K % 4 or M <= 64 or N <= 0 or M % N or x.shape[0] not in (M, N):
        return False
    if style.stride(1) != 1 or Ws.stride(1) != 1 or x.stride(1) != 1:
        return False
    return _ld(style) % 4 == 0 and _ld(Ws) % 4 == 0 and _al16(style) and _al16(Ws)


def can_pool(M: int, N: int) -> bool:
    """Pooling records need whole 128-row tiles inside one shape."""
    return N % ROW_TILE == 0 and M % ROW_TILE == 0


def shared_stats(x_one: Tensor, slope: float, shapes: int) -> Tuple[Tensor, Tensor]:
    """Instance statistics of `shapes` identical copies of the block x_one [N,C], taken from the one copy: ops.colstats' launches on N rows
    and one broadcast copy -> (imean, ivar), each [shapes, C] contiguous.  Identical rows give identical statistics: the bits are those of
    colstats on the materialised copies."""
    N, Cn = x_one.shape
    lib = _lib.load()
    wsb = lib.spgan_colreduce_ws_bytes(N, Cn, N)
    ws = torch.empty((wsb // 4,), dtype=torch.float32, device=x_one.device)
    one = torch.empty((2, 1, Cn), dtype=torch.float32, device=x_one.device)
    check(lib.spgan_colstats(_p(x_one), _ld(x_one), N, Cn, N, float(slope), _p(one[0]), _p(one[1]), _p(ws), wsb, _s()), "colstats", M=N, C=Cn, G=N)
    st = one.expand(2, shapes, Cn).contiguous()
    return st[0], st[1]


def forward(x: Tensor, style: Tensor, Ws: Tensor, bs: Optional[Tensor], N: int, slope: float, imean: Tensor, ivar: Tensor, *,
            gamma_row0: Optional[int] = None, pool: bool = False):
    """out[m,c] = fmaf(gamma, xhat, beta) with [gamma|beta] = style @ Ws^T + bs and xhat = (lrelu(x, slope) - imean[b,c]) * rsqrt(ivar[b,c] + eps).
    x [M,C], or [N,C]: the block every shape reads (per-shape stride 0).  imean / ivar [M/N, C] contiguous.
    gamma_row0 = r: gamma alone is kept for the rows r.. -> [M - r, C] (None: not kept).  pool: also the per-tile records of out.
    -> (out [M,C], gamma | None, (pool_val, pool_arg) | None)"""
    M, K = style.shape
    Cn = x.shape[1]
    B = M // N
    dev = style.device
    out = torch.empty((M, Cn), dtype=torch.float32, device=dev)
    a = GemmNTArgs(); a.mfma_f16 = 0; a.tile_hint = ops._NT_TILE_HINT[0]
    a.A = _p(style); a.lda = _ld(style); a.W = _p(Ws); a.ldw = _ld(Ws); a.Y = _p(out); a.ldy = Cn
    a.M, a.N, a.K = M, 2 * Cn, K
    a.a_mode = ops.A_PLAIN; a.epi_mode = EPI_ADAIN
    a.bias = _p(ops._vec(bs, 2 * Cn, "bias"))
    a.ad_x = _p(x); a.ad_ldx = _ld(x); a.ad_x_shape_stride = 0 if (x.shape[0] == N and B > 1) else N * _ld(x); a.ad_rows = N
    a.ad_mean = _p(ops._vec(imean, B * Cn, "imean")); a.ad_var = _p(ops._vec(ivar, B * Cn, "ivar"))
    a.ad_eps = BN_EPS; a.ad_slope = float(slope)
    gamma = None
    if gamma_row0 is not None:
        if not 0 <= gamma_row0 < M:
            raise ValueError("gamma_row0 must lie in [0, M)")
        gamma = torch.empty((M - gamma_row0, Cn), dtype=torch.float32, device=dev)
        a.ad_gamma = _p(gamma); a.ad_ld_gamma = Cn; a.ad_gamma_row0 = gamma_row0
    rec = None
    if pool:
        if not can_pool(M, N):
            raise ValueError("pooling records need N %% %d == 0" % ROW_TILE)
        tiles = M // ROW_TILE
        rec = (torch.empty((tiles, Cn, 2), dtype=torch.float32, device=dev), torch.empty((tiles, Cn, 2), dtype=torch.int32, device=dev))
        a.pool_val = _p(rec[0]); a.pool_arg = _p(rec[1])
    done = ops.launch_timer("gemm_nt", a) if ops.launch_timer is not None else None
    check(_lib.load().spgan_gemm_nt(C.byref(a), _s()), "gemm_nt(adain)", M=M, C=Cn, K=K, N=N)
    if done is not None:
        done()
    return out, gamma, rec


_ONES = {}


def _unit(G: int, Cn: int, device) -> Tuple[Tensor, Tensor]:
    key = (G, Cn, str(device))
    if key not in _ONES:
        _ONES[key] = (torch.ones((G, Cn), dtype=torch.float32, device=device), torch.zeros((G, Cn), dtype=torch.float32, device=device))
    return _ONES[key]


def pool_from_records(rec, shapes: int, N: int, groups: int = 1) -> Tuple[Tensor, Tensor]:
    """Max over each shape's N rows from the records of `forward(pool=True)` -> (pooled [shapes, C], argmax int32 [shapes, C]): what
    ops.maxpool gives on the rows of each of the `groups` equal row blocks (the arg-max counts rows from its block's first row).
    One launch for all shapes; first row on ties."""
    pval, parg = rec
    Cn = pval.shape[1]
    one, zero = _unit(groups, Cn, pval.device)
    pooled = torch.empty((shapes, Cn), dtype=torch.float32, device=pval.device)
    arg = torch.empty((shapes, Cn), dtype=torch.int32, device=pval.device)
    check(_lib.load().spgan_pool_finalize_groups(_p(pval), _p(parg), shapes, N, Cn, _p(one), _p(zero), Cn, shapes // groups, 1.0, _p(pooled), _p(arg),
                                                 None, 1, _s()), "pool_finalize", B=shapes, rows=N, C=Cn)
    return pooled, arg


def backward(dout: Tensor, x: Tensor, N: int, slope: float, imean: Tensor, ivar: Tensor, gamma: Tensor) -> Tuple[Tensor, Tensor]:
    """ops.adain_bwd with the gamma-only tensor [M,C] of `forward(gamma_row0=...)` in place of gb [M,2C], and x either [M,C] or the one
    [N,C] block every shape shares.  -> (dx [M,C], dgb [M,2C])"""
    M, Cn = dout.shape
    if not (dout.is_contiguous() and x.is_contiguous() and gamma.is_contiguous()) or gamma.shape != dout.shape or x.shape[0] not in (M, N):
        raise ValueError("dout / gamma [M,C] and x [M,C] or [N,C] must be contiguous")
    B = M // N
    xs = 0 if (x.shape[0] == N and B > 1) else N * Cn
    tpg = (N + ROW_TILE - 1) // ROW_TILE
    dgb = torch.empty((M, 2 * Cn), dtype=torch.float32, device=dout.device)
    part = torch.empty((B * tpg, Cn, 2), dtype=torch.float32, device=dout.device)
    lib = _lib.load()
    check(lib.spgan_adain_bwd1(_p(dout), _p(x), M, Cn, N, float(slope), _p(imean), _p(ivar), BN_EPS, _p(gamma), Cn, xs, _p(dgb), _p(part), _s()),
          "adain_bwd1")
    S0, S1 = ops._finalize(part, B, tpg, Cn, N, 1)
    dx = torch.empty((M, Cn), dtype=torch.float32, device=dout.device)
    check(lib.spgan_adain_bwd2(_p(dout), _p(x), M, Cn, N, float(slope), _p(imean), _p(ivar), BN_EPS, _p(gamma), Cn, xs, _p(S0), _p(S1), _p(dx), _s()),
          "adain_bwd2")
    return dx, dgb
