"""Tensor-level wrappers of the dense layers' launchers (csrc/edge_dense.hip; include/spgan_hip.h): the passes behind
`spgan.DenseEdgeModule` and `spgan.DenseModule1D` (edge_conv.DenseEdgeFn / DenseRowsFn).  The operand of a level is the virtual
concatenation of stored pre-norm blocks -- column slices of one wide buffer -- each activated while it is staged; the result goes into
another slice of the same buffer.  Same conventions as spgan.ops: arguments validated, outputs from PyTorch's caching allocator, launches
on the current stream.  Exact fp32 MFMA products: they do not follow ops.set_mfma_operands."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import check
from .ops import _i32, _ld, _p, _rowmajor2d, _s, _vec

Tensor = torch.Tensor


def tile_rows() -> int:
    return _lib.load().spgan_edge_dense_tile_rows()


def _overlap(A: Tensor, K: int, Y: Tensor) -> bool:
    """do the K columns read from A and the columns written to Y share an address?  (both are column slices with a row stride)"""
    if K == 0 or A.untyped_storage().data_ptr() != Y.untyped_storage().data_ptr():
        return False
    if _ld(A) != _ld(Y):
        return True                                                   # two different views of one storage: not a pair of column slices
    a0, y0 = A.storage_offset() % _ld(A), Y.storage_offset() % _ld(Y)
    return a0 < y0 + Y.shape[1] and y0 < a0 + K


def edge_dense_level(A: Optional[Tensor], W: Optional[Tensor], out: Tensor, *, raw_cols: Optional[int] = None, scale: Optional[Tensor] = None,
                     shift: Optional[Tensor] = None, slope: float = 0.2, bias: Optional[Tensor] = None,
                     addend: Optional[Tuple[Tensor, Tensor, Tensor]] = None, stats: bool = False):
    """out [M,N] = op(A) @ W^T (+ bias) (+ Q[m // k] + P[idx[m]]); out is written in place and returned (-> (out, partials, tile_rows) with
    stats=True: the (sum, M2) records edge_max.edge_max_bn finalises).
    A [M,K] and out may be column slices of one buffer (unit column stride, any row stride) as long as the columns do not overlap.
    op: columns below raw_cols as stored, the others lrelu(a * scale[c] + shift[c], slope) with scale, shift [K] (raw_cols=None: K, all
    raw).  addend = (P, Q, idx): P, Q [M/k, N] column slices of one per-point buffer (P in front), idx int32 [M/k, k] rows of it.
    A = W = None: the addend / bias alone (a gather into a slice)."""
    _rowmajor2d(out, "out")
    M_, N = out.shape
    K = 0
    if A is not None:
        _rowmajor2d(A, "A"); _rowmajor2d(W, "W")
        K = A.shape[1]
        if A.shape[0] != M_ or tuple(W.shape) != (N, K):
            raise ValueError("edge_dense_level: A %s, W %s and out %s do not fit" % (tuple(A.shape), tuple(W.shape), tuple(out.shape)))
        if _overlap(A, K, out):
            raise ValueError("edge_dense_level: out overlaps the columns read from A")
    elif addend is None and bias is None:
        raise ValueError("edge_dense_level: nothing to compute (no A, no addend, no bias)")
    raw = K if raw_cols is None else int(raw_cols)
    if not 0 <= raw <= K:
        raise ValueError("edge_dense_level: raw_cols must lie in 0..K=%d, got %d" % (K, raw))
    if raw < K and (scale is None or shift is None):
        raise ValueError("edge_dense_level: activated columns need scale and shift")
    P = idx = None
    k, ldpq, qoff = 1, 0, 0
    if addend is not None:
        P, Q, idx = addend
        _rowmajor2d(P, "P"); _rowmajor2d(Q, "Q"); _i32(idx, "idx")
        k = idx.shape[1]
        ldpq, qoff = _ld(P), (Q.data_ptr() - P.data_ptr()) // 4
        if (tuple(P.shape) != (idx.shape[0], N) or P.shape != Q.shape or idx.shape[0] * k != M_ or _ld(Q) != ldpq
                or P.untyped_storage().data_ptr() != Q.untyped_storage().data_ptr() or qoff < N or qoff + N > ldpq):
            raise ValueError("edge_dense_level: addend P %s / Q %s must be column slices [M/k, N] of one buffer, P first, with idx %s"
                             % (tuple(P.shape), tuple(Q.shape), tuple(idx.shape)))
    lib = _lib.load()
    part = None
    if stats:
        part = torch.empty(((M_ + tile_rows() - 1) // tile_rows(), N, 2), dtype=torch.float32, device=out.device)
    check(lib.spgan_edge_dense_level(_p(A), _ld(A) if A is not None else 0, raw, _p(_vec(scale, K, "scale")), _p(_vec(shift, K, "shift")),
                                     float(slope), _p(W), _ld(W) if W is not None else 0, _p(_vec(bias, N, "bias")), _p(P), ldpq, qoff, _p(idx), k,
                                     M_, N, K, _p(out), _ld(out), _p(part), _s()), "edge_dense_level", M=M_, N=N, K=K)
    return (out, part, tile_rows()) if stats else out


def edge_dense_scatter(D: Tensor, rowptr: Tensor, src: Tensor, k: int) -> Tensor:
    """D [M*k, C] on the edges (a column slice is fine) -> dPQ [M, 2C] = [dP | dQ]: dQ = the sum over a point's k rows, dP = the sum over
    its in-edge list (ops.csr_build), in ascending edge order"""
    _rowmajor2d(D, "D"); _i32(rowptr, "rowptr"); _i32(src, "src")
    E, C = D.shape
    if k < 1 or E % k or rowptr.numel() != E // k + 1 or src.numel() != E:
        raise ValueError("edge_dense_scatter: rowptr [M+1] / src [M*k] do not fit D %s with k=%d" % (tuple(D.shape), k))
    M_ = E // k
    dPQ = torch.empty((M_, 2 * C), dtype=torch.float32, device=D.device)
    check(_lib.load().spgan_edge_dense_scatter(_p(D), _ld(D), _p(rowptr), _p(src), M_, k, C, _p(dPQ), 2 * C, _s()), "edge_dense_scatter",
          M=M_, k=k, C=C)
    return dPQ


def edge_dense_bn_apply(g: Tensor, z: Tensor, mean: Tensor, invstd: Tensor, gamma: Optional[Tensor], sums: Tensor, count: int, out: Tensor) -> Tensor:
    """ops.bn_bwd_apply over column slices: out = gamma*invstd*(g - sum_g/count - xhat(z)*sum_gx/count), written in place and returned"""
    _rowmajor2d(g, "g"); _rowmajor2d(z, "z"); _rowmajor2d(out, "out")
    if g.shape != z.shape or g.shape != out.shape:
        raise ValueError("edge_dense_bn_apply: g, z and out must have equal shapes")
    if out.data_ptr() == g.data_ptr() or out.data_ptr() == z.data_ptr():
        raise ValueError("edge_dense_bn_apply: out must not alias g or z")
    M_, C = g.shape
    check(_lib.load().spgan_edge_dense_bn_apply(_p(g), _ld(g), _p(z), _ld(z), M_, C, _p(_vec(mean, C, "mean")), _p(_vec(invstd, C, "invstd")),
                                                _p(_vec(gamma, C, "gamma")), _p(_vec(sums, 2 * C, "sums")), int(count), _p(out), _ld(out), _s()),
          "edge_dense_bn_apply", M=M_, C=C)
    return out
