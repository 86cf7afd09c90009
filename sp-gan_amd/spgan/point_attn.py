"""Dot-product self-attention over the points of a shape on csrc/point_attn.hip: the core behind spgan.Self_Attn
(the reference's Common/utilities.py:210-245) and Attention(ch, materialize=False) (Generation/modules.py:534-558).

    S_ij = q_i . k_j (unscaled),  P = softmax_j(S),  O_i = sum_j P_ij v_j,  lse_i = log sum_j exp(S_ij)

Nothing of size [B,N,N] is written: the forward keeps O and lse, the backward recomputes P tile by tile in a query-stationary launch (dQ)
and a key-stationary one (dK, dV).  The launchers mirror the C ABI one to one and take [B*N, d] row-major operands whose row stride may
exceed the width, so that slices of one projected tensor are passed as they are.  Nothing here synchronises with the host.
"""
from __future__ import annotations

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib, ops
from ._lib import check
from .edge_conv import refuse_double_backward
from .ops import _p, _s

Tensor = torch.Tensor


def padded_dk(dk: int) -> int:
    """dk rounded up to the kernels' multiple of 4 (the host pads with zero columns: S is unchanged); ValueError outside 1..128."""
    r = _lib.load().spgan_point_attn_padded_dk(int(dk))
    if r == 0:
        raise ValueError("point attention: the query / key width must be in 1..128, got %d" % dk)
    return r


def padded_dv(dv: int) -> int:
    """dv rounded up to a multiple of 4; ValueError outside 1..spgan_point_attn_max_dv()."""
    mx = _lib.load().spgan_point_attn_max_dv()
    if dv < 1 or dv > mx:
        raise ValueError("point attention: the value width must be in 1..%d, got %d" % (mx, dv))
    return (int(dv) + 3) // 4 * 4


def _op(t: Tensor, name: str, rows: int, width=None) -> Tensor:
    ops._rowmajor2d(t, name)
    if t.shape[0] != rows or (width is not None and t.shape[1] != width):
        raise ValueError("%s must be [%d,%s], got %s" % (name, rows, "%d" % width if width is not None else "d", tuple(t.shape)))
    if t.shape[1] % 4 or ops._ld(t) % 4 or t.data_ptr() % 16:
        raise ValueError("%s: width %d and row stride %d must be multiples of 4 and the base 16-byte aligned (pad on the host: padded_dk)"
                         % (name, t.shape[1], ops._ld(t)))
    return t


def _dims(q: Tensor, v: Tensor, b: int, n: int):
    if b < 1 or n < 1:
        raise ValueError("point attention needs b >= 1 and n >= 1, got b=%d n=%d" % (b, n))
    dk, dv = q.shape[1], v.shape[1]
    if dk > 128 or dv > _lib.load().spgan_point_attn_max_dv():
        raise ValueError("point attention serves dk <= 128 and dv <= %d, got dk=%d dv=%d" % (_lib.load().spgan_point_attn_max_dv(), dk, dv))
    return dk, dv


def point_attn_fwd(q: Tensor, k: Tensor, v: Tensor, b: int, n: int):
    """q, k [b*n,dk], v [b*n,dv] (column slices allowed) -> (o [b*n,dv], lse [b*n])"""
    _op(q, "q", b * n); _op(k, "k", b * n, q.shape[1]); _op(v, "v", b * n)
    dk, dv = _dims(q, v, b, n)
    o = torch.empty((b * n, dv), dtype=torch.float32, device=q.device)
    lse = torch.empty((b * n,), dtype=torch.float32, device=q.device)
    check(_lib.load().spgan_point_attn_fwd(_p(q), ops._ld(q), _p(k), ops._ld(k), _p(v), ops._ld(v), b, n, dk, dv, _p(o), ops._ld(o), _p(lse),
                                           _s()), "point_attn_fwd", b=b, n=n, dk=dk, dv=dv)
    return o, lse


def point_attn_bwd(q: Tensor, k: Tensor, v: Tensor, do: Tensor, lse: Tensor, b: int, n: int, dq: Tensor = None,
                   dk_out: Tensor = None, dv_out: Tensor = None):
    """Both roles, in order -> (dq [b*n,dk], dk [b*n,dk], dv [b*n,dv]); the three destinations may be column slices of one buffer."""
    rows = b * n
    _op(q, "q", rows); _op(k, "k", rows, q.shape[1]); _op(v, "v", rows)
    dk, dv = _dims(q, v, b, n)
    _op(do, "do", rows, dv)
    ops._f32(lse, "lse", 1)
    if lse.numel() != rows or not lse.is_contiguous():
        raise ValueError("lse must be a contiguous [%d] vector" % rows)
    new = lambda w: torch.empty((rows, w), dtype=torch.float32, device=q.device)
    dq = _op(new(dk) if dq is None else dq, "dq", rows, dk)
    dk_out = _op(new(dk) if dk_out is None else dk_out, "dk", rows, dk)
    dv_out = _op(new(dv) if dv_out is None else dv_out, "dv", rows, dv)
    D = torch.empty_like(lse)
    lib = _lib.load()
    for role in (0, 1):
        check(lib.spgan_point_attn_bwd(role, _p(q), ops._ld(q), _p(k), ops._ld(k), _p(v), ops._ld(v), _p(do), ops._ld(do),
                                       _p(lse), _p(D), b, n, dk, dv, _p(dq), ops._ld(dq), _p(dk_out), ops._ld(dk_out), _p(dv_out),
                                       ops._ld(dv_out), _s()), "point_attn_bwd", role=role, b=b, n=n, dk=dk, dv=dv)
    return dq, dk_out, dv_out


def _pad_cols(t: Tensor, w: int) -> Tensor:
    return t if t.shape[-1] == w else torch.nn.functional.pad(t, (0, w - t.shape[-1]))


class PointAttnFn(Function):
    """point_attention's autograd node.  Saved: q, k, v (padded) and lse -- O(B N (dk + dv))."""

    @staticmethod
    def forward(ctx, q, k, v):
        for t, nm in ((q, "q"), (k, "k"), (v, "v")):
            ops._f32(t, nm, 3)
        b, n, dk = q.shape
        if tuple(k.shape) != (b, n, dk) or tuple(v.shape[:2]) != (b, n):
            raise ValueError("point_attention: q %s, k %s and v %s disagree" % (tuple(q.shape), tuple(k.shape), tuple(v.shape)))
        if b < 1 or n < 1:
            raise ValueError("point_attention needs b >= 1 and n >= 1")
        dv = v.shape[2]
        dkp, dvp = padded_dk(dk), padded_dv(dv)
        q2 = _pad_cols(q, dkp).reshape(b * n, dkp).contiguous()
        k2 = _pad_cols(k, dkp).reshape(b * n, dkp).contiguous()
        v2 = _pad_cols(v, dvp).reshape(b * n, dvp).contiguous()
        o, lse = point_attn_fwd(q2, k2, v2, b, n)
        ctx.save_for_backward(q2, k2, v2, lse)
        ctx.dims = (b, n, dk, dv)
        return o[:, :dv].reshape(b, n, dv)

    @staticmethod
    def backward(ctx, do):
        refuse_double_backward("point_attention")
        return PointAttnFn._backward(ctx, do)

    @staticmethod
    @once_differentiable
    def _backward(ctx, do):
        q2, k2, v2, lse = ctx.saved_tensors
        b, n, dk, dv = ctx.dims
        do2 = _pad_cols(do, v2.shape[1]).reshape(b * n, v2.shape[1]).contiguous()
        dq, dkk, dvv = point_attn_bwd(q2, k2, v2, do2, lse, b, n)
        return dq[:, :dk].reshape(b, n, dk), dkk[:, :dk].reshape(b, n, dk), dvv[:, :dv].reshape(b, n, dv)


def point_attention(q: Tensor, k: Tensor, v: Tensor) -> Tensor:
    """softmax_j(q_i . k_j) v_j per shape: q, k [B,N,dk], v [B,N,dv] float32 on the GPU -> [B,N,dv].  dk <= 128, dv <= 512 (ValueError), float32
    (TypeError), GPU tensors (RuntimeError).  Differentiable once in all three; create_graph=True raises RuntimeError."""
    return PointAttnFn.apply(q, k, v)


# ---------------------------------------------------------------------------------------------------------------------------------
# The projected form shared by the two modules: one stacked projection [q | k | v], the core on its column slices, one stacked backward.
def stacked_weight(Wq: Tensor, Wk: Tensor, Wv: Tensor):
    """([2 dkp + dvp, C] = the three projection weights, each zero-padded to its kernel width, (dk, dkp, dv, dvp))"""
    dk, dv = Wq.shape[0], Wv.shape[0]
    dkp, dvp = padded_dk(dk), padded_dv(dv)
    C = Wq.shape[1]
    W = torch.zeros((2 * dkp + dvp, C), dtype=torch.float32, device=Wq.device)
    W[:dk] = Wq.reshape(dk, C); W[dkp:dkp + dk] = Wk.reshape(dk, C); W[2 * dkp:2 * dkp + dv] = Wv.reshape(dv, C)
    return W, (dk, dkp, dv, dvp)


def stacked_bias(bq: Tensor, bk: Tensor, bv: Tensor, dims):
    dk, dkp, dv, dvp = dims
    bias = torch.zeros((2 * dkp + dvp,), dtype=torch.float32, device=bq.device)
    bias[:dk] = bq; bias[dkp:dkp + dk] = bk; bias[2 * dkp:2 * dkp + dv] = bv
    return bias


def projected_forward(x: Tensor, W: Tensor, bias, dims, B: int, N: int):
    """x [B*N,C] -> (o [B*N,dvp], cat = x W^T + bias [B*N, 2 dkp + dvp] = [q | k | v], lse [B*N])"""
    dk, dkp, dv, dvp = dims
    cat = ops.gemm_nt(x, W, bias)
    o, lse = point_attn_fwd(cat[:, :dkp], cat[:, dkp:2 * dkp], cat[:, 2 * dkp:], B, N)
    return o, cat, lse


def projected_backward(cat: Tensor, lse: Tensor, d_o: Tensor, dims, B: int, N: int) -> Tensor:
    """d_o [B*N,dvp] -> dcat [B*N, 2 dkp + dvp] = [dq | dk | dv], written by the two backward launches in place"""
    dk, dkp, dv, dvp = dims
    dcat = torch.empty_like(cat)
    point_attn_bwd(cat[:, :dkp], cat[:, dkp:2 * dkp], cat[:, 2 * dkp:], d_o, lse, B, N, dq=dcat[:, :dkp], dk_out=dcat[:, dkp:2 * dkp],
                   dv_out=dcat[:, 2 * dkp:])
    return dcat


class SelfAttnFn(Function):
    """spgan.Self_Attn on point-major rows: x [B*N,C], then query / key / value weights and biases and gamma (the module's order).
    In the reference softmax(query_key, 1) normalises over the FIRST point index and bmm(value, attn) sums over it:
    out_j = sum_i softmax_i(query_i . key_j) value_i -- the core's q is the `key` projection and its k the `query` projection."""

    @staticmethod
    def forward(ctx, holder, x, Wq, bq, Wk, bk, Wv, bv, gamma):
        from . import functions as Fn
        Fn._record_modes(ctx, holder)
        x = x.contiguous()
        W, dims = stacked_weight(Wk, Wq, Wv)                    # core q <- key, core k <- query
        bias = stacked_bias(bk, bq, bv, dims)
        o, cat, lse = projected_forward(x, W, bias, dims, holder.B, holder.N)
        dv = dims[2]
        ov = o if o.shape[1] == dv else o[:, :dv].contiguous()
        y = ops.scale_residual(ov, x, gamma)
        ctx.save_for_backward(x, cat, ov, lse, W, gamma, Wq, bq, Wk, bk, Wv, bv)
        ctx.dims, ctx.BN = dims, (holder.B, holder.N)
        return y

    @staticmethod
    def backward(ctx, dy):
        refuse_double_backward("Self_Attn")
        return SelfAttnFn._backward(ctx, dy)

    @staticmethod
    @once_differentiable
    def _backward(ctx, dy):
        from . import functions as Fn
        x, cat, ov, lse, W, gamma, Wq, bq, Wk, bk, Wv, bv = ctx.saved_tensors
        dk, dkp, dv, dvp = ctx.dims
        B, N = ctx.BN
        dy = dy.contiguous()
        d_o, dgamma = ops.scale_residual_bwd(dy, ov, gamma)
        dcat = projected_backward(cat, lse, _pad_cols(d_o, dvp), ctx.dims, B, N)
        dW = ops.gemm_tn(dcat, x)
        db = ops.colsum(dcat)[0]
        dx = None
        if ctx.needs_input_grad[1]:
            dx = ops.gemm_nt(dcat, W.t().contiguous())
            ops.multi_add([dx], [dy])
        lo = {"k": 0, "q": dkp, "v": 2 * dkp}                   # rows of the stacked weight: (key, query, value)
        # query.bias adds bq . key_j to every score of column j, which the softmax over i cancels: its gradient is an exact zero
        grads = [dW[lo["q"]:lo["q"] + dk].reshape(Wq.shape), torch.zeros_like(bq),
                 dW[lo["k"]:lo["k"] + dk].reshape(Wk.shape), db[lo["k"]:lo["k"] + dk].contiguous(),
                 dW[lo["v"]:lo["v"] + dv].reshape(Wv.shape), db[lo["v"]:lo["v"] + dv].contiguous(), dgamma.reshape(gamma.shape)]
        return (None, dx) + Fn._deliver((Wq, bq, Wk, bk, Wv, bv, gamma), grads, ctx.needs_input_grad[2:], ctx.fused)


SA2_SLOPE = 0.2


class SelfAttn2Fn(Function):
    """spgan.Self_Attn2 (Common/utilities.py:247-290) on point-major rows: x [B*N,C], then (conv weight, conv bias, bn weight, bn bias) of
    query, key and value and gamma.  Each projection is Conv1d -> BatchNorm1d -> LeakyReLU(0.2); the softmax runs over the first point
    index as in Self_Attn, so the activated `key` is the core's q and the activated `query` its k.  One stacked product
    [key | query | value] with its column statistics, one finalise per BatchNorm (running statistics advanced in the order query, key,
    value), one activation pass, the core, the residual.  holder: B, N, training, bns = (query, key, value)'s BatchNorm1d."""

    @staticmethod
    def forward(ctx, holder, x, Wq, bq, gq, eq, Wk, bk, gk, ek, Wv, bv, gv, ev, gamma):
        from . import functions as Fn
        from .edge_conv import bn_stats
        Fn._record_modes(ctx, holder)
        h = holder
        x = x.contiguous()
        M = x.shape[0]
        W, dims = stacked_weight(Wk, Wq, Wv)                    # core q <- key, core k <- query
        dk, dkp, dv, dvp = dims
        bias = stacked_bias(bk, bq, bv, dims)
        if h.training:
            cat, mean, var = ops.gemm_nt(x, W, bias, stats=True, exact=True)
        else:
            cat, mean, var = ops.gemm_nt(x, W, bias, exact=True), None, None
        lo = {"k": 0, "q": dkp, "v": 2 * dkp}
        width = {"k": dk, "q": dk, "v": dv}
        ST = torch.zeros((4, W.shape[0]), dtype=torch.float32, device=x.device)       # (scale, shift, invstd, mean); padding columns stay 0
        GA = torch.zeros((W.shape[0],), dtype=torch.float32, device=x.device)
        for name, bn, g_, e_ in (("q", h.bns[0], gq, eq), ("k", h.bns[1], gk, ek), ("v", h.bns[2], gv, ev)):
            a, b_ = lo[name], lo[name] + width[name]
            mom = None if mean is None else (mean[a:b_].contiguous(), var[a:b_].contiguous())
            ST[:, a:b_] = bn_stats(bn, h.training, M, g_.detach(), e_.detach(), moments=mom)
            GA[a:b_] = g_.detach()
        act = ops.affine_act(cat, ST[0], ST[1], SA2_SLOPE)
        o, lse = point_attn_fwd(act[:, :dkp], act[:, dkp:2 * dkp], act[:, 2 * dkp:], h.B, h.N)
        ov = o if o.shape[1] == dv else o[:, :dv].contiguous()
        y = ops.scale_residual(ov, x, gamma)
        ctx.save_for_backward(x, cat, act, ov, lse, W, ST, GA, gamma, Wq, bq, gq, eq, Wk, bk, gk, ek, Wv, bv, gv, ev)
        ctx.dims, ctx.h = dims, h
        return y

    @staticmethod
    def backward(ctx, dy):
        refuse_double_backward("Self_Attn2")
        return SelfAttn2Fn._backward(ctx, dy)

    @staticmethod
    @once_differentiable
    def _backward(ctx, dy):
        from . import edge_dense, pointnet_util
        from . import functions as Fn
        from .edge_conv import used
        x, cat, act, ov, lse, W, ST, GA, gamma, *prm = ctx.saved_tensors
        Wq, bq, gq, eq, Wk, bk, gk, ek, Wv, bv, gv, ev = prm
        dk, dkp, dv, dvp = ctx.dims
        h = ctx.h
        M, Wt = cat.shape
        dy = dy.contiguous()
        d_o, dgamma = ops.scale_residual_bwd(dy, ov, gamma)
        dact = projected_backward(act, lse, _pad_cols(d_o, dvp), ctx.dims, h.B, h.N)
        # LeakyReLU and BatchNorm of all three projections at once: the mask from the activated value, the two column sums, then dz
        r, sums = pointnet_util._group_max_bwd(dact, act, None, cat, ST[3], ST[2], SA2_SLOPE, 1)
        dz = torch.empty_like(cat)
        edge_dense.edge_dense_bn_apply(r, cat, ST[3], ST[2], GA, used(sums, h.training), M, dz)
        del r, dact
        dW = ops.gemm_tn(dz, x, exact=True)
        db = None if h.training else ops.colsum(dz)[0]
        dx = None
        if ctx.needs_input_grad[1]:
            dx = ops.gemm_nt(dz, W.t().contiguous(), exact=True)
            ops.multi_add([dx], [dy])
        lo = {"k": 0, "q": dkp, "v": 2 * dkp}
        grads = []
        for name, Wp, bp, f in (("q", Wq, bq, dk), ("k", Wk, bk, dk), ("v", Wv, bv, dv)):
            a, b_ = lo[name], lo[name] + f
            # a conv bias in front of a train-mode BatchNorm: the batch mean absorbs it, an exact zero
            grads += [dW[a:b_].reshape(Wp.shape), 0 if db is None else db[a:b_].contiguous(), sums[Wt + a:Wt + b_].contiguous(),
                      sums[a:b_].contiguous()]
        grads.append(dgamma.reshape(gamma.shape))
        return (None, dx) + Fn._deliver(tuple(prm) + (gamma,), grads, ctx.needs_input_grad[2:], ctx.fused)
