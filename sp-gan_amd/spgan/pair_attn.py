"""PointTransformerLayer's all-pairs vector attention (the reference's Generation/modules.py:1602-1644) on csrc/pair_attn.hip.

With r_ij = relu(W_p1 (pos_i - pos_j) + b_p1) the attention MLP's pre-activation is Qa_i - Ka_j + Wc r_ij + c (Qa = q W_a1^T,
Ka = k W_a1^T, Wc = W_a1 W_p2, c = W_a1 b_p2 + b_a1) and sum_j a_ij e_ij = W_p2 R_i + b_p2 with R_i = sum_j a_ij r_ij: the pair
kernel contracts over H = pos_mlp_hidden_dim only and never forms e_ij.  Everything per point is a gemm_nt /
gemm_tn call with exact fp32 operands: the layer does not follow ops.set_mfma_operands.

The launchers below mirror the C ABI one to one; PairAttnFn is the once-differentiable autograd Function behind
spgan.PointTransformerLayer.  Nothing here synchronises with the host.
"""
from __future__ import annotations

from typing import Dict

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib, ops
from ._lib import check
from .edge_conv import cached_images, refuse_double_backward
from .ops import _p, _s

Tensor = torch.Tensor
_IMAGES: Dict[tuple, tuple] = {}


def padded_sizes(dim: int, H: int, mult: int):
    """(Mp, Hp): the padded row count of the attention MLP's hidden layer and of the position MLP's; raises ValueError outside the domain."""
    lib = _lib.load()
    Mp = lib.spgan_pair_attn_padded_m(dim * mult) if dim >= 1 and mult >= 1 else 0
    Hp = lib.spgan_pair_attn_padded_h(H)
    if Mp == 0 or Hp == 0 or dim > lib.spgan_pair_attn_max_dim():
        raise ValueError("PointTransformerLayer(dim=%d, pos_mlp_hidden_dim=%d, attn_mlp_hidden_mult=%d): the pair kernel serves 1 <= dim <= %d, "
                         "1 <= pos_mlp_hidden_dim <= 64 and 1 <= dim * attn_mlp_hidden_mult <= 4096"
                         % (dim, H, mult, lib.spgan_pair_attn_max_dim()))
    return Mp, Hp


def images(Wp1: Tensor, bp1: Tensor, Wp2: Tensor, bp2: Tensor, Wa1: Tensor, ba1: Tensor, Wa2: Tensor, Wqkv: Tensor):
    """The zero-padded operand images, cached on the parameters' versions (edge_conv.cached_images; rebuilt inside a stream capture):
    (Wp1p [Hp,4] = (W_p1 | b_p1), Wa1p [Mp,D], Wa1p^T, Wp2p [D,Hp], Wp2p^T, Wc [Mp,Hp], Wc^T, c [Mp], w_a2 [Mp], W_p1^T [3,Hp], Wqkv^T)."""
    def build(Wp1, bp1, Wp2, bp2, Wa1, ba1, Wa2, Wqkv):
        M, D = Wa1.shape
        H = Wp1.shape[0]
        Mp, Hp = padded_sizes(D, H, M // D)
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=Wa1.device)
        Wp1p = z(Hp, 4); Wp1p[:H, :3] = Wp1; Wp1p[:H, 3] = bp1
        Wa1p = z(Mp, D); Wa1p[:M] = Wa1
        Wp2p = z(D, Hp); Wp2p[:, :H] = Wp2
        Wp2pT = Wp2p.t().contiguous()
        Wc = ops.gemm_nt(Wa1p, Wp2pT, exact=True)
        cvec = z(Mp); cvec[:M] = torch.mv(Wa1, bp2) + ba1
        wa2 = z(Mp); wa2[:M] = Wa2.reshape(-1)
        return (Wp1p, Wa1p, Wa1p.t().contiguous(), Wp2p, Wp2pT, Wc, Wc.t().contiguous(), cvec, wa2, Wp1p[:, :3].t().contiguous(),
                Wqkv.t().contiguous())
    return cached_images(_IMAGES, (Wp1, bp1, Wp2, bp2, Wa1, ba1, Wa2, Wqkv), (), build)


def _sizes(pos: Tensor, QaC: Tensor, Wc: Tensor):
    b, n = pos.shape[0], pos.shape[1]
    Mp, Hp = Wc.shape
    if tuple(pos.shape) != (b, n, 3) or tuple(QaC.shape) != (b * n, Mp):
        raise ValueError("pair_attn: pos %s, QaC %s and Wc %s disagree" % (tuple(pos.shape), tuple(QaC.shape), tuple(Wc.shape)))
    return b, n, Mp, Hp


def _c(t: Tensor, name: str) -> Tensor:
    ops._f32(t, name)
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def pair_attn_fwd(pos: Tensor, Wp1p: Tensor, QaC: Tensor, Ka: Tensor, Wc: Tensor, wa2: Tensor, v: Tensor):
    """-> (Sv [b*n,D] = sum_j a_ij v_j, R [b*n,Hp] = sum_j a_ij r_ij, lse [b*n]); v [b*n,D] may be a column slice."""
    b, n, Mp, Hp = _sizes(pos, QaC, Wc)
    ops._rowmajor2d(v, "v")
    D = v.shape[1]
    for t, nm in ((pos, "pos"), (Wp1p, "Wp1p"), (QaC, "QaC"), (Ka, "Ka"), (Wc, "Wc"), (wa2, "wa2")):
        _c(t, nm)
    Sv = torch.empty((b * n, D), dtype=torch.float32, device=pos.device)
    R = torch.empty((b * n, Hp), dtype=torch.float32, device=pos.device)
    lse = torch.empty((b * n,), dtype=torch.float32, device=pos.device)
    check(_lib.load().spgan_pair_attn_fwd(_p(pos), _p(Wp1p), _p(QaC), _p(Ka), _p(Wc), _p(wa2), _p(v), ops._ld(v), b, n, D, Mp, Hp, None,
                                          _p(Sv), _p(R), _p(lse), None, _s()), "pair_attn_fwd", b=b, n=n, D=D, Mp=Mp, Hp=Hp)
    return Sv, R, lse


def pair_attn_probs(pos: Tensor, Wp1p: Tensor, QaC: Tensor, Ka: Tensor, Wc: Tensor, wa2: Tensor, lse: Tensor) -> Tensor:
    """P [b,n,n] = exp(sim - lse): the attention weights, recomputed for the backward (a scalar per pair; held only there)."""
    b, n, Mp, Hp = _sizes(pos, QaC, Wc)
    for t, nm in ((pos, "pos"), (Wp1p, "Wp1p"), (QaC, "QaC"), (Ka, "Ka"), (Wc, "Wc"), (wa2, "wa2"), (lse, "lse")):
        _c(t, nm)
    P = torch.empty((b, n, n), dtype=torch.float32, device=pos.device)
    check(_lib.load().spgan_pair_attn_fwd(_p(pos), _p(Wp1p), _p(QaC), _p(Ka), _p(Wc), _p(wa2), None, 0, b, n, 1, Mp, Hp, _p(lse),
                                          None, None, None, _p(P), _s()), "pair_attn_fwd(P)", b=b, n=n, Mp=Mp, Hp=Hp)
    return P


def pair_attn_dsim(P: Tensor, dout: Tensor, v: Tensor, dR: Tensor, pos: Tensor, Wp1p: Tensor) -> Tensor:
    """dS [b,n,n] = P_ij (g_ij - delta_i), g_ij = dout_i . v_j + dR_i . r_ij, delta_i = sum_j P_ij g_ij / sum_j P_ij.  dout . v is one
    batched GEMM into dS; the launch adds the r term and applies the softmax Jacobian in place."""
    b, n = P.shape[0], P.shape[1]
    ops._rowmajor2d(v, "v")
    D, Hp = v.shape[1], dR.shape[1]
    for t, nm in ((P, "P"), (dout, "dout"), (dR, "dR"), (pos, "pos"), (Wp1p, "Wp1p")):
        _c(t, nm)
    dS = torch.empty_like(P)
    ops.gemm_nt_batched(dout.view(b, n, D), v.as_strided((b, n, D), (n * v.stride(0), v.stride(0), 1)), out=dS, exact=True)
    check(_lib.load().spgan_pair_attn_dsim(_p(P), _p(dR), _p(pos), _p(Wp1p), b, n, Hp, _p(dS), _s()), "pair_attn_dsim", b=b, n=n, D=D, Hp=Hp)
    return dS


def pair_attn_bwd(role: int, pos: Tensor, Wp1p: Tensor, QaC: Tensor, Ka: Tensor, Wc: Tensor, WcT: Tensor, wa2: Tensor, P: Tensor,
                  dS: Tensor, dR: Tensor):
    """role 0 -> (dQa [b*n,Mp], Zq [groups,b*n,Hp], records [R, Mp*Hp + Mp]); role 1 -> (dKa, Zk [groups,b*n,Hp], None).  Z's groups
    (one per 128 rows of Wc) and the records (partial dWc | dw_a2 per workgroup) are summed by the caller in ascending order."""
    b, n, Mp, Hp = _sizes(pos, QaC, Wc)
    for t, nm in ((pos, "pos"), (Wp1p, "Wp1p"), (QaC, "QaC"), (Ka, "Ka"), (Wc, "Wc"), (WcT, "WcT"), (wa2, "wa2"), (P, "P"), (dS, "dS"), (dR, "dR")):
        _c(t, nm)
    lib = _lib.load()
    dA = torch.empty((b * n, Mp), dtype=torch.float32, device=pos.device)
    Z = torch.empty((Mp // 128, b * n, Hp), dtype=torch.float32, device=pos.device)
    ws, wsb = None, 0
    if role == 0:
        wsb = lib.spgan_pair_attn_bwd_ws_bytes(b, n, Mp, Hp)
        ws = torch.empty((lib.spgan_pair_attn_bwd_records(b, n), Mp * Hp + Mp), dtype=torch.float32, device=pos.device)
    check(lib.spgan_pair_attn_bwd(role, _p(pos), _p(Wp1p), _p(QaC), _p(Ka), _p(Wc), _p(WcT), _p(wa2), _p(P), _p(dS), _p(dR), b, n, Mp, Hp,
                                  _p(dA), _p(Z), _p(ws), wsb, _s()), "pair_attn_bwd", role=role, b=b, n=n, Mp=Mp, Hp=Hp)
    return dA, Z, ws


def _fold(parts: Tensor) -> Tensor:
    """[parts, ...] -> the sum over parts in ascending order"""
    return parts[0] if parts.shape[0] == 1 else ops.reduce_chunks(parts.reshape(parts.shape[0], -1)).view(parts.shape[1:])


class PairAttnFn(Function):
    """out [b,n,dim] of PointTransformerLayer for x [b,n,dim], pos [b,n,3] and the parameters in the reference's order (to_qkv.weight,
    pos_mlp.0.weight / bias, pos_mlp.2.weight / bias, attn_mlp.0.weight / bias, attn_mlp.2.weight / bias).  Saved for the backward:
    qkv, Qa + c, Ka, R and the log-sum-exp per query -- per-point tensors only.  The backward holds two [b,n,n] scalar
    matrices (the attention weights P and dsim) and no per-pair vector."""

    @staticmethod
    def forward(ctx, x, pos, Wqkv, Wp1, bp1, Wp2, bp2, Wa1, ba1, Wa2, ba2):
        b, n, D = x.shape
        x2 = x.reshape(b * n, D).contiguous()
        pos3 = pos.contiguous()
        Wp1p, Wa1p, _, Wp2p, _, Wc, _, cvec, wa2, _, _ = images(Wp1, bp1, Wp2, bp2, Wa1, ba1, Wa2, Wqkv)
        # exact=True: fp32 operands whatever ops.set_mfma_operands selected
        qkv = ops.gemm_nt(x2, Wqkv, exact=True)
        QaC = ops.gemm_nt(qkv[:, :D], Wa1p, cvec, exact=True)
        Ka = ops.gemm_nt(qkv[:, D:2 * D], Wa1p, exact=True)
        Sv, R, lse = pair_attn_fwd(pos3, Wp1p, QaC, Ka, Wc, wa2, qkv[:, 2 * D:])
        out = ops.gemm_nt(R, Wp2p, bp2, exact=True)
        ops.axpby(1.0, Sv, 1.0, out)                                 # out = Sv + R W_p2^T + b_p2
        ctx.save_for_backward(x2, pos3, qkv, QaC, Ka, R, lse, Wqkv, Wp1, bp1, Wp2, bp2, Wa1, ba1, Wa2)
        return out.view(b, n, D)

    @staticmethod
    def backward(ctx, dout):
        refuse_double_backward("PointTransformerLayer")
        return PairAttnFn._backward(ctx, dout)

    @staticmethod
    @once_differentiable
    def _backward(ctx, dout):
        x2, pos3, qkv, QaC, Ka, R, lse, Wqkv, Wp1, bp1, Wp2, bp2, Wa1, ba1, Wa2 = ctx.saved_tensors
        b, n = pos3.shape[0], pos3.shape[1]
        D, H, M = x2.shape[1], Wp1.shape[0], Wa1.shape[0]
        Wp1p, Wa1p, Wa1pT, Wp2p, Wp2pT, Wc, WcT, _, wa2, Wp1T, WqkvT = images(Wp1, bp1, Wp2, bp2, Wa1, ba1, Wa2, Wqkv)
        Mp, Hp = Wc.shape
        need = ctx.needs_input_grad
        g = dout.reshape(b * n, D).contiguous()
        v = qkv[:, 2 * D:]
        dR = ops.gemm_nt(g, Wp2pT, exact=True)                       # dR_i = W_p2^T dout_i
        P = pair_attn_probs(pos3, Wp1p, QaC, Ka, Wc, wa2, lse)
        dS = pair_attn_dsim(P, g, v, dR, pos3, Wp1p)
        dqkv = torch.empty_like(qkv)
        for z in range(b):                                           # dv_j = sum_i a_ij dout_i
            ops.gemm_tn(P[z], g[z * n:(z + 1) * n], out=dqkv[z * n:(z + 1) * n, 2 * D:], exact=True)
        dQa, Zq, rec = pair_attn_bwd(0, pos3, Wp1p, QaC, Ka, Wc, WcT, wa2, P, dS, dR)
        dKa, Zk, _ = pair_attn_bwd(1, pos3, Wp1p, QaC, Ka, Wc, WcT, wa2, P, dS, dR)
        del P, dS
        Zq, Zk, rec = _fold(Zq), _fold(Zk), _fold(rec)
        dWc, dwa2 = rec[:Mp * Hp].view(Mp, Hp), rec[Mp * Hp:]
        ops.gemm_nt(dQa, Wa1pT, out=dqkv[:, :D], exact=True)
        ops.gemm_nt(dKa, Wa1pT, out=dqkv[:, D:2 * D], exact=True)
        dx = ops.gemm_nt(dqkv, WqkvT, exact=True).view(b, n, D) if need[0] else None
        Zd = Zq - Zk                                                 # dpos_i = W_p1^T (sum_j dz_ij - sum_j dz_ji)
        dpos = ops.gemm_nt(Zd, Wp1T, exact=True).view(b, n, 3) if need[1] else None
        dWqkv = ops.gemm_tn(dqkv, x2, exact=True) if need[2] else None
        dWp1 = ops.gemm_tn(Zd, pos3.view(b * n, 3), exact=True)[:H].contiguous() if need[3] else None
        dbp1 = ops.colsum(Zq)[0, :H].contiguous() if need[4] else None
        dWp2 = None
        if need[5]:                                                  # dout^T R + W_a1^T dWc
            dWp2 = (ops.gemm_tn(g, R, exact=True) + ops.gemm_tn(Wa1p, dWc.contiguous(), exact=True))[:, :H].contiguous()
        dc = ops.colsum(dQa)[0]                                      # c enters every query's pre-activation
        dbp2 = ops.colsum(g)[0] + torch.mv(Wa1.t(), dc[:M]) if need[6] else None      # directly, and through c = W_a1 b_p2 + b_a1
        dWa1 = None
        if need[7]:                                                  # through Qa, Ka, Wc = W_a1 W_p2 and c = W_a1 b_p2 + b_a1
            dWa1 = ops.gemm_tn(dQa, qkv[:, :D], exact=True)
            ops.gemm_tn(dKa, qkv[:, D:2 * D], out=dWa1, beta=1.0, exact=True)
            dWa1 = (dWa1 + ops.gemm_nt(dWc.contiguous(), Wp2p, exact=True) + torch.outer(dc, bp2))[:M].contiguous()
        dba1 = dc[:M].contiguous() if need[8] else None
        dWa2 = dwa2[:M].reshape(1, M).contiguous() if need[9] else None
        dba2 = torch.zeros_like(ba1[:1]) if need[10] else None      # b_a2 cancels in the softmax
        return dx, dpos, dWqkv, dWp1, dbp1, dWp2, dbp2, dWa1, dba1, dWa2, dba2


def point_transformer(x: Tensor, pos: Tensor, Wqkv, Wp1, bp1, Wp2, bp2, Wa1, ba1, Wa2, ba2) -> Tensor:
    return PairAttnFn.apply(x, pos, Wqkv, Wp1, bp1, Wp2, bp2, Wa1, ba1, Wa2, ba2)
