"""Plain-PyTorch models of every op in spgan.ops (TEST INFRASTRUCTURE ONLY).

Two uses:
  * `-m gpu` tests compare each HIP kernel against its model on the same inputs;
  * `-m "not gpu"` tests monkeypatch `spgan.ops` with these models to check the *host
    composition* (forward/backward/double-backward pipelines in spgan.nets) against the
    oracle on the CPU.  The product never imports this file.
Signatures mirror spgan/ops.py one to one.
"""
import math
from typing import Optional

import torch
import torch.nn.functional as F

ACT_NONE, ACT_LRELU, ACT_TANH = 0, 1, 2
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def _lrelu(x, s):
    return torch.where(x > 0, x, x * s)


# ----------------------------------------------------------------------------- graph
def knn(x_pm, B, N, k, mode=0):
    C = x_pm.shape[1]
    x = x_pm.view(B, N, C)
    if mode == 1:
        xd = x.double()
        d = ((xd[:, :, None, :] - xd[:, None, :, :]) ** 2).sum(-1)
    else:
        inner = torch.bmm(x, x.transpose(1, 2))
        sq = (x * x).sum(-1)
        d = (-2 * inner + sq[:, :, None]) + sq[:, None, :]
    order = torch.sort(d, dim=2, stable=True)[1][:, :, 1:k + 1]
    off = (torch.arange(B, device=x_pm.device) * N).view(B, 1, 1)
    return (order + off).reshape(B * N, k).to(torch.int32)


def csr_build(idx, B, N):
    M, k = idx.shape
    flat = idx.reshape(-1).long()
    order = torch.sort(flat, stable=True)[1]          # edge ids grouped by target, ascending within a target
    deg = torch.bincount(flat, minlength=M)
    rowptr = torch.zeros(M + 1, dtype=torch.int64, device=idx.device)
    rowptr[1:] = torch.cumsum(deg, 0)
    return rowptr.to(torch.int32), order.to(torch.int32)


def edge_features_cm(x_cm, idx_local, k):
    B, C, N = x_cm.shape
    idx3 = idx_local.view(B, 1, N * k).expand(B, C, N * k)
    nb = torch.gather(x_cm, 2, idx3).view(B, C, N, k)
    ctr = x_cm.unsqueeze(3).expand(B, C, N, k)
    return torch.cat([ctr, nb - ctr], dim=1).contiguous()


def edge_features_cm_bwd(dE, idx_local, k):
    """adjoint of edge_features_cm w.r.t. x (modules.py:708-720): central + '-central' + in-edge scatter."""
    B, C2, N, _ = dE.shape
    C = C2 // 2
    dc, dd = dE[:, :C], dE[:, C:]
    dx = dc.sum(3) - dd.sum(3)
    idx3 = idx_local.view(B, 1, N * k).expand(B, C, N * k)
    return dx.scatter_add(2, idx3, dd.reshape(B, C, N * k)).contiguous()


def idx_to_local64(idx, B, N):
    k = idx.shape[1]
    off = (torch.arange(B, device=idx.device) * N).view(B, 1)
    return (idx.view(B, N * k).long() - off).contiguous()


def idx_from_local64(idx_local, B, N, k):
    off = (torch.arange(B, device=idx_local.device) * N).view(B, 1)
    return (idx_local.view(B, N * k) + off).view(B * N, k).to(torch.int32)


# ----------------------------------------------------------------------------- layout
def cm_to_pm(x_cm):
    B, C, N = x_cm.shape
    return x_cm.permute(0, 2, 1).reshape(B * N, C).contiguous()


def pm_to_cm(x_pm, B, N):
    return x_pm.view(B, N, -1).permute(0, 2, 1).contiguous()


def concat2(a, b):
    return torch.cat([a, b], dim=1).contiguous()


# ----------------------------------------------------------------------------- contractions
def _operand(A, pro, edge, K):
    if edge is not None:
        idx, ebias = edge
        k = idx.shape[1]
        i = torch.arange(idx.shape[0], device=A.device).repeat_interleave(k)
        j = idx.reshape(-1).long()
        a = (A[j, :K] - A[i, :K]) + ebias
    else:
        a = A[:, :K]
    if pro is not None:
        sc, sh, ps = pro
        a = _lrelu(a * sc + sh, ps)
    return a


def gemm_nt(A, W, bias=None, *, pro=None, edge=None, rowbias=None, rows_per_group=0, act=ACT_NONE, slope=0.0, stats=False, M=None, bn=None,
            out=None, exact=False, count_rep=1, out_bf16=False, out_half=False):
    if out_bf16:     # bfloat16 storage of the result (ops.gemm_nt(out_bf16=True))
        return gemm_nt(A, W, bias, pro=pro, edge=edge, rowbias=rowbias, rows_per_group=rows_per_group, M=M).to(torch.bfloat16)
    if out_half:     # float16 storage of the result; statistics / bn from the unrounded values
        r = gemm_nt(A, W, bias, pro=pro, edge=edge, rowbias=rowbias, rows_per_group=rows_per_group, stats=stats, M=M, bn=bn, count_rep=count_rep)
        return (r[0].half(),) + tuple(r[1:]) if isinstance(r, tuple) else r.half()
    if isinstance(A, torch.Tensor) and A.dtype == torch.float16:   # float16-stored operand
        A = A.float()
    if out is not None:
        out.copy_(gemm_nt(A, W, bias, pro=pro, edge=edge, rowbias=rowbias, rows_per_group=rows_per_group, act=act, slope=slope, M=M))
        return out
    if bn is not None:
        y, mean, var = gemm_nt(A, W, bias, pro=pro, edge=edge, rowbias=rowbias, rows_per_group=rows_per_group, act=act, slope=slope, stats=True, M=M)
        gamma, beta, rm, rv = bn
        return y, bn_prepare(mean, var, gamma, beta, y.shape[0] * count_rep, True, rm, rv)
    N, K = W.shape
    A = _dense(A)
    a = _operand(A, pro, edge, K)
    if M is not None:
        a = a[:M]
    y = a @ W.t()
    if bias is not None:
        y = y + bias
    if rowbias is not None:
        y = y + rowbias.repeat_interleave(rows_per_group, dim=0)[:y.shape[0]]
    pre = y
    if act == ACT_LRELU:
        y = _lrelu(y, slope)
    elif act == ACT_TANH:
        y = torch.tanh(y)
    if stats:
        return y.contiguous(), pre.mean(0), pre.var(0, unbiased=False)
    return y.contiguous()


def gemm_nt_batched(A, W, out=None):
    y = torch.bmm(A, W.transpose(1, 2))
    if out is None:
        return y.contiguous()
    out.copy_(y)
    return out


def gemm_nt_maskout(A, W, ref, slope, with_colsum=False):
    y = ((A @ W.t()) * torch.where(ref > 0, 1.0, slope)).contiguous()
    return (y, y.sum(0)) if with_colsum else y


class SparseAffine:
    def __init__(self, y, alpha, beta, sp_val, sp_arg, rows):
        self.y, self.alpha, self.beta, self.sp_val, self.sp_arg, self.rows = y, alpha, beta, sp_val, sp_arg, rows
        self.device = sp_val.device


def sparse_bn_bwd_operand(gval, argmax, y, N, mean, invstd, gamma, sums, count):
    C = gval.shape[1]
    coef = gamma * invstd
    alpha = -(coef * invstd) * (sums[C:] / count)
    beta = -(coef * (sums[:C] / count)) - alpha * mean
    return SparseAffine(y, alpha, beta, gval * coef, argmax, N)


def bn_dbl_coeffs(U0, U1, Ugz, S0, S1, gamma, invstd, count):
    core = Ugz - (U0 * S0 + U1 * S1) / count
    gsM = gamma * invstd / count
    return torch.stack([invstd * core, gamma * core, -gsM * (U0 * S1 + S0 * U1), -2.0 * gsM * (U1 * S1)])


def bn_dbl_phaseb(coeffs, gamma, invstd, s0, s1):
    if isinstance(coeffs, tuple):
        U0, U1, Ugz, S0, S1, count = coeffs
        coeffs = bn_dbl_coeffs(U0, U1, Ugz, S0, S1, gamma, invstd, count)
    a0 = s0 if s0 is not None else torch.zeros_like(gamma)
    a1 = s1 if s1 is not None else torch.zeros_like(gamma)
    return torch.cat([coeffs[2] + gamma * a0, coeffs[3] + gamma * a1 + invstd * coeffs[1]]), coeffs[0] + a1


class Affine2:
    def __init__(self, g, y, coef):
        self.g, self.y, self.coef = g, y, coef
        self.p, self.q, self.r = coef[0], coef[1], coef[2]
        self.shape, self.device = g.shape, g.device

    def dense(self):
        return self.g.float() * self.p + (self.y.float() * self.q + self.r)      # .float(): the 16-bit storage mode hands g / y over as bfloat16 / float16


def bn_bwd_lazy(g, y, mean, invstd, gamma, sums, count):
    C = g.shape[1]
    p = (gamma if gamma is not None else torch.ones_like(invstd)) * invstd
    q = -(p * invstd) * (sums[C:] / count)
    r = -(p * (sums[:C] / count)) - q * mean
    return Affine2(g, y, torch.stack([p, q, r]))


def _dense(A):
    if isinstance(A, Affine2):
        return A.dense()
    if isinstance(A, SparseAffine):
        return A.y * A.alpha + A.beta + scatter_rows(A.sp_val, A.sp_arg, A.y.shape[0])
    return A


def gemm_nt_bnbwd(A, W, y_ref, scale, shift, mean, invstd, slope, edge=None, pro=None, bias=None, rowadd=None, coef_bn=None, phaseb=None, gout=None):
    A = _dense(A)
    if pro is not None:
        A = _lrelu(A * pro[0] + pro[1], pro[2])
    N = W.shape[0]
    if edge is not None:
        idx, ebias = edge
        k = idx.shape[1]
        i = torch.arange(idx.shape[0], device=A.device).repeat_interleave(k)
        y = (y_ref[idx.reshape(-1).long(), :N] - y_ref[i, :N]) + ebias
    else:
        y = y_ref[:, :N]
    z = y * scale + shift
    acc = A @ W.t()
    if bias is not None:
        acc = acc + bias
    if rowadd is not None:
        acc = acc + rowadd
    g = acc * torch.where(z > 0, 1.0, slope)
    xh = (y - mean) * invstd
    if coef_bn is not None:
        s0, s1 = g.sum(0), (g * xh).sum(0)
        return g.contiguous(), s0, s1, bn_bwd_lazy(g, y, mean, invstd, coef_bn[0], torch.cat([s0, s1]), coef_bn[1]).coef
    s0, s1 = g.sum(0), (g * xh).sum(0)
    tail = ()
    if phaseb is not None:
        co, pg, pinv = phaseb[:3]
        sums, dgam = bn_dbl_phaseb(co, pg, pinv, s0, s1)
        tail = (sums, dgam)
        if len(phaseb) == 4:       # coefficients of p*X + q*y + r = pinv*(X - S0/M - xhat*S1/M)
            C_, rM = pinv.numel(), 1.0 / co[5]
            q_ = -(pinv * pinv) * (sums[C_:] * rM)
            tail = tail + (torch.stack([pinv, q_, -(pinv * (sums[:C_] * rM)) - q_ * phaseb[3]]),)
    if gout is not None:
        g = gout[0] + gout[1] * g
    return (g.contiguous(), s0, s1) + tail


def _sparse_dense(val, arg, rows):
    """S [B*rows, Cs] with S[arg[b,c], c] = val[b,c]."""
    B, Cs = val.shape
    S = torch.zeros((B * rows, Cs), dtype=val.dtype, device=val.device)
    S[arg.long().reshape(-1), torch.arange(Cs, device=val.device).repeat(B)] = val.reshape(-1)
    return S


def wgrad_collapse_ok(W, X1, B=0):
    return W.shape[0] % 32 == 0 and X1.shape[0] % 32 == 0 and W.shape[1] % 32 == 0 and 32 <= W.shape[1] <= 256 and B <= 64


def wgrad_collapse(W, X1, a1, b1=None, d1=None, v1=None, *, X2=None, x2_t=False, a2=None, sparse=None, out=None, accumulate=False, want_T=False):
    T = W @ X1.t()
    o = a1[:, None] * T
    if v1 is not None:
        o = o + (a1 * b1 + d1)[:, None] * v1[None, :]
    if X2 is not None:
        o = o + a2[:, None] * (W @ (X2 if x2_t else X2.t()))
    if sparse is not None:
        val, arg, rows, Bm, pro = sparse
        add = torch.zeros_like(o)
        sparse_rows_tn(val, arg, rows, Bm, add, pro=pro)
        o = o + add
    if out is None:
        out = o.contiguous()
    else:
        out.copy_(out + o if accumulate else o)
    return (out, T.contiguous()) if want_T else out


def collapse_prep(W, problems, val, arg, rows):
    outs = [wt_diag_w(W, al) if be is None else wt_diag_w(W, al, be, bi) for al, be, bi in problems]
    if isinstance(val, (list, tuple)):
        return outs, [sparse_rows_nt(v, a, rows, W) for v, a in zip(val, arg)]
    return outs, sparse_rows_nt(val, arg, rows, W)


def sparse_rows_nt(val, arg, rows, W):
    return (_sparse_dense(val, arg, rows) @ W).contiguous()


def sparse_rows_tn(val, arg, rows, Bm, out, pro=None):
    b = Bm if pro is None else _lrelu(Bm * pro[0] + pro[1], pro[2])
    out += _sparse_dense(val, arg, rows).t() @ b
    return out


def gather_rowdot(Q, arg, W):
    B, C = arg.shape
    return (Q[arg.long().reshape(-1)] * W.repeat(B, 1)).sum(1).view(B, C).contiguous()


def dbl_top_dots(Q, arg, W, T, cq):
    return gather_rowdot(Q, arg, W), rowdot(W, T), W @ cq


def rowdot(X, Y):
    return (X * Y).sum(1)


def bn_dbl_pool(uarg, gval, yarg, pooled, U0, quad, bias, mean, invstd, gamma, S0, S1, count, slope):
    rM = 1.0 / count
    U1 = invstd * (quad + (bias - mean) * U0)
    Ugz = (gval * uarg).sum(0)
    core = Ugz - (U0 * S0 + U1 * S1) * rM
    gsM = gamma * invstd * rM
    sbarA = gamma * core
    sum0 = -gsM * (U0 * S1 + S0 * U1)
    sum1 = -2.0 * gsM * (U1 * S1) + invstd * sbarA
    out4 = torch.stack([invstd * core, -gsM * invstd * S1, -invstd * invstd * sum1 * rM, -invstd * sum0 * rM + invstd * invstd * mean * sum1 * rM])
    xh = (yarg - mean) * invstd
    t = gamma * invstd * (uarg - U0 * rM - xh * (U1 * rM)) * torch.where(pooled > 0, 1.0, slope)
    spB = (-gsM * invstd * U1) * gval
    return t.contiguous(), spB.contiguous(), out4.contiguous()


def multi_transpose(srcs):
    return [w.t().contiguous() for w in srcs]


def softmax_rows(S):
    S.copy_(torch.softmax(S, -1))
    return S


def softmax_rows_bwd(P, dP):
    dP.copy_(P * (dP - (dP * P).sum(-1, keepdim=True)))
    return dP


def scale_residual(o, x, gamma):
    return gamma * o + x


def scale_residual_bwd(dy, o, gamma):
    return gamma * dy, (dy * o).sum()


def affine_act(X, scale, shift, slope):
    return _lrelu(X * scale + shift, slope).contiguous()


def rowscale_outer(X, a, b=None, d=None, v=None, out=None, accumulate=False):
    o = a[:, None] * X
    if v is not None:
        o = o + (a * b + d)[:, None] * v[None, :]
    if out is None:
        return o.contiguous()
    out.copy_(out + o if accumulate else o)
    return out


def flush_tn():
    pass


def gemm_tn(A, Bm, *, pro=None, edge=None, out=None, beta=0.0, defer=False, exact=False, with_colsum=False, a_pro=None):
    A = _dense(A)
    if a_pro is not None:
        A = _lrelu(A * a_pro[0] + a_pro[1], a_pro[2])
    if Bm.dtype == torch.float16:      # float16-stored operand
        Bm = Bm.float()
    b = _operand(Bm, pro, edge, Bm.shape[1])
    c = A.t() @ b
    if out is None:
        res = c.contiguous()
    else:
        out.copy_(beta * out + c if beta != 0 else c)          # beta == 0: the destination is not read (it may be uninitialised)
        res = out
    return (res, A.sum(0)) if with_colsum else res


# ----------------------------------------------------------------------------- reductions / norms
def colstats(X, G, slope=1.0):
    M, C = X.shape
    v = _lrelu(X, slope).reshape(M // G, G, C)
    return v.mean(1), v.var(1, unbiased=False)


def colsum(X, G=None):
    M, C = X.shape
    G = M if G is None else G
    return X.reshape(M // G, G, C).sum(1)


def bn_prepare(mean, var, gamma, beta, count, training=True, running_mean=None, running_var=None, momentum=None, eps=BN_EPS):
    if momentum is None:
        from spgan import ops as _ops
        momentum = _ops._BN_MOM[0]                       # ops.bn_momentum(...) contexts apply to the doubles as they do to the kernels
    if training:
        m, v = mean, var.clamp(min=0)
        if running_mean is not None:
            unb = v * (count / (count - 1)) if count > 1 else v
            running_mean.mul_(1 - momentum).add_(momentum * m)
            running_var.mul_(1 - momentum).add_(momentum * unb)
    else:
        m, v = running_mean, running_var
    inv = 1.0 / torch.sqrt(v + eps)
    g = gamma if gamma is not None else torch.ones_like(inv)
    b = beta if beta is not None else torch.zeros_like(inv)
    sc = g * inv
    return sc, b - m * sc, inv, m.clone()


def bn_bwd_apply(g, y, mean, invstd, gamma, sums, count, add=None):
    if add is not None:
        g = g + add[1] * add[0]
    C = g.shape[1]
    xh = (y - mean) * invstd
    ga = gamma if gamma is not None else torch.ones_like(mean)
    return (ga * invstd * (g - sums[:C] / count - xh * (sums[C:] / count))).contiguous()


def maxpool(y, B, N, scale=None, shift=None, slope=1.0):
    C = y.shape[1]
    v = y
    if scale is not None:
        v = v * scale + shift
    v = _lrelu(v, slope).reshape(B, N, C)
    out, arg = v.max(1)
    off = (torch.arange(B, device=y.device) * N).view(B, 1)
    return out.contiguous(), (arg + off).to(torch.int32)


# ----------------------------------------------------------------------------- EdgeBlock gather-side ops
def edge_wcat(Ww0, Wx, transposed=False):
    C = Ww0.shape[1]
    out = torch.cat([Ww0, Wx[:, C:], Wx[:, :C] - Wx[:, C:]], dim=0).contiguous()
    return (out, out.t().contiguous()) if transposed else out


def conv_out_weight_pm(w):
    F_, _, _, k = w.shape
    wo = w[:, :, 0, :].permute(0, 2, 1).reshape(F_, k * F_).contiguous()
    return wo, wo.t().contiguous()


def edge_wcat_bwd(dWcat, H, F_):
    dq, dr = dWcat[H:H + F_], dWcat[H + F_:]
    return dWcat[:H].contiguous(), torch.cat([dr, dq - dr], dim=1).contiguous()


def _edges(idx):
    M, k = idx.shape
    i = torch.arange(M, device=idx.device).repeat_interleave(k)
    return i, idx.reshape(-1).long()


def _edge_pre(PQR, idx, b1, bx):
    H, F_ = b1.numel(), bx.numel()
    i, j = _edges(idx)
    h1 = (PQR[j, :H] - PQR[i, :H]) + b1
    yp = (PQR[i, H + F_:] + PQR[j, H:H + F_]) + bx
    return h1, yp


def edge_stats(PQR, idx, b1, bx):
    h1, yp = _edge_pre(PQR, idx, b1, bx)
    v = torch.cat([h1, yp], dim=1)
    return v.mean(0), v.var(0, unbiased=False)


def _attend(h2pre, sc2, sh2, PQR, idx, bx, scx, shx, slope):
    M, k = idx.shape
    F_ = bx.numel()
    H = PQR.shape[1] - 2 * F_
    _, yp = _edge_pre(PQR, idx, torch.zeros(H, device=PQR.device), bx)
    z2 = (h2pre.float() * sc2 + sh2).view(M, k, F_)
    zy = (yp * scx + shx).view(M, k, F_)
    w = torch.softmax(_lrelu(z2, slope), dim=1)
    return z2, zy, w, _lrelu(zy, slope), yp.view(M, k, F_)


def edge_stats_bn(PQR, idx, b1, bx, bn_w, bn_x, count_rep=1):
    H = b1.numel()
    mean, var = edge_stats(PQR, idx, b1, bx)
    E = idx.shape[0] * idx.shape[1]
    return (bn_prepare(mean[:H].contiguous(), var[:H].contiguous(), bn_w[0], bn_w[1], E * count_rep, True, bn_w[2], bn_w[3]),
            bn_prepare(mean[H:].contiguous(), var[H:].contiguous(), bn_x[0], bn_x[1], E * count_rep, True, bn_x[2], bn_x[3]))


def edge_attend_fwd(h2pre, sc2, sh2, PQR, idx, bx, scx, shx, slope, half=False):
    M, k = idx.shape
    z2, zy, w, yv, _ = _attend(h2pre, sc2, sh2, PQR, idx, bx, scx, shx, slope)
    T = (w * yv).reshape(M, k * bx.numel()).contiguous()
    return T.half() if half else T


def storage16(E, F_, k):
    return False     # the CPU models run the fp32 operand mode


def edge_attend_bwd(dT, h2pre, sc2, sh2, mean2, inv2, PQR, idx, bx, scx, shx, meanx, invx, slope):
    M, k = idx.shape
    F_ = bx.numel()
    z2, zy, w, yv, yp = _attend(h2pre, sc2, sh2, PQR, idx, bx, scx, shx, slope)
    d = dT.float().view(M, k, F_)
    dw = d * yv
    ds = w * (dw - (dw * w).sum(1, keepdim=True))
    g2 = (ds * torch.where(z2 > 0, 1.0, slope)).reshape(M * k, F_)
    gy = (d * w * torch.where(zy > 0, 1.0, slope)).reshape(M * k, F_)
    if dT.dtype == torch.bfloat16:           # 16-bit storage mode: gy is handed on as bfloat16 (statistics from the float values)
        return (g2.to(torch.bfloat16).contiguous(), gy.to(torch.bfloat16).contiguous(), torch.cat([g2.sum(0), (g2 * ((h2pre.float() - mean2) * inv2)).sum(0)]),
                torch.cat([gy.sum(0), (gy * ((yp.reshape(M * k, F_) - meanx) * invx)).sum(0)]))
    xh2 = (h2pre - mean2) * inv2
    xhy = (yp.reshape(M * k, F_) - meanx) * invx
    return (g2.contiguous(), gy.contiguous(), torch.cat([g2.sum(0), (g2 * xh2).sum(0)]), torch.cat([gy.sum(0), (gy * xhy).sum(0)]))


def edge_scatter(g1, gy, PQR, idx, rowptr, src, b1, mean1, inv1, gam1, sums1, bx, meanx, invx, gamx, sumsx):
    gy = gy.float()
    M, k = idx.shape
    H, F_ = b1.numel(), bx.numel()
    E = M * k
    i, j = _edges(idx)
    h1, yp = _edge_pre(PQR, idx, b1, bx)
    xh1 = (h1 - mean1) * inv1
    xhy = (yp - meanx) * invx
    dh1 = gam1 * inv1 * (g1 - sums1[:H] / E - xh1 * (sums1[H:] / E))
    dyp = gamx * invx * (gy - sumsx[:F_] / E - xhy * (sumsx[F_:] / E))
    out = torch.zeros_like(PQR)
    out[:, :H].index_add_(0, j, dh1)
    out[:, :H].index_add_(0, i, -dh1)
    out[:, H:H + F_].index_add_(0, j, dyp)
    out[:, H + F_:].index_add_(0, i, dyp)
    return out


# ----------------------------------------------------------------------------- AdaIN
def _inorm(x, N, slope, imean, ivar):
    M, C = x.shape
    B = M // N
    xa = _lrelu(x, slope).view(B, N, C)
    iv = torch.rsqrt(ivar.view(B, 1, C) + BN_EPS)
    return ((xa - imean.view(B, 1, C)) * iv).reshape(M, C), iv


def adain_fwd(x, N, slope, imean, ivar, gb):
    C = x.shape[1]
    xh, _ = _inorm(x, N, slope, imean, ivar)
    return (gb[:, :C] * xh + gb[:, C:]).contiguous()


def adain_bwd(dout, x, N, slope, imean, ivar, gb):
    M, C = x.shape
    B = M // N
    xh, iv = _inorm(x, N, slope, imean, ivar)
    dgb = torch.cat([dout * xh, dout], dim=1).contiguous()
    dxh = (dout * gb[:, :C]).view(B, N, C)
    xh3 = xh.view(B, N, C)
    dl = iv * (dxh - dxh.mean(1, keepdim=True) - xh3 * (dxh * xh3).mean(1, keepdim=True))
    dx = dl.reshape(M, C) * torch.where(x > 0, 1.0, slope)
    return dx.contiguous(), dgb


# ----------------------------------------------------------------------------- pooled BN backward, misc
def gemm_bn_groups(A, W, bias, bn, groups, pro=None, rows=0, slope=0.0):
    """`groups` separate calls of the single-pass models, in order (running statistics included), results stacked."""
    Mg = A.shape[0] // groups
    ys, outs, pooled, args, yargs = [], [], [], [], []
    for g in range(groups):
        pg = None if pro is None else (pro[0][g], pro[1][g], pro[2])
        Ag = A[g * Mg:(g + 1) * Mg]
        if rows == 0:
            y, st = gemm_nt(Ag, W, bias, pro=pg, bn=bn)
            ys.append(y)
        else:
            _, st, p, a, ya = gemm_bn_pool(Ag, W, bias, bn, rows, slope, pro=pg)
            pooled.append(p); args.append(a); yargs.append(ya)          # argmax already relative to the pass's own rows
        outs.append(torch.stack(list(st)))
    out = torch.stack(outs).permute(1, 0, 2).contiguous()          # [4, groups, N]
    if rows == 0:
        return torch.cat(ys).contiguous(), out
    return out, torch.cat(pooled).contiguous(), torch.cat(args).contiguous(), torch.cat(yargs).contiguous()


def gemm_bn_pool(A, W, bias, bn, rows, slope, pro=None, keep_y=False, before_finalize=None):
    if before_finalize is not None:
        before_finalize()                                   # before this pass touches the running statistics
    y, st = gemm_nt(A, W, bias, pro=pro, bn=bn)
    B = y.shape[0] // rows
    pooled, arg = maxpool(y, B, rows, st[0], st[1], slope)
    cols = torch.arange(y.shape[1], device=y.device).view(1, -1).expand(B, -1)
    return (y if keep_y else None), st, pooled, arg, y[arg.long(), cols].contiguous()


def pool_bwd_stats(gpool, pooled, argmax, y, mean, invstd, slope, prep=None):
    B, C = gpool.shape
    gval = gpool * torch.where(pooled > 0, 1.0, slope)
    cols = torch.arange(C, device=y.device).view(1, C).expand(B, C)
    real_arg = argmax
    if y.shape[0] == B:
        argmax = torch.arange(B, device=y.device).view(B, 1).expand(B, C)
    xh = (y[argmax.long(), cols] - mean) * invstd
    sums = torch.cat([gval.sum(0), (gval * xh).sum(0)])
    if prep is None:
        return gval.contiguous(), sums
    gamma, count, y_full, rows = prep
    return gval.contiguous(), sums, sparse_bn_bwd_operand(gval.contiguous(), real_arg, y_full, rows, mean, invstd, gamma, sums, count)


def bn_bwd_apply_sparse(gval, argmax, y, N, mean, invstd, gamma, sums, count):
    M, C = y.shape
    B = M // N
    g = torch.zeros((M, C), dtype=y.dtype, device=y.device)
    cols = torch.arange(C, device=y.device).view(1, C).expand(B, C)
    g[argmax.long(), cols] = gval
    xh = (y - mean) * invstd
    return (gamma * invstd * (g - sums[:C] / count - xh * (sums[C:] / count))).contiguous()


def maxpool_bwd_add(dpool, argmax, dst):
    B, C = dpool.shape
    cols = torch.arange(C, device=dst.device).view(1, C).expand(B, C)
    dst[argmax.long(), cols] += dpool
    return dst


def tanh_bwd(dy, y):
    return (dy * (1 - y * y)).contiguous()


def stacked_rows(parts):
    parts = list(parts)
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)


def multi_copy(dsts, srcs):
    for d, s in zip(dsts, srcs):
        d.copy_(s)


def axpby(a, x, b, y):
    y.copy_(a * x + (b * y if b != 0 else 0))
    return y


def adam_step(p, g, m, v, step, lr=1e-4, beta1=0.5, beta2=0.99, eps=1e-8, grad_scale=1.0):
    import math
    gr = g * grad_scale
    m.mul_(beta1).add_(gr, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(gr, gr, value=1 - beta2)
    denom = v.sqrt() / math.sqrt(1 - beta2 ** step) + eps
    p.addcdiv_(m, denom, value=-lr / (1 - beta1 ** step))


def adam_step_dev(p, g, m, v, state, lr=1e-4, beta1=0.5, beta2=0.99, eps=1e-8, grad_scale=1.0, zero_grad=False):
    step = int(state[:1].view(torch.int32).item()) + 1
    state[:1].view(torch.int32).fill_(step)
    state[1] = 1.0 - beta1 ** step
    state[2] = 1.0 / math.sqrt(1.0 - beta2 ** step)
    adam_step(p, g, m, v, step, lr * float(state[3]), beta1, beta2, eps, grad_scale)
    if zero_grad:
        g.zero_()


def act_bwd(dy, y, act, slope=0.0):
    if act == ACT_LRELU:
        return (dy * torch.where(y > 0, 1.0, slope)).contiguous()
    if act == ACT_TANH:
        return (dy * (1 - y * y)).contiguous()
    return dy.contiguous()


def scatter_rows(val, argmax, M):
    B, C = val.shape
    out = torch.zeros((M, C), dtype=val.dtype, device=val.device)
    cols = torch.arange(C, device=val.device).view(1, C).expand(B, C)
    out[argmax.long(), cols] = val
    return out


def gather_rows(src, argmax):
    B, C = argmax.shape
    cols = torch.arange(C, device=src.device).view(1, C).expand(B, C)
    return src[argmax.long(), cols].contiguous()


def bn_dbl_stats(u, y, gz, mean, invstd):
    xh = (y - mean) * invstd
    return u.sum(0), (u * xh).sum(0), (u * gz).sum(0)


def bn_dbl_apply(u, y, gz, mean, invstd, scale, shift, slope, gamma, S1, U0, U1, count):
    xh = (y - mean) * invstd
    gs = gamma * invstd
    z = y * scale + shift
    q = gs * (u - U0 / count - xh * (U1 / count)) * torch.where(z > 0, 1.0, slope)
    xbar = -(gs / count) * (u * S1 + gz * U1)
    return q.contiguous(), xbar.contiguous()


def col_scale_add(a, b, gamma):
    return (a + gamma * b).contiguous()


# ----------------------------------------------------------------------------- losses / GP
def gan_loss(mode, which, d_real, d_fake, real_label=None, fake_label=None):
    with torch.enable_grad():
        return _gan_loss(mode, which, d_real, d_fake, real_label, fake_label)


def _gan_loss(mode, which, d_real, d_fake, real_label=None, fake_label=None):
    import torch.nn.functional as F_
    df = d_fake.detach().clone().requires_grad_(True)
    dr = d_real.detach().clone().requires_grad_(True) if d_real is not None else None
    B = df.shape[0]
    acc_r = acc_f = torch.zeros(())
    mse = lambda logit, label: ((logit.view(-1, 1) - label.view(1, -1)) ** 2).mean()
    if mode == 0:
        fl = fake_label if fake_label is not None else (torch.ones(B) if which == 1 else torch.zeros(B))
        lf = mse(df, fl.to(df.device))
        if which == 0:
            rl = real_label if real_label is not None else torch.ones(B)
            lr = mse(dr, rl.to(df.device)); loss = (lf + lr) / 2
            acc_r = (dr >= 0.5).float().mean(); acc_f = (df < 0.5).float().mean()
        else:
            lr = torch.zeros(()); loss = lf
    elif mode == 1:
        lf = df.mean() if which == 0 else -df.mean()
        lr = dr.mean() if which == 0 else torch.zeros(())
        loss = lf - lr if which == 0 else lf
    elif mode == 2:
        if which == 0:
            lr = F_.relu(1.0 - dr).mean(); lf = F_.relu(1.0 + df).mean(); loss = lf + lr
            acc_r = (dr >= 0).float().mean(); acc_f = (df < 0).float().mean()
        else:
            lf = -df.mean(); lr = torch.zeros(()); loss = lf
            acc_f = (df < 0).float().mean()
            acc_r = (dr >= 0).float().mean() if dr is not None else (torch.zeros(B) >= 0).float().mean()
    else:
        if which == 0:
            lf = F_.binary_cross_entropy_with_logits(df, torch.zeros_like(df)); lr = F_.binary_cross_entropy_with_logits(dr, torch.ones_like(dr))
            loss = (lf + lr) / 2
        else:
            lf = F_.binary_cross_entropy_with_logits(df, torch.ones_like(df)); lr = torch.zeros(()); loss = lf
    ins = [df] + ([dr] if (dr is not None and which == 0) else [])
    gs = torch.autograd.grad(loss, ins)
    out5 = torch.stack([loss.detach().reshape(()), lf.detach().reshape(()), torch.as_tensor(lr).detach().reshape(()).to(loss.device),
                        torch.as_tensor(acc_r).reshape(()).to(loss.device), torch.as_tensor(acc_f).reshape(()).to(loss.device)]).float()
    g_real = gs[1] if len(gs) > 1 else (torch.zeros_like(d_real) if d_real is not None else None)
    return out5, g_real, gs[0]


def lerp_rows(real, fake, alpha):
    B = real.shape[0]
    a = alpha.reshape(B, *([1] * (real.dim() - 1)))
    return (real + a * (fake - real)).contiguous()


def gp_penalty_fwd(g, gamma, lam):
    B = g.shape[0]
    norms = g.reshape(B, -1).norm(2, dim=1)
    return (lam * (((norms - gamma) / gamma) ** 2).mean()).reshape(1), norms


def gp_penalty_bwd(g, norms, gamma, lam, upstream):
    B = g.shape[0]
    up = 1.0 if upstream is None else upstream.reshape(())
    c = up * lam * (2.0 / B) * ((norms - gamma) / (gamma * gamma)) / norms
    return (c.reshape(B, *([1] * (g.dim() - 1))) * g).contiguous()


def gp_penalty_fwd_bwd(g, gamma, lam, loss_add=None):
    loss, norms = gp_penalty_fwd(g, gamma, lam)
    v = gp_penalty_bwd(g, norms, gamma, lam, None)
    return loss, norms, v, (None if loss_add is None else loss_add.reshape(1) + loss)


def reduce_chunks(recv, out=None):
    s = recv[0].clone()
    for j in range(1, recv.shape[0]):
        s = s + recv[j]
    if out is None:
        return s
    out.copy_(s.reshape(out.shape))
    return out


def multi_add(dsts, srcs):
    for d, s in zip(dsts, srcs):
        d.add_(s if s.shape == d.shape else s.reshape(d.shape))


def capturing():
    return False


# ----------------------------------------------------------------------------- fused layer backward (csrc/gemm_dual.hip)
GEMM_DUAL = [True]


class ActOperand:
    def __init__(self, x, scale, shift, slope):
        self.x, self.scale, self.shift, self.slope = x, scale, shift, float(slope)
        self.shape, self.device = x.shape, x.device

    def dense(self):
        return _lrelu(self.x * self.scale + self.shift, self.slope)


SPLIT_PAIR = [False]    # tests: True sends the collapsed layer's backward through gemm_tn + gemm_nt_bnbwd (the split-bf16 mode's route)


def collapsed_pair_preferred(M, K):
    return bool(SPLIT_PAIR[0])


def gemm_dual_ok(dy, W, y_ref, edge=None):
    g = dy.g if isinstance(dy, Affine2) else (dy.x if isinstance(dy, ActOperand) else dy)
    ek = 0 if edge is None else int(edge[0].shape[1])
    shape = (W.shape[0], W.shape[1])
    # (the HIP kernel wants M >= 8192; the model takes the small sizes of the CPU host-composition tests too, so that they run the fused route)
    return bool(GEMM_DUAL[0] and g.shape[0] % 32 == 0 and ((shape == (128, 64) and ek in (0, 10)) or (shape in ((256, 128), (256, 256)) and ek == 0)))


def gemm_dual(dy, W, y_ref, scale, shift, mean, invstd, slope, edge=None, coef_bn=None, defer=True, out=None, beta=0.0, bias=None, rowadd=None,
              with_colsum=False, phaseb=None, gout=None):
    """= gemm_tn(dy, y_ref, pro / edge) and gemm_nt_bnbwd(dy, W^T, y_ref, ...) of the same operands."""
    d = dy.dense() if isinstance(dy, ActOperand) else dy
    dW = gemm_tn(d, y_ref, pro=(scale, shift, slope), edge=edge)
    if out is not None:
        out.copy_(beta * out + dW)
        dW = out
    res = gemm_nt_bnbwd(d, W.t().contiguous(), y_ref, scale, shift, mean, invstd, slope, edge=edge, bias=bias, rowadd=rowadd,
                        **({} if coef_bn is None else dict(coef_bn=coef_bn)))
    extra = (_dense(d).sum(0),) if with_colsum else ()
    if phaseb is not None:
        co, pg, pinv = phaseb[:3]
        sums, dgam = bn_dbl_phaseb(co, pg, pinv, res[1], res[2])
        extra = extra + (sums, dgam)
        if len(phaseb) == 4:       # coefficients of p*X + q*y + r = pinv*(X - S0/M - xhat*S1/M)
            C_, rM = pinv.numel(), 1.0 / co[5]
            q_ = -(pinv * pinv) * (sums[C_:] * rM)
            extra = extra + (torch.stack([pinv, q_, -(pinv * (sums[:C_] * rM)) - q_ * phaseb[3]]),)
    res = list(res)
    if gout is not None:
        res[0] = gout[0] + gout[1] * res[0]
    return (dW,) + tuple(res) + extra


def wt_diag_w(W, alpha, beta=None, bias=None):
    G = (W * alpha[:, None]).t() @ W
    if beta is None:
        return G.contiguous()
    return G.contiguous(), ((alpha * bias + beta) @ W).contiguous()


# ----------------------------------------------------------------------------- grouped launches (spgan.ops.*_multi): the same problems, one after the other
GROUPED = [True]


def gemm_dual_multi(specs, defer=True):
    return [gemm_dual(defer=defer, **sp) for sp in specs]


def wgrad_collapse_multi(specs):
    return [wgrad_collapse(**sp) for sp in specs]


def pool_bwd_stats_multi(specs):
    return [pool_bwd_stats(**sp) for sp in specs]


def gemm_tn_narrow_multi(specs):
    return [gemm_tn(sp["A"], sp["Bm"], out=sp.get("out"), beta=sp.get("beta", 0.0), defer=True) for sp in specs]


def multi_addn(dsts, srcs_per_dst):
    for d, ss in zip(dsts, srcs_per_dst):
        for s in ss:
            d.add_(s.reshape(d.shape))


BF16_MAX = float.fromhex("0x1.fep127")       # the largest finite bfloat16


def _split_bf16x3(x):
    """The split-bf16 planes of fp32 x (csrc/split_bf16.hpp): (hi, mid, lo) bfloat16 with hi + mid + lo = x, exactly for |x| >= 2^-110 (below,
    lo is rounded to bf16's subnormal spacing).  Finite x: hi = RN(clamp(x, +-BF16_MAX)) (no plane overflows), mid = RN(x - hi),
    lo = RN(x - hi - mid); non-finite x: (+0, +0, x)."""
    x = x.float()
    fin = torch.isfinite(x)
    xf = torch.where(fin, x, torch.zeros_like(x))
    hi = xf.clamp(-BF16_MAX, BF16_MAX).bfloat16(); r1 = xf - hi.float()
    mid = r1.bfloat16(); r2 = r1 - mid.float()
    return hi, mid, torch.where(fin, r2, x).bfloat16()


def split_image(W, out=None):
    """ops.split_image: the split-bf16 image of W [N,K] (spgan_split_bf16x3_image): the planes of _split_bf16x3,
    laid out [K/16][plane][N][16 bf16], the two 16-byte halves of a row swapped where bit 3 of n is set, rows with bit 5 of n set negated."""
    N, K = W.shape
    assert N % 128 == 0 and K % 16 == 0
    n = torch.arange(N, device=W.device)
    W = torch.where(((n >> 5) & 1).bool()[:, None], -W, W)                           # negated BEFORE the split, like the kernel (an exact-zero residual keeps +0)
    planes = torch.stack(_split_bf16x3(W))                                            # [3, N, K]
    img = planes.view(3, N, K // 16, 2, 8).permute(2, 0, 1, 3, 4)                    # [K/16, 3, N, 2, 8]
    img = torch.where(((n >> 3) & 1).bool()[None, None, :, None, None], img.flip(3), img).contiguous()
    res = img.view(torch.uint8).reshape(-1)
    if out is not None:
        out.copy_(res)
        return out
    return res
