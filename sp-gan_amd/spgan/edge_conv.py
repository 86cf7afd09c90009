"""The gather-side edge convolutions: the autograd Functions behind `spgan.edgeConv`, `upsample_edgeConv`, `deform_edgeConv_simple` /
`_first`, `deform_edgeConv_feat`, `deform_edgeConv` and `bilateral_upsample_edgeConv`, over the launchers of spgan.edge_max / edge_window / edge_rank / edge_weight,
and the tail of the blocks built on them (`BlockTailFn`, over spgan.block_tail).

The family's conventions, stated once:
* A 1x1 convolution over the edge features cat[x_i, x_j - x_i] is one per-point GEMM, PQ [M,2F] = [P | Q] = x.[Wd ; Wc - Wd]^T + [0 ; b]
  (`stacked` / `unstacked_grad`); the value on edge (i, j) is Q_i + P_j and exists only inside the kernels.
* idx is int32 [M,k] with global rows (M = B*N), made by ops.knn or handed in through the holder (modules.check_edge_input).
* Each Function takes holder(B, N, k, training, idx | None, knn_mode, the nn.BatchNorm2d modules, ...), x [B,Fin,N], then (conv weight,
  conv bias, bn weight, bn bias) per layer.  The holder's last_idx receives the graph of the forward.
* The statistics (scale, shift, invstd, mean) of every BatchNorm are made in forward (`bn_stats`) and handed to nobody else: nothing can
  write them between forward and backward, so they ride on ctx instead of through save_for_backward's version check.  The running
  statistics that ARE updated in place are not read by the backward.
* Once differentiable: a selection or a mask is piecewise constant and the backward is a closed form over saved statistics, so a second
  derivative is refused where it is asked for (`refuse_double_backward`): no GradientPenalty on top of these layers.  The one exception is
  opt-in: `edgeConv(double_backward=True)` runs its first backward as a differentiable node (`EdgeMaxConvBwdFn`).
* The rank layers (RankEdgeConvFn's [1,k] product, all of WeightedRankEdgeConvFn, CoordRankEdgeConvFn and BilateralUpsampleEdgeConvFn) compute exact fp32 products: they do not follow
  ops.set_mfma_operands.
* Weight-derived operand images are cached per weight set (`cached_images`)."""
from __future__ import annotations

import weakref
from typing import Callable, Dict, Sequence

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import block_tail, edge_dense, edge_max, edge_rank, edge_weight, edge_window, ops

Tensor = torch.Tensor


# ----------------------------------------------------------------------------- operand images
# one dictionary per builder: a layer that reaches the cap does not evict another layer's images
_IMAGES: Dict[str, Dict[tuple, tuple]] = {"upsample": {}, "rank": {}, "weight": {}, "coord": {}, "bilateral": {}, "tail": {}, "dense_edge": {}, "dense_rows": {}, "dense_side": {}}


def cached_images(cache: Dict[tuple, tuple], weights: Sequence[Tensor], extra: tuple, build: Callable):
    """build(*detached weights), cached in `cache` until a weight changes: the key is the weights' (data_ptr, shape) and `extra`; an entry is stale
    once a weight's (ops.weights_epoch_of, torch version counter) stamp moves -- an in-place write, or an optimiser step of
    spgan.optim.Adam, which rewrites parameters invisibly to torch and bumps the epoch of their storage (the staleness rule of nets._t) --
    or once a weight it was built from has died: the allocator may hand a dead weight's address, with a fresh version counter, to the next
    module's weight of the same shape, so every entry keeps weak references to its weights and counts a dead one as a miss.  Callers
    therefore pass the long-lived weight objects themselves (the Parameters, as autograd hands them to forward and back from
    ctx.saved_tensors): an entry built from a temporary -- a view, a .detach() -- dies with it and never hits.  A rebuild
    overwrites the entry: the bookkeeping does not grow with the number of optimiser steps.
    Inside a capture the cache is neither read nor written: the images are rebuilt there, so that their kernels are part of the graph
    and every replay sees the weights of that moment.  The dictionary is cleared when it holds 64 entries."""
    ws = [w.detach() for w in weights]
    if ops.capturing():
        return build(*ws)
    key = (extra,) + tuple([(w.data_ptr(), w.shape) for w in ws])
    stamp = [(ops.weights_epoch_of(w), w._version) for w in ws]
    hit = cache.get(key)
    if hit is not None and hit[0] == stamp and all(r() is not None for r in hit[2]):
        return hit[1]
    if len(cache) >= 64:
        cache.clear()
    img = build(*ws)
    cache[key] = (stamp, img, [weakref.ref(w) for w in weights])
    return img


def stacked(W: Tensor) -> Tensor:
    """conv weight [F,2C,1,1] over cat[x_i, x_j - x_i] -> [Wd ; Wc - Wd] [2F,C]: rows of P, then rows of Q"""
    F_, C = W.shape[0], W.shape[1] // 2
    Wm = W.reshape(F_, 2 * C)
    Wd = Wm[:, C:]
    return torch.cat([Wd, Wm[:, :C] - Wd], dim=0)


def unstacked_grad(dWst: Tensor) -> Tensor:
    """[2F,C], rows of dW'_P, then of dW'_Q -> the conv weight's gradient [F,2C,1,1]: dWc = dW'_Q, dWd = dW'_P - dW'_Q"""
    F_ = dWst.shape[0] // 2
    return torch.cat([dWst[F_:], dWst[:F_] - dWst[F_:]], dim=1).view(F_, 2 * dWst.shape[1], 1, 1)


def pq_bias(b: Tensor) -> Tensor:
    return torch.cat([torch.zeros_like(b), b])                          # the conv bias belongs to the central half: Q


def upsample_images(W1: Tensor, V: Tensor, C: int, k: int):
    """The operand images of upsample_edgeConv's two conv weights (W1 [4C,2C,1,w], V [F2,2C,1,2k]):
    (Wc1 [4C,C], Wd1 [4C,w*C], Wd1^T, Vc [F2,C], Vd [F2,k*C], Vd^T, V2p [F2,T*4C], V2p^T, Wc1^T, Vc^T).
    Wc = the central halves summed over the taps; Wd = the difference halves, tap-major; V2p = conv2's last k taps with the columns
    permuted from the reference's per-point (2C, k) reading, c'*k + j = o*T + t, to this layer's row order t*4C + o.
    Cached per weight pair (cached_images)."""
    def build(W1, V):
        w = W1.shape[3]
        T = k - w + 1
        F2 = V.shape[0]
        Wc1 = W1[:, :C, 0, :].sum(dim=2)
        Wd1 = W1[:, C:, 0, :].permute(0, 2, 1).reshape(4 * C, w * C)
        Vc = V[:, :C, 0, :k].sum(dim=2)
        Vd = V[:, C:, 0, :k].permute(0, 2, 1).reshape(F2, k * C)
        V2p = V[:, :, 0, k:].reshape(F2, 4 * C, T).permute(0, 2, 1).reshape(F2, T * 4 * C)
        return (Wc1, Wd1, Wd1.t().contiguous(), Vc, Vd, Vd.t().contiguous(), V2p, V2p.t().contiguous(), Wc1.t().contiguous(),
                Vc.t().contiguous())
    return cached_images(_IMAGES["upsample"], (W1, V), (C, k), build)


def rank_images(W1: Tensor, W2: Tensor):
    """The operand images of the full-rank edge convolution's two conv weights (W1 [F1,2Fin,1,1], W2 [Fout,F1,1,k]):
    (Wst [2F1,Fin] = [Wd ; Wc - Wd] (rows of P, then of Q), Wst^T, W2i [Fout, k*F1] tap-major (column r*F1 + c), W2i^T).
    Cached per weight pair (cached_images)."""
    def build(W1, W2):
        Wst = stacked(W1)
        W2i = W2[:, :, 0, :].permute(0, 2, 1).reshape(W2.shape[0], W2.shape[3] * W2.shape[1])
        return Wst, Wst.t().contiguous(), W2i, W2i.t().contiguous()
    return cached_images(_IMAGES["rank"], (W1, W2), (), build)


def weight_images(Wh: Tensor, Wf1: Tensor, Wf2: Tensor, Wf3: Tensor, W2: Tensor):
    """The operand images of deform_edgeConv_feat's five conv weights (inte_conv_hk.0 [Fin,2Fin,1,1], conv_fea.0 [16,2Fin,1,1], conv_fea.3
    [64,16,1,1], conv_fea.6 [Fin,64,1,1], conv2.conv [Fout,Fin,1,k]):
    (Wst_h [2Fin,Fin] and Wst_1 [32,Fin] = [Wd ; Wc - Wd] of the two per-point GEMMs, Wall_t [Fin, 2Fin+32] = their stack transposed,
    Wm2 [64,16], Wm2^T, Wm3 [Fin,64], Wm3^T, W2i [Fout, k*Fin] tap-major, W2i^T).
    Cached per weight set (cached_images)."""
    def build(Wh, Wf1, Wf2, Wf3, W2):
        Wst_h, Wst_1 = stacked(Wh), stacked(Wf1)
        Wm2, Wm3 = Wf2.reshape(Wf2.shape[0], Wf2.shape[1]), Wf3.reshape(Wf3.shape[0], Wf3.shape[1])
        W2i = W2[:, :, 0, :].permute(0, 2, 1).reshape(W2.shape[0], W2.shape[3] * W2.shape[1])
        return (Wst_h, Wst_1, torch.cat([Wst_h, Wst_1], dim=0).t().contiguous(), Wm2.contiguous(), Wm2.t().contiguous(), Wm3.contiguous(),
                Wm3.t().contiguous(), W2i, W2i.t().contiguous())
    return cached_images(_IMAGES["weight"], (Wh, Wf1, Wf2, Wf3, W2), (), build)


def coord_images(Wh: Tensor, Wf: Tensor, Wx: Tensor, Wa2: Tensor, Wa3: Tensor, W2: Tensor):
    """The operand images of deform_edgeConv's six conv weights (inte_conv_hk.0 [Fin,2Fin,1,1], conv_fea.0 [16,2Fin,1,1], conv_xyz.0 [16,6,1,1],
    conv_all.0 [64,16,1,1], conv_all.3 [Fin,64,1,1], conv2.0 [Fout,Fin,1,k]):
    (Wst_h [2Fin,Fin], Wst_f [32,Fin] and Wst_x [32,3] = [Wd ; Wc - Wd] of the three per-point GEMMs, Wall_t [Fin, 2Fin+32] = the two
    feature-side stacks transposed, Wst_x^T [3,32], Wm2 [64,16], Wm2^T, Wm3 [Fin,64], Wm3^T, W2i [Fout, k*Fin] tap-major, W2i^T).
    Cached per weight set (cached_images)."""
    def build(Wh, Wf, Wx, Wa2, Wa3, W2):
        Wst_h, Wst_f, Wst_x = stacked(Wh), stacked(Wf), stacked(Wx)
        Wm2, Wm3 = Wa2.reshape(Wa2.shape[0], Wa2.shape[1]), Wa3.reshape(Wa3.shape[0], Wa3.shape[1])
        W2i = W2[:, :, 0, :].permute(0, 2, 1).reshape(W2.shape[0], W2.shape[3] * W2.shape[1])
        return (Wst_h, Wst_f, Wst_x, torch.cat([Wst_h, Wst_f], dim=0).t().contiguous(), Wst_x.t().contiguous(), Wm2.contiguous(), Wm2.t().contiguous(),
                Wm3.contiguous(), Wm3.t().contiguous(), W2i, W2i.t().contiguous())
    return cached_images(_IMAGES["coord"], (Wh, Wf, Wx, Wa2, Wa3, W2), (), build)


def tail_images(Wa: Tensor, Cs: int):
    """add_cov's Conv1d weight [Fo, Cs + C, 1] over cat[xs broadcast, a] -> (W_s [Fo,Cs], W_e [Fo,C], W_s^T, W_e^T): the halves that meet the
    global vector and the per-point features (BlockTailFn)"""
    def build(Wa):
        Wm = Wa.view(Wa.shape[0], -1)
        Ws, We = Wm[:, :Cs].contiguous(), Wm[:, Cs:].contiguous()
        return Ws, We, Ws.t().contiguous(), We.t().contiguous()
    return cached_images(_IMAGES["tail"], [Wa], (Cs,), build)


def parity_major(t: Tensor, dim: int = 0) -> Tensor:
    """inte_conv_hk's 4C output channels o = 2c' + h along `dim` -> the order o' = h*2C + c' (the bilateral layer's: the [M*T, 4C] rows (i,t)
    then read as [M, k, 2C] rows (i, r' = 2t + h))"""
    n = t.shape[dim] // 2
    return t.unflatten(dim, (n, 2)).transpose(dim, dim + 1).flatten(dim, dim + 1)


def channel_major(t: Tensor, dim: int = 0) -> Tensor:
    """the inverse of parity_major: o' = h*2C + c' along `dim` -> o = 2c' + h"""
    n = t.shape[dim] // 2
    return t.unflatten(dim, (2, n)).transpose(dim, dim + 1).flatten(dim, dim + 1)


def paired_ranks(idx: Tensor) -> Tensor:
    """idx [M,k] -> idxp with idxp[i, 2t + h] = idx[i, h*T + t], T = k/2: the rank order in which the bilateral layer's weight branch runs"""
    M, k = idx.shape
    return idx.view(M, 2, k // 2).transpose(1, 2).reshape(M, k)


def bilateral_images(W1: Tensor, Wf: Tensor, Wx: Tensor, Wa2: Tensor, Wa3: Tensor, V: Tensor, C: int, k: int):
    """The operand images of bilateral_upsample_edgeConv's six conv weights (inte_conv_hk.0 [4C,2C,1,w], conv_fea.0 [16,2C,1,1], conv_xyz.0
    [16,6,1,1], conv_all.0 [64,16,1,1], conv_all.3 [2C,64,1,1], conv2.conv [F2,2C,1,2k]):
    (Wc1 [4C,C], Wd1 [4C,w*C], Wd1^T -- upsample_images' with the output channels in the order o' = h*2C + c' (parity_major) --, Vc [F2,C],
    Vd [F2,k*C], Vd^T, Vc^T, V2i [F2, k*2C] = conv2's last k taps with column r'*2C + c' = tap k + j, r' = 2t + h, j = h*T + t, V2i^T,
    Wst_f [32,C], Wst_x [32,3], Wst_x^T, Wcat_t [C, 4C+32] = [Wc1 ; Wst_f]^T, Wm2 [64,16], Wm2^T, Wm3 [2C,64], Wm3^T).
    Cached per weight set (cached_images)."""
    def build(W1, Wf, Wx, Wa2, Wa3, V):
        w = W1.shape[3]
        T = k - w + 1
        F2 = V.shape[0]
        W1p = parity_major(W1)
        Wc1 = W1p[:, :C, 0, :].sum(dim=2)
        Wd1 = W1p[:, C:, 0, :].permute(0, 2, 1).reshape(4 * C, w * C)
        Vc = V[:, :C, 0, :k].sum(dim=2)
        Vd = V[:, C:, 0, :k].permute(0, 2, 1).reshape(F2, k * C)
        V2i = V[:, :, 0, k:].reshape(F2, 2 * C, 2, T).permute(0, 3, 2, 1).reshape(F2, k * 2 * C)
        Wst_f, Wst_x = stacked(Wf), stacked(Wx)
        Wm2, Wm3 = Wa2.reshape(Wa2.shape[0], Wa2.shape[1]), Wa3.reshape(Wa3.shape[0], Wa3.shape[1])
        Wd1, Vd, V2i = Wd1.contiguous(), Vd.contiguous(), V2i.contiguous()          # C = 1: the reshapes above are strided views
        return (Wc1, Wd1, Wd1.t().contiguous(), Vc, Vd, Vd.t().contiguous(), Vc.t().contiguous(), V2i, V2i.t().contiguous(), Wst_f, Wst_x,
                Wst_x.t().contiguous(), torch.cat([Wc1, Wst_f], dim=0).t().contiguous(), Wm2.contiguous(), Wm2.t().contiguous(), Wm3.contiguous(),
                Wm3.t().contiguous())
    return cached_images(_IMAGES["bilateral"], (W1, Wf, Wx, Wa2, Wa3, V), (C, k), build)


def dense_edge_images(Ws: Sequence[Tensor], C: int):
    """The operand images of DenseEdgeModule's L conv weights (W_l [G, 2C + (l-1)G, 1, 1] over cat[x_j - x_i, x_i, y_1 .. y_{l-1}], l = 1..L):
    (Wst [2LG, C] = rows of P_1 .. P_L, then of Q_1 .. Q_L with P_l = W_l[:, :C] (the difference half comes FIRST here: the other way
    round from `stacked`) and Q_l = W_l[:, C:2C] - W_l[:, :C]; Wst^T; Wy = the y columns W_l[:, 2C:] [G, (l-1)G] of l = 2..L; Wback =
    per m = 1..L-1 the stack [G, (L-m)G] of the transposed y_m columns of every later level, the operand of gy_m = D[:, mG:] . Wback_m^T).
    Cached per weight set (cached_images)."""
    def build(*Ws):
        L, G = len(Ws), Ws[0].shape[0]
        Wm = [W.reshape(W.shape[0], W.shape[1]) for W in Ws]
        Wst = torch.cat([w[:, :C] for w in Wm] + [w[:, C:2 * C] - w[:, :C] for w in Wm], dim=0).contiguous()
        Wy = tuple(Wm[l][:, 2 * C:].contiguous() for l in range(1, L))
        Wback = tuple(torch.cat([Wm[l][:, 2 * C + m * G:2 * C + (m + 1) * G].t() for l in range(m + 1, L)], dim=1).contiguous() for m in range(L - 1))
        return Wst, Wst.t().contiguous(), Wy, Wback
    return cached_images(_IMAGES["dense_edge"], tuple(Ws), (C,), build)


def dense_edge_unstacked_grad(dWst: Tensor, l: int, L: int, G: int) -> Tensor:
    """[2LG, C] (rows of dW'_P, then of dW'_Q) -> level l's gradient of the e0 columns [G, 2C]: dW[:, :C] = dW'_P - dW'_Q, dW[:, C:2C] = dW'_Q"""
    dP, dQ = dWst[l * G:(l + 1) * G], dWst[(L + l) * G:(L + l + 1) * G]
    return torch.cat([dP - dQ, dQ], dim=1)


def dense_rows_images(Ws: Sequence[Tensor], Cin: int):
    """The operand images of DenseModule1D's conv weights (W_l [w_l, Cin + off_l, 1] over cat[x, y_1 .. y_{l-1}], off_l = w_1 + .. + w_{l-1}):
    (Wm = the weights as matrices; Wx_t [Cin, S] = the transposed x columns of every level side by side, S = sum w_l; Wback = per level
    m < L the stack [w_m, S - off_{m+1}] of the transposed y_m columns of every later level).  Cached per weight set (cached_images)."""
    return cached_images(_IMAGES["dense_rows"], tuple(Ws), (Cin,), lambda *Ws: _rows_images(Ws, Cin))


def _rows_images(Ws: Sequence[Tensor], Cin: int):
    L = len(Ws)
    Wm = [W.reshape(W.shape[0], W.shape[1]).contiguous() for W in Ws]
    off = [0]
    for w in Wm:
        off.append(off[-1] + w.shape[0])
    Wx_t = torch.cat([w[:, :Cin].t() for w in Wm], dim=1).contiguous()
    Wback = tuple(torch.cat([Wm[l][:, Cin + off[m]:Cin + off[m + 1]].t() for l in range(m + 1, L)], dim=1).contiguous() for m in range(L - 1))
    return tuple(Wm), Wx_t, Wback


# ----------------------------------------------------------------------------- what the Functions share
def refuse_double_backward(layer: str) -> None:
    """First line of every backward.  @once_differentiable alone fails late and only when the cotangent carries a graph; with
    create_graph=True and a plain cotangent (autograd.grad(out.sum(), x, create_graph=True): the gradient-penalty pattern) it would hand
    back a gradient without a graph and the penalty's second derivative would silently be missing.  Refuse where the request is made."""
    if torch.is_grad_enabled():
        raise RuntimeError("%s is once differentiable: its backward was asked to build a graph (create_graph=True), but it has no "
                           "double backward -- the layer cannot sit under a gradient penalty" % layer)


def bn_stats(bn, train: bool, count: int, gamma: Tensor, beta: Tensor, records=None, moments=None):
    """The statistics of one BatchNorm2d over `count` values: one tensor [4,F] with the rows (scale, shift, invstd, mean), which ctx
    keeps as it is.  Train mode finalises the batch statistics from records = (partials, tile_rows) of a gather / product pass or from
    moments = (mean, var), and updates the module's buffers as nn.BatchNorm2d does; eval mode reads the running statistics."""
    if not train:
        return ops._bn_prepare4(None, None, gamma, beta, count, False, bn.running_mean, bn.running_var, eps=float(bn.eps))
    bn.num_batches_tracked += 1
    if records is not None:
        return edge_max.edge_max_bn(records[0], records[1], count, gamma, beta, bn.running_mean, bn.running_var, float(bn.momentum), float(bn.eps))
    return ops._bn_prepare4(moments[0], moments[1], gamma, beta, count, True, bn.running_mean, bn.running_var, float(bn.momentum), float(bn.eps))


def edge_records(PQ: Tensor, idx: Tensor):
    """The (sum, M2) records of Q_i + P_j over the M*k edges come from edge_max's gather pass; its max / min outputs are dropped"""
    return edge_max.edge_max_gather(PQ, idx)[4:]


def split_records(out, train: bool):
    """A product launched with stats=train -> (y, its (partials, tile_rows) records | None)"""
    return (out[0], out[1:]) if train else (out, None)


def used(sums: Tensor, train: bool) -> Tensor:
    """eval mode: the statistics are constants, the BatchNorm backward is the plain scale"""
    return sums if train else torch.zeros_like(sums)


def dbias(rows: Tensor, train: bool) -> Tensor:
    """a bias in front of a train-mode BatchNorm: exactly zero (the batch mean absorbs it)"""
    return torch.zeros(rows.shape[1], dtype=torch.float32, device=rows.device) if train else ops.colsum(rows)[0]


def gb(sums: Tensor, need, i: int):
    """sums [2F] = [sum g | sum g*xhat] -> (dgamma, dbeta) for the inputs at positions i, i + 1"""
    F_ = sums.numel() // 2
    return (sums[F_:].clone() if need[i] else None, sums[:F_].clone() if need[i + 1] else None)


def relu_bn_bwd(dout: Tensor, Y: Tensor, st, gamma: Tensor, h):
    """The last layer's ReLU + BatchNorm backward: dout [B,F,N] (any view of it), the pre-norm Y [M,F] -> (dy [M,F], sums [2F])"""
    return lrelu_bn_bwd(dout, Y, st, gamma, h, 0.0)


def lrelu_bn_bwd(dout: Tensor, Y: Tensor, st, gamma: Tensor, h, slope: float):
    """relu_bn_bwd for a last layer that ends in LeakyReLU(slope).  With one row per group the pooling backward is the per-row mask: it
    multiplies by 1 where the activated value is positive and by `slope` elsewhere, and the activated value has the pre-activation's sign."""
    from . import pointnet_util
    scale, shift, invstd, mean = st
    g = ops.cm_to_pm(dout.reshape(h.B, Y.shape[1], h.N).contiguous())
    r, sums = pointnet_util._group_max_bwd(g, ops.affine_act(Y, scale, shift, slope), None, Y, mean, invstd, slope, 1)
    return ops.bn_bwd_apply(r, Y, mean, invstd, gamma, used(sums, h.training), Y.shape[0]), sums


def rank_scatter(da: Tensor, rowptr: Tensor, src: Tensor, st, PQ: Tensor, idx: Tensor, sums: Tensor, train: bool) -> Tensor:
    """da [M,k,F] on the edges -> dPQ [M,2F], through the LeakyReLU'd BatchNorm whose statistics are st"""
    scale, _, invstd, mean = st
    if train:
        return edge_rank.edge_rank_scatter(da, rowptr, src, scale, PQ, idx, mean, invstd, sums)
    return edge_rank.edge_rank_scatter(da, rowptr, src, scale)


# ----------------------------------------------------------------------------- the Functions
class EdgeMaxConvFn(Function):
    """out [B,F,N] = max_j relu(bn(conv1x1(cat[x_i, x_j - x_i])))   (the reference's edgeConv, Generation/modules.py:779-796) without the
    [B,2Fin,N,k] edge tensor: the per-point GEMM and gather passes over it (csrc/edge_max.hip).
    holder: bn, double_backward, input_only; also receives last_sel, the selected ranks.
    With holder.double_backward and a backward that is asked to build a graph, the first backward runs as a differentiable node
    (EdgeMaxConvBwdFn); otherwise the layer is once differentiable."""

    @staticmethod
    def forward(ctx, h, x, W, b, gamma, beta):
        B, Fin, N = x.shape
        x_pm = ops.cm_to_pm(x)
        idx = h.idx if h.idx is not None else ops.knn(x_pm, B, N, h.k, h.knn_mode)
        Wst = stacked(W)
        PQ = ops.gemm_nt(x_pm, Wst, pq_bias(b))
        if h.training:
            pmax, pmin, rmax, rmin, part, tile_rows = edge_max.edge_max_gather(PQ, idx)
            st = bn_stats(h.bn, True, idx.numel(), gamma, beta, records=(part, tile_rows))
            out_pm, sel = edge_max.edge_max_finish(PQ, pmax, pmin, rmax, rmin, st[0], st[1])
            del pmax, pmin, rmax, rmin
        else:
            st = bn_stats(h.bn, False, idx.numel(), gamma, beta)
            out_pm, sel = edge_max.edge_max_eval(PQ, idx, st[0], st[1])
        h.last_idx, h.last_sel = idx, sel
        ctx.h, ctx.st = h, st
        # x, not its point-major copy: the input is alive anyway.  The opted-in layer also keeps W and gamma (inputs: no copy), which must
        # reach the differentiable first backward as inputs of its node -- Wst is an image, not a leaf.
        ctx.save_for_backward(x, PQ, sel, idx, Wst, *((W, gamma) if getattr(h, "double_backward", False) else ()))
        return ops.pm_to_cm(out_pm, B, N)

    @staticmethod
    def backward(ctx, dout):
        if getattr(ctx.h, "double_backward", False) and torch.is_grad_enabled():
            x, PQ, sel, idx, Wst, W, gamma = ctx.saved_tensors
            need = tuple(ctx.needs_input_grad)
            if getattr(ctx.h, "input_only", False):              # the penalty consumes dx alone
                need = need[:2] + (False,) * 4
            return (None,) + EdgeMaxConvBwdFn.apply(ctx.h, ctx.st, need, dout, x, W, gamma, PQ, sel, idx, Wst)
        refuse_double_backward("edgeConv")
        return EdgeMaxConvFn._backward(ctx, dout)

    @staticmethod
    @once_differentiable
    def _backward(ctx, dout):
        x, PQ, sel, idx, Wst = ctx.saved_tensors[:5]
        return (None,) + EdgeMaxConvFn.first_backward(ctx.h, ctx.st, ctx.needs_input_grad, dout, x, PQ, sel, idx, Wst, False)[0]

    @staticmethod
    def first_backward(h, st, need, dout, x, PQ, sel, idx, Wst, keep: bool):
        """-> ((dx, dW, db, dgamma, dbeta), keep ? (r, sums, dPQ, rowptr, src) : None); need = needs_input_grad of (h, x, W, b, gamma, beta)"""
        scale, _, invstd, mean = st
        F_ = sel.shape[1]
        r = ops.cm_to_pm(dout)                                           # a fresh [M,F] tensor: overwritten with g * 1[out > 0]
        sums = edge_max.edge_max_bwd_point(r, sel, PQ, idx, mean, invstd)
        rowptr, src = ops.csr_build(idx, h.B, h.N)
        if h.training:
            dPQ = edge_max.edge_max_bwd_graph(r, sel, PQ, h.k, rowptr, src, scale, idx, mean, invstd, sums)
        else:
            dPQ = edge_max.edge_max_bwd_graph(r, sel, PQ, h.k, rowptr, src, scale)
        kept = (r, sums, dPQ, rowptr, src) if keep else None
        del r
        # dW first: its split-K workspace and the point rows die before dx is made
        dW = unstacked_grad(ops.gemm_tn(dPQ, ops.cm_to_pm(x))) if need[2] else None
        dx = ops.pm_to_cm(ops.gemm_nt(dPQ, Wst.t().contiguous()), h.B, h.N) if need[1] else None
        db = dbias(dPQ[:, F_:], h.training) if need[3] else None
        return (dx, dW, db) + gb(sums, need, 4), kept


class EdgeMaxConvBwdFn(Function):
    """EdgeMaxConvFn's first backward as a differentiable node: (dout, x, W, gamma) -> (dx, dW, db, dgamma, dbeta), the same launches in
    the same order as the plain backward.  Its own backward is the closed-form second derivative THROUGH dx: for the
    cotangent v of dx, one more per-point GEMM VPQ = v Wst^T, the two dbl passes of csrc/edge_max.hip -- the direction's edge sums, then the
    cotangents of the incoming cotangent (ghat) and of PQ (PQbar) --, xbar = PQbar Wst and Wstbar = PQbar^T x + dPQ^T v; no per-edge tensor.
    Eval mode (statistics constant): no PQbar, no xbar.  A cotangent on dW, db, dgamma or dbeta is refused (NotImplementedError); a third
    derivative is refused like every second one of this family (RuntimeError).
    Kept between the two backwards: r [M,F], dPQ [M,2F] (kept, not recomputed: DESIGN.md section 27), the [2F] sums and the reverse CSR."""

    OUTPUTS = ("dx", "dW (conv.conv.weight)", "db (conv.conv.bias)", "dgamma (conv.bn.weight)", "dbeta (conv.bn.bias)")

    @staticmethod
    def forward(ctx, h, st, need, dout, x, W, gamma, PQ, sel, idx, Wst):
        grads, (r, sums, dPQ, rowptr, src) = EdgeMaxConvFn.first_backward(h, st, need, dout, x, PQ, sel, idx, Wst, True)
        ctx.h, ctx.st = h, st
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, PQ, sel, idx, Wst, r, sums, dPQ, rowptr, src)
        return grads

    @staticmethod
    def backward(ctx, *cot):
        if torch.is_grad_enabled():
            raise RuntimeError("edgeConv(double_backward=True) is twice differentiable: its double backward was asked to build a graph "
                               "(create_graph=True), but it has no third derivative")
        for name, c in zip(EdgeMaxConvBwdFn.OUTPUTS[1:], cot[1:]):
            if c is not None:
                raise NotImplementedError("edgeConv(double_backward=True): a cotangent arrived on %s of the first backward; only second "
                                          "derivatives through dx are served (gradient penalties, R1)" % name)
        if cot[0] is None:
            return (None,) * 11
        return EdgeMaxConvBwdFn._backward(ctx, cot[0])

    @staticmethod
    @once_differentiable
    def _backward(ctx, v):
        x, PQ, sel, idx, Wst, r, sums, dPQ, rowptr, src = ctx.saved_tensors
        h = ctx.h
        scale, _, invstd, mean = ctx.st
        F_ = sel.shape[1]
        E = float(idx.numel())
        need = ctx.needs_input_grad                                      # (h, st, need, dout, x, W, gamma, ...)
        v_pm = ops.cm_to_pm(v)
        VPQ = ops.gemm_nt(v_pm, Wst)                                     # [VP | VQ]: no bias
        if h.training:
            dsums = edge_max.edge_max_dbl_point(r, sel, PQ, VPQ, idx, mean, invstd)
            ghat, PQbar = edge_max.edge_max_dbl_graph(r, sel, PQ, VPQ, idx, scale, h.k, rowptr, src, mean, invstd, sums, dsums)
            T1, T2, S = dsums[:F_], dsums[F_:2 * F_], dsums[2 * F_:]
            A = S - sums[:F_] * T1 / E - sums[F_:] * T2 / E
        else:
            A = edge_max.edge_max_dbl_point(r, sel, PQ, VPQ, idx)
            ghat, PQbar = edge_max.edge_max_dbl_graph(r, sel, PQ, VPQ, idx, scale, h.k)
        del VPQ
        dgamma = invstd * A if need[6] else None
        dW = None
        if need[5]:
            if PQbar is not None:
                dWst = ops.gemm_tn(PQbar, ops.cm_to_pm(x))
                ops.gemm_tn(dPQ, v_pm, out=dWst, beta=1.0)
            else:
                dWst = ops.gemm_tn(dPQ, v_pm)
            dW = unstacked_grad(dWst)
        dx = ops.pm_to_cm(ops.gemm_nt(PQbar, Wst.t().contiguous()), h.B, h.N) if (need[4] and PQbar is not None) else None
        dg = ops.pm_to_cm(ghat, h.B, h.N) if need[3] else None
        return (None, None, None, dg, dx, dW, dgamma) + (None,) * 4


class UpsampleEdgeConvFn(Function):
    """out [B,Fout,2N] = the reference's upsample_edgeConv (Generation/modules.py:799-845) without the [B,2Fin,N,k] edge tensor, the
    [B,4Fin,N,k/2] chain behind inte_conv_hk or the merged [B,2Fin,N,2k] tensor: both [1,w] convolutions are products over gathered
    neighbour rows (csrc/edge_window.hip), their central halves per-point GEMMs, the transpose / view chain a column permutation of
    conv2's weight (upsample_images), the final view free in a channel-major result.
    holder: slope, bn1, bn2; parameters of inte_conv_hk, then conv2.  Saved: x, the graph, the pre-norm U [M*T,4Fin] (the one edge-sized
    tensor), the pre-norm y [M,2Fout] and the statistics."""

    @staticmethod
    def forward(ctx, h, x, W1, b1, g1, be1, V, b2, g2, be2):
        B, C, N = x.shape
        k, M, train = h.k, B * N, h.training
        T = k - W1.shape[3] + 1
        x_pm = ops.cm_to_pm(x)
        idx = h.idx if h.idx is not None else ops.knn(x_pm, B, N, k, h.knn_mode)
        Wc1, Wd1, _, Vc, Vd, _, V2p, _, _, _ = upsample_images(W1, V, C, k)
        Q1 = ops.gemm_nt(x_pm, Wc1, b1)
        U, rec = split_records(edge_window.edge_window_gemm(x_pm, idx, Wd1, rowadd=Q1, stats=train), train)
        st1 = bn_stats(h.bn1, train, M * T, g1, be1, records=rec)
        del Q1
        # the activated inte tensor is never stored: BatchNorm + LeakyReLU run in the prologue of the product that consumes it
        st1r = st1.repeat(1, T)                            # per column t*4C + o of the [M, T*4C] view
        Y3 = ops.gemm_nt(U.view(M, T * 4 * C), V2p, pro=(st1r[0], st1r[1], h.slope))
        Q2 = ops.gemm_nt(x_pm, Vc, b2)
        Y, rec = split_records(edge_window.edge_window_gemm(x_pm, idx, Vd, rowadd=Q2, add2=Y3, stats=train), train)
        st2 = bn_stats(h.bn2, train, M, g2, be2, records=rec)
        del Q2, Y3
        out_pm = ops.affine_act(Y, st2[0], st2[1], 0.0)
        h.last_idx = idx
        ctx.h, ctx.st1, ctx.st2, ctx.st1r = h, st1, st2, st1r
        ctx.save_for_backward(x, U, Y, idx, W1, V, g1, g2)
        return ops.pm_to_cm(out_pm, B, N).view(B, V.shape[0] // 2, 2 * N)          # out[b, f, s*N + n] = y[b, 2f+s, n]: a view

    @staticmethod
    def backward(ctx, dout):
        refuse_double_backward("upsample_edgeConv")
        return UpsampleEdgeConvFn._backward(ctx, dout)

    @staticmethod
    @once_differentiable
    def _backward(ctx, dout):
        x, U, Y, idx, W1, V, g1, g2 = ctx.saved_tensors
        h = ctx.h
        B, C, N = x.shape
        k, M, train = h.k, B * N, h.training
        w = W1.shape[3]
        T = k - w + 1
        F2 = V.shape[0]
        _, _, inv1, mu1 = ctx.st1
        sc1r, sh1r, inv1r, mu1r = ctx.st1r
        need = ctx.needs_input_grad
        Wc1, Wd1, Wd1t, Vc, Vd, Vdt, V2p, V2pt, Wc1t, Vct = upsample_images(W1, V, C, k)
        x_pm = ops.cm_to_pm(x)
        dy, sums2 = relu_bn_bwd(dout, Y, ctx.st2, g2, h)
        Uf = U.view(M, T * 4 * C)
        dV = None
        if need[6]:
            dV = torch.empty_like(V)
            dV[:, :C, 0, :k] = ops.gemm_tn(dy, x_pm).unsqueeze(2)
            dV[:, C:, 0, :k] = edge_window.edge_window_wgrad(x_pm, idx, dy, k).view(F2, k, C).permute(0, 2, 1)
            dV[:, :, 0, k:] = ops.gemm_tn(dy, Uf, pro=(sc1r, sh1r, h.slope)).view(F2, T, 4 * C).permute(0, 2, 1).reshape(F2, 2 * C, k)
        # LeakyReLU + BatchNorm of inte_conv_hk: the mask and the column sums come out of the product's epilogue
        gz, t1, t2 = ops.gemm_nt_bnbwd(dy, V2pt, Uf, sc1r, sh1r, mu1r, inv1r, h.slope)
        sums1 = torch.cat([t1.view(T, 4 * C).sum(dim=0), t2.view(T, 4 * C).sum(dim=0)])
        dU = ops.bn_bwd_apply(gz.view(M * T, 4 * C), U, mu1, inv1, g1, used(sums1, train), M * T)
        del gz
        dQ1 = ops.colsum(dU, T)                                            # [M,4C]: the central half sees the sum over the window positions
        dW1 = None
        if need[2]:
            dW1 = torch.empty_like(W1)
            dW1[:, :C, 0, :] = ops.gemm_tn(dQ1, x_pm).unsqueeze(2)
            dW1[:, C:, 0, :] = edge_window.edge_window_wgrad(x_pm, idx, dU, w).view(4 * C, w, C).permute(0, 2, 1)
        dx = None
        if need[1]:
            S = edge_window.edge_window_dgrad(dU, Wd1t, k, C)              # [M,k,C]: the only per-edge tensor made here
            edge_window.edge_window_dgrad(dy, Vdt, k, C, out=S)
            rowptr, src = ops.csr_build(idx, B, N)
            dx_pm = edge_window.edge_window_scatter(S, rowptr, src, ops.gemm_nt(dy, Vct), ops.gemm_nt(dQ1, Wc1t))
            del S
            dx = ops.pm_to_cm(dx_pm, B, N)
        db1 = dbias(dU, train) if need[3] else None
        db2 = dbias(dy, train) if need[7] else None
        return (None, dx, dW1, db1) + gb(sums1, need, 4) + (dV, db2) + gb(sums2, need, 8)


class RankEdgeConvFn(Function):
    """out [B,Fout,N] = relu(bn2(conv[1,k](lrelu(bn1(conv1x1(cat[x_i, x_j - x_i]))))))   (the reference's deform_edgeConv_simple /
    deform_edgeConv_first, Generation/modules.py:1394-1466) without the [B,2Fin,N,k] edge tensor or the activated [B,F1,N,k] tensor in
    forward: the per-point GEMM, the first BatchNorm's statistics from edge_max's gather pass over PQ, and the [1,k] convolution as a
    product with K = k*F1 whose A operand is formed in LDS (csrc/edge_rank.hip).
    holder: slope, bn1, bn2; parameters of inte_conv_hk, then conv2.  Saved: x, PQ, the pre-norm y [M,Fout], the graph and the
    statistics; the backward holds one per-edge buffer, da [M,k,F1]."""

    @staticmethod
    def forward(ctx, h, x, W1, b1, g1, be1, W2, b2, g2, be2):
        B, Fin, N = x.shape
        k, M, train = h.k, B * N, h.training
        x_pm = ops.cm_to_pm(x)
        idx = h.idx if h.idx is not None else ops.knn(x_pm, B, N, k, h.knn_mode)
        Wst, _, W2i, _ = rank_images(W1, W2)
        PQ = ops.gemm_nt(x_pm, Wst, pq_bias(b1))
        st1 = bn_stats(h.bn1, train, M * k, g1, be1, records=edge_records(PQ, idx) if train else None)
        Y, rec = split_records(edge_rank.edge_rank_gemm(PQ, idx, st1[0], st1[1], W2i, b2, stats=train, slope=h.slope), train)
        st2 = bn_stats(h.bn2, train, M, g2, be2, records=rec)
        del rec
        out_pm = ops.affine_act(Y, st2[0], st2[1], 0.0)
        h.last_idx = idx
        ctx.h, ctx.st1, ctx.st2 = h, st1, st2
        ctx.save_for_backward(x, PQ, Y, idx, W1, W2, g2)
        return ops.pm_to_cm(out_pm, B, N)

    @staticmethod
    def backward(ctx, dout):
        refuse_double_backward("deform_edgeConv")
        return RankEdgeConvFn._backward(ctx, dout)

    @staticmethod
    @once_differentiable
    def _backward(ctx, dout):
        x, PQ, Y, idx, W1, W2, g2 = ctx.saved_tensors
        h = ctx.h
        B, Fin, N = x.shape
        k, train = h.k, h.training
        F1, Fout = W1.shape[0], W2.shape[0]
        sc1, sh1, inv1, mu1 = ctx.st1
        need = ctx.needs_input_grad
        Wst, Wstt, W2i, W2t = rank_images(W1, W2)
        dy, sums2 = relu_bn_bwd(dout, Y, ctx.st2, g2, h)
        # LeakyReLU + BatchNorm of inte_conv_hk: da [M,k,F1] is the only per-edge tensor of the layer
        da, sums1 = edge_rank.edge_rank_dgrad(dy, W2t, PQ, idx, sc1, sh1, mu1, inv1, h.slope)
        rowptr, src = ops.csr_build(idx, B, N)
        dPQ = rank_scatter(da, rowptr, src, ctx.st1, PQ, idx, sums1, train)
        del da
        dW2 = None
        if need[6]:                                                      # after da has died: its split workspace is not held beside da
            dW2 = edge_rank.edge_rank_wgrad(PQ, idx, sc1, sh1, dy, h.slope).view(Fout, k, F1).permute(0, 2, 1).unsqueeze(2).contiguous()
        dW1 = unstacked_grad(ops.gemm_tn(dPQ, ops.cm_to_pm(x))) if need[2] else None
        dx = ops.pm_to_cm(ops.gemm_nt(dPQ, Wstt), B, N) if need[1] else None
        db1 = dbias(dPQ[:, F1:], train) if need[3] else None
        db2 = dbias(dy, train) if need[7] else None
        return (None, dx, dW1, db1) + gb(sums1, need, 4) + (dW2, db2) + gb(sums2, need, 8)


class WeightedRankEdgeConvFn(Function):
    """out [B,Fout,N] = relu(bn_c(conv[1,k](h * s)))   (the reference's deform_edgeConv_feat, Generation/modules.py:1543-1599) with
    h = lrelu(bn_h(conv1x1(e))), s = softmax over the k ranks of the shared three-layer MLP conv_fea(e) (or the MLP's output itself with
    softmax=False) and e = cat[x_i, x_j - x_i], without e, h, s or h*s in memory, forward or backward.
    Both first layers are per-point GEMMs (PQ_h [M,2Fin], PQ_1 [M,32], statistics from edge_max's gather pass); the MLP's narrow rows
    z1 [M*k,16], z2 [M*k,64] and its pre-norm output z3 [M*k,Fin] (the one edge-sized tensor of the forward) are stored; the [1,k]
    convolution forms h*s in LDS from gathered rows of PQ_h, z3 and the per-(point, channel) softmax normaliser (csrc/edge_rank.hip,
    spgan.edge_weight).  The backward holds two further edge-sized buffers: du and g3 / dz3.
    holder: softmax, slope, bns = the five nn.BatchNorm2d modules (h, 1, 2, 3, c); parameters of inte_conv_hk, conv_fea.0/1,
    conv_fea.3/4, conv_fea.6/7 and conv2."""

    @staticmethod
    def forward(ctx, h, x, *params):
        Wh, bh, gh, beh, Wf1, bf1, g1, be1, Wf2, bf2, g2, be2, Wf3, bf3, g3, be3, W2, b2, gc, bec = params
        B, Fin, N = x.shape
        k, M, train = h.k, B * N, h.training
        E = M * k
        x_pm = ops.cm_to_pm(x)
        idx = h.idx if h.idx is not None else ops.knn(x_pm, B, N, k, h.knn_mode)
        Wst_h, Wst_1, _, Wm2, _, Wm3, _, W2i, _ = weight_images(Wh, Wf1, Wf2, Wf3, W2)
        # exact=True: fp32 operands whatever ops.set_mfma_operands selected
        PQh = ops.gemm_nt(x_pm, Wst_h, pq_bias(bh), exact=True)
        PQ1 = ops.gemm_nt(x_pm, Wst_1, pq_bias(bf1), exact=True)
        sth = bn_stats(h.bns[0], train, E, gh, beh, records=edge_records(PQh, idx) if train else None)
        st1 = bn_stats(h.bns[1], train, E, g1, be1, records=edge_records(PQ1, idx) if train else None)
        z1 = edge_weight.edge_weight_gather(PQ1, idx)
        if train:
            z2, m, v = ops.gemm_nt(z1, Wm2, bf2, pro=(st1[0], st1[1], h.slope), stats=True, exact=True)
            st2 = bn_stats(h.bns[2], True, E, g2, be2, moments=(m, v))
            z3, m, v = ops.gemm_nt(z2, Wm3, bf3, pro=(st2[0], st2[1], h.slope), stats=True, exact=True)
            st3 = bn_stats(h.bns[3], True, E, g3, be3, moments=(m, v))
        else:
            st2 = bn_stats(h.bns[2], False, E, g2, be2)
            z2 = ops.gemm_nt(z1, Wm2, bf2, pro=(st1[0], st1[1], h.slope), exact=True)
            st3 = bn_stats(h.bns[3], False, E, g3, be3)
            z3 = ops.gemm_nt(z2, Wm3, bf3, pro=(st2[0], st2[1], h.slope), exact=True)
        norm = edge_weight.edge_weight_norm(z3, k, st3[0], st3[1], h.slope) if h.softmax else None
        Y, rec = split_records(edge_weight.edge_weight_gemm(PQh, idx, sth[0], sth[1], z3, st3[0], st3[1], norm, W2i, b2, stats=train, slope=h.slope),
                               train)
        stc = bn_stats(h.bns[4], train, M, gc, bec, records=rec)
        del rec
        out_pm = ops.affine_act(Y, stc[0], stc[1], 0.0)
        h.last_idx = idx
        ctx.h, ctx.st, ctx.norm = h, (sth, st1, st2, st3, stc), norm
        ctx.save_for_backward(x, PQh, PQ1, z1, z2, z3, Y, idx, Wh, Wf1, Wf2, Wf3, W2, g2, g3, gc)
        return ops.pm_to_cm(out_pm, B, N)

    @staticmethod
    def backward(ctx, dout):
        refuse_double_backward("deform_edgeConv_feat")
        return WeightedRankEdgeConvFn._backward(ctx, dout)

    @staticmethod
    @once_differentiable
    def _backward(ctx, dout):
        x, PQh, PQ1, z1, z2, z3, Y, idx, Wh, Wf1, Wf2, Wf3, W2, g2, g3, gc = ctx.saved_tensors
        h = ctx.h
        B, Fin, N = x.shape
        k, M, train = h.k, B * N, h.training
        E = M * k
        Fout, F1, Fm = W2.shape[0], Wf1.shape[0], Wf2.shape[0]
        sth, st1, (sc2, sh2, inv2, mu2), (sc3, sh3, inv3, mu3), stc = ctx.st
        (sch, shh, invh, muh), (sc1, sh1, inv1, mu1) = sth, st1
        need = ctx.needs_input_grad
        _, _, Wall_t, _, Wm2t, _, Wm3t, _, W2t = weight_images(Wh, Wf1, Wf2, Wf3, W2)
        dy, sumsc = relu_bn_bwd(dout, Y, stc, gc, h)
        # the product h*s, both LeakyReLUs and the softmax: du and g3 [M,k,Fin] are the two per-edge buffers of the backward
        du, sumsh, gz3, sums3 = edge_weight.edge_weight_dgrad(dy, W2t, PQh, idx, sch, shh, muh, invh, z3, sc3, sh3, mu3, inv3, ctx.norm, h.slope)
        rowptr, src = ops.csr_build(idx, B, N)
        dPQh = rank_scatter(du, rowptr, src, sth, PQh, idx, sumsh, train)
        del du
        # the weight MLP, last layer first
        dz3 = ops.bn_bwd_apply(gz3, z3, mu3, inv3, g3, used(sums3, train), E)
        del gz3
        dWf3 = ops.gemm_tn(dz3, z2, pro=(sc2, sh2, h.slope), exact=True).view(Fin, Fm, 1, 1) if need[14] else None
        dbf3 = dbias(dz3, train) if need[15] else None
        gz2, t1, t2 = ops.gemm_nt_bnbwd(dz3, Wm3t, z2, sc2, sh2, mu2, inv2, h.slope, exact=True)
        del dz3
        sums2 = torch.cat([t1, t2])
        dz2 = ops.bn_bwd_apply(gz2, z2, mu2, inv2, g2, used(sums2, train), E)
        del gz2
        dWf2 = ops.gemm_tn(dz2, z1, pro=(sc1, sh1, h.slope), exact=True).view(Fm, F1, 1, 1) if need[10] else None
        dbf2 = dbias(dz2, train) if need[11] else None
        gz1, t1, t2 = ops.gemm_nt_bnbwd(dz2, Wm2t, z1, sc1, sh1, mu1, inv1, h.slope, exact=True)
        del dz2
        sums1 = torch.cat([t1, t2])
        dPQ1 = rank_scatter(gz1.view(M, k, F1), rowptr, src, st1, PQ1, idx, sums1, train)
        del gz1
        dW2 = None
        if need[18]:                                                     # after du and g3 have died: its split workspace is not held beside them
            dW2 = edge_weight.edge_weight_wgrad(PQh, idx, sch, shh, z3, sc3, sh3, ctx.norm, dy, h.slope)
            dW2 = dW2.view(Fout, k, Fin).permute(0, 2, 1).unsqueeze(2).contiguous()
        dPQ = torch.cat([dPQh, dPQ1], dim=1)                             # [M, 2Fin + 32]: both branches feed one product pair
        dWh = dWf1 = None
        if need[2] or need[6]:
            dWst = ops.gemm_tn(dPQ, ops.cm_to_pm(x), exact=True)         # rows of dW'_P, then of dW'_Q, per branch
            dWh, dWf1 = unstacked_grad(dWst[:2 * Fin]), unstacked_grad(dWst[2 * Fin:])
        dx = ops.pm_to_cm(ops.gemm_nt(dPQ, Wall_t, exact=True), B, N) if need[1] else None
        dbh = dbias(dPQh[:, Fin:], train) if need[3] else None
        dbf1 = dbias(dPQ1[:, F1:], train) if need[7] else None
        db2 = dbias(dy, train) if need[19] else None
        return (None, dx, dWh, dbh) + gb(sumsh, need, 4) + (dWf1, dbf1) + gb(sums1, need, 8) + (dWf2, dbf2) + gb(sums2, need, 12) + \
            (dWf3, dbf3) + gb(sums3, need, 16) + (dW2, db2) + gb(sumsc, need, 20)


class CoordRankEdgeConvFn(Function):
    """out [B,Fout,N] = lrelu(bn_c(conv[1,k](h * s)))   (the reference's deform_edgeConv, Generation/modules.py:1468-1540): the weighted layer
    above with the weight MLP fed by w0 = a_f * a_x, a_f = lrelu(bn_f(conv_fea(e))) over e = cat[x_i, x_j - x_i] and a_x =
    lrelu(bn_x(conv_xyz(y))) over y = cat[pc_i, pc_j - pc_i], both gathered through the one kNN graph of x; s = softmax over the k ranks
    of conv_all(w0) (or conv_all's output itself with softmax=False).  Three per-point GEMMs (PQ_h [M,2Fin], PQ_f [M,32] from x, PQ_x
    [M,32] from pc); of the two 16-wide branches only their product w0 [M*k,16] is stored (edge_weight.edge_weight_gather2) and the
    backward recomputes a_f and a_x from PQ_f, PQ_x and the graph (edge_weight_split).  z2 [M*k,64] and z3 [M*k,Fin] (the one edge-sized
    tensor of the forward) are stored as in the weighted layer; the backward holds du and g3 / dz3 beside it.
    holder: softmax, slope, bns = the six nn.BatchNorm2d modules (h, f, x, 2, 3, c); parameters of inte_conv_hk, conv_fea, conv_xyz,
    conv_all.0/1, conv_all.3/4 and conv2.  Differentiable in x, pc and every parameter."""

    @staticmethod
    def forward(ctx, h, x, pc, *params):
        Wh, bh, gh, beh, Wf, bf, gf, bef, Wx, bx, gx, bex, Wa2, ba2, g2, be2, Wa3, ba3, g3, be3, W2, b2, gc, bec = params
        B, Fin, N = x.shape
        k, M, train = h.k, B * N, h.training
        E = M * k
        x_pm, pc_pm = ops.cm_to_pm(x), ops.cm_to_pm(pc)
        idx = h.idx if h.idx is not None else ops.knn(x_pm, B, N, k, h.knn_mode)
        Wst_h, Wst_f, Wst_x, _, _, Wm2, _, Wm3, _, W2i, _ = coord_images(Wh, Wf, Wx, Wa2, Wa3, W2)
        # exact=True: fp32 operands whatever ops.set_mfma_operands selected
        PQh = ops.gemm_nt(x_pm, Wst_h, pq_bias(bh), exact=True)
        PQf = ops.gemm_nt(x_pm, Wst_f, pq_bias(bf), exact=True)
        PQx = ops.gemm_nt(pc_pm, Wst_x, pq_bias(bx), exact=True)
        sth = bn_stats(h.bns[0], train, E, gh, beh, records=edge_records(PQh, idx) if train else None)
        stf = bn_stats(h.bns[1], train, E, gf, bef, records=edge_records(PQf, idx) if train else None)
        stx = bn_stats(h.bns[2], train, E, gx, bex, records=edge_records(PQx, idx) if train else None)
        w0 = edge_weight.edge_weight_gather2(PQf, PQx, idx, stf[0], stf[1], stx[0], stx[1], h.slope)
        # w0 is activated already: conv_all.0 reads it without a prologue
        if train:
            z2, m, v = ops.gemm_nt(w0, Wm2, ba2, stats=True, exact=True)
            st2 = bn_stats(h.bns[3], True, E, g2, be2, moments=(m, v))
            z3, m, v = ops.gemm_nt(z2, Wm3, ba3, pro=(st2[0], st2[1], h.slope), stats=True, exact=True)
            st3 = bn_stats(h.bns[4], True, E, g3, be3, moments=(m, v))
        else:
            st2 = bn_stats(h.bns[3], False, E, g2, be2)
            z2 = ops.gemm_nt(w0, Wm2, ba2, exact=True)
            st3 = bn_stats(h.bns[4], False, E, g3, be3)
            z3 = ops.gemm_nt(z2, Wm3, ba3, pro=(st2[0], st2[1], h.slope), exact=True)
        norm = edge_weight.edge_weight_norm(z3, k, st3[0], st3[1], h.slope) if h.softmax else None
        Y, rec = split_records(edge_weight.edge_weight_gemm(PQh, idx, sth[0], sth[1], z3, st3[0], st3[1], norm, W2i, b2, stats=train, slope=h.slope),
                               train)
        stc = bn_stats(h.bns[5], train, M, gc, bec, records=rec)
        del rec
        out_pm = ops.affine_act(Y, stc[0], stc[1], h.slope)
        h.last_idx = idx
        ctx.h, ctx.st, ctx.norm = h, (sth, stf, stx, st2, st3, stc), norm
        ctx.save_for_backward(x, pc, PQh, PQf, PQx, w0, z2, z3, Y, idx, Wh, Wf, Wx, Wa2, Wa3, W2, g2, g3, gc)
        return ops.pm_to_cm(out_pm, B, N)

    @staticmethod
    def backward(ctx, dout):
        refuse_double_backward("deform_edgeConv")
        return CoordRankEdgeConvFn._backward(ctx, dout)

    @staticmethod
    @once_differentiable
    def _backward(ctx, dout):
        x, pc, PQh, PQf, PQx, w0, z2, z3, Y, idx, Wh, Wf, Wx, Wa2, Wa3, W2, g2, g3, gc = ctx.saved_tensors
        h = ctx.h
        B, Fin, N = x.shape
        k, M, train = h.k, B * N, h.training
        E = M * k
        Fout, F1, Fm = W2.shape[0], Wf.shape[0], Wa2.shape[0]
        sth, stf, stx, (sc2, sh2, inv2, mu2), (sc3, sh3, inv3, mu3), stc = ctx.st
        sch, shh, invh, muh = sth
        need = ctx.needs_input_grad
        _, _, _, Wall_t, Wst_xt, _, Wm2t, _, Wm3t, _, W2t = coord_images(Wh, Wf, Wx, Wa2, Wa3, W2)
        dy, sumsc = lrelu_bn_bwd(dout, Y, stc, gc, h, h.slope)
        # the product h*s, both LeakyReLUs and the softmax: du and g3 [M,k,Fin] are the two per-edge buffers of the backward
        du, sumsh, gz3, sums3 = edge_weight.edge_weight_dgrad(dy, W2t, PQh, idx, sch, shh, muh, invh, z3, sc3, sh3, mu3, inv3, ctx.norm, h.slope)
        rowptr, src = ops.csr_build(idx, B, N)
        dPQh = rank_scatter(du, rowptr, src, sth, PQh, idx, sumsh, train)
        del du
        # the weight MLP, last layer first
        dz3 = ops.bn_bwd_apply(gz3, z3, mu3, inv3, g3, used(sums3, train), E)
        del gz3
        dWa3 = ops.gemm_tn(dz3, z2, pro=(sc2, sh2, h.slope), exact=True).view(Fin, Fm, 1, 1) if need[19] else None
        dba3 = dbias(dz3, train) if need[20] else None
        gz2, t1, t2 = ops.gemm_nt_bnbwd(dz3, Wm3t, z2, sc2, sh2, mu2, inv2, h.slope, exact=True)
        del dz3
        sums2 = torch.cat([t1, t2])
        dz2 = ops.bn_bwd_apply(gz2, z2, mu2, inv2, g2, used(sums2, train), E)
        del gz2
        dWa2 = ops.gemm_tn(dz2, w0, exact=True).view(Fm, F1, 1, 1) if need[15] else None
        dba2 = dbias(dz2, train) if need[16] else None
        # no BatchNorm between w0 and conv_all.0: a plain product, then the two branches' LeakyReLU'd BatchNorms
        dw0 = ops.gemm_nt(dz2, Wm2t, exact=True)
        del dz2
        gf_, sumsf, gx_, sumsx = edge_weight.edge_weight_split(dw0, PQf, PQx, idx, stf[0], stf[1], stf[3], stf[2], stx[0], stx[1], stx[3], stx[2],
                                                               h.slope)
        del dw0
        dPQf = rank_scatter(gf_, rowptr, src, stf, PQf, idx, sumsf, train)
        del gf_
        dPQx = rank_scatter(gx_, rowptr, src, stx, PQx, idx, sumsx, train)
        del gx_
        dW2 = None
        if need[23]:                                                     # after du and g3 have died: its split workspace is not held beside them
            dW2 = edge_weight.edge_weight_wgrad(PQh, idx, sch, shh, z3, sc3, sh3, ctx.norm, dy, h.slope)
            dW2 = dW2.view(Fout, k, Fin).permute(0, 2, 1).unsqueeze(2).contiguous()
        dPQ = torch.cat([dPQh, dPQf], dim=1)                             # [M, 2Fin + 32]: both feature-side branches feed one product pair
        dWh = dWf = dWx = None
        if need[3] or need[7]:
            dWst = ops.gemm_tn(dPQ, ops.cm_to_pm(x), exact=True)         # rows of dW'_P, then of dW'_Q, per branch
            dWh, dWf = unstacked_grad(dWst[:2 * Fin]), unstacked_grad(dWst[2 * Fin:])
        dx = ops.pm_to_cm(ops.gemm_nt(dPQ, Wall_t, exact=True), B, N) if need[1] else None
        if need[11]:
            dWx = unstacked_grad(ops.gemm_tn(dPQx, ops.cm_to_pm(pc), exact=True))
        dpc = ops.pm_to_cm(ops.gemm_nt(dPQx, Wst_xt, exact=True), B, N) if need[2] else None
        dbh = dbias(dPQh[:, Fin:], train) if need[4] else None
        dbf = dbias(dPQf[:, F1:], train) if need[8] else None
        dbx = dbias(dPQx[:, F1:], train) if need[12] else None
        db2 = dbias(dy, train) if need[24] else None
        return (None, dx, dpc, dWh, dbh) + gb(sumsh, need, 5) + (dWf, dbf) + gb(sumsf, need, 9) + (dWx, dbx) + gb(sumsx, need, 13) + \
            (dWa2, dba2) + gb(sums2, need, 17) + (dWa3, dba3) + gb(sums3, need, 21) + (dW2, db2) + gb(sumsc, need, 25)


class BilateralUpsampleEdgeConvFn(Function):
    """out [B,Fout,2N] = the reference's bilateral_upsample_edgeConv (Generation/modules.py:847-925): upsample_edgeConv whose interpolated
    tensor lrelu(bn1(inte_conv_hk(e))) is multiplied, element by element, by deform_edgeConv's weight s = softmax over the k ranks of
    conv_all(conv_fea(e) * conv_xyz(y)) (2C channels) before conv2 reads it as its taps k..2k-1.
    inte_conv_hk's output channels are computed in the order o' = h*2C + c' (bilateral_images), so that the pre-norm U [M*T, 4C] with rows
    (i,t) is also [M, k, 2C] with rows (i, r' = 2t + h); the weight branch runs over the graph in that rank order (paired_ranks), so that its
    pre-norm output z3 [M*k, 2C] has the same rows.  The product Y3 = (lrelu(bn1(U)) * s).flat V2i^T forms its A operand in LDS from U, z3
    and the softmax normaliser (edge_weight.edge_stored_gemm); the activated tensor, s and their product are never stored.
    Forward keeps U and z3 (two edge-sized tensors, E = 4 M k 2C bytes each) beside w0 [M*k,16] and z2 [M*k,64]; the backward adds gU / dU
    and g3 / dz3 and the window dgrad's S (E/2)  (DESIGN.md section 23).
    holder: softmax, slope, bns = the six nn.BatchNorm2d modules (inte, fea, xyz, all.1, all.4, conv2); parameters of inte_conv_hk, conv_fea,
    conv_xyz, conv_all.0/1, conv_all.3/4 and conv2.  Differentiable in x, pc and every parameter."""

    @staticmethod
    def forward(ctx, h, x, pc, *params):
        W1, b1, g1, be1, Wf, bf, gf, bef, Wx, bx, gx, bex, Wa2, ba2, g2, be2, Wa3, ba3, g3, be3, V, b2, gc, bec = params
        B, C, N = x.shape
        k, M, train = h.k, B * N, h.training
        T, E = k // 2, M * k
        x_pm, pc_pm = ops.cm_to_pm(x), ops.cm_to_pm(pc)
        idx = h.idx if h.idx is not None else ops.knn(x_pm, B, N, k, h.knn_mode)
        idxp = paired_ranks(idx)
        Wc1, Wd1, _, Vc, Vd, _, _, V2i, _, Wst_f, Wst_x, _, _, Wm2, _, Wm3, _ = bilateral_images(W1, Wf, Wx, Wa2, Wa3, V, C, k)
        # exact=True: fp32 operands whatever ops.set_mfma_operands selected
        Q1 = ops.gemm_nt(x_pm, Wc1, parity_major(b1.detach()), exact=True)
        U, rec = split_records(edge_window.edge_window_gemm(x_pm, idx, Wd1, rowadd=Q1, stats=train), train)
        del Q1
        if train:                                          # the module's BatchNorm keeps the reference's channel order
            rec = (channel_major(rec[0], 1),) + tuple(rec[1:])
        st1 = parity_major(bn_stats(h.bns[0], train, M * T, g1, be1, records=rec), 1)
        del rec
        PQf = ops.gemm_nt(x_pm, Wst_f, pq_bias(bf), exact=True)
        PQx = ops.gemm_nt(pc_pm, Wst_x, pq_bias(bx), exact=True)
        stf = bn_stats(h.bns[1], train, E, gf, bef, records=edge_records(PQf, idx) if train else None)
        stx = bn_stats(h.bns[2], train, E, gx, bex, records=edge_records(PQx, idx) if train else None)
        w0 = edge_weight.edge_weight_gather2(PQf, PQx, idxp, stf[0], stf[1], stx[0], stx[1], h.slope)
        if train:
            z2, m, v = ops.gemm_nt(w0, Wm2, ba2, stats=True, exact=True)
            st2 = bn_stats(h.bns[3], True, E, g2, be2, moments=(m, v))
            z3, m, v = ops.gemm_nt(z2, Wm3, ba3, pro=(st2[0], st2[1], h.slope), stats=True, exact=True)
            st3 = bn_stats(h.bns[4], True, E, g3, be3, moments=(m, v))
        else:
            st2 = bn_stats(h.bns[3], False, E, g2, be2)
            z2 = ops.gemm_nt(w0, Wm2, ba2, exact=True)
            st3 = bn_stats(h.bns[4], False, E, g3, be3)
            z3 = ops.gemm_nt(z2, Wm3, ba3, pro=(st2[0], st2[1], h.slope), exact=True)
        norm = edge_weight.edge_weight_norm(z3, k, st3[0], st3[1], h.slope) if h.softmax else None
        Y3 = edge_weight.edge_stored_gemm(U, k, st1[0], st1[1], z3, st3[0], st3[1], norm, V2i, slope=h.slope)
        Q2 = ops.gemm_nt(x_pm, Vc, b2, exact=True)
        Y, rec = split_records(edge_window.edge_window_gemm(x_pm, idx, Vd, rowadd=Q2, add2=Y3, stats=train), train)
        stc = bn_stats(h.bns[5], train, M, gc, bec, records=rec)
        del Q2, Y3, rec
        out_pm = ops.affine_act(Y, stc[0], stc[1], 0.0)
        h.last_idx = idx
        ctx.h, ctx.st, ctx.norm = h, (st1, stf, stx, st2, st3, stc), norm
        ctx.save_for_backward(x, pc, U, PQf, PQx, w0, z2, z3, Y, idx, W1, Wf, Wx, Wa2, Wa3, V, g1, g2, g3, gc)
        return ops.pm_to_cm(out_pm, B, N).view(B, V.shape[0] // 2, 2 * N)          # out[b, f, s*N + n] = y[b, 2f+s, n]: a view

    @staticmethod
    def backward(ctx, dout):
        refuse_double_backward("bilateral_upsample_edgeConv")
        return BilateralUpsampleEdgeConvFn._backward(ctx, dout)

    @staticmethod
    @once_differentiable
    def _backward(ctx, dout):
        x, pc, U, PQf, PQx, w0, z2, z3, Y, idx, W1, Wf, Wx, Wa2, Wa3, V, g1, g2, g3, gc = ctx.saved_tensors
        h = ctx.h
        B, C, N = x.shape
        k, M, train = h.k, B * N, h.training
        w = W1.shape[3]
        T, E = k // 2, M * k
        F2, F1, Fm, Fw = V.shape[0], Wf.shape[0], Wa2.shape[0], 2 * C
        (sc1, sh1, inv1, mu1), stf, stx, (sc2, sh2, inv2, mu2), (sc3, sh3, inv3, mu3), stc = ctx.st
        need = ctx.needs_input_grad
        _, _, Wd1t, _, _, Vdt, Vct, _, V2it, _, _, Wst_xt, Wcat_t, _, Wm2t, _, Wm3t = bilateral_images(W1, Wf, Wx, Wa2, Wa3, V, C, k)
        x_pm = ops.cm_to_pm(x)
        idxp = paired_ranks(idx)
        dy, sumsc = relu_bn_bwd(dout, Y, stc, gc, h)
        # the product act(U) * s, both LeakyReLUs and the softmax: gU and gz3 [M,k,2C] are the two per-edge buffers of the backward
        gU, sums1, gz3, sums3 = edge_weight.edge_stored_dgrad(dy, V2it, U, k, sc1, sh1, mu1, inv1, z3, sc3, sh3, mu3, inv3, ctx.norm, h.slope)
        # the weight MLP, last layer first
        dz3 = ops.bn_bwd_apply(gz3, z3, mu3, inv3, g3, used(sums3, train), E)
        del gz3
        dWa3 = ops.gemm_tn(dz3, z2, pro=(sc2, sh2, h.slope), exact=True).view(Fw, Fm, 1, 1) if need[19] else None
        dba3 = dbias(dz3, train) if need[20] else None
        gz2, t1, t2 = ops.gemm_nt_bnbwd(dz3, Wm3t, z2, sc2, sh2, mu2, inv2, h.slope, exact=True)
        del dz3
        sums2 = torch.cat([t1, t2])
        dz2 = ops.bn_bwd_apply(gz2, z2, mu2, inv2, g2, used(sums2, train), E)
        del gz2
        dWa2 = ops.gemm_tn(dz2, w0, exact=True).view(Fm, F1, 1, 1) if need[15] else None
        dba2 = dbias(dz2, train) if need[16] else None
        dw0 = ops.gemm_nt(dz2, Wm2t, exact=True)
        del dz2
        gf_, sumsf, gx_, sumsx = edge_weight.edge_weight_split(dw0, PQf, PQx, idxp, stf[0], stf[1], stf[3], stf[2], stx[0], stx[1], stx[3], stx[2],
                                                               h.slope)
        del dw0
        rowptr, src = ops.csr_build(idxp, B, N)
        dPQf = rank_scatter(gf_, rowptr, src, stf, PQf, idxp, sumsf, train)
        del gf_
        dPQx = rank_scatter(gx_, rowptr, src, stx, PQx, idxp, sumsx, train)
        del gx_
        # LeakyReLU + BatchNorm of inte_conv_hk, in the channel order o' of U
        dU = ops.bn_bwd_apply(gU.view(M * T, 4 * C), U, mu1, inv1, parity_major(g1.detach()), used(sums1, train), M * T)
        del gU
        dQ1 = ops.colsum(dU, T)                                            # [M,4C]: the central half sees the sum over the window positions
        dV = None
        if need[23]:
            dV = torch.empty_like(V)
            dV[:, :C, 0, :k] = ops.gemm_tn(dy, x_pm, exact=True).unsqueeze(2)
            dV[:, C:, 0, :k] = edge_window.edge_window_wgrad(x_pm, idx, dy, k).view(F2, k, C).permute(0, 2, 1)
            dV2i = edge_weight.edge_stored_wgrad(U, k, sc1, sh1, z3, sc3, sh3, ctx.norm, dy, h.slope)
            dV[:, :, 0, k:] = dV2i.view(F2, T, 2, 2 * C).permute(0, 3, 2, 1).reshape(F2, 2 * C, k)
        dW1 = None
        if need[3]:
            dW1p = torch.empty((4 * C, 2 * C, 1, w), dtype=torch.float32, device=x.device)
            dW1p[:, :C, 0, :] = ops.gemm_tn(dQ1, x_pm, exact=True).unsqueeze(2)
            dW1p[:, C:, 0, :] = edge_window.edge_window_wgrad(x_pm, idx, dU, w).view(4 * C, w, C).permute(0, 2, 1)
            dW1 = channel_major(dW1p)
        dx = None
        if need[1]:
            S = edge_window.edge_window_dgrad(dU, Wd1t, k, C)              # [M,k,C]
            edge_window.edge_window_dgrad(dy, Vdt, k, C, out=S)
            rowptr, src = ops.csr_build(idx, B, N)
            # both per-point products of the inte and the conv_fea branch in one: [dQ1 | dPQf] [Wc1 ; Wst_f]
            dx_pm = edge_window.edge_window_scatter(S, rowptr, src, ops.gemm_nt(dy, Vct, exact=True),
                                                    ops.gemm_nt(torch.cat([dQ1, dPQf], dim=1), Wcat_t, exact=True))
            del S
            dx = ops.pm_to_cm(dx_pm, B, N)
        dWf = unstacked_grad(ops.gemm_tn(dPQf, x_pm, exact=True)) if need[7] else None
        dWx = unstacked_grad(ops.gemm_tn(dPQx, ops.cm_to_pm(pc), exact=True)) if need[11] else None
        dpc = ops.pm_to_cm(ops.gemm_nt(dPQx, Wst_xt, exact=True), B, N) if need[2] else None
        db1 = channel_major(dbias(dU, train)) if need[4] else None
        dbf = dbias(dPQf[:, F1:], train) if need[8] else None
        dbx = dbias(dPQx[:, F1:], train) if need[12] else None
        db2 = dbias(dy, train) if need[24] else None
        s1 = channel_major(sums1.view(2, 4 * C), 1).reshape(-1)           # [sum g | sum g*uhat], each back in the module's channel order
        return (None, dx, dpc, dW1, db1) + gb(s1, need, 5) + (dWf, dbf) + gb(sumsf, need, 9) + (dWx, dbx) + gb(sumsx, need, 13) + \
            (dWa2, dba2) + gb(sums2, need, 17) + (dWa3, dba3) + gb(sums3, need, 21) + (dV, db2) + gb(sumsc, need, 25)


# ----------------------------------------------------------------------------- the blocks' tail
class PointMaxFn(Function):
    """[B,C,N] -> [B,C]: the max over the points in front of a block's global branch (torch.max(x, 2) / MaxPool2d((1, N)) in the reference);
    the cotangent goes to the arg-max point."""

    @staticmethod
    def forward(ctx, x):
        B, C, N = x.shape
        out, arg = ops.maxpool(ops.cm_to_pm(x), B, N)
        ctx.B, ctx.N = B, N
        ctx.save_for_backward(arg)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        arg, = ctx.saved_tensors
        return ops.pm_to_cm(ops.scatter_rows(dout, arg, ctx.B * ctx.N), ctx.B, ctx.N)


class _Shape:
    def __init__(self, B, N, training):
        self.B, self.N, self.training = B, N, training


class BlockTailFn(Function):
    """(x_out, g_out) of a bilateral / deform block (Generation/modules.py:928-1391) from Y [B,C,L], the channel-major output of the block's
    edge convolution, and the global vectors xs [B,Cs], g [B,Cg] | None.  With a = lrelu(bn(Y)), the block's BatchNorm1d + LeakyReLU:
      plain blocks:   x_out = cat[xs broadcast, a] [B,Cs+C,L], g_out = cat[g broadcast, a] [B,Cg+C,L] | None -- one pass over Y writes both
                      (csrc/block_tail.hip); neither a nor the repeated vectors exist on their own.
      middle blocks   (Wa, ba, ga, bea = add_cov's Conv1d(Cs+C -> Fo) and BatchNorm1d given): x_out = lrelu(bn_add(Wa cat[xs broadcast, a] + ba))
                      [B,Fo,L] without the concatenation: Wa = [W_s | W_e], W_s xs[b] + ba enters the product as a per-shape bias, a as the
                      operand prologue on the point-major copy of Y, bn_add's statistics come from the product's epilogue.  In backward
                      the cotangent of a through the product is brought to channel-major once and joins g_out's inside the tail's backward
                      (`extra`), so that the block's BatchNorm backward sees one summed cotangent; dxs and dW_s come from the per-shape
                      column sums of the product's cotangent.
    holder: name, training, slope, bn (the block's BatchNorm1d), bn_add (middle blocks).  An output nobody uses reaches the kernels as a
    NULL cotangent, not as zeros.  Saved (all through save_for_backward, so that nothing of the tail outlives its backward): Y, the
    statistics and, in the middle blocks, the point-major copy of Y and the pre-norm product Z [B*L,Fo]."""

    @staticmethod
    def forward(ctx, h, Y, xs, g, gamma, beta, Wa, ba, ga, bea):
        B, C, L = Y.shape
        train, middle = h.training, Wa is not None
        st = bn_stats(h.bn, train, B * L, gamma, beta, records=block_tail.cm_stats(Y) if train else None)
        x_out = g_out = Z = sta = Y_pm = None
        if not middle or g is not None:
            x_out, g_out = block_tail.block_tail_fwd(Y, None if middle else xs, g, st[0], st[1], h.slope, want_x=not middle, want_g=g is not None)
        if middle:
            Ws, We, _, _ = tail_images(Wa, xs.shape[1])
            rb = ops.gemm_nt(xs, Ws, ba, exact=True)                                  # [B,Fo]: W_s xs[b] + ba
            pro, bna = (st[0], st[1], h.slope), h.bn_add
            Y_pm = ops.cm_to_pm(Y)                                                    # kept for the weight gradient: one transpose per step
            if train:
                Z, sta = ops.gemm_nt(Y_pm, We, rowbias=rb, rows_per_group=L, pro=pro, bn=(ga, bea, bna.running_mean, bna.running_var),
                                     exact=True)
                bna.num_batches_tracked += 1
            else:
                Z = ops.gemm_nt(Y_pm, We, rowbias=rb, rows_per_group=L, pro=pro, exact=True)
                sta = ops.bn_prepare(None, None, ga, bea, B * L, False, bna.running_mean, bna.running_var, eps=float(bna.eps))
            x_out = ops.pm_to_cm(ops.affine_act(Z, sta[0], sta[1], h.slope), B, L)
        ctx.h, ctx.Cg = h, 0 if g is None else g.shape[1]
        # the statistics are saved tensors, not attributes: autograd drops them with this node's backward, before the layer's backward runs
        ctx.save_for_backward(Y, xs, gamma, Wa, ga, Z, Y_pm, st, *(sta if sta is not None else (None,) * 4))
        return x_out, g_out

    @staticmethod
    def backward(ctx, dx_out, dg_out):
        refuse_double_backward(ctx.h.name)
        return BlockTailFn._backward(ctx, dx_out, dg_out)

    @staticmethod
    @once_differentiable
    def _backward(ctx, dx_out, dg_out):
        Y, xs, gamma, Wa, ga, Z, Y_pm, st, *sta = ctx.saved_tensors
        h = ctx.h
        B, C, L = Y.shape
        train, middle, Cg = h.training, Wa is not None, ctx.Cg
        scale, shift, invstd, mean = st
        need = ctx.needs_input_grad
        dout_g = None if dg_out is None else dg_out.contiguous()
        dout_x = extra = dxs = dWa = dba = dga = dbea = None
        if not middle:
            Cs = xs.shape[1]
            dout_x = None if dx_out is None else dx_out.contiguous()
        elif dx_out is not None:
            Cs = 0
            _, _, Wst, Wet = tail_images(Wa, xs.shape[1])
            dz, sums_a = lrelu_bn_bwd(dx_out, Z, sta, ga, _Shape(B, L, train), h.slope)
            cs = ops.colsum(dz, L)                                                     # [B,Fo]: what the per-shape bias sees
            if need[6]:
                dWa = torch.cat([ops.gemm_tn(cs, xs, exact=True), ops.gemm_tn(dz, Y_pm, pro=(scale, shift, h.slope), exact=True)],
                                dim=1).view_as(Wa)
            dxs = ops.gemm_nt(cs, Wst, exact=True) if need[2] else None
            extra = ops.pm_to_cm(ops.gemm_nt(dz, Wet, exact=True), B, L)
            dba = dbias(dz, train) if need[7] else None
            dga, dbea = gb(sums_a, need, 8)
            del dz
        else:
            Cs = 0
        sums, dxs_t, dg = block_tail.block_tail_bwd_reduce(Y, dout_x, dout_g, extra, Cs, Cg, scale, shift, mean, invstd, h.slope,
                                                           want_dxs=need[2], want_dg=need[3])
        dY = None
        if need[1]:
            dY = block_tail.block_tail_bwd_apply(Y, dout_x, dout_g, extra, Cs, Cg, scale, shift, mean, invstd, gamma, sums if train else None, h.slope)
        if not middle:
            dxs = dxs_t
        return (None, dY, dxs if need[2] else None, dg) + gb(sums, need, 4) + (dWa, dba, dga, dbea)


DENSE_SLOPE = 0.2


class DenseEdgeFn(Function):
    """out [B,G,N] = max_j y_L(i,j), y_l = lrelu(bn_l(W_l . cat[e0, y_1 .. y_{l-1}] + b_l), 0.2), e0(i,j) = cat[x_j - x_i, x_i]   (the
    reference's DenseEdgeModule, Common/utilities.py:123-144) without the [B,2C,N,k] edge tensor, any concatenation or any activated
    per-edge tensor, forward or backward.  The e0 part of all levels is ONE per-point GEMM, PQ [M, 2LG] = [P_1 .. P_L | Q_1 .. Q_L]
    (dense_edge_images); level l's pre-norm rows z_l go into column slice l of one buffer Z [E, LG], formed from the slices in front of
    it -- activated while they are staged -- plus Q_l[i] + P_l[j] (csrc/edge_dense.hip), with the BatchNorm records from the same launch.
    The backward holds D [E, LG] (the gradients reaching z_l, last level first: gy_m is ONE product over the finished slices behind m)
    and one [E,G] buffer; D scatters to dPQ through the reverse CSR.
    holder: B, N, k, training, idx, knn_mode, bns; parameters (W, b, gamma, beta) per level.  Saved: x, Z, the graph, the pooled result
    and its arg-max, the per-column (scale, shift) and the statistics."""

    @staticmethod
    def forward(ctx, h, x, *params):
        from . import pointnet_util
        B, C, N = x.shape
        L, k, M, train = len(h.bns), h.k, B * N, h.training
        Ws, bs, gammas, betas = params[0::4], params[1::4], params[2::4], params[3::4]
        G = Ws[0].shape[0]
        E, LG = M * k, L * G
        x_pm = ops.cm_to_pm(x)
        idx = h.idx if h.idx is not None else dense_graph(x_pm, B, N, k, h.knn_mode)
        Wst, _, Wy, _ = dense_edge_images(Ws, C)
        # exact=True: fp32 operands whatever ops.set_mfma_operands selected
        PQ = ops.gemm_nt(x_pm, Wst, torch.cat([torch.zeros_like(b) for b in bs] + [b.detach() for b in bs]), exact=True)
        Z = torch.empty((E, LG), dtype=torch.float32, device=x.device)
        SC = torch.empty((2, LG), dtype=torch.float32, device=x.device)      # (scale | shift) of every column of Z
        sts = []
        for l in range(L):
            lo, hi = l * G, (l + 1) * G
            res = edge_dense.edge_dense_level(Z[:, :lo] if l else None, Wy[l - 1] if l else None, Z[:, lo:hi], raw_cols=0, scale=SC[0, :lo],
                                              shift=SC[1, :lo], slope=DENSE_SLOPE, addend=(PQ[:, lo:hi], PQ[:, LG + lo:LG + hi], idx), stats=train)
            st = bn_stats(h.bns[l], train, E, gammas[l], betas[l], records=res[1:] if train else None)
            SC[:, lo:hi] = st[:2]
            sts.append(st)
        del PQ
        out_pm, arg = pointnet_util._group_max(Z[:, LG - G:], M, k, sts[-1][0], sts[-1][1], DENSE_SLOPE)
        h.last_idx = idx
        ctx.h, ctx.sts = h, sts
        ctx.save_for_backward(x, Z, idx, out_pm, arg, SC, *Ws, *gammas)
        return ops.pm_to_cm(out_pm, B, N)

    @staticmethod
    def backward(ctx, dout):
        refuse_double_backward("DenseEdgeModule")
        return DenseEdgeFn._backward(ctx, dout)

    @staticmethod
    @once_differentiable
    def _backward(ctx, dout):
        from . import pointnet_util
        h, sts = ctx.h, ctx.sts
        L = len(sts)
        x, Z, idx, out_pm, arg, SC = ctx.saved_tensors[:6]
        Ws, gammas = ctx.saved_tensors[6:6 + L], ctx.saved_tensors[6 + L:]
        B, C, N = x.shape
        k, M, train = h.k, B * N, h.training
        G = Ws[0].shape[0]
        E, LG = M * k, L * G
        need = ctx.needs_input_grad
        _, Wst_t, _, Wback = dense_edge_images(Ws, C)
        D = torch.empty((E, LG), dtype=torch.float32, device=x.device)
        sums = [None] * L
        _, _, inv, mu = sts[-1]
        r, sums[-1] = pointnet_util._group_max_bwd(ops.cm_to_pm(dout), out_pm, arg, Z[:, LG - G:], mu, inv, DENSE_SLOPE, k)
        edge_dense.edge_dense_bn_apply(r, Z[:, LG - G:], mu, inv, gammas[-1], used(sums[-1], train), E, D[:, LG - G:])
        del r
        for m in range(L - 2, -1, -1):
            lo, hi = m * G, (m + 1) * G
            sc, sh, inv, mu = sts[m]
            # the LeakyReLU mask of z_m and the two BatchNorm sums come out of the product's epilogue
            gz, t1, t2 = ops.gemm_nt_bnbwd(D[:, hi:], Wback[m], Z[:, lo:hi], sc, sh, mu, inv, DENSE_SLOPE, exact=True)
            sums[m] = torch.cat([t1, t2])
            edge_dense.edge_dense_bn_apply(gz, Z[:, lo:hi], mu, inv, gammas[m], used(sums[m], train), E, D[:, lo:hi])
            del gz
        rowptr, src = ops.csr_build(idx, B, N)
        dPQ = edge_dense.edge_dense_scatter(D, rowptr, src, k)
        del rowptr, src
        dWst = ops.gemm_tn(dPQ, ops.cm_to_pm(x), exact=True) if any(need[2 + 4 * l] for l in range(L)) else None
        grads = []
        for l in range(L):
            lo, hi = l * G, (l + 1) * G
            dW = None
            if need[2 + 4 * l]:
                parts = [dense_edge_unstacked_grad(dWst, l, L, G)]
                if l:
                    parts.append(ops.gemm_tn(D[:, lo:hi], Z[:, :lo], pro=(SC[0, :lo], SC[1, :lo], DENSE_SLOPE), exact=True))
                dW = torch.cat(parts, dim=1).view_as(Ws[l])
            db = dbias(dPQ[:, LG + lo:LG + hi], train) if need[3 + 4 * l] else None
            grads += [dW, db, *gb(sums[l], need, 4 + 4 * l)]
        del D
        dx = ops.pm_to_cm(ops.gemm_nt(dPQ, Wst_t, exact=True), B, N) if need[1] else None
        return (None, dx, *grads)


def dense_graph(x_pm: Tensor, B: int, N: int, k: int, knn_mode: int) -> Tensor:
    """The reference's graph for the dense edge layers (Common/ops.py:129-135: topk of the negative squared distance, so the point itself
    is a neighbour): idx int32 [M,k] = the point itself, then its k-1 nearest neighbours by ascending distance (ops.knn)"""
    M = B * N
    idx = torch.empty((M, k), dtype=torch.int32, device=x_pm.device)
    idx[:, 0] = torch.arange(M, dtype=torch.int32, device=x_pm.device)
    idx[:, 1:] = ops.knn(x_pm, B, N, k - 1, knn_mode)
    return idx


def dense_side_images(Ws: Sequence[Tensor], widths: Sequence[int]):
    """MultiDenseMLP's conv weights (W_l [w_l, K_l, 1, 1] over cat[x_0, y_0, x_1, y_1, .. y_{l-1}, x_l], Common/utilities.py:112-121) as
    images over the buffer [x_0 .. x_{n-1} | z_0 .. z_{n-1}] DenseRowsFn keeps: level l's image [w_l, Cin + off_l] has its columns moved
    to the buffer's order and ZERO columns for the side inputs x_j, j > l, it does not see yet (Cin = sum widths).
    -> ((Wm, Wx_t, Wback) of the images as dense_rows_images forms them, maps): maps[l] int64 [K_l] = the buffer column of every column
    of W_l.  One cache entry per weight set, in a dictionary of its own: the images are temporaries and never enter another cache."""
    def build(*Ws):
        n, Cin = len(Ws), sum(widths)
        xoff, zoff = [0], [0]
        for c in widths:
            xoff.append(xoff[-1] + c)
        for W in Ws:
            zoff.append(zoff[-1] + W.shape[0])
        maps, imgs = [], []
        for l, W in enumerate(Ws):
            spans = []
            for j in range(l + 1):
                spans.append((xoff[j], xoff[j + 1]))
                if j < l:
                    spans.append((Cin + zoff[j], Cin + zoff[j + 1]))
            if sum(b - a for a, b in spans) != W.shape[1]:
                raise ValueError("MultiDenseMLP: level %d's weight has %d input channels, the inputs give %d"
                                 % (l, W.shape[1], sum(b - a for a, b in spans)))
            m = torch.cat([torch.arange(a, b, dtype=torch.int64, device=W.device) for a, b in spans])   # built on the device: capturable
            img = torch.zeros((W.shape[0], Cin + zoff[l]), dtype=torch.float32, device=W.device)
            img[:, m] = W.reshape(W.shape[0], W.shape[1])
            maps.append(m)
            imgs.append(img)
        return _rows_images(imgs, Cin), tuple(maps)
    return cached_images(_IMAGES["dense_side"], tuple(Ws), tuple(widths), build)


class DenseRowsFn(Function):
    """out [B,w_L,N] = y_L, y_l = lrelu(bn_l(W_l . cat[x, y_1 .. y_{l-1}] + b_l), slope)   (the reference's DenseModule1D / DenseModule2D,
    Common/utilities.py:22-65) without the concatenations or the activated tensors: one buffer R [M, Cin + S] = [x | z_1 | .. | z_L] of
    the raw input and the pre-norm rows, each level a product over the columns in front of its slice with x taken as stored and the z
    columns activated while they are staged (csrc/edge_dense.hip, raw_cols = Cin).  The backward mirrors DenseEdgeFn's with k = 1.
    holder: B, N, training, bns; parameters (W, b, gamma, beta) per level; the level widths are the weights'.  Optional holder fields:
    slope (0.2; 0.0 = ReLU), name (the layer named in refusals), pm (x and out are point-major rows [M,C], no layout conversion) and
    sides = the widths (c_0, .., c_{n-1}) of MultiDenseMLP's raw inputs: then x is followed by the n - 1 side inputs [B,c_i,N], the raw
    block of R is [x_0 | .. | x_{n-1}] and the weights act through dense_side_images."""

    @staticmethod
    def forward(ctx, h, x, *rest):
        from . import pointnet_util
        slope, pm, sides = getattr(h, "slope", DENSE_SLOPE), getattr(h, "pm", False), getattr(h, "sides", None)
        ns = len(sides) - 1 if sides else 0
        xs, params = (x,) + tuple(rest[:ns]), rest[ns:]
        L, M, train = len(h.bns), h.B * h.N, h.training
        Ws, bs, gammas, betas = params[0::4], params[1::4], params[2::4], params[3::4]
        Cin = sum(sides) if sides else x.shape[1]
        maps = None
        if sides:
            (Wm, _, _), maps = dense_side_images(Ws, sides)
        else:
            Wm, _, _ = dense_rows_images(Ws, Cin)
        off = [Cin]
        for w in Wm:
            off.append(off[-1] + w.shape[0])
        R = torch.empty((M, off[-1]), dtype=torch.float32, device=x.device)
        if pm:
            R[:, :Cin].copy_(x)
        else:
            col = 0
            for t in xs:
                pointnet_util._cm_to_rows(t.contiguous(), R, col)
                col += t.shape[1]
        SC = torch.empty((2, off[-1]), dtype=torch.float32, device=x.device)  # (scale | shift) per column of R; the x columns are not read
        sts = []
        for l in range(L):
            lo, hi = off[l], off[l + 1]
            res = edge_dense.edge_dense_level(R[:, :lo], Wm[l], R[:, lo:hi], raw_cols=Cin, scale=SC[0, :lo], shift=SC[1, :lo], slope=slope,
                                              bias=bs[l].detach(), stats=train)
            st = bn_stats(h.bns[l], train, M, gammas[l], betas[l], records=res[1:] if train else None)
            SC[:, lo:hi] = st[:2]
            sts.append(st)
        out_pm = ops.affine_act(R[:, off[-2]:], sts[-1][0], sts[-1][1], slope)
        ctx.h, ctx.sts, ctx.off, ctx.ns = h, sts, off, ns
        ctx.save_for_backward(R, out_pm, SC, *Ws, *gammas)
        return out_pm if pm else ops.pm_to_cm(out_pm, h.B, h.N)

    @staticmethod
    def backward(ctx, dout):
        refuse_double_backward(getattr(ctx.h, "name", "DenseModule1D"))
        return DenseRowsFn._backward(ctx, dout)

    @staticmethod
    @once_differentiable
    def _backward(ctx, dout):
        from . import pointnet_util
        h, sts, off, ns = ctx.h, ctx.sts, ctx.off, ctx.ns
        slope, pm, sides = getattr(h, "slope", DENSE_SLOPE), getattr(h, "pm", False), getattr(h, "sides", None)
        L = len(sts)
        R, out_pm, SC = ctx.saved_tensors[:3]
        Ws, gammas = ctx.saved_tensors[3:3 + L], ctx.saved_tensors[3 + L:]
        M, Cin, train = R.shape[0], off[0], h.training
        need = ctx.needs_input_grad
        p0 = 2 + ns                                                                    # the first parameter's position among the inputs
        maps = None
        if sides:
            (_, Wx_t, Wback), maps = dense_side_images(Ws, sides)
        else:
            _, Wx_t, Wback = dense_rows_images(Ws, Cin)
        D = torch.empty((M, off[-1] - Cin), dtype=torch.float32, device=R.device)      # column c of D belongs to column Cin + c of R
        sums = [None] * L
        _, _, inv, mu = sts[-1]
        r, sums[-1] = pointnet_util._group_max_bwd(dout.contiguous() if pm else ops.cm_to_pm(dout), out_pm, None, R[:, off[-2]:], mu, inv, slope, 1)
        edge_dense.edge_dense_bn_apply(r, R[:, off[-2]:], mu, inv, gammas[-1], used(sums[-1], train), M, D[:, off[-2] - Cin:])
        del r
        for m in range(L - 2, -1, -1):
            lo, hi = off[m], off[m + 1]
            sc, sh, inv, mu = sts[m]
            gz, t1, t2 = ops.gemm_nt_bnbwd(D[:, hi - Cin:], Wback[m], R[:, lo:hi], sc, sh, mu, inv, slope, exact=True)
            sums[m] = torch.cat([t1, t2])
            edge_dense.edge_dense_bn_apply(gz, R[:, lo:hi], mu, inv, gammas[m], used(sums[m], train), M, D[:, lo - Cin:hi - Cin])
            del gz
        grads = []
        for l in range(L):
            lo, hi = off[l], off[l + 1]
            Dl = D[:, lo - Cin:hi - Cin]
            dW = None
            if need[p0 + 4 * l]:
                parts = [ops.gemm_tn(Dl, R[:, :Cin], exact=True)]
                if l:
                    parts.append(ops.gemm_tn(Dl, R[:, Cin:lo], pro=(SC[0, Cin:lo], SC[1, Cin:lo], slope), exact=True))
                dW = torch.cat(parts, dim=1)
                dW = (dW if maps is None else dW[:, maps[l]]).reshape(Ws[l].shape)
            db = dbias(Dl, train) if need[p0 + 1 + 4 * l] else None
            grads += [dW, db, *gb(sums[l], need, p0 + 2 + 4 * l)]
        dxs = [None] * (1 + ns)
        if any(need[1:p0]):
            dR = ops.gemm_nt(D, Wx_t, exact=True)
            if pm:
                dxs[0] = dR
            elif not sides:
                dxs[0] = ops.pm_to_cm(dR, h.B, h.N)
            else:
                col = 0
                for i, c in enumerate(sides):
                    if need[1 + i]:
                        dxs[i] = pointnet_util._rows_to_cm(dR, col, h.B, c, h.N)
                    col += c
        return (None, *dxs, *grads)
