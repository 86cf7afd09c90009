"""metrics/pointnet2/pointnet2_modules.py of the reference on HIP: PointnetSAModuleMSG, PointnetSAModule, PointnetFPModule with the
reference's keyword-only constructors, attribute names (groupers, mlps, mlp) and state_dict keys.

    sa = PointnetSAModuleMSG(npoint=512, radii=[0.1, 0.2], nsamples=[16, 32], mlps=[[64, 64, 128], [64, 64, 128]])
    new_xyz, new_features = sa(xyz, features)               # xyz [B,N,3], features [B,C,N] | None -> [B,npoint,3], [B, sum mlp[-1], npoint]
    fp = PointnetFPModule(mlp=[128 + 64, 128])
    out = fp(unknown, known, unknow_feats, known_feats)     # [B,mlp[-1],n]

Each module has an attribute `fused` (default True).

fused=False is the reference's forward written over spgan.pointnet2_utils and spgan.pytorch_utils: one ball query per scale, the grouped
[B,3+C,npoint,nsample] tensor, the SharedMLP, torch pooling, torch.cat.  instance_norm=True always takes it.

fused=True (csrc/sa_group.hip) never forms the grouped tensor.  The first 1x1 convolution is linear in [x_j - c_i | f_j], so
  * one launch answers the ball queries of all scales (pointnet2_utils.ball_query_multi);
  * one per-point product P = [xyz | f] W1^T covers all scales (stacked output columns, B*N rows, the fp32-MFMA GEMM), and one per-centre
    product Qc = new_xyz W1[:, :3]^T (B*npoint rows);
  * per scale one gather launch writes Y1[(i,k), :] = P[idx[i,k]] - Qc[i] (+ bias without bn) as the row-major operand of layer 2 and, with
    bn, the BatchNorm column records;
  * layers 2 .. and the pooling are those of spgan.pointnet_util (GEMM with statistics epilogue, BatchNorm + ReLU on the operand load,
    spgan_group_max); the pooled rows of every scale go into channel slices of one [B, sum Cout, npoint] tensor.
Backward: dY1 -> dP through the reverse CSR of the padded index lists (spgan_gather_csr), dQc[i] = -sum_k dY1[(i,k)],
weight and input gradients from gemm_tn / gemm_nt on per-point rows; both sums are one launch per scale (spgan_sa_scatter) into column
slices of the buffers all scales share.  Once differentiable.  npoint=None (GroupAll) has no centre: the
rows [xyz | f] go through the same layer chain with one group of N rows per cloud.
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from . import pointnet2_utils
from . import pytorch_utils as pt_utils
from .edge_conv import refuse_double_backward
from .ops import _p, _s, check
from .pointnet_util import (RELU, _cm_to_rows, _group_max, _group_max_bwd, _rows_to_cm, _RowsToCmFn, _three_interpolate_bwd,
                            _three_interpolate_into, gather_csr, index_points)

Tensor = torch.Tensor


# ----------------------------------------------------------------------------------------------------------------------------------
# the layer chain shared by every route: (1x1 conv -> [BatchNorm] -> ReLU) per layer, then max / average over the K rows of a group
# ----------------------------------------------------------------------------------------------------------------------------------
class _Spec:
    """What a SharedMLP holds, in the order the autograd functions take it: per layer (weight, bias | None, gamma | None, beta | None)."""

    def __init__(self, mlp: pt_utils.SharedMLP):
        self.convs, self.bns = [], []
        for layer in mlp.layers():
            self.convs.append(layer.conv)
            self.bns.append(layer.bn.bn if hasattr(layer, "bn") else None)
        self.bn = self.bns[0] is not None
        self.widths = [c.out_channels for c in self.convs]

    def params(self):
        out = []
        for conv, bn in zip(self.convs, self.bns):
            out += [conv.weight, conv.bias, None if bn is None else bn.weight, None if bn is None else bn.bias]
        return out


def _identity_stats(Cn: int, device):
    one, zero = torch.ones(Cn, dtype=torch.float32, device=device), torch.zeros(Cn, dtype=torch.float32, device=device)
    return one, zero, one, zero          # scale, shift, invstd, mean


def _layer_stats(bn, part, tiles, tile_rows, Cn, M, gamma, beta, training, device):
    """(scale, shift, invstd, mean) of one layer from the records `part` of its pre-norm product (train) or the running statistics."""
    if bn is None:
        return _identity_stats(Cn, device)
    if training:
        out = torch.empty((4, Cn), dtype=torch.float32, device=device)
        check(_lib.load().spgan_colstats_finalize_bn(_p(part), tiles, Cn, M, tile_rows, _p(gamma), _p(beta), ops.BN_EPS, ops._BN_MOM[0],
                                                     _p(bn.running_mean), _p(bn.running_var), _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]),
                                                     _s()), "colstats_finalize_bn", N=Cn, M=M)
        bn.num_batches_tracked += 1
        return out[0], out[1], out[2], out[3]
    return ops.bn_prepare(None, None, gamma, beta, M, False, bn.running_mean, bn.running_var)


def _chain_forward(y0: Tensor, st0, spec: _Spec, params, training: bool, K: int, pool: str):
    """Layers 2 .. of a chain whose first pre-norm product y0 [Q*K, C1] and statistics st0 are given, then the pooling.
    -> (pooled [Q, Cout], saved = (ys, stats, act, arg))."""
    M = y0.shape[0]
    Q = M // K
    ys, sts = [y0], [st0]
    a, pro = y0, (st0[0], st0[1], RELU)
    for li in range(1, len(spec.convs)):
        W, b, gamma, beta = params[4 * li:4 * li + 4]
        W2 = W.view(W.shape[0], W.shape[1])
        bn = spec.bns[li]
        if bn is not None and training:
            y, st = ops.gemm_nt(a, W2, b, bn=(gamma, beta, bn.running_mean, bn.running_var), pro=pro)
            bn.num_batches_tracked += 1
        else:
            y = ops.gemm_nt(a, W2, b, pro=pro)
            st = _layer_stats(bn, None, 0, 0, W2.shape[0], M, gamma, beta, False, y.device)
        ys.append(y); sts.append(st)
        a, pro = y, (st[0], st[1], RELU)
    sc, sh = sts[-1][0], sts[-1][1]
    act = arg = None
    if pool == "max" and K > 1:
        pooled, arg = _group_max(ys[-1], Q, K, sc, sh, RELU)
    else:
        act = ops.affine_act(ys[-1], sc, sh, RELU)
        pooled = act if K == 1 else ops.colsum(act, K) / float(K)
    return pooled, (ys, sts, act, arg)


def _chain_backward(gpool: Tensor, pooled: Tensor, saved, spec_bn: List[bool], params, training: bool, K: int, pool: str, a0: Optional[Tensor],
                    need_a0: bool):
    """-> (dy0 [Q*K, C1] = the gradient of the first pre-norm product, grads per parameter; with a0 given also the first layer's weight
    gradient and, when asked, da0)."""
    ys, sts, act, arg = saved
    L = len(ys)
    M = ys[0].shape[0]
    grads = [None] * (4 * L)
    gpool = gpool.contiguous()
    if pool == "max" and K > 1:
        g, sums = _group_max_bwd(gpool, pooled, arg, ys[-1], sts[-1][3], sts[-1][2], RELU, K)
    else:
        if K > 1:      # the average: every row of a group takes 1/K of its gradient
            gpool = (gpool / float(K)).repeat_interleave(K, dim=0)
        g, sums = _group_max_bwd(gpool, act, None, ys[-1], sts[-1][3], sts[-1][2], RELU, 1)
    dy = da0 = None
    for li in range(L - 1, -1, -1):
        W, b, gamma, beta = [None if p is None else p.detach() for p in params[4 * li:4 * li + 4]]
        W2 = W.view(W.shape[0], W.shape[1])
        Cn = W2.shape[0]
        sc, sh, inv, mu = sts[li]
        if spec_bn[li]:
            grads[4 * li + 2], grads[4 * li + 3] = sums[Cn:].clone(), sums[:Cn].clone()
            dy = ops.bn_bwd_apply(g, ys[li], mu, inv, gamma, sums if training else torch.zeros_like(sums), M)
        else:
            dy = g
            grads[4 * li + 1] = sums[:Cn].clone()
        if li > 0:
            psc, psh, pinv, pmu = sts[li - 1]
            grads[4 * li] = ops.gemm_tn(dy, ys[li - 1], pro=(psc, psh, RELU)).view_as(W)
            g, s0, s1 = ops.gemm_nt_bnbwd(dy, W2.t().contiguous(), ys[li - 1], psc, psh, pmu, pinv, RELU)
            sums = torch.cat([s0, s1])
        elif a0 is not None:
            grads[0] = ops.gemm_tn(dy, a0).view_as(W)
            if need_a0:
                da0 = ops.gemm_nt(dy, W2.t().contiguous())
    return dy, grads, da0


class _Holder:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class _RowsMLPFn(torch.autograd.Function):
    """rows a0 [Q*K, Cin] -> [Q, Cout]: the layer chain on given rows (a stand-alone SharedMLP, GroupAll, feature propagation)."""

    @staticmethod
    def forward(ctx, holder, a0, *params):
        spec, training, K, pool = holder.spec, holder.training, holder.K, holder.pool
        W, b, gamma, beta = params[0:4]
        W2 = W.view(W.shape[0], W.shape[1])
        bn = spec.bns[0]
        if bn is not None and training:
            y0, st0 = ops.gemm_nt(a0, W2, b, bn=(gamma, beta, bn.running_mean, bn.running_var))
            bn.num_batches_tracked += 1
        else:
            y0 = ops.gemm_nt(a0, W2, b)
            st0 = _layer_stats(bn, None, 0, 0, W2.shape[0], a0.shape[0], gamma, beta, False, a0.device)
        pooled, (ys, sts, act, arg) = _chain_forward(y0, st0, spec, params, training, K, pool)
        ctx.cfg = (training, K, pool, len(ys), [x is not None for x in spec.bns])
        ctx.save_for_backward(a0, pooled, act, arg, *params, *ys, *[t for st in sts for t in st])
        return pooled

    @staticmethod
    def backward(ctx, dout):
        refuse_double_backward("PointnetSAModule / PointnetFPModule / SharedMLP")
        training, K, pool, L, spec_bn = ctx.cfg
        a0, pooled, act, arg, *rest = ctx.saved_tensors
        params, ys, flat = rest[:4 * L], rest[4 * L:5 * L], rest[5 * L:]
        sts = [flat[4 * i:4 * i + 4] for i in range(L)]
        _, grads, da0 = _chain_backward(dout, pooled, (ys, sts, act, arg), spec_bn, params, training, K, pool, a0, ctx.needs_input_grad[1])
        return (None, da0) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:]))


def rows_mlp(rows: Tensor, mlp: pt_utils.SharedMLP, K: int, pool: str, training: bool) -> Tensor:
    """rows [Q*K, Cin] through `mlp` and the pooling over each K consecutive rows ('max', 'avg'; K = 1 / 'none': the activations)."""
    spec = _Spec(mlp)
    return _RowsMLPFn.apply(_Holder(spec=spec, training=training, K=K, pool=pool), rows.contiguous(), *spec.params())


class _LinearFn(torch.autograd.Function):
    """A [M,K] @ W[N,K]^T on the MFMA GEMM (the hoisted per-point and per-centre products)."""

    @staticmethod
    def forward(ctx, A, W):
        ctx.save_for_backward(A, W)
        return ops.gemm_nt(A, W)

    @staticmethod
    def backward(ctx, dY):
        refuse_double_backward("PointnetSAModule")
        A, W = ctx.saved_tensors
        dY = dY.contiguous()
        dA = ops.gemm_nt(dY, W.t().contiguous()) if ctx.needs_input_grad[0] else None
        dW = ops.gemm_tn(dY, A) if ctx.needs_input_grad[1] else None
        return dA, dW


def _sa_gather(P: Tensor, Qc: Tensor, col0: int, C1: int, bias: Optional[Tensor], idx: Tensor, n: int, want_stats: bool):
    """-> (Y1 [B*m*K, C1], records | None, tiles, tile_rows)."""
    B, m, K = idx.shape
    lib = _lib.load()
    Y = torch.empty((B * m * K, C1), dtype=torch.float32, device=P.device)
    tile_rows = lib.spgan_sa_gather_tile_rows(K)
    tiles = (B * m * K + tile_rows - 1) // tile_rows
    part = torch.empty((tiles, C1, 2), dtype=torch.float32, device=P.device) if want_stats else None
    bad = ops.index_check_flag(P.device)
    check(lib.spgan_sa_gather(_p(P), P.shape[1], col0, _p(Qc), Qc.shape[1], col0, _p(bias), _p(idx), B, n, m, K, C1, _p(Y), C1, _p(part), _p(bad),
                              _s()), "sa_gather", B=B, n=n, m=m, K=K, C=C1)
    ops.index_check_raise(bad, "sa_gather: an index lies outside [0, %d)" % n)
    return Y, part, tiles, tile_rows


class _SAFusedFn(torch.autograd.Function):
    """(P [B*N, sum C1], Qc [B*S, sum C1], idx per scale) -> [B, sum Cout, S]: per scale the gather, layers 2 .., the pooling, and the
    pooled rows written channel-major into that scale's slice."""

    @staticmethod
    def forward(ctx, holder, P, Qc, *rest):
        specs, training, pool, B, n, m = holder.specs, holder.training, holder.pool, holder.B, holder.n, holder.m
        S = len(specs)
        idxs, params = rest[:S], rest[S:]
        Ctot = sum(sp.widths[-1] for sp in specs)
        out = torch.empty((B, Ctot, m), dtype=torch.float32, device=P.device)
        lib = _lib.load()
        saved, cfg = [], []
        p0 = col0 = co = 0
        for s, spec in enumerate(specs):
            L = len(spec.convs)
            prm = params[p0:p0 + 4 * L]
            W, b, gamma, beta = prm[0:4]
            C1, K, bn = spec.widths[0], idxs[s].shape[2], spec.bns[0]
            y0, part, tiles, tile_rows = _sa_gather(P, Qc, col0, C1, b, idxs[s], n, bn is not None and training)
            st0 = _layer_stats(bn, part, tiles, tile_rows, C1, y0.shape[0], gamma, beta, training, P.device)
            pooled, (ys, sts, act, arg) = _chain_forward(y0, st0, spec, prm, training, K, pool)
            Cout = spec.widths[-1]
            check(lib.spgan_sa_rows_to_cm_slice(_p(pooled), B, m, Cout, co, Ctot, _p(out), _s()), "sa_rows_to_cm_slice", B=B, S=m, C=Cout)
            cfg.append((L, K, C1, Cout, [x is not None for x in spec.bns], act is not None, arg is not None))
            saved += [idxs[s], pooled] + ([act] if act is not None else []) + ([arg] if arg is not None else []) + list(ys) + [t for st in sts for t in st]
            p0 += 4 * L; col0 += C1; co += Cout
        ctx.cfg = (cfg, training, pool, B, n, m, Ctot, len(params))
        ctx.save_for_backward(*params, *saved)
        return out

    @staticmethod
    def backward(ctx, dout):
        refuse_double_backward("PointnetSAModule / PointnetFPModule / SharedMLP")
        cfg, training, pool, B, n, m, Ctot, nparams = ctx.cfg
        tensors = ctx.saved_tensors
        params, saved = tensors[:nparams], list(tensors[nparams:])
        dout = dout.contiguous()
        lib = _lib.load()
        need_P, need_Q = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        wide = sum(c[2] for c in cfg)
        dP = torch.empty((B * n, wide), dtype=torch.float32, device=dout.device) if need_P else None
        dQ = torch.empty((B * m, wide), dtype=torch.float32, device=dout.device) if need_Q else None
        grads = []
        p0 = co = col0 = at = 0
        for (L, K, C1, Cout, spec_bn, has_act, has_arg) in cfg:
            idx, pooled = saved[at], saved[at + 1]; at += 2
            act = arg = None
            if has_act:
                act = saved[at]; at += 1
            if has_arg:
                arg = saved[at]; at += 1
            ys = saved[at:at + L]; at += L
            sts = [saved[at + 4 * i:at + 4 * i + 4] for i in range(L)]; at += 4 * L
            gp = torch.empty((B * m, Cout), dtype=torch.float32, device=dout.device)
            check(lib.spgan_sa_cm_slice_to_rows(_p(dout), B, m, Cout, co, Ctot, _p(gp), _s()), "sa_cm_slice_to_rows", B=B, S=m, C=Cout)
            dy, g, _ = _chain_backward(gp, pooled, (ys, sts, act, arg), spec_bn, params[p0:p0 + 4 * L], training, K, pool, None, False)
            grads += g
            if need_P or need_Q:
                rowptr = src = None
                if need_P:
                    rowptr, src = gather_csr(idx.view(B, m * K).to(torch.int64), n)
                # both sums of this scale in one launch, into the column slices of the buffers all scales share
                check(lib.spgan_sa_scatter(_p(dy), C1, C1, _p(rowptr), _p(src), B * n, _p(dP), wide, col0, B * m, K, _p(dQ), wide, col0, _s()),
                      "sa_scatter", B=B, n=n, m=m, K=K, C=C1)
            del dy, gp
            p0 += 4 * L; co += Cout; col0 += C1
        ng = ctx.needs_input_grad[3 + len(cfg):]
        return (None, dP, dQ) + (None,) * len(cfg) + tuple(g if need else None for g, need in zip(grads, ng))


class _PointRowsFn(torch.autograd.Function):
    """rows [B*N, 3+C] = [xyz | features^T] in one buffer (the operand of the hoisted per-point product; no torch.cat)."""

    @staticmethod
    def forward(ctx, xyz, features, use_xyz):
        B, N, _ = xyz.shape
        c3 = 3 if use_xyz else 0
        C = 0 if features is None else features.shape[1]
        rows = torch.empty((B * N, c3 + C), dtype=torch.float32, device=xyz.device)
        if c3:
            rows[:, :3] = xyz.reshape(B * N, 3)
        if C:
            _cm_to_rows(features, rows, c3)
        ctx.dims = (B, N, c3, C)
        return rows

    @staticmethod
    def backward(ctx, drows):
        refuse_double_backward("PointnetSAModule / PointnetFPModule")
        B, N, c3, C = ctx.dims
        drows = drows.contiguous()
        dxyz = drows[:, :3].reshape(B, N, 3).contiguous() if c3 and ctx.needs_input_grad[0] else None
        dfeat = _rows_to_cm(drows, c3, B, C, N) if C and ctx.needs_input_grad[1] else None
        return dxyz, dfeat, None


# ----------------------------------------------------------------------------------------------------------------------------------
# modules
# ----------------------------------------------------------------------------------------------------------------------------------
class _PointnetSAModuleBase(nn.Module):
    def __init__(self):
        super().__init__()
        self.npoint = None
        self.groupers = None
        self.mlps = None
        self.pool_method = "max_pool"
        self.fused = True
        self.use_xyz = True
        self.instance_norm = False

    # ------------------------------------------------------------------ the reference's forward over the ops of this package
    def _forward_unfused(self, xyz: Tensor, features: Optional[Tensor], new_xyz: Optional[Tensor]):
        new_features_list = []
        xyz_flipped = xyz.transpose(1, 2).contiguous()
        if new_xyz is None and self.npoint is not None:
            new_xyz = pointnet2_utils.gather_operation(xyz_flipped, pointnet2_utils.furthest_point_sample(xyz, self.npoint)).transpose(1, 2).contiguous()
        for i in range(len(self.groupers)):
            new_features = self.groupers[i](xyz, new_xyz, features)            # [B, C, npoint, nsample]
            new_features = self.mlps[i](new_features)                            # [B, mlp[-1], npoint, nsample]
            if self.pool_method == "max_pool":
                new_features = F.max_pool2d(new_features, kernel_size=[1, new_features.size(3)])
            elif self.pool_method == "avg_pool":
                new_features = F.avg_pool2d(new_features, kernel_size=[1, new_features.size(3)])
            else:
                raise NotImplementedError
            new_features_list.append(new_features.squeeze(-1))
        return new_xyz, torch.cat(new_features_list, dim=1)

    # ------------------------------------------------------------------ the hoisted route
    def _pool(self) -> str:
        if self.pool_method == "max_pool":
            return "max"
        if self.pool_method == "avg_pool":
            return "avg"
        raise NotImplementedError

    def _forward_group_all(self, xyz: Tensor, features: Optional[Tensor]):
        B, N, _ = xyz.shape
        use_xyz = self.use_xyz or features is None
        rows = _PointRowsFn.apply(xyz, features, use_xyz)
        outs = [_RowsToCmFn.apply(rows_mlp(rows, mlp, N, self._pool(), self.training).view(B, 1, -1)) for mlp in self.mlps]
        return None, outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)

    def _forward_fused(self, xyz: Tensor, features: Optional[Tensor], new_xyz: Optional[Tensor]):
        B, N, _ = xyz.shape
        pool = self._pool()
        if self.npoint is None:
            return self._forward_group_all(xyz, features)
        if features is None and not self.use_xyz:
            raise AssertionError("Cannot have not features and not use xyz as a feature!")
        specs = [_Spec(mlp) for mlp in self.mlps]
        W1 = [sp.convs[0].weight.view(sp.widths[0], -1) for sp in specs]
        Wcat = W1[0] if len(W1) == 1 else torch.cat(W1, dim=0)                    # parameters only: [sum C1, 3 + C]
        rows = _PointRowsFn.apply(xyz, features, self.use_xyz)
        P = _LinearFn.apply(rows, Wcat)
        own = new_xyz is None
        if own:
            fps = pointnet2_utils.furthest_point_sample(xyz, self.npoint).to(torch.int64)
            new_xyz = index_points(xyz, fps)
        m = new_xyz.shape[1]
        if not self.use_xyz:
            Qc = torch.zeros((B * m, Wcat.shape[0]), dtype=torch.float32, device=xyz.device)
        elif own and features is None:
            # the centres are cloud points and P is the coordinate product alone: its rows ARE the centre terms, so a ball that holds
            # only its own centre gives exact zeros, as the reference's subtraction does
            Qc = index_points(P.view(B, N, -1), fps).view(B * m, -1)
        else:
            Qc = _LinearFn.apply(new_xyz.reshape(B * m, 3), Wcat[:, :3].contiguous())
        idxs = pointnet2_utils.ball_query_multi([g.radius for g in self.groupers], [g.nsample for g in self.groupers], xyz, new_xyz)
        params = [p for sp in specs for p in sp.params()]
        holder = _Holder(specs=specs, training=self.training, pool=pool, B=B, n=N, m=m)
        return new_xyz, _SAFusedFn.apply(holder, P, Qc, *idxs, *params)

    def forward(self, xyz: Tensor, features: Tensor = None, new_xyz=None) -> (Tensor, Tensor):
        """xyz [B,N,3], features [B,C,N] | None, new_xyz [B,npoint,3] | None (None: farthest point sampling draws the centres)
        -> (new_xyz [B,npoint,3] (None with npoint=None), new_features [B, sum_k mlps[k][-1], npoint])."""
        xyz = pointnet2_utils._cloud(xyz, "xyz")
        if features is not None:
            features = pointnet2_utils._gpu(features, "features", torch.float32, 3)
            if features.shape[0] != xyz.shape[0] or features.shape[2] != xyz.shape[1]:
                raise ValueError("features must be [B = %d, C, N = %d], got %s" % (xyz.shape[0], xyz.shape[1], tuple(features.shape)))
        if new_xyz is not None:
            new_xyz = pointnet2_utils._cloud(new_xyz, "new_xyz")
            if new_xyz.shape[0] != xyz.shape[0]:
                raise ValueError("xyz and new_xyz differ in B: %s, %s" % (tuple(xyz.shape), tuple(new_xyz.shape)))
        hip = all(mlp.hip_route for mlp in self.mlps)
        if self.fused and hip and not self.instance_norm:
            return self._forward_fused(xyz, features, new_xyz)
        return self._forward_unfused(xyz, features, new_xyz)


class PointnetSAModuleMSG(_PointnetSAModuleBase):
    """Set abstraction with multi-scale grouping: one ball query and one SharedMLP per radius around the same centres."""

    def __init__(self, *, npoint: int, radii: List[float], nsamples: List[int], mlps: List[List[int]], bn: bool = True, use_xyz: bool = True,
                 pool_method="max_pool", instance_norm=False, first_layer=False):
        super().__init__()
        assert len(radii) == len(nsamples) == len(mlps)
        self.npoint = npoint
        self.groupers = nn.ModuleList()
        self.mlps = nn.ModuleList()
        for i in range(len(radii)):
            self.groupers.append(pointnet2_utils.QueryAndGroup(radii[i], nsamples[i], use_xyz=use_xyz) if npoint is not None
                                 else pointnet2_utils.GroupAll(use_xyz))
            mlp_spec = mlps[i]
            if use_xyz:
                mlp_spec[0] += 3              # in the caller's list, as the reference does
            self.mlps.append(pt_utils.SharedMLP(mlp_spec, bn=bn, instance_norm=instance_norm))
        self.pool_method = pool_method
        self.use_xyz = use_xyz
        self.instance_norm = instance_norm


class PointnetSAModule(PointnetSAModuleMSG):
    """Set abstraction with one scale; npoint=None groups the whole cloud."""

    def __init__(self, *, mlp: List[int], npoint: int = None, radius: float = None, nsample: int = None, bn: bool = True, use_xyz: bool = True,
                 pool_method="max_pool", instance_norm=False):
        super().__init__(mlps=[mlp], npoint=npoint, radii=[radius], nsamples=[nsample], bn=bn, use_xyz=use_xyz, pool_method=pool_method,
                         instance_norm=instance_norm)


class _FPInputFn(torch.autograd.Function):
    """rows [B*n, C2 + C1] = [three_interpolate(known_feats) | unknow_feats] written into ONE buffer (no torch.cat); idx int64 [B,n,k]."""

    @staticmethod
    def forward(ctx, known_feats, unknow_feats, idx, weight):
        B, C2, m = known_feats.shape
        n = idx.shape[1]
        C1 = 0 if unknow_feats is None else unknow_feats.shape[1]
        rows = torch.empty((B * n, C2 + C1), dtype=torch.float32, device=known_feats.device)
        p2 = torch.empty((B * m, C2), dtype=torch.float32, device=known_feats.device)
        _cm_to_rows(known_feats, p2, 0)
        _three_interpolate_into(p2.view(B, m, C2), idx, weight, rows, 0)
        if C1:
            _cm_to_rows(unknow_feats, rows, C2)
        ctx.save_for_backward(idx, weight)
        ctx.dims = (B, n, m, C1, C2)
        return rows

    @staticmethod
    def backward(ctx, drows):
        refuse_double_backward("PointnetSAModule / PointnetFPModule")
        idx, weight = ctx.saved_tensors
        B, n, m, C1, C2 = ctx.dims
        drows = drows.contiguous()
        dk = du = None
        if ctx.needs_input_grad[0]:
            dp2 = _three_interpolate_bwd(drows, 0, C2, idx, weight, m)
            dk = _rows_to_cm(dp2.view(B * m, C2), 0, B, C2, m)
        if C1 and ctx.needs_input_grad[1]:
            du = _rows_to_cm(drows, C2, B, C1, n)
        return dk, du, None, None


class PointnetFPModule(nn.Module):
    """Feature propagation: the features of `known` interpolated onto `unknown` by the inverse distances of the three nearest, joined
    with `unknow_feats`, through a SharedMLP."""

    def __init__(self, *, mlp: List[int], bn: bool = True):
        super().__init__()
        self.mlp = pt_utils.SharedMLP(mlp, bn=bn)
        self.fused = True

    def _weights(self, unknown: Tensor, known: Tensor):
        dist, idx = pointnet2_utils.three_nn(unknown, known)
        dist_recip = 1.0 / (dist + 1e-8)
        norm = torch.sum(dist_recip, dim=2, keepdim=True)
        return idx, dist_recip / norm

    def _forward_unfused(self, unknown, known, unknow_feats, known_feats):
        if known is not None:
            idx, weight = self._weights(unknown, known)
            interpolated_feats = pointnet2_utils.three_interpolate(known_feats, idx, weight)
        else:
            interpolated_feats = known_feats.expand(*known_feats.size()[0:2], unknown.size(1))
        if unknow_feats is not None:
            new_features = torch.cat([interpolated_feats, unknow_feats], dim=1)       # [B, C2 + C1, n]
        else:
            new_features = interpolated_feats
        return self.mlp(new_features.unsqueeze(-1).contiguous()).squeeze(-1)

    def forward(self, unknown: Tensor, known: Tensor, unknow_feats: Tensor, known_feats: Tensor) -> Tensor:
        """unknown [B,n,3], known [B,m,3] | None (None: known_feats [B,C2,1] is repeated), unknow_feats [B,C1,n] | None, known_feats [B,C2,m]
        -> [B, mlp[-1], n].  The interpolation weights carry no gradient (three_nn has none in the reference either)."""
        unknown = pointnet2_utils._cloud(unknown, "unknown")
        known_feats = pointnet2_utils._gpu(known_feats, "known_feats", torch.float32, 3)
        B, n, _ = unknown.shape
        if known is not None:
            known = pointnet2_utils._cloud(known, "known")
            if known.shape[0] != B or known_feats.shape[0] != B or known_feats.shape[2] != known.shape[1]:
                raise ValueError("known [B,m,3] and known_feats [B,C2,m] do not match: %s, %s" % (tuple(known.shape), tuple(known_feats.shape)))
        elif known_feats.shape[0] != B or known_feats.shape[2] != 1:
            raise ValueError("with known=None known_feats must be [B,C2,1], got %s" % (tuple(known_feats.shape),))
        if unknow_feats is not None:
            unknow_feats = pointnet2_utils._gpu(unknow_feats, "unknow_feats", torch.float32, 3)
            if unknow_feats.shape[0] != B or unknow_feats.shape[2] != n:
                raise ValueError("unknow_feats must be [B = %d, C1, n = %d], got %s" % (B, n, tuple(unknow_feats.shape)))
        if not (self.fused and self.mlp.hip_route):
            return self._forward_unfused(unknown, known, unknow_feats, known_feats)
        if known is not None:
            idx, weight = self._weights(unknown, known)
            idx = idx.to(torch.int64)
        else:
            idx = torch.zeros((B, n, 1), dtype=torch.int64, device=unknown.device)
            weight = torch.ones((B, n, 1), dtype=torch.float32, device=unknown.device)
        rows = _FPInputFn.apply(known_feats, unknow_feats, idx, weight.contiguous())
        out = rows_mlp(rows, self.mlp, 1, "none", self.training)
        return _RowsToCmFn.apply(out.view(B, n, -1))
