"""nn.Module surface of the hot path: drop-in for the reference's `Generator`, `Discriminator`,
`EdgeBlock`, `AdaptivePointNorm` (Generation/Generator.py, Generation/Discriminator.py).

The modules own torch.nn layers purely as *parameter containers*: constructed in the reference's
order, so `state_dict()` keys/shapes and default initial values match and reference checkpoints
load both ways.  Their `forward` never calls those layers: it runs the HIP pipelines of
`functions.py` / `edge_conv.py` / `nets.py`.  There is no CPU path: inputs must be on the GPU.
"""
from __future__ import annotations

import math
import weakref
from typing import List, Optional

import torch
import torch.nn as nn

from . import edge_conv
from . import functions as Fn
from . import nets, ops
from .functions import _Holder

NEG = nets.NEG


class _EqualLR(nn.Module):
    """Equalised learning rate (`EqualLR` / `EqualConv1d` / `EqualLinear`, Generation/modules.py:202-239,259-288): the wrapped
    layer keeps `weight_orig` ~ N(0,1) and a zero bias as parameters (state_dict keys `<name>.conv.weight_orig`,
    `<name>.conv.bias` / `<name>.linear.*`), and every forward uses weight_orig * sqrt(2 / fan_in)."""
    _inner = "conv"

    def _wrap(self, layer: nn.Module):
        with torch.no_grad():
            layer.weight.normal_()
            layer.bias.zero_()
        w = layer.weight
        del layer._parameters["weight"]
        layer.register_parameter("weight_orig", nn.Parameter(w.data))
        fan_in = w.shape[1] * (w[0][0].numel() if w.dim() > 2 else 1)
        self.scale = math.sqrt(2.0 / fan_in)
        setattr(self, self._inner, layer)

    @property
    def weight(self):
        return Fn.ScaleFn.apply(getattr(self, self._inner).weight_orig, self.scale)

    @property
    def bias(self):
        return getattr(self, self._inner).bias


class EqualConv1d(_EqualLR):
    def __init__(self, *args, **kwargs):
        super().__init__()
        self._wrap(nn.Conv1d(*args, **kwargs))


class EqualLinear(_EqualLR):
    _inner = "linear"

    def __init__(self, in_dim, out_dim):
        super().__init__()
        self._wrap(nn.Linear(in_dim, out_dim))


class Attention(nn.Module):
    """Generation/modules.py:534-558: non-local block over the points of a shape.  forward(x [B,ch,N]) -> [B,ch,N].
    materialize=True (the default) writes the [B,N,N] attention map and keeps it for the backward.  materialize=False (the argument,
    or the attribute set afterwards) runs spgan.point_attn's online softmax instead: memory O(B N ch), no map; it
    serves ch // 8 <= 128 and ch // 2 <= 512 (ValueError otherwise).  The parameters and the state_dict are the same either way."""

    def __init__(self, ch: int, name: str = "attention", materialize: bool = True):
        super().__init__()
        self.ch = ch
        self.materialize = bool(materialize)
        if not self.materialize:
            self._check_fused_domain()
        self.theta = nn.Conv1d(ch, ch // 8, 1, bias=False)
        self.phi = nn.Conv1d(ch, ch // 8, 1, bias=False)
        self.g = nn.Conv1d(ch, ch // 2, 1, bias=False)
        self.o = nn.Conv1d(ch // 2, ch, 1, bias=False)
        self.gamma = nn.Parameter(torch.tensor(0.), requires_grad=True)

    def _check_fused_domain(self):
        from . import point_attn
        try:
            point_attn.padded_dk(self.ch // 8)
            point_attn.padded_dv(self.ch // 2)
        except ValueError as e:
            raise ValueError("Attention(ch=%d, materialize=False): %s" % (self.ch, e)) from None

    def forward_pm(self, x_pm, B: int, N: int):
        if not self.materialize:
            self._check_fused_domain()
        return Fn.AttentionFn.apply(_Holder(B=B, N=N, materialize=bool(self.materialize)), x_pm, self.theta.weight, self.phi.weight,
                                    self.g.weight, self.o.weight, self.gamma)

    def forward(self, x, y=None):
        _require_gpu(x, "Attention")
        B, C, N = x.shape
        return Fn.PmToCm.apply(self.forward_pm(Fn.CmToPm.apply(x), B, N), B, N)


class Self_Attn(nn.Module):
    """Common/utilities.py:210-245: the SAGAN block over the points of a shape.  forward(x [B,C,N]) -> [B,C,N] = gamma * attn + x with
    out[:, :, j] = sum_i softmax_i(query_i . key_j) value_i: the reference normalises over the FIRST point index (softmax(query_key, 1))
    and sums over it, so `key` plays the attending side.  query / key / value are nn.Conv1d with bias, in the reference's order:
    state_dicts load strictly both ways.  Runs on spgan.point_attn (no [B,N,N] map); in_dim in 8..512 (ValueError otherwise), and
    B * N * C a multiple of 4.  Differentiable once in x and every parameter.  `activation` is stored and unused, as in the reference."""

    def __init__(self, in_dim: int = 128, activation: str = "relu"):
        super().__init__()
        from . import point_attn
        in_dim = int(in_dim)
        try:
            point_attn.padded_dk(in_dim // 8)
            point_attn.padded_dv(in_dim)
        except ValueError as e:
            raise ValueError("Self_Attn(in_dim=%d): %s" % (in_dim, e)) from None
        self.chanel_in = in_dim
        self.activation = activation
        self.query = nn.Conv1d(in_channels=in_dim, out_channels=in_dim // 8, kernel_size=1)
        self.key = nn.Conv1d(in_channels=in_dim, out_channels=in_dim // 8, kernel_size=1)
        self.value = nn.Conv1d(in_channels=in_dim, out_channels=in_dim, kernel_size=1)
        self.gamma = nn.Parameter(torch.zeros(1))

    def forward_pm(self, x_pm, B: int, N: int):
        from . import point_attn
        return point_attn.SelfAttnFn.apply(_Holder(B=B, N=N), x_pm, self.query.weight, self.query.bias, self.key.weight, self.key.bias,
                                           self.value.weight, self.value.bias, self.gamma)

    def forward(self, x):
        _require_gpu(x, "Self_Attn")
        if x.dim() != 3 or x.shape[1] != self.chanel_in:
            raise ValueError("Self_Attn: x must be [B,%d,N], got %s" % (self.chanel_in, tuple(x.shape)))
        B, C, N = x.shape
        return Fn.PmToCm.apply(self.forward_pm(Fn.CmToPm.apply(x), B, N), B, N)


def _stack(spec, eql: bool = False):
    """spec: list of ('conv1d'|'conv2d'|'linear', cin, cout[, ksize]) | ('bn1d'|'bn2d', c) | ('lrelu',) | ('tanh',).
    eql: Conv1d / Linear become their equalised-LR wrappers."""
    layers = []
    for s in spec:
        kind = s[0]
        if kind == "conv1d" and eql:
            layers.append(EqualConv1d(s[1], s[2], 1))
        elif kind == "linear" and eql:
            layers.append(EqualLinear(s[1], s[2]))
        elif kind == "conv1d":
            layers.append(nn.Conv1d(s[1], s[2], 1))
        elif kind == "conv2d":
            layers.append(nn.Conv2d(s[1], s[2], s[3] if len(s) > 3 else 1))
        elif kind == "linear":
            layers.append(nn.Linear(s[1], s[2]))
        elif kind == "bn1d":
            layers.append(nn.BatchNorm1d(s[1]))
        elif kind == "bn2d":
            layers.append(nn.BatchNorm2d(s[1]))
        elif kind == "lrelu":
            layers.append(nn.LeakyReLU(NEG, inplace=True))
        elif kind == "tanh":
            layers.append(nn.Tanh())
        else:
            raise ValueError(kind)
    return nn.Sequential(*layers)


def _require_gpu(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError("%s: spgan modules run only on the GPU through libspgan_hip.so (no CPU fallback); got a %s tensor" % (what, t.device))


def _named(module: nn.Module, prefix: str = ""):
    names = [n for n, _ in module.named_parameters()]
    params = [p for _, p in module.named_parameters()]
    return [prefix + n for n in names], params


def _buffers(module: nn.Module, prefix: str = ""):
    d = {prefix + n: b for n, b in module.named_buffers()}
    if isinstance(module, _BNCounts):
        d["__pending_counts__"] = module._pending(prefix)
    return d


class _BNCounts:
    """BatchNorm's `num_batches_tracked` is bookkeeping only (momentum is fixed): the increments are counted on the host
    and written to the int64 buffers when somebody looks (state_dict(), flush_bn_counts()), instead of one tiny
    kernel launch per BatchNorm per forward (36 per train step)."""

    def _pending(self, prefix: str) -> dict:
        store = self.__dict__.setdefault("_bn_pending", {})
        return store.setdefault(prefix, {})

    def _flush_own(self):
        bufs = dict(self.named_buffers())
        for prefix, pend in self.__dict__.get("_bn_pending", {}).items():
            for key, n in pend.items():
                if n:
                    bufs[key[len(prefix):]] += n
            pend.clear()

    def flush_bn_counts(self):
        """Write the host-side BatchNorm call counts of this module and its sub-modules into `num_batches_tracked`."""
        for m in self.modules():
            if isinstance(m, _BNCounts):
                m._flush_own()

    def _discard_own(self, *args):
        """load_state_dict replaces `num_batches_tracked`: counts of forwards that ran before the load must not be added later."""
        for pend in self.__dict__.get("_bn_pending", {}).values():
            pend.clear()

    def _install_count_hook(self):
        self.register_state_dict_pre_hook(lambda module, prefix, keep_vars: module._flush_own())
        self._register_load_state_dict_pre_hook(self._discard_own)


class AdaptivePointNorm(nn.Module):
    """Generator.py:24-45: out = gamma*InstanceNorm(x) + beta, [gamma|beta] = Conv1d(style_dim, 2C, 1)(style) per point.
    forward(input [B,C,N], style [B,S,N]) -> [B,C,N]"""

    def __init__(self, in_channel: int, style_dim: int, use_eql: bool = False):
        super().__init__()
        if use_eql:
            raise NotImplementedError("equalised-LR AdaIN (--eql) is not part of the accelerated path yet")
        self.norm = nn.InstanceNorm1d(in_channel)
        self.style = nn.Conv1d(style_dim, in_channel * 2, 1)
        with torch.no_grad():
            self.style.weight.normal_()
            self.style.bias.zero_()
            self.style.bias[:in_channel] = 1

    def forward_pm(self, x_pm, style_pm, N: int, slope: float = 1.0, style_chain=None, reuse=None):
        """style_chain = (dict, role): two AdaIN layers fed by the SAME style tensor (the generator's adain1 / adain2) hand the style
        gradient along instead of leaving its sum to autograd -- see Fn.AdaINFn.backward.  reuse = (out, ctx): already evaluated
        (nets.g_pair_forward), only the autograd node is built."""
        return Fn.AdaINFn.apply(_Holder(prefix="a", N=N, slope=slope, style_chain=style_chain, reuse=reuse), x_pm, style_pm, self.style.weight,
                                self.style.bias)

    def forward(self, input, style):
        _require_gpu(input, "AdaptivePointNorm")
        B, C, N = input.shape
        out = self.forward_pm(Fn.CmToPm.apply(input), Fn.CmToPm.apply(style), N)
        return Fn.PmToCm.apply(out, B, N)


class EdgeBlock(nn.Module, _BNCounts):
    """Generator.py:47-88.  forward(x [B,Fin,N]) -> [B,Fout,N]."""

    def __init__(self, Fin: int, Fout: int, k: int, attn: bool = True):
        super().__init__()
        self.k, self.Fin, self.Fout = k, Fin, Fout
        self.conv_w = _stack([("conv2d", Fin, Fout // 2), ("bn2d", Fout // 2), ("lrelu",), ("conv2d", Fout // 2, Fout), ("bn2d", Fout), ("lrelu",)])
        self.conv_x = _stack([("conv2d", 2 * Fin, Fout, [1, 1]), ("bn2d", Fout), ("lrelu",)])
        self.conv_out = nn.Conv2d(Fout, Fout, [1, k], [1, 1])
        self.last_idx: Optional[torch.Tensor] = None      # int32 [B*N, k] global rows of the most recent forward
        self._install_count_hook()

    def forward_pm(self, x_pm, B: int, N: int, idx: Optional[torch.Tensor] = None, knn_mode: Optional[int] = None,
                   graph_cache: Optional[dict] = None, count_rep: int = 1, bn_repeats: int = 1, reuse=None, keep: Optional[dict] = None,
                   update_running: bool = True):
        """bn_repeats / reuse / keep: one evaluation standing for several identical forwards (Generator: the two forwards of a train
        step see the same sphere prior and the same weights).  keep: a dict that receives (out, ctx) of this evaluation;
        reuse = (out, ctx): skip the evaluation, return `out` with `ctx` behind it for the backward pass."""
        names, params = _named(self, "e.")
        if knn_mode is None:
            knn_mode = 1 if self.Fin <= 4 else 0          # coordinates: exact fp64 order; features: fp32 expanded form
        if graph_cache is not None and idx is None:
            idx = graph_cache.get("idx")
        h = _Holder(prefix="e", names=names, buffers=_buffers(self, "e."), B=B, N=N, k=self.k, training=self.training,
                    knn_mode=knn_mode, idx=idx, last_idx=None, graph_cache=graph_cache, count_rep=count_rep, bn_repeats=bn_repeats,
                    reuse=reuse, keep=keep, update_running=update_running)
        out = Fn.EdgeBlockFn.apply(h, x_pm, *params)
        self.last_idx = h.last_idx
        if graph_cache is not None and graph_cache.get("idx") is None:
            graph_cache["idx"] = h.last_idx
        return out

    def forward(self, x, idx: Optional[torch.Tensor] = None):
        _require_gpu(x, "EdgeBlock")
        B, C, N = x.shape
        if idx is not None and idx.dtype == torch.int64:
            idx = ops.idx_from_local64(idx, B, N, self.k)
        out = self.forward_pm(Fn.CmToPm.apply(x), B, N, idx)
        return Fn.PmToCm.apply(out, B, N)


class Generator(nn.Module, _BNCounts):
    """Generation/Generator.py:91-198.  forward(x [B,N,3], z [B,N,nz]) -> [B,3,N].
    opts fields read: np, nk, nz, softmax, off, attn, use_head, eql, z_norm."""

    def __init__(self, opts):
        super().__init__()
        self.opts = opts
        self.np = opts.np
        self.nk = opts.nk // 2
        self.nz = opts.nz
        self.off = opts.off
        self.use_attn = opts.attn
        self.use_head = opts.use_head
        eql = bool(getattr(opts, "eql", False))      # Generator.py:103-104: head, global_conv's Linear and pc_head only
        dim = 128
        self.head = _stack([("conv1d", 3 + self.nz, dim), ("lrelu",), ("conv1d", dim, dim), ("lrelu",)], eql)
        if self.use_attn:
            self.attn = Attention(dim + 512)
        self.global_conv = _stack([("linear", dim, dim), ("bn1d", dim), ("lrelu",), ("linear", dim, 512), ("bn1d", 512), ("lrelu",)], eql)
        self.tail = _stack([("conv1d", 512 + dim, 256), ("lrelu",), ("conv1d", 256, 64), ("lrelu",), ("conv1d", 64, 3), ("tanh",)])
        if self.use_head:
            self.pc_head = _stack([("conv1d", 3, dim // 2), ("lrelu",), ("conv1d", dim // 2, dim), ("lrelu",)], eql)
            self.EdgeConv1 = EdgeBlock(dim, dim, self.nk)
            self.adain1 = AdaptivePointNorm(dim, dim)
            self.EdgeConv2 = EdgeBlock(dim, dim, self.nk)
            self.adain2 = AdaptivePointNorm(dim, dim)
        else:
            self.EdgeConv1 = EdgeBlock(3, 64, self.nk)
            self.adain1 = AdaptivePointNorm(64, dim)
            self.EdgeConv2 = EdgeBlock(64, dim, self.nk)
            self.adain2 = AdaptivePointNorm(dim, dim)
        self.lrelu1 = nn.LeakyReLU(nets.NEG_2)
        self.lrelu2 = nn.LeakyReLU(nets.NEG_2)
        self._install_count_hook()

    def _params_of(self, names):
        """The tensors behind reference-style names ('global_conv.0.weight'): parameters, or for equalised-LR layers the
        scaled weight computed on the fly."""
        out = []
        for n in names:
            mod, attr = n.rsplit(".", 1)
            out.append(getattr(self.get_submodule(mod), attr))
        return out

    def _mlp2(self, seq: nn.Sequential, x_pm):
        h = _Holder(names=["l0", "l2"], acts=[ops.ACT_LRELU, ops.ACT_LRELU], slope=NEG)
        return Fn.MLPFn.apply(h, x_pm, seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias)

    def _style(self, x, z):
        """head(cat[x, z]) (Generator.py:163-169).  z [B,N,nz] as in the reference, or [B,1,nz]: one latent per shape, i.e. what the
        default noise_generator tiles over the points -- then the latent half of head.0 is evaluated once per shape (HeadFn)."""
        B, N, _ = x.shape
        if self.opts.z_norm:
            z = z / (z.norm(p=2, dim=-1, keepdim=True) + 1e-8)
        if z.dim() == 3 and z.shape[1] == 1 and N > 1:
            h0, h2 = self.head[0], self.head[2]
            return Fn.HeadFn.apply(_Holder(N=N), x.reshape(B * N, 3), z.reshape(B, -1), h0.weight, h0.bias, h2.weight, h2.bias)
        hz = ops.concat2(x.reshape(B * N, 3), z.reshape(B * N, -1))
        return self._mlp2(self.head, hz)

    def _sphere_entry(self, x):
        """The cache entry of the sphere prior x [B,N,3]: its kNN graph, the CSR of its in-edges and whether every shape carries the same prior."""
        B = x.shape[0]
        # a few entries (most recent first): the training prior stays cached while an occasional call with another tensor -- a
        # sample dump with its own batch size, an eval forward -- comes and goes (building an entry costs a host sync, which a
        # stream capture that finds its entry evicted could not afford)
        sgs = self.__dict__.setdefault("_sphere_graphs", [])
        key = (x._version, tuple(x.shape), self.nk)
        sg = next((e for e in sgs if e["ref"]() is x and e["key"] == key), None)        # same tensor OBJECT (not just address), unmodified
        if sg is None:
            # Does every shape of the batch carry the SAME prior (sphere_generator(static=True) tiles one template,
            # model.py:169-171)?  Checked once per (tensor, version) -- one host sync when the cache entry is built.
            shared = B > 1 and getattr(self, "dedup_sphere", True) and bool(torch.equal(x, x[:1].expand_as(x)))
            sg = {"ref": weakref.ref(x), "key": key, "idx": None, "csr": None, "shared": shared, "idx_full": None}
            sgs[:] = [e for e in sgs if e["ref"]() is not None and e["ref"]() is not x][:3]
        else:
            sgs[:] = [e for e in sgs if e is not sg]
        sgs.insert(0, sg)
        self.__dict__["_sphere_graph"] = sg
        return sg

    def pair_ok(self, x, z_d, z_g) -> bool:
        """Can forward_pair evaluate G(x, z_d) and G(x, z_g) as one pipeline?  The default generator in train mode, one latent per shape
        ([B,1,nz]), every shape carrying the same prior (its cache entry exists or can be built: not inside a stream capture)."""
        if (self.use_head or self.use_attn or self.off or not self.training or bool(getattr(self.opts, "eql", False))
                or x.dim() != 3 or z_d.shape != z_g.shape or z_d.dim() != 3 or z_d.shape[1] != 1 or x.shape[1] <= 1):
            return False
        return bool(self._sphere_entry(x)["shared"])

    def forward_pair(self, x, z_d, z_g):
        """(G(x, z_d).detach(), G(x, z_g)), both point-major [B*N,3]: the two generator forwards of one train step (model.py:246-248 and
        264-271) as ONE pipeline over the rows of both passes (nets.g_pair_forward) -- same prior, same weights, and the second depends on
        nothing the D step in between produces.  EdgeConv1 is evaluated once for one copy of the prior (as in the twin protocol of _body),
        the per-point / per-shape stages run once on 2B shapes, the BatchNorm stages per pass in the reference's order; the autograd graph of
        the second forward is built from the saved contexts of its rows only.  Values, running statistics and call counts are those of the
        two separate calls."""
        B, N, _ = x.shape
        M = B * N
        cache = self._sphere_entry(x)
        pc = x.reshape(M, 3).contiguous()
        slope = nets.NEG_2
        if self.opts.z_norm:
            z_d = z_d / (z_d.norm(p=2, dim=-1, keepdim=True) + 1e-8)
            z_g = z_g / (z_g.norm(p=2, dim=-1, keepdim=True) + 1e-8)
        self.__dict__["_ec1_twin"] = None
        x1_one = self.EdgeConv1.forward_pm(pc[:N], 1, N, knn_mode=1, graph_cache=cache, count_rep=B, bn_repeats=2)
        if cache["idx_full"] is None:
            off = (torch.arange(B, device=x.device, dtype=torch.int32) * N).view(B, 1, 1)
            cache["idx_full"] = (cache["idx"].view(1, N, -1) + off).reshape(B * N, -1).contiguous()
        self.EdgeConv1.last_idx = cache["idx_full"]
        h0, h2 = self.head[0], self.head[2]
        Ph = {"head.0.weight": h0.weight, "head.0.bias": h0.bias, "head.2.weight": h2.weight, "head.2.bias": h2.bias}
        Pa1 = {"a.style.weight": self.adain1.style.weight, "a.style.bias": self.adain1.style.bias}
        Pa2 = {"a.style.weight": self.adain2.style.weight, "a.style.bias": self.adain2.style.bias}
        en, ep = _named(self.EdgeConv2, "e.")
        gt_params = self._params_of(Fn.GT_NAMES)
        q = self.__dict__.get("_graph2_queue")
        idx2 = [q.pop(0) if q else None, q.pop(0) if q else None]
        idx2 = [None if g is None else (g if g.dtype == torch.int32 else ops.idx_from_local64(g.to(torch.int64).reshape(B, -1), B, N, self.nk)) for g in idx2]
        zg = z_g.reshape(B, -1)
        with torch.no_grad():
            pc2 = cache.get("pc2")                  # the prior's rows for both passes: constant, kept with the prior's cache entry
            if pc2 is None:
                pc2 = pc.repeat(2, 1)
                if not ops.capturing():
                    cache["pc2"] = pc2
            zb2 = torch.cat([z_d.reshape(B, -1), zg], dim=0)
            pre = nets.g_pair_forward({k_: nets.owned(v) for k_, v in Ph.items()}, {k_: nets.owned(v) for k_, v in Pa1.items()},
                                      dict(zip(en, [nets.owned(p) for p in ep])), _buffers(self.EdgeConv2, "e."),
                                      {k_: nets.owned(v) for k_, v in Pa2.items()}, dict(zip(Fn.GT_NAMES, [nets.owned(p) for p in gt_params])),
                                      _buffers(self), pc2, zb2, x1_one.detach(), B, N, self.nk, slope, self.training, idx2=idx2)
        # the autograd graph of the second forward: the usual nodes, adopting their rows and saved contexts
        style = Fn.HeadFn.apply(_Holder(N=N, reuse=pre["head"]), pc, zg, h0.weight, h0.bias, h2.weight, h2.bias)
        x1 = Fn.RepeatRowsFn.apply(x1_one, B, pre["x1"])
        chain = {} if torch.is_grad_enabled() else None
        a1 = self.adain1.forward_pm(x1, style, N, slope, style_chain=None if chain is None else (chain, "last"), reuse=pre["adain1"])
        self.last_x1 = pre["x1_in"].detach()
        x2 = self.EdgeConv2.forward_pm(a1, B, N, knn_mode=0, reuse=pre["ec2"])
        a2 = self.adain2.forward_pm(x2, style, N, slope, style_chain=None if chain is None else (chain, "first"), reuse=pre["adain2"])
        self.last_x2 = pre["a2"].detach()
        h = _Holder(buffers=_buffers(self), B=B, N=N, training=self.training, reuse=pre["tail"])
        out = Fn.GlobalTailFn.apply(h, a2, *gt_params)
        self.__dict__["_pair_idx"] = pre["idx"]
        return pre["fake_d"], out

    def _body(self, x, style, pm_out: bool = False):
        B, N, _ = x.shape
        pc = x.reshape(B * N, 3).contiguous()
        feat = self._mlp2(self.pc_head, pc) if self.use_head else pc
        slope = nets.NEG_2
        # The sphere prior is the same tensor every step (Generation/model.py:231): its kNN graph (and the CSR of
        # its in-edges) is built once per (buffer, version, shape) and reused.  Any in-place write
        # to x bumps _version and invalidates the cache.
        cache = None if self.use_head else self._sphere_entry(x)
        if cache is not None and cache["shared"]:
            # EdgeConv1 sees the same N points in every shape: evaluate it for ONE copy (B times less work in forward and
            # backward; exact -- batch statistics of identical copies are those of one copy, and the backward is linear in the
            # upstream gradient, which RepeatRowsFn sums over the copies) and repeat the rows for the per-shape AdaIN.
            # TrainStep announces that this forward and the next one see the same prior and the same weights (D step, then G step):
            # EdgeConv1 is evaluated once, its running statistics advanced twice (`twin_forward`: "first" / "second")
            twin = getattr(self, "twin_forward", None)
            saved = self.__dict__.get("_ec1_twin")
            stamp = (id(cache), tuple(p._version for p in self.EdgeConv1.parameters()), ops.weights_epoch_of(next(self.EdgeConv1.parameters())), B, N)
            if twin == "second" and saved is not None and saved["stamp"] == stamp and self.training:
                x1_one = self.EdgeConv1.forward_pm(feat[:N], 1, N, knn_mode=1, graph_cache=cache, count_rep=B, reuse=(saved["out"], saved["ctx"]))
                self.__dict__["_ec1_twin"] = None
            elif twin == "first" and self.training:
                keep = {"stamp": stamp}
                x1_one = self.EdgeConv1.forward_pm(feat[:N], 1, N, knn_mode=1, graph_cache=cache, count_rep=B, bn_repeats=2, keep=keep)
                self.__dict__["_ec1_twin"] = keep
            elif twin == "second" and saved is not None and self.training:
                # announced as the twin of an earlier forward that already advanced EdgeConv1's running statistics for BOTH, but its
                # output cannot be reused (the weights, the prior or the batch changed in between): evaluate, do not advance them a
                # third time
                self.__dict__["_ec1_twin"] = None
                x1_one = self.EdgeConv1.forward_pm(feat[:N], 1, N, knn_mode=1, graph_cache=cache, count_rep=B, update_running=False)
            else:
                if twin is not None:                 # a forward outside the twin protocol (eval call, sample dump) leaves a pending twin alone
                    self.__dict__["_ec1_twin"] = None
                x1_one = self.EdgeConv1.forward_pm(feat[:N], 1, N, knn_mode=1, graph_cache=cache, count_rep=B)
            if cache["idx_full"] is None:
                off = (torch.arange(B, device=x.device, dtype=torch.int32) * N).view(B, 1, 1)
                cache["idx_full"] = (cache["idx"].view(1, N, -1) + off).reshape(B * N, -1).contiguous()
            self.EdgeConv1.last_idx = cache["idx_full"]
            x1 = Fn.RepeatRowsFn.apply(x1_one, B)
        else:
            x1 = self.EdgeConv1.forward_pm(feat, B, N, knn_mode=0 if self.use_head else 1, graph_cache=cache)
        # both AdaIN layers read the same style tensor: adain2's backward (which runs first) stashes its style gradient, adain1's adds it
        # in the epilogue of its own style-gradient GEMM -- instead of an autograd add over a [B*N, 128] tensor
        chain = {} if (style.requires_grad and torch.is_grad_enabled()) else None
        x1 = self.adain1.forward_pm(x1, style, N, slope, style_chain=None if chain is None else (chain, "last"))    # lrelu1 fused into the instance norm (Generator.py:175-176)
        self.last_x1 = x1.detach()                                 # [M,64] input of EdgeConv2's graph (diagnostics / parity tests)
        # Tie-aware parity protocol: a caller may hand over EdgeConv2's kNN graph(s) for the next forward(s) --
        # `inject_graph2([idx, ...])`, int32 [B*N,k] global rows or the reference's int64 [B,N*k] local indices -- e.g. the graph
        # the reference itself built on this stage, so that everything behind the discrete choice is compared tightly.
        q = self.__dict__.get("_graph2_queue")
        idx2 = q.pop(0) if q else None
        if idx2 is not None and idx2.dtype != torch.int32:
            idx2 = ops.idx_from_local64(idx2.to(torch.int64).reshape(B, -1), B, N, self.nk)
        x2 = self.EdgeConv2.forward_pm(x1, B, N, idx=idx2, knn_mode=0)
        x2 = self.adain2.forward_pm(x2, style, N, slope, style_chain=None if chain is None else (chain, "first"))
        self.last_x2 = x2.detach()                                 # [M,128] adain2's output (parity tests)
        h = _Holder(buffers=_buffers(self), B=B, N=N, training=self.training)
        if self.use_attn:
            feat = Fn.GlobalFeatFn.apply(h, x2, *self._params_of(Fn.GF_NAMES))                    # [M,640], Generator.py:183-189
            feat = self.attn.forward_pm(feat, B, N)                                              # Generator.py:191-192
            th = _Holder(names=["tail.0", "tail.2", "tail.4"], acts=[ops.ACT_LRELU, ops.ACT_LRELU, ops.ACT_TANH], slope=NEG)
            out = Fn.MLPFn.apply(th, feat, *self._params_of(Fn.GT_NAMES[len(Fn.GF_NAMES):]))
        else:
            out = Fn.GlobalTailFn.apply(h, x2, *self._params_of(Fn.GT_NAMES))
        if pm_out and not self.off:
            return out                              # [B*N,3] point-major: TrainStep's internal route hands it to the Discriminator as it is
        out = Fn.PmToCm.apply(out, B, N)
        return x.transpose(2, 1) + out if self.off else out

    def forward(self, x, z, pm_out: bool = False):
        """pm_out=True (TrainStep's internal route; not with --off): return the cloud point-major [B*N,3], i.e. without the final layout
        change to the reference's [B,3,N] -- Discriminator.forward_stacks_grouped / forward(..., pm_shape=(B,N)) take it as it is."""
        _require_gpu(x, "Generator")
        return self._body(x, self._style(x, z), pm_out=pm_out)

    def inject_graph2(self, graphs) -> None:
        """EdgeConv2's neighbour graph for the next len(graphs) forwards, consumed in order (see _body).  None = build it."""
        self.__dict__["_graph2_queue"] = [None if g is None else g.to(next(self.parameters()).device) for g in graphs]

    def interpolate(self, x, z1, z2, selection, alpha, use_latent: bool = False):
        """Generator.py:200-261: blend two latents (or two styles) on the selected points."""
        sel = selection == 1
        if not use_latent:
            z = z1
            z[:, sel] = z1[:, sel] * (1 - alpha) + z2[:, sel] * alpha
            style = self._style(x, z)
        else:
            s1, s2 = self._style(x, z1), self._style(x, z2)
            B, N, _ = x.shape
            s1 = s1.view(B, N, -1); s2 = s2.view(B, N, -1)
            s1[:, sel] = s1[:, sel] * (1 - alpha) + s2[:, sel] * alpha
            style = s1.reshape(B * N, -1)
        return self._body(x, style)


class Discriminator(nn.Module, _BNCounts):
    """Generation/Discriminator.py:48-115.  forward(x [B,3,N]) -> [B,1].  Supports autograd.grad(create_graph=True)
    w.r.t. its input followed by backward() (WGAN-GP)."""

    def __init__(self, opts, num_point: int = 2048):
        super().__init__()
        self.num_point = num_point
        self.small_d = opts.small_d
        self.mlps = _stack([("conv1d", 3, 64), ("bn1d", 64), ("lrelu",), ("conv1d", 64, 128), ("bn1d", 128), ("lrelu",),
                            ("conv1d", 128, 256), ("bn1d", 256), ("lrelu",)])
        self.mode = "max"
        dim = 512 if self.small_d else 1024
        self.fc2 = _stack([("conv1d", 256, dim), ("bn1d", dim), ("lrelu",)])
        self.mlp = _stack([("linear", dim, 512), ("lrelu",), ("linear", 512, 256), ("lrelu",), ("linear", 256, 64), ("lrelu",), ("linear", 64, 1)])
        self._install_count_hook()

    def forward(self, x, pre=None):
        """pre: this input's entry of `forward_stacks_grouped(...)` -- its conv stack was evaluated there, only the head runs here."""
        _require_gpu(x, "Discriminator")
        names, params = _named(self)
        h = _Holder(names=names, buffers=_buffers(self), training=self.training, pre=pre)
        return Fn.DiscriminatorFn.apply(h, x.contiguous(), *params)

    def forward_stack_after_stats_pass(self, stats_x, x, pm_shape=None):
        """The side effect of a train-mode D(stats_x) whose result nobody reads (`advance_running_stats`) followed by the conv stack of
        D(x), the shared first three layers of the two passes as one batch (nets.d_forward_after_stats_pass): the G step's
        D(real); D(G(z)).  Returns the entry to hand to `forward(x, pre=...)`."""
        _require_gpu(x, "Discriminator"); _require_gpu(stats_x, "Discriminator")
        if not self.training:
            raise RuntimeError("forward_stack_after_stats_pass is a train-mode path (batch statistics)")
        from . import nets
        names, params = _named(self)
        with torch.no_grad():
            P = dict(zip(names, [nets.owned(p) for p in params]))
            return nets.d_forward_after_stats_pass(P, _buffers(self), stats_x.detach(), x.detach(), pm_shape=pm_shape)

    def forward_stacks_grouped(self, xs, pm_shape=None):
        """The conv stacks of several train-mode passes as ONE batch (nets.d_forward_groups): one GEMM and one finalize launch per layer
        for all of them, per-pass BatchNorm statistics, running statistics advanced in list order -- bit-identical to separate calls.
        Returns one opaque entry per input, to be handed to `forward(x, pre=...)` or `forward_stack(x, pre=...)` of the same input."""
        for x in xs:
            _require_gpu(x, "Discriminator")
        if not self.training:
            raise RuntimeError("forward_stacks_grouped is a train-mode path (batch statistics)")
        from . import nets
        names, params = _named(self)
        with torch.no_grad():
            P = dict(zip(names, [nets.owned(p) for p in params]))
            return nets.d_forward_groups(P, _buffers(self), [x.detach() for x in xs], pm_shape=pm_shape)


def _discriminator_forward_many(self, *xs):
    """[D(x) for x in xs] with the per-shape MLP head of all passes evaluated as ONE batch: the conv stacks run one after the other
    (each with its own train-mode BatchNorm statistics and running-statistics update, in call order -- exactly what separate calls
    do), the head has no BatchNorm, so its rows are independent and cat[pooled...] goes through it once (4 launches forward and 16
    backward once instead of once per pass).  First-order only: the WGAN-GP route uses forward()."""
    return self.forward_heads([self.forward_stack(x) for x in xs])


def _discriminator_forward_stack(self, x, pre=None):
    """The conv stack up to the max-pool: x [B,3,N] -> pooled [B,C4] (train-mode BatchNorm statistics and running-statistics update
    of this pass).  pre: this input's entry of forward_stacks_grouped(...) (already evaluated there)."""
    _require_gpu(x, "Discriminator")
    sn, sp = _named(self.mlps, "mlps.")
    fn, fp = _named(self.fc2, "fc2.")
    h = _Holder(names=sn + fn, buffers=_buffers(self), training=self.training, pre=pre)
    return Fn.DStackFn.apply(h, x.contiguous(), *(sp + fp))


def _discriminator_forward_heads(self, pooled):
    """The per-shape MLP head of several forward_stack() results as one batch -> one logits tensor per pass."""
    hn, hp = _named(self.mlp, "mlp.")
    pooled = list(pooled)
    joined = pooled[0] if len(pooled) == 1 else Fn.JoinRowsFn.apply(*pooled)       # a view when one grouped launch produced the passes
    outs = Fn.DHeadFn.apply(_Holder(names=hn, sizes=[p.shape[0] for p in pooled]), joined, *hp)
    return list(outs)


def _discriminator_stacks_joint(self, firsts, hat=None):
    """The D step's passes behind one autograd node (Fn.DStacksJointFn): firsts / hat are entries of forward_stacks_grouped(...).
    -> [pooled of every first-order pass ..., gx] with gx = d sum(D(x_hat)) / d x_hat of the `hat` entry (differentiable once more: its
    backward is the penalty's double backward).  The backward work of all these passes then runs in lock step, every layer's launch issued
    once (nets.d_backward_joint) -- results as from forward_stack(pre=...) per pass and the WGAN-GP route of forward(pre=...)."""
    names, params = _named(self)
    h = _Holder(names=names, firsts=list(firsts), hat=hat)
    return list(Fn.DStacksJointFn.apply(h, *params))


def _discriminator_joint_ok(self, entries) -> bool:
    from . import nets
    names, params = _named(self)
    return nets.d_joint_ok(dict(zip(names, params)), [c for _, c in entries])


Discriminator.stacks_joint = _discriminator_stacks_joint
Discriminator.joint_ok = _discriminator_joint_ok
Discriminator.forward_many = _discriminator_forward_many
Discriminator.forward_stack = _discriminator_forward_stack
Discriminator.forward_heads = _discriminator_forward_heads


def _discriminator_advance_running_stats(self, x):
    """Train-mode D(x) reduced to its only lasting effect when the logits are not used: the BatchNorm running statistics and
    call counts (TrainStep uses it for the reference's D(real) call inside the G step, Generation/model.py:272-273)."""
    _require_gpu(x, "Discriminator")
    if not self.training:
        return
    with torch.no_grad():
        nets.d_advance_running_stats(dict(self.named_parameters()), _buffers(self), x.contiguous())


Discriminator.advance_running_stats = _discriminator_advance_running_stats


def get_edge_features(x, k, num=-1, idx=None, return_idx=False):
    """Generation/modules.py:683-725: x [B,C,N] -> ee [B,2C,N,k] (= cat[central, neighbour-central]); optional injected /
    returned idx is int64 [B, N*k] with per-shape local indices, like the reference.  Differentiable in x like the reference's
    gather/concat (the indices carry no gradient): the backward sums, per point, its own k central / difference terms and the
    difference terms of the edges that gathered it, in edge order (Fn.EdgeFeaturesFn; no float atomics).  The Generator path itself
    never materialises ee -- EdgeBlock carries its own fused backward."""
    _require_gpu(x, "get_edge_features")
    B, C, N = x.shape
    x = x.contiguous()
    if idx is None:
        with torch.no_grad():
            gidx = ops.knn(ops.cm_to_pm(x.detach()), B, N, k, 1 if C <= 4 else 0)
            idx = ops.idx_to_local64(gidx, B, N)
    idx = idx.contiguous().view(B, N * k)
    if x.requires_grad and torch.is_grad_enabled():
        ee = Fn.EdgeFeaturesFn.apply(x, idx, k)
    else:
        ee = ops.edge_features_cm(x, idx, k)
    return (ee, idx) if return_idx else ee


class conv2dbr(nn.Module):
    """Generation/modules.py:612-626: Conv2d -> BatchNorm2d -> ReLU, [B,Fin,H,W] -> [B,Fout,H,W].  Only the 1x1 / stride-1 case runs (a GEMM
    over the B*H*W positions with the BatchNorm statistics in its epilogue: the shared-MLP layer path of pointnet_util); the module is
    the parameter container of `edgeConv`, whose forward never materialises this layer's input."""

    def __init__(self, Fin, Fout, kernel_size, stride=[1, 1]):
        super().__init__()
        self.conv = nn.Conv2d(Fin, Fout, kernel_size, stride)
        self.bn = nn.BatchNorm2d(Fout)
        self.ac = nn.ReLU(True)

    def forward(self, x):
        _require_gpu(x, "conv2dbr")
        if tuple(self.conv.kernel_size) != (1, 1) or tuple(self.conv.stride) != (1, 1):
            raise NotImplementedError("conv2dbr runs only the 1x1, stride-1 convolution (kernel_size %s, stride %s)"
                                      % (tuple(self.conv.kernel_size), tuple(self.conv.stride)))
        from . import pointnet_util
        B, C, H, W = x.shape
        rows = x.permute(0, 2, 3, 1).reshape(B * H * W, C)
        out = pointnet_util._shared_mlp(rows, 1, [self.conv], [self.bn], self.training)
        return out.view(B, H, W, -1).permute(0, 3, 1, 2)


def check_edge_input(name: str, x, idx, k: int, Fin: int, Fout: int, bns, unsupported: Optional[str] = None):
    """The input check of the gather-side edge convolutions (spgan.edge_conv) -> (B, N, idx, knn_mode): x [B,Fin,N] on the GPU, BatchNorm
    modules that keep running statistics with a momentum, and an injected graph -- int64 [B, N*k] local indices, range-checked outside a
    capture, are converted to the layers' int32 [B*N,k] global rows; a graph already in that format is trusted.  unsupported: a layer's
    own refusal of its settings, raised with the BatchNorm refusals (before idx is looked at)."""
    _require_gpu(x, name)
    B, C, N = x.shape
    if C != Fin:
        raise ValueError("%s(%d, %d, %d) got an input with %d channels" % (name, Fin, Fout, k, C))
    for bn in bns:
        if bn.momentum is None or not bn.track_running_stats:
            raise NotImplementedError("%s: BatchNorm2d with momentum=None or track_running_stats=False is not supported" % name)
    if unsupported is not None:
        raise NotImplementedError("%s: %s" % (name, unsupported))
    if idx is not None:
        _require_gpu(idx, name + " idx")
        if idx.dtype == torch.int64:
            if idx.numel() != B * N * k:
                raise ValueError("%s: idx must hold B*N*k = %d indices, got %s" % (name, B * N * k, tuple(idx.shape)))
            if not ops.capturing() and (int(idx.min()) < 0 or int(idx.max()) >= N):
                raise IndexError("%s: a neighbour index lies outside [0, %d)" % (name, N))
            idx = ops.idx_from_local64(idx.reshape(B, N * k), B, N, k)
        elif idx.dtype != torch.int32 or tuple(idx.shape) != (B * N, k):
            raise ValueError("%s: idx must be int64 [B, N*k] (local) or int32 [B*N, k] (global rows)" % name)
    return B, N, idx, 1 if Fin <= 4 else 0


class edgeConv(nn.Module):
    """Generation/modules.py:779-796: max over the k neighbours of conv2dbr(get_edge_features(x)), [B,Fin,N] -> [B,Fout,N], evaluated per
    point (edge_conv.EdgeMaxConvFn): no [B,2Fin,N,k] tensor in forward or backward.  idx (an extension): the graph to use instead of the kNN
    graph of x, int64 [B, N*k] local indices as get_edge_features returns them (or int32 [B*N,k] global rows: the layer's own format, trusted -- only
    int64 graphs are range-checked).  A negative bn.weight
    entry takes the min branch.  last_idx / last_sel: the graph and the selected ranks of the latest forward.
    double_backward (an extension, and a plain attribute; not part of the state_dict): False -- the default -- leaves the layer once
    differentiable: a backward asked to build a graph (create_graph=True) raises.  True makes the input gradient differentiable once
    more (edge_conv.EdgeMaxConvBwdFn): torch.autograd.grad(out, x, create_graph=True) returns a dx with a graph whose
    backward delivers gradients for x (train mode; None in eval mode, where the statistics are constants), conv.conv.weight,
    conv.bn.weight and the incoming cotangent (which chains stacked layers); conv.conv.bias and conv.bn.bias have no second derivative
    (None).  That is what a gradient penalty needs (spgan.GradientPenalty, R1); only second derivatives THROUGH dx are served: a cotangent
    on the first backward's parameter gradients raises NotImplementedError, and a third derivative raises RuntimeError.  Without
    create_graph the same launches run in the same order as in the default layer.  Inside functions.input_grad_only() (GradientPenalty's
    forward) the differentiable first backward skips the parameter gradients (dW, db, dgamma, dbeta), which the penalty never consumes, and
    returns None for them."""

    def __init__(self, Fin, Fout, k, double_backward: bool = False):
        super().__init__()
        if not 1 <= k <= 127:
            raise ValueError("edgeConv: k must lie in 1..127")
        self.k = k
        self.double_backward = bool(double_backward)
        self.Fin = Fin
        self.Fout = Fout
        self.conv = conv2dbr(2 * Fin, Fout, 1)
        self.last_idx: Optional[torch.Tensor] = None
        self.last_sel: Optional[torch.Tensor] = None

    def forward(self, x, idx: Optional[torch.Tensor] = None):
        bn = self.conv.bn
        B, N, idx, knn_mode = check_edge_input("edgeConv", x, idx, self.k, self.Fin, self.Fout, (bn,))
        h = _Holder(B=B, N=N, k=self.k, training=self.training, idx=idx, knn_mode=knn_mode, bn=bn, last_idx=None, last_sel=None,
                    double_backward=bool(self.double_backward), input_only=Fn._mode("input_only"))
        out = edge_conv.EdgeMaxConvFn.apply(h, x.contiguous(), self.conv.conv.weight, self.conv.conv.bias, bn.weight, bn.bias)
        self.last_idx, self.last_sel = h.last_idx, h.last_sel
        return out


def get_edge_features_xyz(x, pc, k, num=-1):
    """Generation/modules.py:727-776: x [B,C,N], pc [B,3,N] -> (e_fea [B,2C,N,k], e_xyz [B,6,N,k]): ONE kNN graph, built in the feature
    space of x, gathers both tensors (cat[central, neighbour-central] each).  Differentiable in x and pc through get_edge_features'
    backward; the indices carry no gradient."""
    _require_gpu(x, "get_edge_features_xyz")
    _require_gpu(pc, "get_edge_features_xyz pc")
    if pc.dim() != 3 or pc.shape[0] != x.shape[0] or pc.shape[1] != 3 or pc.shape[2] != x.shape[2]:
        raise ValueError("get_edge_features_xyz: pc must be [B,3,N] for x [B,C,N], got %s and %s" % (tuple(pc.shape), tuple(x.shape)))
    e_fea, idx = get_edge_features(x, k, num, return_idx=True)
    return e_fea, get_edge_features(pc, k, num, idx=idx)


class upsample_edgeConv(nn.Module):
    """Generation/modules.py:799-845: the point-doubling edge convolution, [B,Fin,N] -> [B,Fout,2N]:
    conv2(cat(ee, reshuffled inte_conv_hk(ee))) with ee = get_edge_features(x), evaluated over gathered neighbour rows
    (edge_conv.UpsampleEdgeConvFn, csrc/edge_window.hip): neither ee nor the merged [B,2Fin,N,2k] tensor exists in forward or backward.
    The sub-modules are parameter containers in the reference's order (state_dicts load strictly both ways); conv2 on its own still
    refuses its [1,2k] kernel.  idx (an extension, as edgeConv's): the graph to use instead of the kNN graph of x, int64 [B, N*k] local
    indices (range-checked outside a capture) or int32 [B*N,k] global rows (trusted).  Once differentiable.  last_idx: the graph of
    the latest forward."""

    def __init__(self, Fin, Fout, k, num):
        super().__init__()
        if k % 2 or k < 2:
            raise ValueError("upsample_edgeConv: k must be even (the reference's view of the [.., k/2] tensor as [.., k] fails otherwise), got %d" % k)
        if k > 28:
            raise ValueError("upsample_edgeConv: k must not exceed 28")
        self.k = k
        self.Fin = Fin
        self.Fout = Fout
        self.num = num
        self.conv2 = conv2dbr(2 * Fin, 2 * Fout, [1, 2 * k], [1, 1])
        self.inte_conv_hk = nn.Sequential(
            nn.Conv2d(2 * Fin, 4 * Fin, [1, k // 2 + 1], [1, 1]),
            nn.BatchNorm2d(4 * Fin),
            nn.LeakyReLU(inplace=True)
        )
        self.last_idx: Optional[torch.Tensor] = None

    def forward(self, x, idx: Optional[torch.Tensor] = None):
        conv1, bn1, act = self.inte_conv_hk[0], self.inte_conv_hk[1], self.inte_conv_hk[2]
        bn2 = self.conv2.bn
        B, N, idx, knn_mode = check_edge_input("upsample_edgeConv", x, idx, self.k, self.Fin, self.Fout, (bn1, bn2))
        h = _Holder(B=B, N=N, k=self.k, training=self.training, idx=idx, knn_mode=knn_mode, slope=float(act.negative_slope),
                    bn1=bn1, bn2=bn2, last_idx=None)
        out = edge_conv.UpsampleEdgeConvFn.apply(h, x.contiguous(), conv1.weight, conv1.bias, bn1.weight, bn1.bias,
                                                 self.conv2.conv.weight, self.conv2.conv.bias, bn2.weight, bn2.bias)
        self.last_idx = h.last_idx
        return out


class _RankEdgeConv(nn.Module):
    """The shared body of deform_edgeConv_simple / deform_edgeConv_first: conv2(inte_conv_hk(get_edge_features(x))) with
    inte_conv_hk = Conv2d(2Fin -> F1, 1x1) + BatchNorm2d + LeakyReLU and conv2 = conv2dbr(F1 -> Fout, [1,k]), evaluated over gathered rows
    of one per-point GEMM (edge_conv.RankEdgeConvFn, csrc/edge_rank.hip): neither the [B,2Fin,N,k] edge tensor nor the activated [B,F1,N,k]
    tensor exists in forward; the backward holds one [B*N,k,F1] buffer.  The sub-modules are parameter containers with the reference's
    names (state_dicts load strictly both ways); conv2 on its own still refuses its [1,k] kernel for k > 1."""

    def __init__(self, Fin, F1, Fout, k):
        super().__init__()
        name = type(self).__name__
        if not 1 <= k <= 32:
            raise ValueError("%s: k must lie in 1..32, got k=%d (Fin=%d, Fout=%d)" % (name, k, Fin, Fout))
        if Fin < 1 or Fout < 1:
            raise ValueError("%s: Fin and Fout must be positive, got Fin=%d, Fout=%d" % (name, Fin, Fout))
        self.k = k
        self.Fin = Fin
        self.Fout = Fout
        self.conv2 = conv2dbr(F1, Fout, [1, k], [1, 1])
        self.inte_conv_hk = nn.Sequential(
            nn.Conv2d(2 * Fin, F1, [1, 1], [1, 1]),
            nn.BatchNorm2d(F1),
            nn.LeakyReLU(inplace=True)
        )
        self.last_idx: Optional[torch.Tensor] = None

    def _run(self, x, idx):
        conv1, bn1, act = self.inte_conv_hk[0], self.inte_conv_hk[1], self.inte_conv_hk[2]
        bn2 = self.conv2.bn
        B, N, idx, knn_mode = check_edge_input(type(self).__name__, x, idx, self.k, self.Fin, self.Fout, (bn1, bn2))
        h = _Holder(B=B, N=N, k=self.k, training=self.training, idx=idx, knn_mode=knn_mode, slope=float(act.negative_slope),
                    bn1=bn1, bn2=bn2, last_idx=None)
        out = edge_conv.RankEdgeConvFn.apply(h, x.contiguous(), conv1.weight, conv1.bias, bn1.weight, bn1.bias,
                                             self.conv2.conv.weight, self.conv2.conv.bias, bn2.weight, bn2.bias)
        self.last_idx = h.last_idx
        return out


class deform_edgeConv_simple(_RankEdgeConv):
    """Generation/modules.py:1432-1466: [B,Fin,N] -> [B,Fout,N], Conv2d(2Fin -> Fout, 1x1) + BatchNorm2d + LeakyReLU over the edge features,
    then conv2dbr(Fout -> Fout, [1,k]) over the k neighbour ranks.  pc is accepted and unused, as in the reference.  idx (an extension, as
    edgeConv's): the graph to use instead of the kNN graph of x, int64 [B, N*k] local indices (range-checked outside a capture) or int32
    [B*N,k] global rows (trusted).  1 <= k <= 32.  Once differentiable.  last_idx: the graph of the latest forward."""

    def __init__(self, Fin, Fout, k):
        super().__init__(Fin, Fout, Fout, k)

    def forward(self, x, pc=None, idx: Optional[torch.Tensor] = None):
        return self._run(x, idx)


class deform_edgeConv_first(_RankEdgeConv):
    """Generation/modules.py:1394-1428: Conv2d(2Fin -> Fin, 1x1) + BatchNorm2d + LeakyReLU over the edge features, then
    conv2dbr(Fin -> Fout, [1,k]) over the k neighbour ranks.  The result has the reference's literal shape [B,Fout,N,1,1]: the reference
    applies `unsqueeze(3)` to its [B,Fout,N,1] tensor where deform_edgeConv_simple squeezes; this is the reference's behaviour, kept so
    that swapped imports see the same shapes, and `.view(B, Fout, N)` of the result is free.  idx, k and last_idx as deform_edgeConv_simple."""

    def __init__(self, Fin, Fout, k):
        super().__init__(Fin, Fin, Fout, k)

    def forward(self, x, idx: Optional[torch.Tensor] = None):
        out = self._run(x, idx)
        return out.view(out.shape[0], out.shape[1], out.shape[2], 1, 1)


class deform_edgeConv_feat(nn.Module):
    """Generation/modules.py:1543-1599: [B,Fin,N] -> [B,Fout,N], conv2dbr(Fin -> Fout, [1,k]) over inte_conv_hk(e) * w with e =
    get_edge_features(x), inte_conv_hk = Conv2d(2Fin -> Fin, 1x1) + BatchNorm2d + LeakyReLU and w = conv_fea(e), a shared MLP
    2Fin -> 16 -> 64 -> Fin (each Conv2d 1x1 + BatchNorm2d + LeakyReLU), normalised by a softmax over the k neighbours (softmax=True).
    Evaluated by edge_conv.WeightedRankEdgeConvFn (csrc/edge_rank.hip): e, the activated tensor, the weight and their product never exist in
    memory; the forward keeps one [B*N,k,Fin] tensor, the backward two more.  The sub-modules are parameter containers in the reference's
    order and names (state_dicts load strictly both ways).  idx (an extension, as edgeConv's): the graph to use instead of the kNN graph
    of x, int64 [B, N*k] local indices (range-checked outside a capture) or int32 [B*N,k] global rows (trusted).  1 <= k <= 32.  Once
    differentiable.  last_idx: the graph of the latest forward."""

    def __init__(self, Fin, Fout, k, softmax=True):
        super().__init__()
        if not 1 <= k <= 32:
            raise ValueError("deform_edgeConv_feat: k must lie in 1..32, got k=%d (Fin=%d, Fout=%d)" % (k, Fin, Fout))
        if Fin < 1 or Fout < 1:
            raise ValueError("deform_edgeConv_feat: Fin and Fout must be positive, got Fin=%d, Fout=%d" % (Fin, Fout))
        self.k = k
        self.Fin = Fin
        self.Fout = Fout
        self.softmax = softmax
        self.conv2 = conv2dbr(Fin, Fout, [1, k], [1, 1])
        self.conv_fea = nn.Sequential(
            nn.Conv2d(2 * Fin, 16, 1),
            nn.BatchNorm2d(16),
            nn.LeakyReLU(inplace=True),
            nn.Conv2d(16, 64, 1),
            nn.BatchNorm2d(64),
            nn.LeakyReLU(inplace=True),
            nn.Conv2d(64, Fin, 1),
            nn.BatchNorm2d(Fin),
            nn.LeakyReLU(inplace=True)
        )
        self.inte_conv_hk = nn.Sequential(
            nn.Conv2d(2 * Fin, Fin, [1, 1], [1, 1]),
            nn.BatchNorm2d(Fin),
            nn.LeakyReLU(inplace=True)
        )
        self.last_idx: Optional[torch.Tensor] = None

    def forward(self, x, idx: Optional[torch.Tensor] = None):
        name = "deform_edgeConv_feat"
        layers = [(self.inte_conv_hk[0], self.inte_conv_hk[1])] + [(self.conv_fea[i], self.conv_fea[i + 1]) for i in (0, 3, 6)] + \
            [(self.conv2.conv, self.conv2.bn)]
        slopes = {float(a.negative_slope) for a in (self.inte_conv_hk[2], self.conv_fea[2], self.conv_fea[5], self.conv_fea[8])}
        B, N, idx, knn_mode = check_edge_input(name, x, idx, self.k, self.Fin, self.Fout, [bn for _, bn in layers],
                                               None if len(slopes) == 1 else "the four LeakyReLUs must share one slope, got %s" % sorted(slopes))
        h = _Holder(B=B, N=N, k=self.k, training=self.training, softmax=bool(self.softmax), idx=idx, knn_mode=knn_mode,
                    slope=slopes.pop(), bns=tuple(bn for _, bn in layers), last_idx=None)
        params = [t for conv, bn in layers for t in (conv.weight, conv.bias, bn.weight, bn.bias)]
        out = edge_conv.WeightedRankEdgeConvFn.apply(h, x.contiguous(), *params)
        self.last_idx = h.last_idx
        return out


class deform_edgeConv(nn.Module):
    """Generation/modules.py:1468-1540: [B,Fin,N] x [B,3,N] -> [B,Fout,N], the coordinate-guided full-rank edge convolution:
    conv2(inte_conv_hk(e) * w) with (e, y) = get_edge_features_xyz(x, pc), w = conv_all(conv_fea(e) * conv_xyz(y)) -- conv_fea 2Fin -> 16,
    conv_xyz 6 -> 16, conv_all 16 -> 64 -> Fin, each Conv2d 1x1 + BatchNorm2d + LeakyReLU -- normalised by a softmax over the k neighbours
    (softmax=True), and conv2 = Conv2d(Fin -> Fout, [1,k]) + BatchNorm2d + LeakyReLU.  Evaluated by edge_conv.CoordRankEdgeConvFn
    (csrc/edge_rank.hip): neither edge tensor, the two 16-channel branches, the activated tensor, the weight nor their product exist in
    memory; the forward keeps one [B*N,k,Fin] tensor, the backward two more.
    As in the reference, conv2 is a plain nn.Sequential (keys conv2.0 / conv2.1) whose BatchNorm2d has Fin channels over the Fout channels
    of its convolution: the constructor accepts any pair, so that reference state_dicts load strictly both ways, and the layer runs only
    with Fin == Fout (forward raises ValueError otherwise, where the reference raises from batch_norm).
    idx (an extension, as edgeConv's): the graph to use instead of the kNN graph of x, int64 [B, N*k] local indices (range-checked outside
    a capture) or int32 [B*N,k] global rows (trusted).  1 <= k <= 32.  Once differentiable in x, pc and the parameters.  last_idx: the
    graph of the latest forward."""

    def __init__(self, Fin, Fout, k, softmax=True):
        super().__init__()
        if not 1 <= k <= 32:
            raise ValueError("deform_edgeConv: k must lie in 1..32, got k=%d (Fin=%d, Fout=%d)" % (k, Fin, Fout))
        if Fin < 1 or Fout < 1:
            raise ValueError("deform_edgeConv: Fin and Fout must be positive, got Fin=%d, Fout=%d" % (Fin, Fout))
        self.k = k
        self.Fin = Fin
        self.Fout = Fout
        self.softmax = softmax
        self.conv2 = nn.Sequential(
            nn.Conv2d(Fin, Fout, [1, k], [1, 1]),
            nn.BatchNorm2d(Fin),
            nn.LeakyReLU(inplace=True)
        )
        self.conv_xyz = nn.Sequential(
            nn.Conv2d(6, 16, 1),
            nn.BatchNorm2d(16),
            nn.LeakyReLU(inplace=True)
        )
        self.conv_fea = nn.Sequential(
            nn.Conv2d(2 * Fin, 16, 1),
            nn.BatchNorm2d(16),
            nn.LeakyReLU(inplace=True)
        )
        self.conv_all = nn.Sequential(
            nn.Conv2d(16, 64, 1),
            nn.BatchNorm2d(64),
            nn.LeakyReLU(inplace=True),
            nn.Conv2d(64, Fin, 1),
            nn.BatchNorm2d(Fin),
            nn.LeakyReLU(inplace=True)
        )
        self.inte_conv_hk = nn.Sequential(
            nn.Conv2d(2 * Fin, Fin, [1, 1], [1, 1]),
            nn.BatchNorm2d(Fin),
            nn.LeakyReLU(inplace=True)
        )
        self.last_idx: Optional[torch.Tensor] = None

    def forward(self, x, pc, idx: Optional[torch.Tensor] = None):
        name = "deform_edgeConv"
        if self.Fin != self.Fout:
            raise ValueError("%s: conv2's BatchNorm2d has Fin=%d channels over the Fout=%d channels of its convolution: the layer runs only "
                             "with Fin == Fout" % (name, self.Fin, self.Fout))
        layers = [(self.inte_conv_hk[0], self.inte_conv_hk[1]), (self.conv_fea[0], self.conv_fea[1]), (self.conv_xyz[0], self.conv_xyz[1]),
                  (self.conv_all[0], self.conv_all[1]), (self.conv_all[3], self.conv_all[4]), (self.conv2[0], self.conv2[1])]
        slopes = {float(a.negative_slope) for a in (self.inte_conv_hk[2], self.conv_fea[2], self.conv_xyz[2], self.conv_all[2], self.conv_all[5],
                                                    self.conv2[2])}
        B, N, idx, knn_mode = check_edge_input(name, x, idx, self.k, self.Fin, self.Fout, [bn for _, bn in layers],
                                               None if len(slopes) == 1 else "the six LeakyReLUs must share one slope, got %s" % sorted(slopes))
        _require_gpu(pc, name + " pc")
        if pc.dim() != 3 or pc.shape[0] != B or pc.shape[1] != 3 or pc.shape[2] != N:
            raise ValueError("%s: pc must be [B,3,N] for x [B,C,N], got %s and %s" % (name, tuple(pc.shape), tuple(x.shape)))
        h = _Holder(B=B, N=N, k=self.k, training=self.training, softmax=bool(self.softmax), idx=idx, knn_mode=knn_mode,
                    slope=slopes.pop(), bns=tuple(bn for _, bn in layers), last_idx=None)
        params = [t for conv, bn in layers for t in (conv.weight, conv.bias, bn.weight, bn.bias)]
        out = edge_conv.CoordRankEdgeConvFn.apply(h, x.contiguous(), pc.contiguous(), *params)
        self.last_idx = h.last_idx
        return out


class bilateral_upsample_edgeConv(nn.Module):
    """Generation/modules.py:847-925: [B,Fin,N] x [B,3,N] -> [B,Fout,2N], the point-doubling edge convolution with a coordinate-guided
    weight: conv2(cat(e, reshuffled inte_conv_hk(e) * w)) with (e, y) = get_edge_features_xyz(x, pc), inte_conv_hk = Conv2d(2Fin -> 4Fin,
    [1, k/2+1]) + BatchNorm2d + LeakyReLU as in upsample_edgeConv, w = conv_all(conv_fea(e) * conv_xyz(y)) -- conv_fea 2Fin -> 16, conv_xyz
    6 -> 16, conv_all 16 -> 64 -> 2Fin, each Conv2d 1x1 + BatchNorm2d + LeakyReLU -- normalised by a softmax over the k neighbours
    (softmax=True), and conv2 = conv2dbr(2Fin -> 2Fout, [1,2k]).  Evaluated by edge_conv.BilateralUpsampleEdgeConvFn (csrc/edge_window.hip,
    csrc/edge_rank.hip): neither edge tensor, the activated interpolation, the weight, their product nor the merged [B,2Fin,N,2k] tensor
    exist in forward or backward; the forward keeps two [B*N,k,2Fin] tensors.  The sub-modules are parameter containers in the reference's
    order and names (state_dicts load strictly both ways); num is kept and unused, as in the reference.
    idx (an extension, as edgeConv's): the graph to use instead of the kNN graph of x, int64 [B, N*k] local indices (range-checked outside
    a capture) or int32 [B*N,k] global rows (trusted).  k even, 2 <= k <= 28.  Once differentiable in x, pc and the parameters.  last_idx:
    the graph of the latest forward."""

    def __init__(self, Fin, Fout, k, num, softmax=True):
        super().__init__()
        if k % 2 or not 2 <= k <= 28:
            raise ValueError("bilateral_upsample_edgeConv: k must be even and lie in 2..28 (the reference's view of the [.., k/2] tensor as "
                             "[.., k] fails for an odd k), got k=%d (Fin=%d, Fout=%d)" % (k, Fin, Fout))
        if Fin < 1 or Fout < 1:
            raise ValueError("bilateral_upsample_edgeConv: Fin and Fout must be positive, got Fin=%d, Fout=%d" % (Fin, Fout))
        self.k = k
        self.Fin = Fin
        self.Fout = Fout
        self.softmax = softmax
        self.num = num
        self.conv2 = conv2dbr(2 * Fin, 2 * Fout, [1, 2 * k], [1, 1])
        self.conv_xyz = nn.Sequential(
            nn.Conv2d(6, 16, 1),
            nn.BatchNorm2d(16),
            nn.LeakyReLU(inplace=True)
        )
        self.conv_fea = nn.Sequential(
            nn.Conv2d(2 * Fin, 16, 1),
            nn.BatchNorm2d(16),
            nn.LeakyReLU(inplace=True)
        )
        self.conv_all = nn.Sequential(
            nn.Conv2d(16, 64, 1),
            nn.BatchNorm2d(64),
            nn.LeakyReLU(inplace=True),
            nn.Conv2d(64, 2 * Fin, 1),
            nn.BatchNorm2d(2 * Fin),
            nn.LeakyReLU(inplace=True)
        )
        self.inte_conv_hk = nn.Sequential(
            nn.Conv2d(2 * Fin, 4 * Fin, [1, k // 2 + 1], [1, 1]),
            nn.BatchNorm2d(4 * Fin),
            nn.LeakyReLU(inplace=True)
        )
        self.last_idx: Optional[torch.Tensor] = None

    def forward(self, x, pc, idx: Optional[torch.Tensor] = None):
        name = "bilateral_upsample_edgeConv"
        layers = [(self.inte_conv_hk[0], self.inte_conv_hk[1]), (self.conv_fea[0], self.conv_fea[1]), (self.conv_xyz[0], self.conv_xyz[1]),
                  (self.conv_all[0], self.conv_all[1]), (self.conv_all[3], self.conv_all[4]), (self.conv2.conv, self.conv2.bn)]
        slopes = {float(a.negative_slope) for a in (self.inte_conv_hk[2], self.conv_fea[2], self.conv_xyz[2], self.conv_all[2], self.conv_all[5])}
        B, N, idx, knn_mode = check_edge_input(name, x, idx, self.k, self.Fin, self.Fout, [bn for _, bn in layers],
                                               None if len(slopes) == 1 else "the five LeakyReLUs must share one slope, got %s" % sorted(slopes))
        _require_gpu(pc, name + " pc")
        if pc.dim() != 3 or pc.shape[0] != B or pc.shape[1] != 3 or pc.shape[2] != N:
            raise ValueError("%s: pc must be [B,3,N] for x [B,C,N], got %s and %s" % (name, tuple(pc.shape), tuple(x.shape)))
        h = _Holder(B=B, N=N, k=self.k, training=self.training, softmax=bool(self.softmax), idx=idx, knn_mode=knn_mode,
                    slope=slopes.pop(), bns=tuple(bn for _, bn in layers), last_idx=None)
        params = [t for conv, bn in layers for t in (conv.weight, conv.bias, bn.weight, bn.bias)]
        out = edge_conv.BilateralUpsampleEdgeConvFn.apply(h, x.contiguous(), pc.contiguous(), *params)
        self.last_idx = h.last_idx
        return out


# ----------------------------------------------------------------------------- the blocks of Generation/modules.py:928-1391
def _fc(Fin, Fout):
    return nn.Sequential(nn.Linear(Fin, Fin), nn.BatchNorm1d(Fin), nn.LeakyReLU(inplace=True),
                         nn.Linear(Fin, Fout), nn.BatchNorm1d(Fout), nn.LeakyReLU(inplace=True))


def _g_fc(Fout):
    return nn.Sequential(nn.Linear(Fout, 512), nn.BatchNorm1d(512), nn.LeakyReLU(inplace=True))


def _add_cov(Fout):
    return nn.Sequential(nn.Conv1d(2 * Fout, Fout, 1), nn.BatchNorm1d(Fout), nn.LeakyReLU(inplace=True))


class _Block(nn.Module):
    """The shared body of the bilateral / deform blocks: an edge convolution, BatchNorm1d + LeakyReLU over its output, a global branch
    (max over the points -> fc [-> g_fc], on B rows: the existing GEMM / BatchNorm launchers through pointnet_util._SharedMLPFn) and the
    concatenation of the broadcast global vectors with the per-point features -- in the middle blocks followed by add_cov, a Conv1d + BatchNorm1d +
    LeakyReLU over that concatenation.  Everything behind the layer is edge_conv.BlockTailFn (csrc/block_tail.hip): no repeated vector, no
    activated copy of the layer's output and, in the middle blocks, no concatenated [B,2Fout,N] tensor exists in forward or backward.
    The sub-modules are parameter containers with the reference's names and order: reference state_dicts load strictly both ways.
    idx (an extension, as on the layers): the graph for the block's edge convolution.  last_idx: the graph of the latest forward.
    Train mode needs B > 1 (BatchNorm1d over the B rows of the global branch), as in the reference.  Once differentiable."""
    _pc = False              # forward(x, pc)
    _two = False             # returns (x_out, g_out)

    def _parts(self):
        """-> (layer, bn, act) of the block"""
        seq = self.upsample_cov if hasattr(self, "upsample_cov") else self.deform_cov
        if isinstance(seq, nn.Sequential):
            return seq[0], seq[1], seq[2]
        return seq, self.bn_uc, self.relu_uc

    @property
    def last_idx(self) -> Optional[torch.Tensor]:
        return self._parts()[0].last_idx

    def _run(self, x, pc, idx):
        name = type(self).__name__
        layer, bn, act = self._parts()
        if x.dim() != 3:
            raise ValueError("%s: x must be [B,Fin,N], got %s" % (name, tuple(x.shape)))
        B, _, N = x.shape
        pool = getattr(self, "maxpool", None)
        if pool is not None:
            mp = pool.kernel_size[1]
            if mp != N:
                raise ValueError("%s: maxpool=%d must equal the number of points N=%d (the pooled [B,Fin,N-maxpool+1] tensor is viewed as the "
                                 "[B,Fin] input of fc)" % (name, mp, N))
        if self.training and B == 1:
            raise ValueError("%s: train mode needs more than one shape per batch (BatchNorm1d over the B rows of the global branch), got B=1" % name)
        g_fc, add_cov = getattr(self, "g_fc", None), getattr(self, "add_cov", None)
        acts = [act, self.fc[2], self.fc[5]] + ([g_fc[2]] if g_fc is not None else []) + ([add_cov[2]] if add_cov is not None else [])
        slopes = {float(a.negative_slope) for a in acts}
        if len(slopes) != 1:
            raise NotImplementedError("%s: the block's LeakyReLUs must share one slope, got %s" % (name, sorted(slopes)))
        slope = slopes.pop()
        gemm_bns = [self.fc[1], self.fc[4]] + ([g_fc[1]] if g_fc is not None else []) + ([add_cov[1]] if add_cov is not None else [])
        for b_ in gemm_bns + [bn]:
            if b_.momentum is None or not b_.track_running_stats:
                raise NotImplementedError("%s: BatchNorm1d with momentum=None or track_running_stats=False is not supported" % name)
        for b_ in gemm_bns:          # their statistics are finalised in the epilogue of the producing GEMM, with the library's constants
            if float(b_.eps) != ops.BN_EPS or float(b_.momentum) != ops.BN_MOMENTUM:
                raise NotImplementedError("%s: the BatchNorm1d of fc / g_fc / add_cov must keep eps=%g and momentum=%g" % (name, ops.BN_EPS, ops.BN_MOMENTUM))
        # The global branch runs in front of the layer, as in the reference.  Autograd runs the nodes of a graph latest first, so the
        # branch's backward then runs after the layer's, where the block's memory peaks: the dense [B,Fin,N] cotangent of the max and the
        # gradients of fc / g_fc do not exist yet while the layer's backward holds its tensors, only the branch's saved [B,*] rows do
        # (without g, which nothing but the tail's forward reads: keep_out=False).
        # x is looked at here only as far as the branch's launchers need; the layer checks x (and pc, idx) and refuses a CPU tensor, and
        # what it refuses on its own (Fin != Fout) comes first, as on the layer.
        xs = g = None
        if x.is_cuda and x.dtype == torch.float32 and x.shape[1] == layer.Fin:          # otherwise the layer refuses x below
            from . import pointnet_util
            mlp = pointnet_util._SharedMLPFn.apply
            xs = mlp(pointnet_util._Holder(K=1, training=self.training, bns=[self.fc[1], self.fc[4]], slope=slope), edge_conv.PointMaxFn.apply(x.contiguous()),
                     self.fc[0].weight, self.fc[0].bias, self.fc[1].weight, self.fc[1].bias, self.fc[3].weight, self.fc[3].bias, self.fc[4].weight, self.fc[4].bias)
            if g_fc is not None:
                g = mlp(pointnet_util._Holder(K=1, training=self.training, bns=[g_fc[1]], slope=slope, keep_out=False), xs, g_fc[0].weight, g_fc[0].bias, g_fc[1].weight, g_fc[1].bias)
        y = layer(x, pc, idx=idx) if self._pc else layer(x, idx=idx)
        h = _Holder(name=name, training=self.training, slope=slope, bn=bn, bn_add=None if add_cov is None else add_cov[1])
        ac = (None, None, None, None) if add_cov is None else (add_cov[0].weight, add_cov[0].bias, add_cov[1].weight, add_cov[1].bias)
        x_out, g_out = edge_conv.BlockTailFn.apply(h, y.contiguous(), xs, g, bn.weight, bn.bias, *ac)
        return (x_out, g_out) if self._two else x_out


class bilateral_block_l1(_Block):
    """Generation/modules.py:928-973: forward(x [B,Fin,N], idx=None) -> (x_out [B,2Fout,2N], g_out [B,512+Fout,2N]) around
    upsample_edgeConv(Fin, Fout, num_k // 2).  maxpool must equal N (ValueError otherwise; the reference fails inside fc's Linear).  See _Block."""
    _two = True

    def __init__(self, Fin, Fout, maxpool, stride=1, num_k=20):
        super().__init__()
        self.maxpool = nn.MaxPool2d((1, maxpool), (1, 1))
        self.upsample_cov = nn.Sequential(upsample_edgeConv(Fin, Fout, num_k // 2, 1), nn.BatchNorm1d(Fout), nn.LeakyReLU(inplace=True))
        self.fc = _fc(Fin, Fout)
        self.g_fc = _g_fc(Fout)

    def forward(self, x, idx: Optional[torch.Tensor] = None):
        return self._run(x, None, idx)


class bilateral_block_l2(_Block):
    """Generation/modules.py:976-1020: forward(x [B,Fin,N], pc [B,3,N], idx=None) -> (x_out [B,2Fout,2N], g_out [B,512+Fout,2N]) around
    bilateral_upsample_edgeConv(Fin, Fout, num_k // 2).  maxpool must equal N (ValueError otherwise).  See _Block."""
    _pc = True
    _two = True

    def __init__(self, Fin, Fout, maxpool, stride=1, num_k=20, softmax=True):
        super().__init__()
        self.maxpool = nn.MaxPool2d((1, maxpool), (1, 1))
        self.upsample_cov = bilateral_upsample_edgeConv(Fin, Fout, num_k // 2, 1, softmax=softmax)
        self.bn_uc = nn.BatchNorm1d(Fout)
        self.relu_uc = nn.LeakyReLU(inplace=True)
        self.fc = _fc(Fin, Fout)
        if self._two:
            self.g_fc = _g_fc(Fout)

    def forward(self, x, pc, idx: Optional[torch.Tensor] = None):
        return self._run(x, pc, idx)


class bilateral_block_l3(bilateral_block_l2):
    """Generation/modules.py:1023-1069: as bilateral_block_l2."""


class bilateral_block_l4(bilateral_block_l2):
    """Generation/modules.py:1072-1106: bilateral_block_l2 without g_fc: forward(x, pc, idx=None) -> x_out [B,2Fout,2N]."""
    _two = False


class bilateral_block(_Block):
    """Generation/modules.py:1109-1144: forward(x [B,Fin,N], idx=None) -> x_out [B,2Fout,2N] around upsample_edgeConv(Fin, Fout, num_k // 2).
    maxpool is accepted and unused, as in the reference (the pooling is torch.max).  See _Block."""

    def __init__(self, Fin, Fout, maxpool, stride=1, num_k=20):
        super().__init__()
        self.upsample_cov = nn.Sequential(upsample_edgeConv(Fin, Fout, num_k // 2, 1), nn.BatchNorm1d(Fout), nn.LeakyReLU(inplace=True))
        self.fc = _fc(Fin, Fout)

    def forward(self, x, idx: Optional[torch.Tensor] = None):
        return self._run(x, None, idx)


class deform_block_middle(_Block):
    """Generation/modules.py:1195-1253: forward(x [B,Fin,N], pc [B,3,N], idx=None) -> (x_out [B,Fout,N], g_out [B,512+Fout,N]) around
    deform_edgeConv(Fin, Fout, num_k), with add_cov over cat[xs, x_ec].  The constructor accepts any (Fin, Fout) so that state_dicts load;
    the forward raises ValueError unless Fin == Fout, as the layer does.  softmax is accepted and unused, as in the reference.  See _Block."""
    _pc = True
    _two = True

    def __init__(self, Fin, Fout, stride=1, num_k=20, softmax=True):
        super().__init__()
        self.deform_cov = deform_edgeConv(Fin, Fout, num_k)
        self.add_cov = _add_cov(Fout)
        self.bn_uc = nn.BatchNorm1d(Fout)
        self.relu_uc = nn.LeakyReLU(inplace=True)
        self.fc = _fc(Fin, Fout)
        self.g_fc = _g_fc(Fout)

    def forward(self, x, pc, idx: Optional[torch.Tensor] = None):
        return self._run(x, pc, idx)


class deform_block_tail(_Block):
    """Generation/modules.py:1256-1290: forward(x [B,Fin,N], pc [B,3,N], idx=None) -> x_out [B,2Fout,N] around deform_edgeConv(Fin, Fout, num_k);
    runs only with Fin == Fout (ValueError otherwise), as the layer.  softmax is accepted and unused, as in the reference.  See _Block."""
    _pc = True

    def __init__(self, Fin, Fout, stride=1, num_k=20, softmax=True):
        super().__init__()
        self.deform_cov = deform_edgeConv(Fin, Fout, num_k)
        self.bn_uc = nn.BatchNorm1d(Fout)
        self.relu_uc = nn.LeakyReLU(inplace=True)
        self.fc = _fc(Fin, Fout)

    def forward(self, x, pc, idx: Optional[torch.Tensor] = None):
        return self._run(x, pc, idx)


class deform_block_feat_middle(_Block):
    """Generation/modules.py:1293-1337: forward(x [B,Fin,N], idx=None) -> x_out [B,Fout,N] around deform_edgeConv_feat(Fin, Fout, num_k,
    softmax), with add_cov over cat[xs, x_ec].  See _Block."""

    def __init__(self, Fin, Fout, stride=1, num_k=20, softmax=True):
        super().__init__()
        self.deform_cov = deform_edgeConv_feat(Fin, Fout, num_k, softmax=softmax)
        self.add_cov = _add_cov(Fout)
        self.bn_uc = nn.BatchNorm1d(Fout)
        self.relu_uc = nn.LeakyReLU(inplace=True)
        self.fc = _fc(Fin, Fout)
        if self._two:
            self.g_fc = _g_fc(Fout)

    def forward(self, x, idx: Optional[torch.Tensor] = None):
        return self._run(x, None, idx)


class deform_block_feat(deform_block_feat_middle):
    """Generation/modules.py:1339-1391: deform_block_feat_middle with g_fc: forward(x, idx=None) -> (x_out [B,Fout,N], g_out [B,512+Fout,N])."""
    _two = True


class PointTransformerLayer(nn.Module):
    """Generation/modules.py:1602-1644: forward(x [b,n,dim], pos [b,n,3]) -> [b,n,dim], point-major.  Pairwise vector attention:
    a = softmax_j(attn_mlp(q_i - k_j + pos_mlp(pos_i - pos_j))), out_i = sum_j a_ij (v_j + pos_mlp(pos_i - pos_j)), computed by
    pair_attn.PairAttnFn without any per-pair vector in memory, so that n is bounded by time and not by [b,n,n,dim] tensors.
    Sub-modules carry the reference's names in its order (to_qkv, pos_mlp.0/2, attn_mlp.0/2): state_dicts load strictly both ways.
    Domain (ValueError otherwise): dim <= 512, pos_mlp_hidden_dim <= 64, dim * attn_mlp_hidden_mult <= 4096.  Differentiable once in
    x, pos and every parameter (attn_mlp.2.bias cancels in the softmax: its gradient is exactly zero)."""

    def __init__(self, dim, pos_mlp_hidden_dim=64, attn_mlp_hidden_mult=4):
        super().__init__()
        from . import pair_attn
        pair_attn.padded_sizes(int(dim), int(pos_mlp_hidden_dim), int(attn_mlp_hidden_mult))
        self.dim = int(dim)
        self.to_qkv = nn.Linear(dim, dim * 3, bias=False)
        self.pos_mlp = nn.Sequential(nn.Linear(3, pos_mlp_hidden_dim), nn.ReLU(), nn.Linear(pos_mlp_hidden_dim, dim))
        self.attn_mlp = nn.Sequential(nn.Linear(dim, dim * attn_mlp_hidden_mult), nn.ReLU(), nn.Linear(dim * attn_mlp_hidden_mult, 1))

    def forward(self, x, pos):
        from . import pair_attn
        _require_gpu(x, "PointTransformerLayer")
        _require_gpu(pos, "PointTransformerLayer")
        if x.dim() != 3 or x.shape[2] != self.dim or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError("PointTransformerLayer(dim=%d): x must be [b,n,%d], got %s" % (self.dim, self.dim, tuple(x.shape)))
        if tuple(pos.shape) != (x.shape[0], x.shape[1], 3):
            raise ValueError("PointTransformerLayer: pos must be [b,n,3] = %s for x %s, got %s"
                             % ((x.shape[0], x.shape[1], 3), tuple(x.shape), tuple(pos.shape)))
        if x.dtype != torch.float32 or pos.dtype != torch.float32:
            raise TypeError("PointTransformerLayer: x and pos must be float32, got %s and %s" % (x.dtype, pos.dtype))
        p0, p2, a0, a2 = self.pos_mlp[0], self.pos_mlp[2], self.attn_mlp[0], self.attn_mlp[2]
        return pair_attn.point_transformer(x, pos, self.to_qkv.weight, p0.weight, p0.bias, p2.weight, p2.bias, a0.weight, a0.bias,
                                           a2.weight, a2.bias)


# ----------------------------------------------------------------------------- the dense family of Common/utilities.py
DENSE_K_MIN, DENSE_K_MAX = 2, 32       # the point itself + ops.knn(k - 1); spgan_knn selects at most 32


def _dense_k(name: str, k) -> int:
    if not isinstance(k, int) or not DENSE_K_MIN <= k <= DENSE_K_MAX:
        raise ValueError("%s: k must be an integer in %d..%d (the point itself plus at most %d neighbours of the kNN kernel), got %r"
                         % (name, DENSE_K_MIN, DENSE_K_MAX, DENSE_K_MAX - 1, k))
    return k


def get_graph_feature(x, k=20, idx=None):
    """Common/ops.py:138-162: x [B,C,N] -> [B,2C,N,k] = cat[x_j - x_i, x_i] (the difference FIRST: the other way round from
    get_edge_features) over the reference's own graph, the topk of the negative squared distance, in which every point is its own first
    neighbour: rank 0 is the point itself, ranks 1..k-1 its nearest neighbours by ascending distance (ops.knn with k - 1).  idx: int64
    local indices [B,N,k] (or [B,N*k]) as the reference's knn returns them, used instead.  k in 2..32.  The materialising function, for
    parity; DenseEdgeModule never forms this tensor.  Differentiable in x through get_edge_features' backward."""
    _require_gpu(x, "get_graph_feature")
    k = _dense_k("get_graph_feature", k)
    B, C, N = x.shape
    x = x.contiguous()
    if idx is None:
        with torch.no_grad():
            gidx = edge_conv.dense_graph(ops.cm_to_pm(x.detach()), B, N, k, 1 if C <= 4 else 0)
            idx = ops.idx_to_local64(gidx, B, N)
    else:
        _require_gpu(idx, "get_graph_feature idx")
        if idx.dtype != torch.int64 or idx.numel() != B * N * k:
            raise ValueError("get_graph_feature: idx must be int64 with B*N*k = %d local indices, got %s %s" % (B * N * k, idx.dtype, tuple(idx.shape)))
        if not ops.capturing() and (int(idx.min()) < 0 or int(idx.max()) >= N):
            raise IndexError("get_graph_feature: a neighbour index lies outside [0, %d)" % N)
    ee = get_edge_features(x, k, idx=idx.reshape(B, N * k))                   # cat[x_i, x_j - x_i]
    return torch.cat([ee[:, C:], ee[:, :C]], dim=1)


class DenseEdgeModule(nn.Module):
    """Common/utilities.py:123-144: the densely connected EdgeConv, forward(x [B,C,N], idx=None) -> [B,growth_rate,N] = the max over the k
    neighbours of the last of `levels` Conv2d 1x1 + BatchNorm2d + LeakyReLU(0.2) layers, each fed the concatenation of the edge
    features cat[x_j - x_i, x_i] and every earlier level's output.  input_channel is the edge-feature width: 2*C.  Evaluated by
    edge_conv.DenseEdgeFn: neither the [B,2C,N,k] edge tensor, nor a concatenation, nor an activated per-edge tensor exists in forward or
    backward (per-edge storage: the pre-norm buffer [E, levels*growth_rate], in backward a gradient buffer of that size and one [E,
    growth_rate] buffer).  Sub-modules carry the reference's names (dense_modules.{l}.{0,1,2}): state_dicts load strictly both ways.
    The graph is the reference's (get_graph_feature: the point itself is a neighbour); k in 2..32.  idx (an extension): the graph to use
    instead, int64 local indices [B,N,k] or [B,N*k] as the reference's knn returns them (range-checked), or int32 [B*N,k] global rows
    (trusted).  last_idx: the graph of the latest forward.  Train and eval mode; once differentiable; exact fp32 products."""

    def __init__(self, input_channel=64, levels=4, growth_rate=64, k=20):
        super().__init__()
        self.k = _dense_k("DenseEdgeModule", k)
        if levels < 1 or growth_rate < 1 or input_channel < 2 or input_channel % 2:
            raise ValueError("DenseEdgeModule: levels >= 1, growth_rate >= 1 and an even input_channel = 2*C are required, got (%r, %r, %r)"
                             % (input_channel, levels, growth_rate))
        self.input_channel = input_channel
        self.dense_modules = nn.ModuleList()
        c = input_channel
        for _ in range(levels):
            self.dense_modules.append(nn.Sequential(nn.Conv2d(c, growth_rate, kernel_size=1, bias=True), nn.BatchNorm2d(growth_rate),
                                                    nn.LeakyReLU(negative_slope=0.2)))
            c += growth_rate
        self.last_idx: Optional[torch.Tensor] = None

    def forward(self, x, idx: Optional[torch.Tensor] = None):
        _require_gpu(x, "DenseEdgeModule")
        if x.dim() != 3 or 2 * x.shape[1] != self.input_channel:
            raise ValueError("DenseEdgeModule(input_channel=%d): x must be [B,%d,N] (input_channel = 2*C), got %s"
                             % (self.input_channel, self.input_channel // 2, tuple(x.shape)))
        bns = [m[1] for m in self.dense_modules]
        G = self.dense_modules[0][0].out_channels
        B, N, idx, knn_mode = check_edge_input("DenseEdgeModule", x, idx, self.k, x.shape[1], G, bns)
        if idx is None and N < self.k:
            raise ValueError("DenseEdgeModule: k=%d neighbours (the point itself included) need N >= %d points, got %d" % (self.k, self.k, N))
        h = _Holder(B=B, N=N, k=self.k, training=self.training, idx=idx, knn_mode=knn_mode, bns=bns, last_idx=None)
        params = [p for m in self.dense_modules for p in (m[0].weight, m[0].bias, m[1].weight, m[1].bias)]
        out = edge_conv.DenseEdgeFn.apply(h, x.contiguous(), *params)
        self.last_idx = h.last_idx
        return out


class DenseModule1D(nn.Module):
    """Common/utilities.py:22-42: the per-point analogue, forward(x [B,in_dim,N]) -> [B,in_dim,N] = the last of `levels` Conv1d +
    BatchNorm1d + LeakyReLU(0.2) layers, each fed the concatenation of x and every earlier level's output; the last level is in_dim wide.
    Evaluated by edge_conv.DenseRowsFn without the concatenations.  Sub-modules as in the reference: state_dicts load strictly both ways."""

    def __init__(self, in_dim=64, levels=3, growth_rate=64):
        super().__init__()
        if levels < 1 or growth_rate < 1 or in_dim < 1:
            raise ValueError("DenseModule1D: in_dim, levels and growth_rate must be positive, got (%r, %r, %r)" % (in_dim, levels, growth_rate))
        self.dense_modules = nn.ModuleList()
        self.in_dim = in_dim
        self.input_channel = in_dim
        for i in range(levels):
            if i == levels - 1:
                growth_rate = in_dim
            self.dense_modules.append(nn.Sequential(nn.Conv1d(self.input_channel, growth_rate, kernel_size=1, bias=True), nn.BatchNorm1d(growth_rate),
                                                    nn.LeakyReLU(negative_slope=0.2)))
            self.input_channel = self.input_channel + growth_rate

    def forward(self, x):
        _require_gpu(x, "DenseModule1D")
        if x.dim() != 3 or x.shape[1] != self.in_dim:
            raise ValueError("DenseModule1D(in_dim=%d): x must be [B,%d,N], got %s" % (self.in_dim, self.in_dim, tuple(x.shape)))
        bns = [m[1] for m in self.dense_modules]
        for bn in bns:
            if bn.momentum is None or not bn.track_running_stats:
                raise NotImplementedError("DenseModule1D: BatchNorm1d with momentum=None or track_running_stats=False is not supported")
        h = _Holder(B=x.shape[0], N=x.shape[2], training=self.training, bns=bns)
        params = [p for m in self.dense_modules for p in (m[0].weight, m[0].bias, m[1].weight, m[1].bias)]
        return edge_conv.DenseRowsFn.apply(h, x.contiguous(), *params)


class Dense_Attn(nn.Module):
    """Common/utilities.py:292-321: forward(x [B,in_dim,N], res=True) -> dense(atten(x)) (+ x with res): Self_Attn followed by
    DenseModule1D(in_dim, 3, in_dim).  `activation` is accepted and ignored, as in the reference."""

    def __init__(self, in_dim=128, activation="relu"):
        super().__init__()
        self.atten = Self_Attn(in_dim=in_dim)
        self.dense = DenseModule1D(in_dim=in_dim, levels=3, growth_rate=in_dim)

    def forward(self, x, res=True):
        pt = x
        x = self.dense(self.atten(x))
        return pt + x if res else x


class GC_attn(nn.Module):
    """Common/utilities.py:357-426: global-context attention, forward(x [B,in_dim,...]) -> x * mul + add of the input's shape, with
    ctx = sum_n softmax_n(conv_mask(x))_n x_n (pool='att') or the mean over the positions (a pool string without 'att'), and
    add = channel_add_conv(ctx), mul = channel_mul_conv(ctx) (Conv1d -> LayerNorm -> ReLU -> Conv1d [-> Sigmoid]); the multiplication
    comes first, a fusion that is not listed is skipped, no fusion at all returns x.  The children are parameter containers created in
    the reference's order (state_dicts load strictly both ways, a seed gives the reference's initial values); forward runs spgan.gc_attn:
    two reads of x per direction, cost linear in the number of positions, nothing of x's size saved but x.  1 <= in_dim, out_dim <= 1024.
    A pool string that contains 'att' without being 'att' builds a module the reference cannot run: ValueError here.  Once differentiable."""

    def __init__(self, in_dim, out_dim=None, pool="att", fusions=["channel_add", "channel_mul"]):
        super().__init__()
        from . import gc_attn
        self.in_dim = int(in_dim)
        self.out_dim = int(out_dim) if out_dim is not None else self.in_dim
        if not isinstance(pool, str) or ("att" in pool and pool != "att"):
            raise ValueError("GC_attn: pool must be 'att' or a string without 'att' (average pooling), got %r" % (pool,))
        gc_attn.check_dims(1, self.in_dim, 1, self.out_dim)
        self.pool = pool
        self.fusions = fusions
        if pool == "att":
            self.conv_mask = nn.Conv1d(self.in_dim, 1, kernel_size=1)
            self.softmax = nn.Softmax(dim=2)
        else:
            self.avg_pool = nn.AdaptiveAvgPool1d(1)

        def branch(sigmoid):
            layers = [nn.Conv1d(self.in_dim, self.out_dim, kernel_size=1), nn.LayerNorm([self.out_dim, 1]), nn.ReLU(inplace=True),
                      nn.Conv1d(self.out_dim, self.in_dim, kernel_size=1)]
            return nn.Sequential(*(layers + ([nn.Sigmoid()] if sigmoid else [])))
        self.channel_add_conv = branch(False) if "channel_add" in fusions else None
        self.channel_mul_conv = branch(True) if "channel_mul" in fusions else None

    def _apply_fn(self, x, layout, B, L):
        from . import gc_attn
        add, mul = self.channel_add_conv, self.channel_mul_conv
        params = []
        if self.pool == "att":
            params += [self.conv_mask.weight, self.conv_mask.bias]
        eps = 1e-5
        for br in (add, mul):
            if br is not None:
                if not br[1].elementwise_affine:
                    raise NotImplementedError("GC_attn: a LayerNorm without elementwise_affine is not supported")
                eps = float(br[1].eps)
                params += [br[0].weight, br[0].bias, br[1].weight, br[1].bias, br[3].weight, br[3].bias]
        h = _Holder(layout=layout, B=B, L=L, att=self.pool == "att", has_add=add is not None, has_mul=mul is not None, eps=eps)
        return gc_attn.GCAttnFn.apply(h, x, *params)

    def _check(self, x):
        _require_gpu(x, "GC_attn")
        if x.dtype != torch.float32:
            raise TypeError("GC_attn: x must be float32, got %s" % x.dtype)

    def forward_pm(self, x_pm, B: int, L: int):
        """x_pm [B*L, in_dim] point-major rows (the row stride may exceed in_dim) -> [B*L, in_dim]"""
        self._check(x_pm)
        if x_pm.dim() != 2 or tuple(x_pm.shape) != (B * L, self.in_dim):
            raise ValueError("GC_attn.forward_pm: x must be [%d,%d] rows, got %s" % (B * L, self.in_dim, tuple(x_pm.shape)))
        if self.channel_add_conv is None and self.channel_mul_conv is None:
            return x_pm
        return self._apply_fn(x_pm, "pm", B, L)

    def forward(self, x):
        self._check(x)
        if x.dim() < 3 or x.shape[1] != self.in_dim or x.numel() == 0:
            raise ValueError("GC_attn(in_dim=%d): x must be a non-empty [B,%d,...] tensor with dim >= 3, got %s" % (self.in_dim, self.in_dim, tuple(x.shape)))
        if self.channel_add_conv is None and self.channel_mul_conv is None:
            return x
        size = x.shape
        flat = x.reshape(size[0], size[1], -1)
        return self._apply_fn(flat, "cm", size[0], flat.shape[2]).view(*size)


def _check_f32(t: torch.Tensor, what: str):
    _require_gpu(t, what)
    if t.dtype != torch.float32:
        raise TypeError("%s: inputs must be float32, got %s" % (what, t.dtype))


def _check_bns(what, bns):
    for bn in bns:
        if bn.momentum is None or not bn.track_running_stats:
            raise NotImplementedError("%s: a BatchNorm with momentum=None or track_running_stats=False is not supported" % what)


class DenseModule2D(nn.Module):
    """Common/utilities.py:45-65: forward(x [B,in_dim,H,W]) -> [B,mlps[-1],H,W] = the last of len(mlps) - 1 Conv2d 1x1 + BatchNorm2d +
    LeakyReLU(0.2) layers over the B*H*W positions, level i (mlps[i] wide, i >= 1) fed the concatenation of x and every earlier level's
    output.  levels, growth_rate and mlps[0] are ignored, as in the reference; fewer than two entries of mlps leave the reference without
    a layer (its forward fails): ValueError here.  Evaluated by edge_conv.DenseRowsFn without the concatenations.  Sub-modules as in the
    reference: state_dicts load strictly both ways.  forward_pm(x [B*L, in_dim] rows, B, L) -> [B*L, mlps[-1]] rows."""

    def __init__(self, in_dim=64, levels=3, growth_rate=64, mlps=[]):
        super().__init__()
        if len(mlps) < 2 or in_dim < 1 or any(int(w) < 1 for w in mlps[1:]):
            raise ValueError("DenseModule2D: mlps must list at least two widths (mlps[0] is ignored) and every width must be positive, got in_dim=%r mlps=%r"
                             % (in_dim, mlps))
        self.dense_modules = nn.ModuleList()
        self.in_dim = in_dim
        self.input_channel = in_dim
        for i in range(1, len(mlps)):
            growth_rate = mlps[i]
            self.dense_modules.append(nn.Sequential(nn.Conv2d(self.input_channel, growth_rate, kernel_size=1, bias=True), nn.BatchNorm2d(growth_rate),
                                                    nn.LeakyReLU(negative_slope=0.2)))
            self.input_channel = self.input_channel + growth_rate

    def _run(self, x, B, L, pm):
        bns = [m[1] for m in self.dense_modules]
        _check_bns("DenseModule2D", bns)
        h = _Holder(B=B, N=L, training=self.training, bns=bns, pm=pm, name="DenseModule2D")
        params = [p for m in self.dense_modules for p in (m[0].weight, m[0].bias, m[1].weight, m[1].bias)]
        return edge_conv.DenseRowsFn.apply(h, x, *params)

    def forward_pm(self, x_pm, B: int, L: int):
        _check_f32(x_pm, "DenseModule2D")
        if x_pm.dim() != 2 or tuple(x_pm.shape) != (B * L, self.in_dim):
            raise ValueError("DenseModule2D.forward_pm: x must be [%d,%d] rows, got %s" % (B * L, self.in_dim, tuple(x_pm.shape)))
        return self._run(x_pm, B, L, True)

    def forward(self, x):
        _check_f32(x, "DenseModule2D")
        if x.dim() != 4 or x.shape[1] != self.in_dim:
            raise ValueError("DenseModule2D(in_dim=%d): x must be [B,%d,H,W], got %s" % (self.in_dim, self.in_dim, tuple(x.shape)))
        B, _, H, W = x.shape
        return self._run(x.reshape(B, self.in_dim, H * W).contiguous(), B, H * W, False).view(B, -1, H, W)


class MultiDenseMLP(nn.Module):
    """Common/utilities.py:92-121: forward(x: list, x[i] [B,mlps2[i],H,W]) -> [B,mlps[-1],H,W].  Level i is Conv2d 1x1 (-> mlps[i]) +
    BatchNorm2d + ReLU over pc, and pc = cat[pc, y_i, x[i+1]] feeds the next one.  Evaluated by edge_conv.DenseRowsFn with slope 0 on one
    buffer [x_0 .. x_{n-1} | z_0 ..]: a level's weight image has zero columns for the side inputs it does not see yet
    (edge_conv.dense_side_images).  Gradients reach every x[i] and every parameter.  Sub-modules as in the reference."""

    def __init__(self, mlps, mlps2):
        super().__init__()
        if len(mlps) != len(mlps2) or len(mlps) < 1 or any(int(w) < 1 for w in list(mlps) + list(mlps2)):
            raise ValueError("MultiDenseMLP: mlps and mlps2 must be equally long lists of positive widths, got %r and %r" % (mlps, mlps2))
        self.mlps, self.mlps2 = [int(w) for w in mlps], [int(w) for w in mlps2]
        self.dense_modules = nn.ModuleList()
        c_in = mlps2[0]
        for i in range(len(mlps)):
            c_out = mlps[i]
            self.dense_modules.append(nn.Sequential(nn.Conv2d(c_in, c_out, kernel_size=1, bias=True), nn.BatchNorm2d(c_out), nn.ReLU(inplace=True)))
            if i < len(mlps) - 1:
                c_in = c_in + c_out + mlps2[i + 1]

    def forward(self, x):
        n = len(self.mlps)
        if not isinstance(x, (list, tuple)) or len(x) != n:
            raise ValueError("MultiDenseMLP: x must be a list of %d tensors, got %r" % (n, type(x)))
        for i, t in enumerate(x):
            _check_f32(t, "MultiDenseMLP")
            if t.dim() != 4 or t.shape[1] != self.mlps2[i] or t.shape[0] != x[0].shape[0] or t.shape[2:] != x[0].shape[2:]:
                raise ValueError("MultiDenseMLP: x[%d] must be [B,%d,H,W] like x[0], got %s" % (i, self.mlps2[i], tuple(t.shape)))
        B, _, H, W = x[0].shape
        bns = [m[1] for m in self.dense_modules]
        _check_bns("MultiDenseMLP", bns)
        h = _Holder(B=B, N=H * W, training=self.training, bns=bns, slope=0.0, sides=tuple(self.mlps2), name="MultiDenseMLP")
        params = [p for m in self.dense_modules for p in (m[0].weight, m[0].bias, m[1].weight, m[1].bias)]
        flat = [t.reshape(B, t.shape[1], H * W).contiguous() for t in x]
        return edge_conv.DenseRowsFn.apply(h, *flat, *params).view(B, -1, H, W)


class Dense_Attn_2D(nn.Module):
    """Common/utilities.py:323-353: forward(x [B,in_dim,H,W], res=True) -> atten(dense(x)) [B,mlps[-1],H,W] with dense =
    DenseModule2D(in_dim, mlps=mlps) and atten = GC_attn(mlps[-1]) (atten='gc') or Self_Attn(mlps[-1]) (anything else), created in the
    reference's order (atten first).  res and activation are accepted and ignored, as in the reference.  The chain runs on point-major
    rows over the L = H*W positions (dense.forward_pm, atten.forward_pm): one layout conversion at each end, and with Self_Attn no
    [B,L,L] map."""

    def __init__(self, in_dim=128, activation="relu", mlps=[], atten="gc"):
        super().__init__()
        if len(mlps) < 2:
            raise ValueError("Dense_Attn_2D: mlps must list at least two widths, got %r" % (mlps,))
        self.atten = GC_attn(in_dim=mlps[-1]) if atten == "gc" else Self_Attn(in_dim=mlps[-1])
        self.dense = DenseModule2D(in_dim=in_dim, mlps=mlps)

    def forward(self, x, res=True):
        _check_f32(x, "Dense_Attn_2D")
        if x.dim() != 4 or x.shape[1] != self.dense.in_dim:
            raise ValueError("Dense_Attn_2D: x must be [B,%d,H,W], got %s" % (self.dense.in_dim, tuple(x.shape)))
        B, C, H, W = x.shape
        L = H * W
        y = self.dense.forward_pm(Fn.CmToPm.apply(x.reshape(B, C, L)), B, L)
        y = self.atten.forward_pm(y, B, L)
        return Fn.PmToCm.apply(y, B, L).view(B, -1, H, W)


class Self_Attn2(nn.Module):
    """Common/utilities.py:247-290: Self_Attn whose query / key / value are Sequential(Conv1d, BatchNorm1d, LeakyReLU(0.2)).
    forward(x [B,in_dim,...]) -> gamma * attn + x of x's shape, out[:, :, j] = sum_i softmax_i(query_i . key_j) value_i over the
    flattened positions.  Runs on spgan.point_attn (no [B,N,N] map) with the existing GEMM, BatchNorm and activation launches; train
    and eval mode; in_dim in 8..512 (ValueError otherwise) and B * N * in_dim a multiple of 4.  The state_dict (gamma first, 22
    entries) loads strictly both ways.  `activation` is stored and unused, as in the reference.  Once differentiable."""

    def __init__(self, in_dim: int = 128, activation: str = "relu"):
        super().__init__()
        from . import point_attn
        in_dim = int(in_dim)
        try:
            point_attn.padded_dk(in_dim // 8)
            point_attn.padded_dv(in_dim)
        except ValueError as e:
            raise ValueError("Self_Attn2(in_dim=%d): %s" % (in_dim, e)) from None
        self.chanel_in = in_dim
        self.activation = activation

        def proj(out):
            return nn.Sequential(nn.Conv1d(in_channels=in_dim, out_channels=out, kernel_size=1, bias=True), nn.BatchNorm1d(out),
                                 nn.LeakyReLU(negative_slope=0.2))
        self.query = proj(in_dim // 8)
        self.key = proj(in_dim // 8)
        self.value = proj(in_dim)
        self.gamma = nn.Parameter(torch.zeros(1))

    def forward_pm(self, x_pm, B: int, N: int):
        from . import point_attn
        _check_f32(x_pm, "Self_Attn2")
        if x_pm.dim() != 2 or tuple(x_pm.shape) != (B * N, self.chanel_in):
            raise ValueError("Self_Attn2.forward_pm: x must be [%d,%d] rows, got %s" % (B * N, self.chanel_in, tuple(x_pm.shape)))
        bns = [self.query[1], self.key[1], self.value[1]]
        _check_bns("Self_Attn2", bns)
        params = [p for m in (self.query, self.key, self.value) for p in (m[0].weight, m[0].bias, m[1].weight, m[1].bias)]
        return point_attn.SelfAttn2Fn.apply(_Holder(B=B, N=N, training=self.training, bns=bns), x_pm, *params, self.gamma)

    def forward(self, x):
        _check_f32(x, "Self_Attn2")
        if x.dim() < 3 or x.shape[1] != self.chanel_in:
            raise ValueError("Self_Attn2: x must be [B,%d,...], got %s" % (self.chanel_in, tuple(x.shape)))
        size = x.shape
        flat = x.reshape(size[0], size[1], -1)
        N = flat.shape[2]
        return Fn.PmToCm.apply(self.forward_pm(Fn.CmToPm.apply(flat), size[0], N), size[0], N).view(*size)
