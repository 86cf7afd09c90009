"""The GAN-stabiliser and StyleGAN-style layers of Generation/modules.py:32-390, 437-496 on csrc/gan_layers.hip:

    SpectralNorm, spectral_norm, spectral_norm_network, snconv2d, snlinear, l2normalize
    MinibatchStdDev, StddevLayer
    PixelNorm, PixelwiseNorm, NoiseLayer, NoiseInjection, LayerEpilogue, AdaptiveInstanceNorm, WScaleLayer, Truncation

fp32 only; no float atomics and fixed summation orders, so results repeat bit for bit; no host synchronisation, so every layer runs inside
spgan.CapturedBody.  CPU tensors raise RuntimeError.  Every layer is differentiable once: create_graph=True raises RuntimeError.

Spectral normalisation is evaluated for a GROUP of weights per call (`sn_group`): 4 launches per power iteration + 1, whatever the number of
weights (at most SN_MAX = 32 per call; a longer list takes ceil(n / 32) calls).  `spectral_norm_network(net)` puts every Conv1d / Conv2d /
Linear of `net` into one group that a forward-pre-hook on `net` evaluates; that equals applying `spectral_norm` to each layer as long as
each layer runs ONCE per forward of `net` (a layer that runs twice would iterate twice per forward in the per-layer form, once here).

LayerEpilogue on a 3-D input [B,C,N] normalises each sample over (C, N) JOINTLY: the reference hands that tensor to nn.InstanceNorm2d,
which reads a 3-D tensor as one unbatched image with B channels.  A 4-D input [B,C,H,W] (use_noise=False) is normalised per (b, c).
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import List, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function

from . import _lib
from ._lib import EPILOGUE_MAX_C, SN_MAX, EpilogueArgs, SnArgs, check
from .edge_conv import refuse_double_backward
from .ops import _f32, _p, _s

Tensor = torch.Tensor

RULE_L2NORMALIZE, RULE_F_NORMALIZE = 0, 1          # x / (|x| + eps)  |  x / max(|x|, eps)
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
PN_NONE, PN_RSQRT, PN_SQRT_DIV = 0, 1, 2           # PixelNorm: x * rsqrt(mean + eps)  |  PixelwiseNorm: x / sqrt(mean + eps)
STATS_NONE, STATS_CHANNEL, STATS_JOINT = 0, 1, 2   # per (b, c) over L  |  per b over C*L


def l2normalize(v: Tensor, eps: float = 1e-12) -> Tensor:
    """modules.py:437 (plain torch: it initialises u and v where the module is built, usually on the CPU)"""
    return v / (v.norm() + eps)


# --------------------------------------------------------------------------------------------------------- spectral normalisation
def pack_sn_group(shapes: Sequence[Sequence[int]], u_sizes: Sequence[int], v_sizes: Sequence[int]):
    """The geometry of a group: [(h, w, save offset, workspace offset)], total save floats, total workspace floats.  h = shape[0],
    w = the rest flattened.  ValueError on an empty group, an empty weight, a weight of fewer than 1 dimension, or u / v of the wrong size."""
    if len(shapes) == 0:
        raise ValueError("spectral norm group: no weights")
    if not (len(shapes) == len(u_sizes) == len(v_sizes)):
        raise ValueError("spectral norm group: %d weights, %d u, %d v" % (len(shapes), len(u_sizes), len(v_sizes)))
    geo, so, wo = [], 0, 0
    for i, (shp, nu, nv) in enumerate(zip(shapes, u_sizes, v_sizes)):
        shp = tuple(int(d) for d in shp)
        if len(shp) < 1 or any(d <= 0 for d in shp):
            raise ValueError("spectral norm group: weight %d has shape %s" % (i, shp))
        h, w = shp[0], 1
        for d in shp[1:]:
            w *= d
        if h * w >= 2 ** 31:
            raise ValueError("spectral norm group: weight %d has %d elements (limit 2^31 - 1)" % (i, h * w))
        if nu != h or nv != w:
            raise ValueError("spectral norm group: weight %d is [%d,%d] flattened, u has %d and v %d elements" % (i, h, w, nu, nv))
        geo.append((h, w, so, wo))
        so += 1 + h + w
        wo += -(-h // 16) * w + h + -(-(h * w) // 2048)
    return geo, so, wo


def _sn_call(entry, geo, ptrs, extra, what):
    lib = _lib.load()
    for i0 in range(0, len(geo), SN_MAX):
        a = SnArgs()
        a.count = min(SN_MAX, len(geo) - i0)
        for t in range(a.count):
            a.h[t], a.w[t] = geo[i0 + t][0], geo[i0 + t][1]
            for field, arr in ptrs.items():
                getattr(a, field)[t] = arr[i0 + t]
        check(getattr(lib, entry)(C.byref(a), *extra, _s()), what, count=a.count)


class _SNGroupFn(Function):
    """inputs: n_iter, rule, eps, us, vs, *weights -> the weights divided by their sigma"""

    @staticmethod
    def forward(ctx, n_iter, rule, eps, us, vs, *weights):
        ws = [_f32(w, "weight %d" % i).contiguous() for i, w in enumerate(weights)]
        for i, (u, v) in enumerate(zip(us, vs)):
            _f32(u, "u %d" % i), _f32(v, "v %d" % i)
            if not (u.is_contiguous() and v.is_contiguous()):
                raise ValueError("spectral norm group: u %d / v %d must be contiguous" % (i, i))
        geo, nsave, nws = pack_sn_group([w.shape for w in ws], [u.numel() for u in us], [v.numel() for v in vs])
        dev = ws[0].device
        save = torch.empty(nsave, dtype=torch.float32, device=dev)
        work = torch.empty(nws, dtype=torch.float32, device=dev)
        outs = [torch.empty_like(w) for w in ws]
        ptrs = {"W": [w.data_ptr() for w in ws], "u": [u.data_ptr() for u in us], "v": [v.data_ptr() for v in vs],
                "out": [o.data_ptr() for o in outs], "save": [save.data_ptr() + 4 * g[2] for g in geo],
                "ws": [work.data_ptr() + 4 * g[3] for g in geo]}
        _sn_call("spgan_sn_forward", geo, ptrs, (int(n_iter), int(rule), float(eps)), "sn_forward")
        ctx.geo, ctx.nws = geo, nws
        ctx.save_for_backward(save, *ws)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        refuse_double_backward("spectral norm")
        save, ws = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        pick = [i for i, g in enumerate(grads) if g is not None and ctx.needs_input_grad[5 + i]]
        out: List[Optional[Tensor]] = [None] * len(ws)
        if pick:
            gs = [_f32(grads[i], "grad %d" % i).contiguous() for i in pick]
            geo = [ctx.geo[i] for i in pick]
            work = torch.empty(ctx.nws, dtype=torch.float32, device=save.device)
            dws = [torch.empty_like(ws[i]) for i in pick]
            ptrs = {"W": [ws[i].data_ptr() for i in pick], "G": [g.data_ptr() for g in gs], "dW": [d.data_ptr() for d in dws],
                    "save": [save.data_ptr() + 4 * g[2] for g in geo], "ws": [work.data_ptr() + 4 * g[3] for g in geo]}
            _sn_call("spgan_sn_backward", geo, ptrs, (), "sn_backward")
            for i, d in zip(pick, dws):
                out[i] = d
        return (None, None, None, None, None) + tuple(out)


def sn_group(weights: Sequence[Tensor], us: Sequence[Tensor], vs: Sequence[Tensor], n_iter: int = 1, rule: int = RULE_F_NORMALIZE,
             eps: float = 1e-12) -> List[Tensor]:
    """[W_l / sigma_l] for a group of weights in one grouped call.  u_l [h_l], v_l [w_l] are updated IN PLACE by n_iter power iterations
    (n_iter = 0: left alone); the gradient treats them as constants: dW = G / sigma - (<G,W> / sigma^2) u v^T."""
    if n_iter < 0:
        raise ValueError("n_iter must be >= 0, got %d" % n_iter)
    if rule not in (RULE_L2NORMALIZE, RULE_F_NORMALIZE):
        raise ValueError("rule must be RULE_L2NORMALIZE or RULE_F_NORMALIZE")
    pack_sn_group([tuple(w.shape) for w in weights], [u.numel() for u in us], [v.numel() for v in vs])
    return list(_SNGroupFn.apply(n_iter, rule, eps, tuple(us), tuple(vs), *weights))


class SpectralNorm(nn.Module):
    """modules.py:441-495, the reference's wrapper class: parameters <name>_bar, <name>_u, <name>_v on the wrapped module (the last two
    with requires_grad=False), l2normalize's rule x / (|x| + 1e-12), and `power_iterations` iterations on EVERY forward, in eval mode too."""

    def __init__(self, module: nn.Module, name: str = "weight", power_iterations: int = 1):
        super().__init__()
        self.module = module
        self.name = name
        self.power_iterations = power_iterations
        if not self._made_params():
            self._make_params()

    def _update_u_v(self):
        u = getattr(self.module, self.name + "_u")
        v = getattr(self.module, self.name + "_v")
        w = getattr(self.module, self.name + "_bar")
        setattr(self.module, self.name, sn_group([w], [u.data], [v.data], self.power_iterations, RULE_L2NORMALIZE, 1e-12)[0])

    def _made_params(self) -> bool:
        return all(hasattr(self.module, self.name + s) for s in ("_u", "_v", "_bar"))

    def _make_params(self):
        w = getattr(self.module, self.name)
        height = w.data.shape[0]
        width = w.view(height, -1).data.shape[1]
        u = nn.Parameter(w.data.new(height).normal_(0, 1), requires_grad=False)
        v = nn.Parameter(w.data.new(width).normal_(0, 1), requires_grad=False)
        u.data = l2normalize(u.data)
        v.data = l2normalize(v.data)
        w_bar = nn.Parameter(w.data)
        del self.module._parameters[self.name]
        self.module.register_parameter(self.name + "_u", u)
        self.module.register_parameter(self.name + "_v", v)
        self.module.register_parameter(self.name + "_bar", w_bar)

    def forward(self, *args):
        self._update_u_v()
        return self.module.forward(*args)


class _SpectralNormHook:
    """torch.nn.utils.spectral_norm's forward-pre-hook on the grouped kernels: <name>_orig, buffers <name>_u / <name>_v, F.normalize's rule,
    power iterations only in training mode."""

    def __init__(self, name: str, n_power_iterations: int, eps: float):
        if n_power_iterations <= 0:
            raise ValueError("Expected n_power_iterations to be positive, but got n_power_iterations=%d" % n_power_iterations)
        self.name, self.n_power_iterations, self.eps = name, n_power_iterations, eps
        self.grouped = False               # True: a spectral_norm_network hook evaluates this weight with its group

    def tensors(self, module):
        return getattr(module, self.name + "_orig"), getattr(module, self.name + "_u"), getattr(module, self.name + "_v")

    def __call__(self, module, inputs):
        if self.grouped:
            return
        w, u, v = self.tensors(module)
        setattr(module, self.name, sn_group([w], [u], [v], self.n_power_iterations if module.training else 0, RULE_F_NORMALIZE, self.eps)[0])


def _sn_hook_of(module: nn.Module, name: str) -> Optional[_SpectralNormHook]:
    for hook in module._forward_pre_hooks.values():
        if isinstance(hook, _SpectralNormHook) and hook.name == name:
            return hook
    return None


def spectral_norm(module: nn.Module, name: str = "weight", n_power_iterations: int = 1, eps: float = 1e-12) -> nn.Module:
    """torch.nn.utils.spectral_norm(module, name, n_power_iterations, eps) with dim = 0; the state_dict (<name>_orig, <name>_u, <name>_v)
    loads strictly into torch's and back."""
    if _sn_hook_of(module, name) is not None:
        raise RuntimeError("Cannot register two spectral_norm hooks on the same parameter %s" % name)
    if isinstance(module, (nn.ConvTranspose1d, nn.ConvTranspose2d, nn.ConvTranspose3d)):
        raise ValueError("spgan.spectral_norm flattens from dim 0; transposed convolutions (dim 1) are not served")
    weight = module._parameters.get(name)
    if weight is None:
        raise ValueError("`spectral_norm` cannot be applied as parameter `%s` is None" % name)
    fn = _SpectralNormHook(name, n_power_iterations, eps)
    with torch.no_grad():
        h = weight.shape[0]
        w = weight.reshape(h, -1).shape[1]
        u = F.normalize(weight.new_empty(h).normal_(0, 1), dim=0, eps=eps)
        v = F.normalize(weight.new_empty(w).normal_(0, 1), dim=0, eps=eps)
    delattr(module, name)
    module.register_parameter(name + "_orig", weight)
    setattr(module, name, weight.data)
    module.register_buffer(name + "_u", u)
    module.register_buffer(name + "_v", v)
    module.register_forward_pre_hook(fn)
    return module


def snconv2d(in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True):
    """modules.py:298"""
    return spectral_norm(nn.Conv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, stride=stride,
                                   padding=padding, dilation=dilation, groups=groups, bias=bias))


def snlinear(in_features, out_features):
    """modules.py:303"""
    return spectral_norm(nn.Linear(in_features=in_features, out_features=out_features))


class _SNNetworkHook:
    def __init__(self, name: str):
        self.name = name

    def __call__(self, net, inputs):
        members = []
        for sub in net.modules():
            fn = _sn_hook_of(sub, self.name)
            if fn is not None and fn.grouped:
                members.append((sub, fn))
        # one grouped call per (mode, iteration count, eps): one call when the whole network is in one mode, as it normally is
        calls = OrderedDict()
        for sub, fn in members:
            calls.setdefault((fn.n_power_iterations if sub.training else 0, fn.eps), []).append((sub, fn))
        for (n_iter, eps), group in calls.items():
            ts = [fn.tensors(sub) for sub, fn in group]
            outs = sn_group([t[0] for t in ts], [t[1] for t in ts], [t[2] for t in ts], n_iter, RULE_F_NORMALIZE, eps)
            for (sub, fn), o in zip(group, outs):
                setattr(sub, fn.name, o)


def spectral_norm_network(net: nn.Module, name: str = "weight", n_power_iterations: int = 1, eps: float = 1e-12) -> nn.Module:
    """spectral_norm on every Conv1d / Conv2d / Linear inside `net` (the state_dict keys are those of the per-layer form), all of their
    weights evaluated by ONE grouped call in a forward-pre-hook on `net`.  Equal to the per-layer form when each layer runs once per
    forward of `net`; calling a wrapped layer on its own, outside net's forward, uses the weight of net's last forward."""
    for sub in net.modules():
        if isinstance(sub, (nn.Conv1d, nn.Conv2d, nn.Linear)) and sub._parameters.get(name) is not None:
            spectral_norm(sub, name, n_power_iterations, eps)
            _sn_hook_of(sub, name).grouped = True
    net.register_forward_pre_hook(_SNNetworkHook(name))
    return net


# --------------------------------------------------------------------------------------------------------- minibatch stddev
def mbstd_groups(B: int, C: int, group_size: int, num_new_features: int = 1, strict: bool = False):
    """-> (G, M): G = min(group_size, B) samples per statistic, M = B / G statistics.  ValueError naming the sizes where the reference
    asserts (strict: MinibatchStdDev's B > group_size and B % group_size != 0) or fails in its reshape (B % G != 0, C % F != 0)."""
    if group_size < 1 or num_new_features < 1:
        raise ValueError("group_size and num_new_features must be >= 1, got %d and %d" % (group_size, num_new_features))
    if strict and B > group_size and B % group_size != 0:
        raise ValueError("batch_size %d should be perfectly divisible by group_size %d" % (B, group_size))
    G = min(group_size, B)
    if B % G != 0:
        raise ValueError("batch size %d is not divisible by the group size min(%d, %d) = %d" % (B, group_size, B, G))
    if C % num_new_features != 0:
        raise ValueError("%d channels are not divisible by num_new_features = %d" % (C, num_new_features))
    return G, B // G


def _cm3(x: Tensor, name: str):
    _f32(x, name, 3)
    if x.numel() == 0:
        raise ValueError("%s must be a non-empty [B,C,N] tensor, got %s" % (name, tuple(x.shape)))
    return x.contiguous()


class _MbStdFn(Function):
    @staticmethod
    def forward(ctx, x, G, Fn, alpha):
        B, Cc, N = x.shape
        lib = _lib.load()
        out = torch.empty((B, Cc + Fn, N), dtype=torch.float32, device=x.device)
        ws = torch.empty(lib.spgan_mbstd_ws_floats(B, Cc, N, G), dtype=torch.float32, device=x.device)
        check(lib.spgan_mbstd_forward(_p(x), B, Cc, N, G, Fn, float(alpha), _p(out), _p(ws), _s()), "mbstd_forward", B=B, C=Cc, N=N, G=G, F=Fn)
        ctx.cfg = (G, Fn, float(alpha))
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, dout):
        refuse_double_backward("minibatch stddev")
        (x,) = ctx.saved_tensors
        G, Fn, alpha = ctx.cfg
        B, Cc, N = x.shape
        dout = _f32(dout, "dout", 3).contiguous()
        dx = torch.empty_like(x)
        S = torch.empty(((B // G) * Fn,), dtype=torch.float32, device=x.device)
        check(_lib.load().spgan_mbstd_backward(_p(x), _p(dout), B, Cc, N, G, Fn, alpha, _p(dx), _p(S), _s()), "mbstd_backward", B=B, C=Cc, N=N)
        return dx, None, None, None


def minibatch_stddev(x: Tensor, group_size: int = 4, num_new_features: int = 1, alpha: float = 1e-8, strict: bool = False) -> Tensor:
    """x [B,C,N] -> [B,C+F,N]: x, then F channels holding, for sample b = g*M + m, the mean over a feature group's channels and the points
    of sqrt(mean_g (x - mean_g)^2 + alpha)."""
    x = _cm3(x, "x")
    G, _ = mbstd_groups(x.shape[0], x.shape[1], group_size, num_new_features, strict)
    return _MbStdFn.apply(x, G, num_new_features, alpha)


class MinibatchStdDev(nn.Module):
    """modules.py:78-135"""

    def __init__(self, group_size: int = 4):
        super().__init__()
        self.group_size = group_size

    def extra_repr(self) -> str:
        return f"group_size={self.group_size}"

    def forward(self, x, alpha=1e-8):
        return minibatch_stddev(x, self.group_size, 1, alpha, strict=True)


class StddevLayer(nn.Module):
    """modules.py:54-76"""

    def __init__(self, group_size: int = 4, num_new_features: int = 1):
        super().__init__()
        self.group_size = group_size
        self.num_new_features = num_new_features

    def forward(self, x):
        return minibatch_stddev(x, self.group_size, self.num_new_features, 1e-8)


# --------------------------------------------------------------------------------------------------------- the layer epilogue
def epilogue_domain(C: int, L: int, stats: int) -> None:
    """ValueError outside the kernels' domain: C <= 1024, L >= 1, and C*L > 1 when statistics are taken."""
    if C < 1 or C > EPILOGUE_MAX_C:
        raise ValueError("the layer epilogue serves 1 <= C <= %d channels, got C = %d" % (EPILOGUE_MAX_C, C))
    if L < 1:
        raise ValueError("the layer epilogue needs L >= 1 points, got L = %d" % L)
    if stats != STATS_NONE and C * L <= 1:
        raise ValueError("instance statistics need more than one value per sample, got C = %d, L = %d" % (C, L))


def _epi_args(x, noise, w, gb, cfg, rs, stat, rec) -> EpilogueArgs:
    act, slope, pn, pn_eps, stats, in_eps = cfg
    B, Cc, L = x.shape
    a = EpilogueArgs()
    a.x, a.noise, a.w = _p(x), _p(noise), _p(w)
    if gb is not None:
        a.gamma, a.beta, a.ld_gb = gb.data_ptr(), gb.data_ptr() + 4 * Cc, 2 * Cc
    a.B, a.C, a.L, a.act, a.pn, a.stats = B, Cc, L, act, pn, stats
    a.slope, a.pn_eps, a.in_eps = float(slope), float(pn_eps), float(in_eps)
    a.rs, a.stat, a.rec = _p(rs), _p(stat), _p(rec)
    return a


class _EpilogueFn(Function):
    """inputs: x [B,C,L], noise [B,L] | None, w [C] | None, gb [B,2C] = (gamma | beta) | None, cfg"""

    @staticmethod
    def forward(ctx, x, noise, w, gb, cfg):
        act, slope, pn, pn_eps, stats, in_eps = cfg
        B, Cc, L = x.shape
        dev = x.device
        lib = _lib.load()
        rs = torch.empty((B, L), dtype=torch.float32, device=dev) if pn else None
        stat = torch.empty((B, Cc, 2) if stats == STATS_CHANNEL else (B, 2), dtype=torch.float32, device=dev) if stats else None
        rec = torch.empty(lib.spgan_epilogue_rec_floats(B, Cc, L), dtype=torch.float32, device=dev) if stats else None
        y = torch.empty_like(x)
        check(lib.spgan_epilogue_forward(C.byref(_epi_args(x, noise, w, gb, cfg, rs, stat, rec)), _p(y), _s()), "epilogue_forward",
              B=B, C=Cc, L=L, act=act, pn=pn, stats=stats)
        ctx.cfg = cfg
        ctx.has = (noise is not None, gb is not None, pn != 0, stats != 0)
        ctx.save_for_backward(*[t for t in (x, noise, w, gb, rs, stat) if t is not None])
        return y

    @staticmethod
    def backward(ctx, dy):
        refuse_double_backward("the layer epilogue")
        saved = list(ctx.saved_tensors)
        x = saved.pop(0)
        noise = saved.pop(0) if ctx.has[0] else None
        w = saved.pop(0) if ctx.has[0] else None
        gb = saved.pop(0) if ctx.has[1] else None
        rs = saved.pop(0) if ctx.has[2] else None
        stat = saved.pop(0) if ctx.has[3] else None
        B, Cc, L = x.shape
        dev = x.device
        need_x, need_n, need_w, need_gb = ctx.needs_input_grad[:4]
        need_n, need_w, need_gb = need_n and noise is not None, need_w and w is not None, need_gb and gb is not None
        if not (need_x or need_n or need_w or need_gb):
            return None, None, None, None, None
        lib = _lib.load()
        dy = _f32(dy, "dy", 3).contiguous()
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)                                    # noqa: E731
        rec = new(lib.spgan_epilogue_rec_floats(B, Cc, L)) if (ctx.has[3] or need_gb or need_w) else None
        grp = (new(B, Cc, 2) if ctx.cfg[4] == STATS_CHANNEL else new(B, 2)) if ctx.has[3] else None
        dx = torch.empty_like(x) if need_x else None
        dn = new(B, L) if need_n else None
        dw = new(Cc) if need_w else None
        dgb = new(B, 2 * Cc) if need_gb else None
        a = _epi_args(x, noise, w, gb, ctx.cfg, rs, stat, rec)
        check(lib.spgan_epilogue_backward(C.byref(a), _p(dy), _p(dx), _p(dn), _p(dw), _p(dgb), None if dgb is None else dgb.data_ptr() + 4 * Cc,
                                          2 * Cc, _p(grp), _s()), "epilogue_backward", B=B, C=Cc, L=L)
        return dx, dn, dw, dgb, None


def layer_epilogue(x: Tensor, noise: Optional[Tensor] = None, weight: Optional[Tensor] = None, act: int = ACT_NONE, slope: float = 0.2,
                   pixel_norm: int = PN_NONE, pn_eps: float = 1e-8, stats: int = STATS_NONE, in_eps: float = 1e-5,
                   gb: Optional[Tensor] = None) -> Tensor:
    """y = gamma * IN(PN(act(x + weight * noise))) + beta on x [B,C,L]; every stage optional.  noise: B*L values (one per point), weight:
    C values; gb [B,2C]: gamma in columns [0,C), beta in [C,2C).  See the module docstring for the two groupings of the statistics."""
    x = _cm3(x, "x")
    B, Cc, L = x.shape
    epilogue_domain(Cc, L, stats)
    if (noise is None) != (weight is None):
        raise ValueError("noise and weight come together")
    if noise is not None:
        _f32(noise, "noise"), _f32(weight, "weight")
        if noise.numel() != B * L:
            noise = noise.expand(B, 1, L)
        noise = noise.contiguous().view(B, L)
        if weight.numel() != Cc:
            raise ValueError("weight must hold C = %d values, got %s" % (Cc, tuple(weight.shape)))
        weight = weight.contiguous().view(Cc)
    if gb is not None:
        _f32(gb, "gb", 2)
        if tuple(gb.shape) != (B, 2 * Cc):
            raise ValueError("gb must be [B,2C] = [%d,%d], got %s" % (B, 2 * Cc, tuple(gb.shape)))
        gb = gb.contiguous()
    if act not in (ACT_NONE, ACT_RELU, ACT_LRELU) or pixel_norm not in (PN_NONE, PN_RSQRT, PN_SQRT_DIV) or \
            stats not in (STATS_NONE, STATS_CHANNEL, STATS_JOINT):
        raise ValueError("unknown act / pixel_norm / stats code")
    return _EpilogueFn.apply(x, noise, weight, gb, (act, float(slope), pixel_norm, float(pn_eps), stats, float(in_eps)))


def _as_cm3(x: Tensor, name: str):
    """[B,C,*] -> ([B,C,L] contiguous, original shape)"""
    _f32(x, name)
    if x.dim() < 2:
        raise ValueError("%s must be [B,C,...], got %s" % (name, tuple(x.shape)))
    return x.contiguous().view(x.shape[0], x.shape[1], -1), x.shape


class PixelNorm(nn.Module):
    """modules.py:175: x * rsqrt(mean_c x^2 + epsilon) on [B,C,...]"""

    def __init__(self, epsilon: float = 1e-8):
        super().__init__()
        self.epsilon = epsilon

    def forward(self, x):
        x3, shp = _as_cm3(x, "x")
        return layer_epilogue(x3, pixel_norm=PN_RSQRT, pn_eps=self.epsilon).view(shp)


class PixelwiseNorm(nn.Module):
    """modules.py:184: x / sqrt(mean_c x^2 + alpha) on [B,C,...]"""

    @staticmethod
    def forward(x, alpha=1e-8):
        x3, shp = _as_cm3(x, "x")
        return layer_epilogue(x3, pixel_norm=PN_SQRT_DIV, pn_eps=alpha).view(shp)


class NoiseLayer(nn.Module):
    """modules.py:372: x [B,C,N] + weight[c] * noise[b,0,n].  noise: the argument, else the `.noise` attribute, else 0.2 * randn drawn on
    the device."""

    def __init__(self, channels: int):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(1, channels, 1))
        self.noise = None

    def pick_noise(self, x: Tensor, noise: Optional[Tensor]) -> Tensor:
        if noise is None and self.noise is None:
            return 0.2 * torch.randn(x.size(0), 1, x.size(2), device=x.device, dtype=x.dtype)
        return self.noise if noise is None else noise

    def forward(self, x, noise=None):
        _f32(x, "x", 3)
        return layer_epilogue(x, self.pick_noise(x, noise), self.weight)


class NoiseInjection(nn.Module):
    """modules.py:362: image [B,C,H,W] + weight[c] * noise [B,1,H,W]"""

    def __init__(self, channel: int):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(1, channel, 1, 1))

    def forward(self, image, noise):
        _f32(image, "image", 4)
        x3, shp = _as_cm3(image, "image")
        return layer_epilogue(x3, _f32(noise, "noise").expand(shp[0], 1, shp[2], shp[3]), self.weight).view(shp)


def _act_code(layer):
    if layer is None or isinstance(layer, nn.Identity):
        return ACT_NONE, 0.0
    if isinstance(layer, nn.ReLU):
        return ACT_RELU, 0.0
    if isinstance(layer, nn.LeakyReLU):
        return ACT_LRELU, float(layer.negative_slope)
    raise ValueError("LayerEpilogue fuses nn.ReLU, nn.LeakyReLU, nn.Identity or None as activation_layer, got %r" % (layer,))


class LayerEpilogue(nn.Module):
    """modules.py:152-173, one fused kernel family instead of the Sequential's passes: noise, activation, pixel norm, instance norm.
    A 3-D input [B,C,N] is normalised per sample over (C, N) jointly, as the reference's nn.InstanceNorm2d does with a 3-D tensor; a 4-D
    input [B,C,H,W] (use_noise=False: NoiseLayer takes 3-D tensors only) per (b, c).  `top_epi` keeps the reference's children, so the
    state_dict (`top_epi.noise.weight`) is the reference's."""

    def __init__(self, channels, dlatent_size, use_wscale, use_noise, use_pixel_norm, use_instance_norm, use_styles, activation_layer):
        super().__init__()
        self.act = _act_code(activation_layer)
        layers = []
        if use_noise:
            layers.append(("noise", NoiseLayer(channels)))
        layers.append(("activation", activation_layer if activation_layer is not None else nn.Identity()))
        if use_pixel_norm:
            layers.append(("pixel_norm", PixelNorm()))
        if use_instance_norm:
            layers.append(("instance_norm", nn.InstanceNorm2d(channels)))
        self.top_epi = nn.Sequential(OrderedDict(layers))
        self.use_noise, self.use_pixel_norm, self.use_instance_norm = bool(use_noise), bool(use_pixel_norm), bool(use_instance_norm)

    def forward(self, x, dlatents_in_slice=None, noise=None):
        _f32(x, "x")
        if x.dim() == 3:
            stats = STATS_JOINT
        elif x.dim() == 4:
            if self.use_noise:
                raise ValueError("LayerEpilogue(use_noise=True) takes [B,C,N]; a 4-D input %s needs use_noise=False" % (tuple(x.shape),))
            stats = STATS_CHANNEL
        else:
            raise ValueError("LayerEpilogue takes [B,C,N] or [B,C,H,W], got %s" % (tuple(x.shape),))
        x3, shp = _as_cm3(x, "x")
        nz = w = None
        if self.use_noise:
            nz, w = self.top_epi.noise.pick_noise(x3, noise), self.top_epi.noise.weight
        eps = self.top_epi.pixel_norm.epsilon if self.use_pixel_norm else 1e-8
        return layer_epilogue(x3, nz, w, self.act[0], self.act[1], PN_RSQRT if self.use_pixel_norm else PN_NONE, eps,
                              stats if self.use_instance_norm else STATS_NONE, 1e-5).view(shp)


class AdaptiveInstanceNorm(nn.Module):
    """modules.py:343-360 on [B,C,H,W]: gamma * IN(x) + beta with (gamma | beta) = EqualLinear(style); bias 1 for gamma, 0 for beta."""

    def __init__(self, in_channel: int, style_dim: int):
        super().__init__()
        from .modules import EqualLinear
        self.norm = nn.InstanceNorm2d(in_channel)
        self.style = EqualLinear(style_dim, in_channel * 2)
        self.style.linear.bias.data[:in_channel] = 1
        self.style.linear.bias.data[in_channel:] = 0

    def forward(self, input, style):
        _f32(input, "input", 4), _f32(style, "style", 2)
        gb = F.linear(style, self.style.weight, self.style.bias)
        x3, shp = _as_cm3(input, "input")
        return layer_epilogue(x3, stats=STATS_CHANNEL, in_eps=self.norm.eps, gb=gb).view(shp)


class _ScaleFn(Function):
    @staticmethod
    def forward(ctx, x, c):
        from .ops import axpby
        ctx.c = c
        return axpby(c, x, 0.0, torch.empty_like(x))

    @staticmethod
    def backward(ctx, g):
        from .ops import axpby
        refuse_double_backward("WScaleLayer")
        g = g.contiguous()
        return axpby(ctx.c, g, 0.0, torch.empty_like(g)), None


class WScaleLayer(nn.Module):
    """modules.py:138: input * sqrt(gain / fan_in of `incoming`)"""

    def __init__(self, incoming, gain=2):
        super().__init__()
        self.gain = gain
        self.scale = (self.gain / incoming.weight[0].numel()) ** 0.5

    def forward(self, input):
        return _ScaleFn.apply(_f32(input, "input").contiguous(), float(self.scale))

    def __repr__(self):
        return "{}(gain={})".format(self.__class__.__name__, self.gain)


class _TruncationFn(Function):
    @staticmethod
    def forward(ctx, x, avg, per_layer, max_layer, thr):
        B, Lr, D = x.shape
        out = torch.empty_like(x)
        check(_lib.load().spgan_truncation(_p(x), _p(avg), int(per_layer), B, Lr, D, int(max_layer), float(thr), 0, _p(out), _s()), "truncation",
              B=B, L=Lr, D=D)
        ctx.cfg = (max_layer, thr)
        return out

    @staticmethod
    def backward(ctx, g):
        refuse_double_backward("Truncation")
        g = g.contiguous()
        B, Lr, D = g.shape
        dx = torch.empty_like(g)
        check(_lib.load().spgan_truncation(_p(g), None, 0, B, Lr, D, int(ctx.cfg[0]), float(ctx.cfg[1]), 1, _p(dx), _s()), "truncation_bwd")
        return dx, None, None, None, None


class Truncation(nn.Module):
    """modules.py:312-327: the first max_layer rows of x [B,layers,D] pulled towards avg_latent ([D], or one row per layer)."""

    def __init__(self, avg_latent, max_layer=8, threshold=0.7, beta=0.995):
        super().__init__()
        self.max_layer = max_layer
        self.threshold = threshold
        self.beta = beta
        self.register_buffer("avg_latent", avg_latent)

    def update(self, last_avg):
        self.avg_latent.copy_(self.beta * self.avg_latent + (1. - self.beta) * last_avg)

    def forward(self, x):
        _f32(x, "x", 3)
        avg = _f32(self.avg_latent, "avg_latent").contiguous()
        B, Lr, D = x.shape
        if avg.numel() == D:
            per_layer = False
        elif avg.numel() == Lr * D and avg.shape[-1] == D:
            per_layer = True
        else:
            raise ValueError("avg_latent must hold D = %d or layers*D = %d values, got %s" % (D, Lr * D, tuple(avg.shape)))
        return _TruncationFn.apply(x.contiguous(), avg, per_layer, self.max_layer, self.threshold)
