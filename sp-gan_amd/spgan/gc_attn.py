"""Global-context attention on csrc/gc_attn.hip: the launchers and the autograd node behind spgan.GC_attn
(the reference's Common/utilities.py:357-426).  Per sample over its L positions, x_n in R^C:

    m_n = w . x_n + b,  p = softmax_n(m)  (average pooling: p_n = 1/L),  ctx = sum_n p_n x_n,
    add = branch_add(ctx),  mul = sigmoid(branch_mul(ctx)),  out_n = x_n * mul + add,
    branch = Conv1d(C,O,1) -> LayerNorm([O,1]) -> ReLU -> Conv1d(O,C,1)

Forward makes two passes over x (pool, apply) and backward two more (reduce, apply), each reading x from memory once -- channel-major with more
than 484 channels excepted, where pool and the backward apply load x twice (csrc/gc_attn.hip) -- and nothing of x's size is kept but x.  The launchers mirror the C ABI
one to one.  layout "cm": x, g, out, dx are contiguous [B,C,L] (the public layout, no transpose on either side); layout "pm":
point-major rows [B*L, C] whose row stride may exceed C (the library's internal layout).  Nothing here synchronises with the host.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib, ops
from ._lib import GcBranch, check
from .edge_conv import refuse_double_backward
from .ops import _p, _s

Tensor = torch.Tensor
MAX_DIM, MAX_B = 1024, 65535
LAYOUTS = {"cm": 0, "pm": 1}
Branch = Optional[Sequence[Tensor]]      # (W1 [O,C], b1 [O], ln.weight [O], ln.bias [O], W2 [C,O], b2 [C]) or None


def chunk_points(layout: str) -> int:
    """The number of positions of a sample one workgroup reduces in `layout` ("cm" / "pm")"""
    return _lib.load().spgan_gc_attn_chunk_points(_layout(layout))


def _layout(layout: str) -> int:
    if layout not in LAYOUTS:
        raise ValueError("gc_attn: layout must be 'cm' or 'pm', got %r" % (layout,))
    return LAYOUTS[layout]


def check_dims(B: int, C: int, L: int, O: Optional[int] = None) -> None:
    if not 1 <= C <= MAX_DIM:
        raise ValueError("gc_attn serves 1 <= C <= %d channels, got C=%d" % (MAX_DIM, C))
    if O is not None and not 1 <= O <= MAX_DIM:
        raise ValueError("gc_attn serves 1 <= O <= %d hidden channels, got O=%d" % (MAX_DIM, O))
    if not 1 <= B <= MAX_B:
        raise ValueError("gc_attn serves 1 <= B <= %d samples, got B=%d" % (MAX_B, B))
    if L < 1:
        raise ValueError("gc_attn needs L >= 1 positions, got L=%d" % L)


def _operand(t: Tensor, name: str, layout: str, B: int, L: int, C: Optional[int] = None) -> Tuple[int, int]:
    """-> (C, row stride) of x / g / out / dx in `layout`"""
    _layout(layout)
    if layout == "cm":
        ops._f32(t, name, 3)
        if not t.is_contiguous() or t.shape[0] != B or t.shape[2] != L or (C is not None and t.shape[1] != C):
            raise ValueError("%s must be contiguous [%d,%s,%d], got %s strides %s" % (name, B, C or "C", L, tuple(t.shape), t.stride()))
        return t.shape[1], L
    ops._rowmajor2d(t, name)
    if t.shape[0] != B * L or (C is not None and t.shape[1] != C):
        raise ValueError("%s must be [%d,%s] rows, got %s" % (name, B * L, C or "C", tuple(t.shape)))
    return t.shape[1], ops._ld(t)


def _new(x: Tensor, layout: str) -> Tensor:
    return torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)


def _nch(layout: str, L: int) -> int:
    c = chunk_points(layout)
    return (L + c - 1) // c


def _vecs(B: int, n: int, *ts: Optional[Tensor]):
    for i, t in enumerate(ts):
        ops._vec(t, B * n, "gc_attn vector %d" % i)


def _branch(p: Branch, C: int, O: int, keep: list) -> Optional[GcBranch]:
    if p is None:
        return None
    W1, b1, lw, lb, W2, b2 = p
    ts = [ops._vec(W1, O * C, "W1"), ops._vec(b1, O, "b1"), ops._vec(lw, O, "ln.weight"), ops._vec(lb, O, "ln.bias"), ops._vec(W2, C * O, "W2"),
          ops._vec(b2, C, "b2")]
    keep.extend(ts)
    return GcBranch(*[t.data_ptr() for t in ts])


def _ref(b: Optional[GcBranch]):
    import ctypes
    return ctypes.byref(b) if b is not None else None


def _hidden(add_p: Branch, mul_p: Branch) -> int:
    p = add_p if add_p is not None else mul_p
    if p is None:
        raise ValueError("gc_attn: at least one of the two branches is required")
    return p[1].numel()


def pool_fwd(x: Tensor, layout: str, B: int, L: int, w: Optional[Tensor] = None, bias: Optional[Tensor] = None):
    """-> (ctx [B,C], lse [B], stat [B,2] = (max logit, sum exp(m - max)), m [B,L] logits or None).  w [C] = conv_mask.weight (None:
    average pooling, lse = log L), bias [1] = conv_mask.bias."""
    C, ld = _operand(x, "x", layout, B, L)
    check_dims(B, C, L)
    ops._vec(w, C, "w"); ops._vec(bias, 1, "bias")
    dev = x.device
    part = torch.empty((B * _nch(layout, L) * (C + 2),), dtype=torch.float32, device=dev)
    m = torch.empty((B, L), dtype=torch.float32, device=dev) if w is not None else None
    ctx = torch.empty((B, C), dtype=torch.float32, device=dev)
    lse = torch.empty((B,), dtype=torch.float32, device=dev)
    stat = torch.empty((B, 2), dtype=torch.float32, device=dev)
    check(_lib.load().spgan_gc_attn_pool_fwd(_p(x), _layout(layout), ld, B, C, L, _p(w), _p(bias), _p(part), _p(m), _p(ctx), _p(lse), _p(stat),
                                             _s()), "gc_attn_pool_fwd", B=B, C=C, L=L, layout=layout)
    return ctx, lse, stat, m


def channel_fwd(ctx: Tensor, add_p: Branch, mul_p: Branch, eps: float = 1e-5):
    """ctx [B,C] -> (add [B,C] or None, mul [B,C] or None, hid [2,B,O], lnstat [2,B,2]): both branches in one launch"""
    ops._f32(ctx, "ctx", 2)
    B, C = ctx.shape
    O = _hidden(add_p, mul_p)
    check_dims(B, C, 1, O)
    _vecs(B, C, ctx)
    keep: list = []
    a, m = _branch(add_p, C, O, keep), _branch(mul_p, C, O, keep)
    dev = ctx.device
    hid = torch.empty((2, B, O), dtype=torch.float32, device=dev)
    lnstat = torch.empty((2, B, 2), dtype=torch.float32, device=dev)
    add = torch.empty((B, C), dtype=torch.float32, device=dev) if a is not None else None
    mul = torch.empty((B, C), dtype=torch.float32, device=dev) if m is not None else None
    check(_lib.load().spgan_gc_attn_channel_fwd(_p(ctx), B, C, O, _ref(a), _ref(m), float(eps), _p(hid), _p(lnstat), _p(add), _p(mul), _s()),
          "gc_attn_channel_fwd", B=B, C=C, O=O)
    return add, mul, hid, lnstat


def channel_slices(C: int, O: int, add_p: Branch, mul_p: Branch):
    """{branch: {name: (lo, hi)}} columns of channel_bwd's G: dt (C), dh, dlnw, dlnb, r (O each), the add branch first"""
    out, off = {}, 0
    for name, p in (("add", add_p), ("mul", mul_p)):
        if p is None:
            continue
        out[name] = {"dt": (off, off + C), "dh": (off + C, off + C + O), "dlnw": (off + C + O, off + C + 2 * O),
                     "dlnb": (off + C + 2 * O, off + C + 3 * O), "r": (off + C + 3 * O, off + C + 4 * O)}
        off += C + 4 * O
    return out, off


def channel_bwd(dadd: Optional[Tensor], dmul: Optional[Tensor], mul: Optional[Tensor], hid: Tensor, lnstat: Tensor, add_p: Branch, mul_p: Branch):
    """-> (G [B, nb*(C + 4 O)] = the per-sample factors of the parameter gradients (channel_slices), dctx [B,C]): one launch"""
    O = _hidden(add_p, mul_p)
    ref = dadd if dadd is not None else dmul
    ops._f32(ref, "dadd / dmul", 2)
    B, C = ref.shape
    check_dims(B, C, 1, O)
    _vecs(B, C, dadd, dmul, mul)
    ops._vec(hid, 2 * B * O, "hid"); ops._vec(lnstat, 4 * B, "lnstat")
    keep: list = []
    a, m = _branch(add_p, C, O, keep), _branch(mul_p, C, O, keep)
    if (a is not None and dadd is None) or (m is not None and (dmul is None or mul is None)):
        raise ValueError("gc_attn channel_bwd: a branch without its cotangent")
    width = channel_slices(C, O, add_p, mul_p)[1]
    G = torch.empty((B, width), dtype=torch.float32, device=ref.device)
    dctx = torch.empty((B, C), dtype=torch.float32, device=ref.device)
    check(_lib.load().spgan_gc_attn_channel_bwd(_p(dadd), _p(dmul), _p(mul), _p(hid), _p(lnstat), B, C, O, _ref(a), _ref(m), _p(G), _p(dctx), _s()),
          "gc_attn_channel_bwd", B=B, C=C, O=O)
    return G, dctx


def apply_fwd(x: Tensor, layout: str, B: int, L: int, mul: Optional[Tensor], add: Optional[Tensor], out: Optional[Tensor] = None) -> Tensor:
    """out = x * mul[b] + add[b] (None: 1 / 0; at least one is required): one read, one write"""
    C, ldx = _operand(x, "x", layout, B, L)
    check_dims(B, C, L)
    if mul is None and add is None:
        raise ValueError("gc_attn apply_fwd needs mul or add")
    _vecs(B, C, mul, add)
    out = _new(x, layout) if out is None else out
    ldo = _operand(out, "out", layout, B, L, C)[1]
    check(_lib.load().spgan_gc_attn_apply_fwd(_p(x), _layout(layout), ldx, B, C, L, _p(mul), _p(add), _p(out), ldo, _s()), "gc_attn_apply_fwd",
          B=B, C=C, L=L, layout=layout)
    return out


def bwd_reduce(x: Tensor, g: Tensor, layout: str, B: int, L: int, want_mul: bool = True, want_add: bool = True):
    """-> (dmul [B,C] = sum_n g_n * x_n or None, dadd [B,C] = sum_n g_n or None) from one read of x and g"""
    C, ldx = _operand(x, "x", layout, B, L)
    ldg = _operand(g, "g", layout, B, L, C)[1]
    check_dims(B, C, L)
    if not (want_mul or want_add):
        raise ValueError("gc_attn bwd_reduce: nothing to compute")
    dev = x.device
    part = torch.empty((B * _nch(layout, L) * 2 * C,), dtype=torch.float32, device=dev) if layout == "pm" else None
    dmul = torch.empty((B, C), dtype=torch.float32, device=dev) if want_mul else None
    dadd = torch.empty((B, C), dtype=torch.float32, device=dev) if want_add else None
    check(_lib.load().spgan_gc_attn_bwd_reduce(_p(x), ldx, _p(g), ldg, _layout(layout), B, C, L, _p(part), _p(dmul), _p(dadd), _s()),
          "gc_attn_bwd_reduce", B=B, C=C, L=L, layout=layout)
    return dmul, dadd


def bwd_apply(x: Tensor, g: Tensor, layout: str, B: int, L: int, mul: Optional[Tensor], dctx: Tensor, ctx: Optional[Tensor] = None,
              w: Optional[Tensor] = None, m: Optional[Tensor] = None, stat: Optional[Tensor] = None):
    """-> (dx, dwpart [B*nch, C] or None).  dx_n = g_n * mul + p_n dctx + s_n w with s_n = p_n (dctx . x_n - dctx . ctx) and
    p = exp(m - stat[:,0]) / stat[:,1]; the column sums of dwpart are the gradient of w.  w None: average pooling, dx_n = g_n * mul + dctx / L."""
    C, ldx = _operand(x, "x", layout, B, L)
    ldg = _operand(g, "g", layout, B, L, C)[1]
    check_dims(B, C, L)
    _vecs(B, C, mul, dctx)
    if dctx is None:
        raise ValueError("gc_attn bwd_apply needs dctx")
    dwpart = None
    if w is not None:
        if ctx is None or m is None or stat is None:
            raise ValueError("gc_attn bwd_apply: attention pooling needs ctx, m and stat")
        ops._vec(w, C, "w"); _vecs(B, C, ctx); _vecs(B, L, m); _vecs(B, 2, stat)
        dwpart = torch.empty((B * _nch(layout, L), C), dtype=torch.float32, device=x.device)
    dx = _new(x, layout)
    check(_lib.load().spgan_gc_attn_bwd_apply(_p(x), ldx, _p(g), ldg, _layout(layout), B, C, L, _p(mul), _p(dctx), _p(ctx), _p(w), _p(m), _p(stat),
                                              _p(dx), _operand(dx, "dx", layout, B, L, C)[1], _p(dwpart), _s()),
          "gc_attn_bwd_apply", B=B, C=C, L=L, layout=layout)
    return dx, dwpart


# ---------------------------------------------------------------------------------------------------------------------------------
class GCAttnFn(Function):
    """spgan.GC_attn's autograd node.  holder: layout, B, L, att (attention pooling), has_add, has_mul, eps.  x is [B,C,L] ("cm") or
    [B*L,C] rows ("pm"); the parameters follow in the module's order: conv_mask (weight, bias) with att, then channel_add_conv's six,
    then channel_mul_conv's six.  Saved: x and tensors of size O(B (C + O + L)): ctx, stat, the logits, mul, hid, lnstat."""

    @staticmethod
    def forward(ctx, holder, x, *params):
        from . import functions as Fn
        Fn._record_modes(ctx, holder)
        h = holder
        if h.layout == "cm":
            x = x.contiguous()
        elif x.dim() == 2 and x.shape[1] > 1 and x.stride(1) != 1:
            x = x.contiguous()
        flat = [p.detach().reshape(-1) for p in params]
        i = 0
        w = bias = add_p = mul_p = None
        if h.att:
            w, bias = flat[0], flat[1]; i = 2
        if h.has_add:
            add_p = flat[i:i + 6]; i += 6
        if h.has_mul:
            mul_p = flat[i:i + 6]; i += 6
        cv, lse, stat, m = pool_fwd(x, h.layout, h.B, h.L, w, bias)
        add, mul, hid, lnstat = channel_fwd(cv, add_p, mul_p, h.eps)
        out = apply_fwd(x, h.layout, h.B, h.L, mul, add)
        ctx.h = h
        ctx.n_params = len(params)
        ctx.has = (m is not None, mul is not None)
        ctx.save_for_backward(x, cv, stat, hid, lnstat, *([m] if m is not None else []), *([mul] if mul is not None else []), *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        refuse_double_backward("GC_attn")
        return GCAttnFn._backward(ctx, dout)

    @staticmethod
    @once_differentiable
    def _backward(ctx, dout):
        from . import functions as Fn
        h = ctx.h
        saved = list(ctx.saved_tensors)
        x, cv, stat, hid, lnstat = saved[:5]
        k = 5
        m = mul = None
        if ctx.has[0]:
            m = saved[k]; k += 1
        if ctx.has[1]:
            mul = saved[k]; k += 1
        params = saved[k:]
        flat = [p.detach().reshape(-1) for p in params]
        i = 0
        w = add_p = mul_p = None
        if h.att:
            w = flat[0]; i = 2
        if h.has_add:
            add_p = flat[i:i + 6]; i += 6
        if h.has_mul:
            mul_p = flat[i:i + 6]; i += 6
        g = dout.contiguous() if (h.layout == "cm" or (dout.shape[1] > 1 and dout.stride(1) != 1)) else dout
        C = cv.shape[1]
        O = _hidden(add_p, mul_p)
        need = ctx.needs_input_grad
        want_p = list(need[2:])
        if not need[1] and not any(want_p):
            return (None,) * len(need)
        dmul, dadd = bwd_reduce(x, g, h.layout, h.B, h.L, want_mul=h.has_mul, want_add=h.has_add)
        G, dctx = channel_bwd(dadd, dmul, mul, hid, lnstat, add_p, mul_p)
        dx = dwpart = None
        if need[1] or (h.att and want_p[0]):                                      # dx and the records of dw come out of one launch
            dx, dwpart = bwd_apply(x, g, h.layout, h.B, h.L, mul, dctx, cv, w, m, stat)
        grads = []
        if h.att:
            grads += [ops.colsum(dwpart)[0].reshape(params[0].shape) if want_p[0] else None, 0]   # the softmax is shift-invariant: an exact zero
        j = 2 if h.att else 0
        sums = ops.colsum(G)[0] if any(want_p[j:]) else None
        sl = channel_slices(C, O, add_p, mul_p)[0]
        col = lambda s: G[:, s[0]:s[1]]                                            # noqa: E731
        vec = lambda s, k: sums[s[0]:s[1]].contiguous().reshape(params[k].shape) if want_p[k] else None   # noqa: E731
        for name in ("add", "mul"):
            if name not in sl:
                continue
            s = sl[name]
            dW1 = ops.gemm_tn(col(s["dh"]), cv, exact=True).reshape(params[j].shape) if want_p[j] else None            # [O,C]
            dW2 = ops.gemm_tn(col(s["dt"]), col(s["r"]), exact=True).reshape(params[j + 4].shape) if want_p[j + 4] else None   # [C,O]
            grads += [dW1, vec(s["dh"], j + 1), vec(s["dlnw"], j + 2), vec(s["dlnb"], j + 3), dW2, vec(s["dt"], j + 5)]
            j += 6
        return (None, dx if need[1] else None) + Fn._deliver(tuple(params), grads, need[2:], ctx.fused)
