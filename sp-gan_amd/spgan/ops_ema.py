"""Wrappers of the generator-EMA entry points of libspgan_hip.so (include/spgan_hip.h: spgan_adam_ema_step_dev, spgan_adam_ema_step,
spgan_ema_update_dev), re-exported by spgan.ops as ops.adam_ema_step_dev / ops.adam_ema_step / ops.ema_update_dev.  Argument checks as
ops.adam_step_dev's."""
from __future__ import annotations

import torch

from . import _lib
from .ops import Tensor, _f32, _p, _s, check


def _ema_args(what: str, rate: float, flats) -> None:
    n0 = flats[0][0].numel()
    for t, n in flats:
        _f32(t, n)
        if not t.is_contiguous() or t.numel() != n0:
            raise ValueError("%s: %s must be contiguous with %d elements" % (what, n, n0))
    if not 0.0 <= float(rate) <= 1.0:
        raise ValueError("%s: ema_rate must lie in [0, 1], got %r" % (what, rate))


def adam_ema_step_dev(p: Tensor, g: Tensor, m: Tensor, v: Tensor, e: Tensor, state: Tensor, lr: float = 1e-4, beta1: float = 0.5,
                      beta2: float = 0.99, eps: float = 1e-8, grad_scale: float = 1.0, zero_grad: bool = False, ema_rate: float = 0.999,
                      ema_warmup: bool = True) -> None:
    """adam_step_dev (same state, same launches; p, m, v, g bit-identical to it) with the generator EMA e <- a*e + (1-a)*p_new applied
    in the update launch.  a = min(1 - 1/t, ema_rate) with ema_warmup (Common/network_utils.py:104-108, exp_mov_avg with
    global_step = t-1), else ema_rate (accumulate, :97-101); t = the step count in `state` after this update."""
    _ema_args("adam_ema_step_dev", ema_rate, ((p, "p"), (g, "g"), (m, "m"), (v, "v"), (e, "e")))
    _f32(state, "state")
    if state.numel() != 4 or not state.is_contiguous():
        raise ValueError("adam_ema_step_dev: state must be 4 contiguous floats (step bits, two bias corrections, lr multiplier)")
    check(_lib.load().spgan_adam_ema_step_dev(_p(p), _p(g), _p(m), _p(v), _p(e), p.numel(), lr, beta1, beta2, eps, _p(state), grad_scale,
                                              1 if zero_grad else 0, float(ema_rate), 1 if ema_warmup else 0, _s()), "adam_ema_step_dev")


def adam_ema_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, e: Tensor, step: int, lr: float = 1e-4, beta1: float = 0.5,
                  beta2: float = 0.99, eps: float = 1e-8, grad_scale: float = 1.0, ema_rate: float = 0.999, ema_warmup: bool = True) -> None:
    """adam_step (p, m, v bit-identical to it) with the EMA of adam_ema_step_dev at t = step."""
    _ema_args("adam_ema_step", ema_rate, ((p, "p"), (g, "g"), (m, "m"), (v, "v"), (e, "e")))
    check(_lib.load().spgan_adam_ema_step(_p(p), _p(g), _p(m), _p(v), _p(e), p.numel(), lr, beta1, beta2, eps, int(step), grad_scale,
                                          float(ema_rate), 1 if ema_warmup else 0, _s()), "adam_ema_step")


def ema_update_dev(e: Tensor, p: Tensor, counter: Tensor, ema_rate: float = 0.999, ema_warmup: bool = True) -> None:
    """The EMA alone (callers with their own optimiser): counter (one int32 on the device) is advanced first, t = its new value; the
    same coefficient and per-element update as adam_ema_step_dev.  Nothing host-side changes between calls: capturable."""
    _ema_args("ema_update_dev", ema_rate, ((e, "e"), (p, "p")))
    if counter.dtype != torch.int32 or counter.numel() != 1 or not counter.is_contiguous():
        raise ValueError("ema_update_dev: counter must be one contiguous int32")
    if not counter.is_cuda:
        raise RuntimeError("ema_update_dev: counter must live on the GPU")
    check(_lib.load().spgan_ema_update_dev(_p(e), _p(p), e.numel(), float(ema_rate), 1 if ema_warmup else 0, _p(counter), _s()), "ema_update_dev")
