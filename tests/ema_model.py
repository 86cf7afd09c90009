"""CPU doubles of the generator-EMA ops (spgan.ops.adam_ema_step_dev / adam_ema_step / ema_update_dev) for the host-composition tests,
installed on top of the kernel models (helpers.kernel_models / the spgan_cpu fixture) with `install(monkeypatch)`.  Same contract as the
HIP entry points: the coefficient a = min(1 - 1/t, rate) (warm-up) or rate, a and 1 - a evaluated in double and rounded once;
e <- a*e + (1-a)*p, evaluated in double and rounded once."""
import numpy as np
import torch

import kernel_model as km


def coef(t: int, rate: float, warmup: bool):
    ad = float(rate)
    if warmup:
        ad = min(1.0 - 1.0 / max(int(t), 1), ad)
    return float(np.float32(ad)), float(np.float32(1.0 - ad))


def ema_apply(e: torch.Tensor, p: torch.Tensor, t: int, rate: float, warmup: bool) -> None:
    a, b = coef(t, rate, warmup)
    e.copy_((a * e.double() + b * p.double()).to(e.dtype))


def adam_ema_step_dev(p, g, m, v, e, state, lr=1e-4, beta1=0.5, beta2=0.99, eps=1e-8, grad_scale=1.0, zero_grad=False, ema_rate=0.999,
                      ema_warmup=True):
    km.adam_step_dev(p, g, m, v, state, lr, beta1, beta2, eps, grad_scale, zero_grad)
    ema_apply(e, p, int(state[:1].view(torch.int32).item()), ema_rate, ema_warmup)


def adam_ema_step(p, g, m, v, e, step, lr=1e-4, beta1=0.5, beta2=0.99, eps=1e-8, grad_scale=1.0, ema_rate=0.999, ema_warmup=True):
    km.adam_step(p, g, m, v, step, lr, beta1, beta2, eps, grad_scale)
    ema_apply(e, p, step, ema_rate, ema_warmup)


def ema_update_dev(e, p, counter, ema_rate=0.999, ema_warmup=True):
    counter += 1
    ema_apply(e, p, int(counter.item()), ema_rate, ema_warmup)


def install(monkeypatch):
    import spgan.ops as ops
    for fn in (adam_ema_step_dev, adam_ema_step, ema_update_dev):
        monkeypatch.setattr(ops, fn.__name__, fn)
