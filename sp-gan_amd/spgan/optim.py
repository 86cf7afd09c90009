"""Flat-buffer Adam (torch.optim.Adam semantics, Generation/model.py:94-97) and the flat
parameter/gradient layout shared with the data-parallel reducer.

`flatten_module(m)` re-points every parameter of `m` at a slice of ONE contiguous fp32 buffer and
pre-binds `.grad` to the matching slice of ONE gradient buffer: the optimiser update is a single
HIP launch and the data-parallel all-reduce a single RCCL collective per network.
state_dict() is unaffected (parameters keep their names/shapes).

`EMA` is the generator weight average of Common/network_utils.py:97-108 over such a flat buffer; `Adam.attach_ema` folds its update
into the optimiser's launch.
"""
from __future__ import annotations

import copy
from typing import Iterable, List, Optional

import torch
import torch.nn as nn

from . import ops


class FlatParams:
    def __init__(self, module: nn.Module):
        params = [p for p in module.parameters()]
        if not params:
            raise ValueError("module has no parameters")
        dev = params[0].device
        # every slice starts on a 16-byte boundary (float4 operand loads in the GEMM fast path); the padding
        # elements stay zero in both buffers, so Adam and the all-reduce may run over the whole buffer.
        self.offsets = []
        n = 0
        for p in params:
            self.offsets.append(n)
            n += (p.numel() + 3) // 4 * 4
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.params = params
        with torch.no_grad():
            for p, off in zip(params, self.offsets):
                k = p.numel()
                self.flat[off:off + k].copy_(p.reshape(-1))
                p.data = self.flat[off:off + k].view_as(p)
                p.grad = self.grad[off:off + k].view_as(p)
        self.numel = n

    def zero_grad(self):
        """Zero in place and re-bind (autograd accumulates into the flat slices)."""
        self.grad.zero_()
        for p, off in zip(self.params, self.offsets):
            k = p.numel()
            if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + 4 * off:
                p.grad = self.grad[off:off + k].view_as(p)


def flatten_module(module: nn.Module) -> FlatParams:
    fp = getattr(module, "_spgan_flat", None)
    if fp is None or any(p.data_ptr() < fp.flat.data_ptr() or p.data_ptr() >= fp.flat.data_ptr() + 4 * fp.numel for p in module.parameters()):
        fp = FlatParams(module)
        module.__dict__["_spgan_flat"] = fp
    return fp


class Adam:
    """Adam over a module's flat buffer.  `step()` == torch.optim.Adam(lr, betas, eps=1e-8).step();
    `zero_grad()` zeroes the flat gradient buffer in place."""

    def __init__(self, module: nn.Module, lr: float = 1e-4, betas=(0.5, 0.99), eps: float = 1e-8, capturable: bool = False,
                 zero_grad_in_step: bool = False):
        self.fp = flatten_module(module)
        self.lr, self.betas, self.eps = lr, betas, eps
        self.m = torch.zeros_like(self.fp.flat)
        self.v = torch.zeros_like(self.fp.flat)
        self.t = 0
        # capturable: the step count (and its bias corrections) live on the device, so that a hipGraph of the train step can
        # be replayed; `t` stays the host-side mirror (state_dict)
        self.capturable = capturable
        self.dev_state = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float32, device=self.fp.flat.device) if capturable else None
        self.base_lr = lr
        self.ema: Optional["EMA"] = None          # attach_ema(): step() also advances this shadow, in the same launch
        # zero_grad_in_step (capturable mode; TrainStep): step() leaves the flat gradient buffer zeroed -- the kernel has every gradient in a
        # register anyway -- and the zero_grad() that follows it is a no-op instead of a fill launch.  Only for an owner that writes the
        # gradients exclusively between zero_grad() and step().
        self.zero_grad_in_step = bool(zero_grad_in_step and capturable)
        self._grad_clean = False

    def invalidate_grads(self) -> None:
        """Restore "the flat gradient buffer is zero" after anything OUTSIDE the owner's zero_grad() .. step() window wrote into the
        parameters' `.grad` (a diagnostic backward between two steps, a regulariser of the caller's): zero_grad_in_step skips the
        fill on the host flag alone, and a captured step records no fill at all, so such a write would be added to the next step's
        gradients.  Zeroes the buffer now (one fill launch) and forgets the flag.  Contract of zero_grad_in_step otherwise: `p.grad`
        reads as zero after step()."""
        self._grad_clean = False
        self.fp.zero_grad()
        self._grad_clean = self.zero_grad_in_step

    def zero_grad(self, set_to_none: bool = False):
        if self._grad_clean:
            self._grad_clean = False         # the previous step() zeroed the buffer; the parameters' .grad views are bound to it
            return
        self.fp.zero_grad()

    def attach_ema(self, ema: "EMA") -> None:
        """From now on step() also updates `ema`'s shadow from the freshly updated parameters, inside the same launch
        (ops.adam_ema_step_dev / adam_ema_step; the parameters, moments and gradients come out bit-identical to a step without it).
        The shadow's warm-up position is then this optimiser's step count t."""
        if ema.src.flat.data_ptr() != self.fp.flat.data_ptr():
            raise ValueError("attach_ema: the EMA averages another module's parameters")
        if ema._opt is not None and ema._opt is not self:
            raise ValueError("attach_ema: the EMA is attached to another optimiser")
        self.ema = ema
        ema._opt = self

    def step(self, grad_scale: float = 1.0):
        self.t += 1
        ops.bump_weights_epoch(self.fp.flat)
        ema = self.ema
        if ema is not None:
            ops.bump_weights_epoch(ema.fp.flat)         # the shadow's host-side weight caches are stale as well
        if self.capturable:
            if ema is None:
                ops.adam_step_dev(self.fp.flat, self.fp.grad, self.m, self.v, self.dev_state, self.lr, self.betas[0], self.betas[1], self.eps, grad_scale,
                                  zero_grad=self.zero_grad_in_step)
            else:
                ops.adam_ema_step_dev(self.fp.flat, self.fp.grad, self.m, self.v, ema.fp.flat, self.dev_state, self.lr, self.betas[0], self.betas[1],
                                      self.eps, grad_scale, zero_grad=self.zero_grad_in_step, ema_rate=ema.rate, ema_warmup=ema.warmup)
            self._grad_clean = self.zero_grad_in_step
        elif ema is None:
            ops.adam_step(self.fp.flat, self.fp.grad, self.m, self.v, self.t, self.lr, self.betas[0], self.betas[1], self.eps, grad_scale)
        else:
            ops.adam_ema_step(self.fp.flat, self.fp.grad, self.m, self.v, ema.fp.flat, self.t, self.lr, self.betas[0], self.betas[1], self.eps,
                              grad_scale, ema_rate=ema.rate, ema_warmup=ema.warmup)

    def set_lr(self, lr: float) -> None:
        """Change the learning rate (lr schedules).  In capturable mode the captured kernels keep the lr they were recorded with;
        the new value enters through the multiplier in the device state, so replayed graphs follow it."""
        if self.capturable:
            self.dev_state[3:4].fill_(float(lr) / self.base_lr)
            self._lr_now = float(lr)
        else:
            self.lr = float(lr)

    def get_lr(self) -> float:
        return getattr(self, "_lr_now", self.lr) if self.capturable else self.lr

    def state_dict(self):
        return {"m": self.m, "v": self.v, "t": self.t, "lr": self.get_lr(), "betas": self.betas, "eps": self.eps}

    def load_state_dict(self, sd):
        self.m.copy_(sd["m"]); self.v.copy_(sd["v"]); self.t = int(sd["t"])
        self.betas, self.eps = tuple(sd["betas"]), sd["eps"]
        self.set_lr(sd["lr"])
        if self.capturable:
            self.dev_state[:1].view(torch.int32).fill_(self.t)


class StepLR:
    """torch.optim.lr_scheduler.StepLR for spgan.optim.Adam (Generation/model.py:99-110: step_size = lr_decay_feq, gamma =
    lr_decay_rate, stepped once per epoch at model.py:309-312): lr = base_lr * gamma ** (epoch // step_size)."""

    def __init__(self, optimizer: Adam, step_size: int, gamma: float = 0.1):
        self.opt, self.step_size, self.gamma = optimizer, int(step_size), float(gamma)
        self.base_lr = optimizer.get_lr()
        self.last_epoch = 0

    def step(self) -> None:
        self.last_epoch += 1
        self.opt.set_lr(self.base_lr * self.gamma ** (self.last_epoch // self.step_size))

    def get_last_lr(self):
        return [self.opt.get_lr()]

    def state_dict(self):
        return {"step_size": self.step_size, "gamma": self.gamma, "base_lr": self.base_lr, "last_epoch": self.last_epoch}

    def load_state_dict(self, sd) -> None:
        """Restores the schedule's position and sets the optimiser's lr to the one it prescribes there (what Adam.load_state_dict
        restored, for a pair saved together)."""
        self.step_size, self.gamma = int(sd["step_size"]), float(sd["gamma"])
        self.base_lr, self.last_epoch = float(sd["base_lr"]), int(sd["last_epoch"])
        self.opt.set_lr(self.base_lr * self.gamma ** (self.last_epoch // self.step_size))


# per-module host-side caches (kNN graphs of the sphere prior, EdgeConv1's twin-forward output, pending BatchNorm counts, the flat
# layout, a communicator): never copied into a shadow -- it derives its own
_MODULE_CACHES = ("_spgan_flat", "_ec1_twin", "_sphere_graph", "_sphere_graphs", "_graph2_queue", "_pair_idx", "_bn_pending", "_comm")


class EMA:
    """Exponential moving average of a module's parameters (the generator EMA of Common/network_utils.py:97-108; the reference
    declares --ema / --ema_rate, Generation/config.py:112,125).

    `module` is flattened (flatten_module); `EMA.module` is a deep copy of it whose parameters live in a flat buffer with the SAME
    offsets (asserted), so one launch averages the whole network: e <- a*e + (1-a)*p with a = min(1 - 1/t, rate) when `warmup`
    (exp_mov_avg with global_step = t-1: the first update copies p), else a = rate (accumulate).  The shadow parameters do not
    require gradients; `EMA.module` is an ordinary module (eval, interpolate, metrics, state_dict).

    update() is the standalone update (ops.ema_update_dev, its own device-side step counter: capturable) for callers with their own
    optimiser; Adam.attach_ema(ema) instead folds the update into that optimiser's step (t = its step count).

    Buffers are not averaged (accumulate averages parameters only): copy_buffers() copies the source's BatchNorm running statistics
    and counts into the shadow -- the StyleGAN convention; call it before using the shadow in eval mode and before its state_dict().
    This deliberately differs from the reference helpers applied to a deep-copied G, whose buffers would stay frozen at the copy."""

    def __init__(self, module: nn.Module, rate: float = 0.999, warmup: bool = True):
        if not 0.0 <= float(rate) <= 1.0:
            raise ValueError("EMA rate must lie in [0, 1], got %r" % (rate,))
        self.src = flatten_module(module)
        memo = {}
        for m in module.modules():
            for k in _MODULE_CACHES:
                if k in m.__dict__:
                    memo[id(m.__dict__[k])] = None              # deepcopy returns None for these; removed from the copy below
        shadow = copy.deepcopy(module, memo)
        for m in shadow.modules():
            for k in _MODULE_CACHES:
                m.__dict__.pop(k, None)
        for p in shadow.parameters():
            p.requires_grad_(False)
        self.fp = flatten_module(shadow)
        assert self.fp.offsets == self.src.offsets and self.fp.numel == self.src.numel, "EMA shadow: flat layout differs from the source's"
        self.source, self.module = module, shadow
        self.rate, self.warmup = float(rate), bool(warmup)
        self._t = 0
        self.counter = torch.zeros(1, dtype=torch.int32, device=self.fp.flat.device)     # update()'s device-side step count
        self._opt: Optional[Adam] = None

    @property
    def t(self) -> int:
        """Updates applied so far (the warm-up position): the attached optimiser's step count, else update()'s own."""
        return self._opt.t if self._opt is not None else self._t

    def update(self) -> None:
        """One EMA update from the source's current parameters (two launches: counter advance + update).  Inside a captured graph
        the host-side bookkeeping happens once, at capture: after each replay call mark_updated()."""
        if self._opt is not None:
            raise RuntimeError("EMA.update: this EMA is attached to an optimiser, whose step() updates it")
        if flatten_module(self.source) is not self.src:
            raise RuntimeError("EMA.update: the source module's parameters were re-flattened since the EMA was built")
        self.mark_updated()
        ops.ema_update_dev(self.fp.flat, self.src.flat, self.counter, self.rate, self.warmup)

    def mark_updated(self) -> None:
        """Host-side bookkeeping of one standalone update: the step count and the shadow's weight caches (ops.bump_weights_epoch)."""
        self._t += 1
        ops.bump_weights_epoch(self.fp.flat)

    def copy_buffers(self) -> None:
        """Shadow buffers (BatchNorm running statistics, num_batches_tracked) := the source's, pending counts flushed first."""
        if hasattr(self.source, "flush_bn_counts"):
            self.source.flush_bn_counts()
        if hasattr(self.module, "flush_bn_counts"):
            self.module.flush_bn_counts()
        with torch.no_grad():
            for (n, b), (n2, b2) in zip(self.source.named_buffers(), self.module.named_buffers()):
                assert n == n2, (n, n2)
                b2.copy_(b)

    def state_dict(self):
        """Shadow parameters and buffers (module state_dict, tensors cloned), rate, warm-up flag and step count."""
        return {"module": {k: v.detach().clone() for k, v in self.module.state_dict().items()}, "rate": self.rate, "warmup": self.warmup,
                "t": self.t}

    def load_state_dict(self, sd) -> None:
        """Copies into the existing shadow tensors (a captured graph that updates them stays valid)."""
        self.module.load_state_dict(sd["module"])
        self.rate, self.warmup = float(sd["rate"]), bool(sd["warmup"])
        self._t = int(sd["t"])
        self.counter.fill_(self._t)
        ops.bump_weights_epoch(self.fp.flat)
