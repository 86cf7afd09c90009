#!/usr/bin/env python3
"""Generate tests/golden/g22_ema.npz (G22): the reference's generator-EMA helpers `accumulate` and `exp_mov_avg`
(Common/network_utils.py:97-108, imported from the read-only reference checkout; torch only) run over a fixed trajectory of
generator-shaped parameter sets.  Runs only in the build container; the tests read the .npz.

    python tests/golden/make_golden_ema.py

The parameter set is the 15 tensors of the Generator's state_dict with at most 64 elements (803 values: biases and BatchNorm affine
parameters of EdgeConv1, the first layers of EdgeConv2 and the last two tail layers; a flat length that is not a multiple of 4).  The
rule is element-wise, so a small set pins it (and keeps the file small); the kernels' own tests cover the full 2.34 MB flat buffer.
Step t = 1..T moves the parameters by 1e-2 N(0,1) (seeded) and then applies one update of each rule to its own shadow, both starting
from the same shadow e0 (p0 plus 5e-2 N(0,1): a shadow that does not equal p, so the first accumulate step is not trivial):
    accumulate(shadow, live, decay=RATE)                      -> acc[t-1]
    exp_mov_avg(shadow, live, alpha=RATE, global_step=t-1)    -> ema[t-1]     (t = 1: a copy of p1)
The legacy `add_(alpha, tensor)` overload both helpers use still runs on current torch (with a deprecation warning).
"""
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "sp-gan_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from spgan import fixture_rng as fr                                   # noqa: E402
from oracle import spgan_oracle as orc                                # noqa: E402
from Common.network_utils import accumulate, exp_mov_avg              # noqa: E402

RATE, T, MAX_NUMEL = 0.999, 12, 64


class Params(nn.Module):
    """The parameter set as a module (the helpers walk named_parameters / parameters)."""

    def __init__(self, tensors):
        super().__init__()
        for i, t in enumerate(tensors):
            self.register_parameter("p%02d" % i, nn.Parameter(t.clone(), requires_grad=False))

    def flat(self):
        return torch.cat([p.detach().reshape(-1) for p in self.parameters()]).numpy().copy()


def main():
    shapes = {k: v for k, v in orc.generator_shapes().items() if int(np.prod(v)) <= MAX_NUMEL}
    p0 = fr.init_params(shapes, salt=22)
    names = list(shapes)
    g = torch.Generator().manual_seed(22)
    live = Params([p0[n] for n in names])
    e0 = [p0[n] + 0.05 * torch.randn(p0[n].shape, generator=g) for n in names]
    acc_sh, ema_sh = Params(e0), Params(e0)
    ps, acc, ema = [live.flat()], [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        for t in range(1, T + 1):
            with torch.no_grad():
                for p in live.parameters():
                    p.add_(0.01 * torch.randn(p.shape, generator=g))
            accumulate(acc_sh, live, decay=RATE)
            exp_mov_avg(ema_sh, live, alpha=RATE, global_step=t - 1)
            ps.append(live.flat()); acc.append(acc_sh.flat()); ema.append(ema_sh.flat())
    out = os.path.join(HERE, "g22_ema.npz")
    np.savez_compressed(out, names=np.array(names), numel=np.array([int(np.prod(shapes[n])) for n in names]), rate=np.float64(RATE),
                        p=np.stack(ps).astype(np.float32), e0=Params(e0).flat().astype(np.float32),
                        acc=np.stack(acc).astype(np.float32), ema=np.stack(ema).astype(np.float32))
    print("wrote", out, "n =", ps[0].size)


if __name__ == "__main__":
    main()
