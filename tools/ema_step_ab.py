#!/usr/bin/env python3
"""A/B of the generator EMA's cost in the replayed bench-shape train step (N=2048, batch 32, WGAN-GP, TrainStep(graph=True)):
the same models and inputs with and without `ema_rate` (the EMA fused into G's Adam launch), two TrainSteps in ONE process, timed in
interleaved rounds (A, B, A, B, ...) of `--steps` replayed steps each; reports both medians of the per-step time and the median of
the per-round differences.  `python tools/ema_step_ab.py [--rounds 20 --steps 20]`.  Output -> profiles/ema_step_ab.txt.
`--only plain|ema` runs one variant (for a `rocprofv3 --kernel-trace --stats` run of each: same launch count per step)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sp-gan_amd")]

import torch                                                   # noqa: E402

import bench                                                   # noqa: E402  (models, inputs and shape of the headline run)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--only", choices=("plain", "ema"), default=None)
    a = ap.parse_args()
    tags = (a.only,) if a.only else ("plain", "ema")
    import spgan
    dev = torch.device("cuda", 0)
    x, real, zs, alpha = bench.make_inputs(dev, 0, a.batch)
    steps = {}
    for tag, rate in (("plain", None), ("ema", 0.999)):
        if tag not in tags:
            continue
        G, D = bench.build_models(dev)
        steps[tag] = spgan.TrainStep(G, D, gan="wgan", use_gp=True, lambda_gp=10.0, lr_g=1e-4, lr_d=1e-4, graph=True, ema_rate=rate)
        for _ in range(8):                                     # eager warm-up, capture, replays
            steps[tag].step(x, real, zs[0], zs[1], alpha=alpha)
        assert steps[tag]._graph is not None, "the step was not captured"
    torch.cuda.synchronize()
    per = {tag: [] for tag in tags}
    for _ in range(a.rounds):
        for tag in tags:
            tr = steps[tag]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                tr.step(x, real, zs[0], zs[1], alpha=alpha)
            e1.record()
            torch.cuda.synchronize()
            per[tag].append(e0.elapsed_time(e1) / a.steps)
    print("# replayed train step, N=%d, batch %d, WGAN-GP, %d interleaved rounds x %d steps (%s)" % (
        bench.N_POINTS, a.batch, a.rounds, a.steps, torch.cuda.get_device_name(0)))
    for tag in tags:
        v = sorted(per[tag])
        print("%-6s median %.4f ms/step  min %.4f  max %.4f" % (tag, statistics.median(v), v[0], v[-1]))
    if len(tags) == 2:
        d = sorted(b - p for p, b in zip(per["plain"], per["ema"]))
        print("ema - plain: median %+.2f us/step  (per-round range %+.2f .. %+.2f us)" % (statistics.median(d) * 1e3, d[0] * 1e3, d[-1] * 1e3))
    for tag in tags:
        print("%-6s final lossD %.6f" % (tag, float(steps[tag]._static_info["loss_d"])))


if __name__ == "__main__":
    main()
