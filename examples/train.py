#!/usr/bin/env python3
"""The reference's training loop (Generation/model.py:199-330) over the MI355X path, end to end on one GPU:
device-resident dataset -> sphere prior + latent noise drawn on the device -> TrainStep (hipGraph replay) -> checkpoints in the
reference's layout ({'G_model','G_optimizer','G_epoch'} / {'D_model','D_optimizer','D_epoch'}, model.py:505-525) -> sample dump.

    python examples/train.py --data chair.npy --np 2048 --bs 32 --epochs 2 --out runs/chair
    python examples/train.py --synthetic 256 --np 512 --bs 8 --epochs 1 --out /tmp/run      # no dataset needed

--ema keeps a generator weight EMA (Generation/config.py:112,125 declare --ema / --ema_rate; the update is
Common/network_utils.py:97-108, fused into G's Adam launch): the G checkpoint gains a 'G_ema_model' key and the samples come from
the EMA generator.  Every epoch also writes <tag>_state.pth (epoch, step count, scheduler, RNG states of the dataset, the sampler and
torch).  --restore <out>/<epoch>_<choice> continues such a run at the next epoch from <tag>_G.pth, <tag>_D.pth and <tag>_state.pth,
bit for bit as if it had not stopped -- the reference's --restore + --pretrain_model_G/D (model.py:187-196,460-503), except that
D's optimiser state is restored as well (the reference reloads only G's, model.py:496).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sp-gan_amd"), ROOT]

import torch                                                   # noqa: E402
import spgan                                                   # noqa: E402
from spgan import fixture_rng as fr                            # noqa: E402
from spgan.dataset import DeviceDataset                        # noqa: E402
from spgan.sampling import InputSampler, save_xyz              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=None, help=".npy/.npz/.h5 with [S, P, 3] clouds")
    ap.add_argument("--synthetic", type=int, default=0, help="use this many synthetic clouds instead of --data")
    ap.add_argument("--np", type=int, default=2048); ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--nz", type=int, default=128); ap.add_argument("--nk", type=int, default=20)
    ap.add_argument("--nv", type=float, default=0.2); ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--gan", default="ls"); ap.add_argument("--gp", action="store_true")
    ap.add_argument("--lr_g", type=float, default=1e-4); ap.add_argument("--lr_d", type=float, default=1e-4)
    ap.add_argument("--augment", action="store_true"); ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--augment_set", choices=("ref", "full"), default=None,
                    help="augment every batch in one call of the device-side kernel (spgan.augment): 'ref' = point shuffle, rotation about y "
                         "and scale as --augment; 'full' = the reference's point_transform (H5DataLoader.py:21-31) on top of the shuffle")
    ap.add_argument("--out", default="runs/spgan"); ap.add_argument("--choice", default="chair")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--mfma", choices=("f32", "f16", "bf16x3"), default="f32", help="operand mode of the matrix products (INTEGRATION.md section 4a)")
    ap.add_argument("--lr_decay", action="store_true", help="StepLR on both optimisers, stepped once per epoch (Generation/model.py:99-110,309-312)")
    ap.add_argument("--lr_decay_feq", type=int, default=40); ap.add_argument("--lr_decay_rate", type=float, default=0.7)
    ap.add_argument("--ema", action="store_true", help="generator weight EMA (Common/network_utils.py:97-108)")
    ap.add_argument("--ema_rate", type=float, default=0.999)
    ap.add_argument("--ema_warmup", action=argparse.BooleanOptionalAction, default=True,
                    help="a = min(1 - 1/t, ema_rate) (exp_mov_avg) instead of the constant ema_rate (accumulate)")
    ap.add_argument("--restore", default=None, metavar="TAG", help="continue the run saved as TAG_{G,D,state}.pth (TAG = <out>/<epoch>_<choice>)")
    a = ap.parse_args()
    spgan.ops.set_mfma_operands(a.mfma)

    class Opts:                                                # the fields of Generation/config.py the modules read
        np = a.np; nk = a.nk; nz = a.nz; nv = a.nv; softmax = True; off = False; attn = False; use_head = False
        eql = False; z_norm = False; small_d = False; n_rand = False; n_mix = False

    dev = torch.device("cuda", 0)
    torch.manual_seed(123)                                     # model.py:38-41
    src = a.data if a.data else torch.cat([fr.synthetic_real(64, a.np, seed=i) for i in range((a.synthetic + 63) // 64)])[:a.synthetic or 64]
    transform = spgan.augment.reference_transform(a.augment_set, seed=0, device=dev) if a.augment_set else None
    data = DeviceDataset(src, num_points=a.np, batch_size=a.bs, scale=a.scale, augment=a.augment, device=dev, seed=0, transform=transform)
    G, D = spgan.Generator(Opts).to(dev), spgan.Discriminator(Opts, num_point=a.np).to(dev)
    step = spgan.TrainStep(G, D, gan=a.gan, use_gp=a.gp, lr_g=a.lr_g, lr_d=a.lr_d, graph=not a.no_graph,
                           ema_rate=a.ema_rate if a.ema else None, ema_warmup=a.ema_warmup)
    smp = InputSampler(Opts, device=dev, seed=1)
    x = smp.sphere_generator(a.bs)                             # model.py:231
    os.makedirs(a.out, exist_ok=True)
    it = 0
    scheds = [spgan.optim.StepLR(o, a.lr_decay_feq, a.lr_decay_rate) for o in (step.optG, step.optD)] if a.lr_decay else []
    start = 0
    if a.restore:
        ckG, ckD = (torch.load(a.restore + suf, map_location=dev) for suf in ("_G.pth", "_D.pth"))
        st = torch.load(a.restore + "_state.pth", map_location="cpu", weights_only=False)      # RNG states stay host tensors
        if ("G_ema_model" in ckG) != a.ema:
            raise SystemExit("--restore: the checkpoint was written %s --ema" % ("with" if "G_ema_model" in ckG else "without"))
        sd = {"G": ckG["G_model"], "D": ckD["D_model"], "optG": ckG["G_optimizer"], "optD": ckD["D_optimizer"]}
        if a.ema:
            sd["ema"] = {"module": ckG["G_ema_model"], "rate": a.ema_rate, "warmup": a.ema_warmup, "t": ckG["G_optimizer"]["t"]}
        step.load_state_dict(sd)
        if len(st["scheds"]) != len(scheds):
            raise SystemExit("--restore: the checkpoint was written %s --lr_decay" % ("with" if st["scheds"] else "without"))
        for sch, ss in zip(scheds, st["scheds"]):
            sch.load_state_dict(ss)
        data.set_state(st["data"]); smp.set_state(st["sampler"])
        torch.set_rng_state(st["torch_rng"]); torch.cuda.set_rng_state(st["cuda_rng"], dev)
        start, it = st["epoch"] + 1, st["step"]
        print("restored %s: continuing at epoch %d (step %d)" % (a.restore, start, it))
    for epoch in range(start, a.epochs):
        t0 = time.time()
        for real in data:
            info = step.step(x, real, smp.noise_generator(a.bs, compact=True), smp.noise_generator(a.bs, compact=True))
            it += 1
        torch.cuda.synchronize()
        print("epoch %d: %d steps, %.1f shapes/s, lossD %.4f lossG %.4f real_acc %.2f fake_acc %.2f" % (
            epoch, data.num_batches, data.num_batches * a.bs / (time.time() - t0), info["loss_d"].item(), info["loss_g"].item(),
            info["real_acc"].item(), info["fake_acc"].item()))
        tag = os.path.join(a.out, "%d_%s" % (epoch, a.choice))
        for sch in scheds:
            sch.step()
        ckG = {"G_model": G.state_dict(), "G_optimizer": step.optG.state_dict(), "G_epoch": epoch}
        if a.ema:
            step.ema.copy_buffers()                            # the shadow's BatchNorm buffers are G's (spgan.optim.EMA)
            ckG["G_ema_model"] = step.G_ema.state_dict()
        torch.save(ckG, tag + "_G.pth")
        torch.save({"D_model": D.state_dict(), "D_optimizer": step.optD.state_dict(), "D_epoch": epoch}, tag + "_D.pth")
        torch.save({"epoch": epoch, "step": it, "scheds": [sch.state_dict() for sch in scheds], "data": data.get_state(),
                    "sampler": smp.get_state(), "torch_rng": torch.get_rng_state(), "cuda_rng": torch.cuda.get_rng_state(dev)}, tag + "_state.pth")
    gen = G
    if a.ema:
        step.ema.copy_buffers()
        gen = step.G_ema
    gen.eval()
    with torch.no_grad():
        out = gen(x[:4], smp.noise_generator(4))
    for i in range(4):
        save_xyz(os.path.join(a.out, "sample", "%d.xyz" % i), out[i])
    print("wrote %s" % a.out)


if __name__ == "__main__":
    main()
