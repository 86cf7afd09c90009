"""CPU: the generator EMA and the resume state (spgan.optim.EMA, Adam.attach_ema, StepLR / sampler / dataset state, TrainStep(ema_rate=...)
state_dict) over the kernel models plus the CPU doubles of the EMA ops (tests/ema_model.py), pinned against G22 -- the reference's
`accumulate` / `exp_mov_avg` (Common/network_utils.py:97-108) run over a fixed parameter trajectory (tests/golden/make_golden_ema.py)."""
import numpy as np
import pytest
import torch

import ema_model
from helpers import golden
from oracle import spgan_oracle as orc
from spgan import fixture_rng as fr
from test_host_cpu import Opts, spgan_cpu, _load   # noqa: F401  (fixture import)


@pytest.fixture()
def spgan_ema_cpu(spgan_cpu, monkeypatch):
    ema_model.install(monkeypatch)
    return spgan_cpu


def ulp32(x):
    x = np.abs(np.asarray(x, np.float32))
    return np.spacing(np.maximum(x, np.float32(1e-30)))


def ema_ulps(got, ref, prev, p, t, rate, warmup):
    """|got - ref| in float32 ulps of the update's largest operand (result, a*e, (1-a)*p): the terms cancel where e ~ -p/a."""
    a, b = ema_model.coef(t, rate, warmup)
    scale = np.maximum(np.abs(ref), np.maximum(a * np.abs(prev), b * np.abs(p)))
    return np.abs(np.asarray(got, np.float64) - ref) / ulp32(scale)


@pytest.mark.parametrize("rule", ["acc", "ema"])
def test_cpu_double_against_g22(rule):
    """One update per step from the reference's previous shadow: the double's rounding stays within 2 ulp of the reference's float32
    helpers, every step."""
    d = golden("g22_ema.npz")
    warm = rule == "ema"
    prev = torch.from_numpy(d["e0"].copy())
    for t in range(1, d[rule].shape[0] + 1):
        e = prev.clone()
        ema_model.ema_apply(e, torch.from_numpy(d["p"][t]), t, float(d["rate"]), warm)
        ref = d[rule][t - 1]
        err = ema_ulps(e.numpy(), ref, prev.numpy(), d["p"][t], t, float(d["rate"]), warm)
        assert err.max() <= 2.0, (rule, t, float(err.max()))
        if warm and t == 1:
            assert np.array_equal(e.numpy(), d["p"][1])          # exp_mov_avg at global_step 0 copies p
        prev = torch.from_numpy(ref.copy())


def test_ema_coefficient():
    assert ema_model.coef(1, 0.999, True) == (0.0, 1.0)
    assert ema_model.coef(2, 0.999, True) == (0.5, 0.5)
    a, _ = ema_model.coef(10 ** 6, 0.999, True)
    assert a == float(np.float32(0.999)) and ema_model.coef(1, 0.999, False)[0] == a


def _gen(salt=8):
    import spgan
    return _load(spgan.Generator(Opts), fr.init_params(orc.generator_shapes(), salt=salt))


def test_ema_module_layout_and_state_round_trip(spgan_ema_cpu):
    import spgan
    G = _gen()
    ema = spgan.EMA(G, rate=0.9, warmup=False)
    assert ema.fp.offsets == spgan.flatten_module(G).offsets
    assert isinstance(ema.module, spgan.Generator) and not any(p.requires_grad for p in ema.module.parameters())
    for (n, a), (n2, b) in zip(G.named_parameters(), ema.module.named_parameters()):
        assert n == n2 and torch.equal(a, b) and a.data_ptr() != b.data_ptr()
    for s in range(3):
        with torch.no_grad():
            for i, p in enumerate(G.parameters()):                 # in place: the flat buffer's padding stays zero, as under Adam
                p.add_(fr.normal("ema.rt%d.%d" % (s, i), tuple(p.shape)) * 1e-2)
        ema.update()
    assert ema.t == 3 and int(ema.counter.item()) == 3
    with torch.no_grad():
        G.global_conv[1].running_mean.add_(1.0)
    ema.copy_buffers()
    assert torch.equal(ema.module.global_conv[1].running_mean, G.global_conv[1].running_mean)
    sd = ema.state_dict()
    ema2 = spgan.EMA(_gen(salt=9), rate=0.5, warmup=True)
    flat_ptr = ema2.fp.flat.data_ptr()
    ema2.load_state_dict(sd)
    assert ema2.fp.flat.data_ptr() == flat_ptr                   # copied into the same buffer
    assert (ema2.rate, ema2.warmup, ema2.t, int(ema2.counter.item())) == (0.9, False, 3, 3)
    assert torch.equal(ema2.fp.flat, ema.fp.flat)
    for k, v in ema.module.state_dict().items():
        assert torch.equal(v, ema2.module.state_dict()[k]), k
    # the next update continues identically
    ema.update(); ema2.source = ema.source; ema2.src = ema.src; ema2.update()
    assert torch.equal(ema2.fp.flat, ema.fp.flat)


def test_steplr_state(spgan_ema_cpu):
    import spgan
    G = _gen()
    opt = spgan.Adam(G, lr=1e-3)
    sch = spgan.StepLR(opt, step_size=2, gamma=0.5)
    for _ in range(5):
        sch.step()
    opt2 = spgan.Adam(_gen(salt=9), lr=1e-3)
    sch2 = spgan.StepLR(opt2, step_size=7, gamma=0.9)
    sch2.load_state_dict(sch.state_dict())
    assert sch2.last_epoch == 5 and sch2.get_last_lr() == sch.get_last_lr() == [1e-3 * 0.25]
    sch.step(); sch2.step()
    assert sch2.get_last_lr() == sch.get_last_lr() == [1e-3 * 0.125]


def test_sampler_and_dataset_rng_state():
    from spgan import dataset, sampling

    class O:
        np = 256; nz = 8; nv = 0.2; n_rand = False; n_mix = False
    src = fr.synthetic_real(20, 64, seed=5)
    for make in (lambda seed: dataset.DeviceDataset(src, num_points=64, batch_size=4, augment=True, device="cpu", seed=seed),
                 lambda seed: dataset.HostStagedLoader(src.numpy(), num_points=64, batch_size=4, augment=True, device="cpu", seed=seed)):
        a = make(3)
        for _ in a:
            pass
        st = a.get_state()
        assert st["epoch"] == 1
        b = make(4)
        b.set_state(st)
        assert b.epoch == 1
        xs, ys = [t.clone() for t in a], [t.clone() for t in b]
        assert len(xs) == len(ys) == 5 and all(torch.equal(x, y) for x, y in zip(xs, ys))
        assert a.epoch == b.epoch == 2
    s1 = sampling.InputSampler(O, device="cpu", seed=1)
    s1.noise_generator(3)
    st = s1.get_state()
    s2 = sampling.InputSampler(O, device="cpu", seed=2)
    s2.set_state(st)
    assert torch.equal(s1.noise_generator(3, compact=True), s2.noise_generator(3, compact=True))
    assert torch.equal(s1.sphere_generator(2, static=False), s2.sphere_generator(2, static=False))


def _train(ema_rate, warmup=True, steps=3, B=2, N=256):
    import spgan
    G = _gen()
    D = _load(spgan.Discriminator(Opts), fr.init_params(orc.discriminator_shapes(), salt=8))
    tr = spgan.TrainStep(G, D, gan="wgan", use_gp=True, ema_rate=ema_rate, ema_warmup=warmup)
    x = fr.sphere_template(N)[None].repeat(B, 1, 1)
    traj = [tr.optG.fp.flat.clone().double()]
    for s in range(steps):
        tr.step(x, fr.synthetic_real(B, N, seed=90 + s), fr.latent(B, N, seed=100 + s), fr.latent(B, N, seed=110 + s),
                alpha=fr.uniform("ema.alpha%d" % s, (B, 1, 1), 0.0, 1.0))
        traj.append(tr.optG.fp.flat.clone().double())
    return tr, traj


@pytest.mark.parametrize("warmup", [True, False])
def test_trainstep_ema_equals_float64_replay(spgan_ema_cpu, warmup):
    """Eager TrainStep(ema_rate=...): G_ema == the rule replayed in float64 over G's recorded parameters; G, D and both optimisers are
    bit-identical to the run without EMA."""
    rate = 0.9
    tr, traj = _train(rate, warmup)
    assert tr.G_ema is tr.ema.module and tr.ema.t == 3
    e = traj[0].clone()
    for t in range(1, len(traj)):
        a = min(1.0 - 1.0 / t, rate) if warmup else rate
        e = a * e + (1.0 - a) * traj[t]
    got = tr.ema.fp.flat.double()
    assert float((got - e).abs().max()) <= 4 * 2.0 ** -24 * float(e.abs().max()) + 1e-12
    ref, _ = _train(None)
    assert ref.G_ema is None
    for a_, b_ in ((tr.G, ref.G), (tr.D, ref.D)):
        for k, v in a_.state_dict().items():
            assert torch.equal(v, b_.state_dict()[k]), k
    for o, r in ((tr.optG, ref.optG), (tr.optD, ref.optD)):
        assert torch.equal(o.m, r.m) and torch.equal(o.v, r.v) and o.t == r.t


def test_trainstep_state_dict_resume(spgan_ema_cpu):
    """2 eager steps == 1 step, state_dict -> fresh TrainStep -> load_state_dict -> 1 step (G, D, G_ema, both Adams, BN buffers)."""
    import spgan
    full, _ = _train(0.999, steps=2)
    half, _ = _train(0.999, steps=1)
    sd = half.state_dict()
    G = _gen(salt=3)
    D = _load(spgan.Discriminator(Opts), fr.init_params(orc.discriminator_shapes(), salt=3))
    tr = spgan.TrainStep(G, D, gan="wgan", use_gp=True, ema_rate=0.5, ema_warmup=False)
    tr.load_state_dict(sd)
    assert tr.ema.rate == 0.999 and tr.ema.warmup and tr.ema.t == 1
    B, N, s = 2, 256, 1
    x = fr.sphere_template(N)[None].repeat(B, 1, 1)
    tr.step(x, fr.synthetic_real(B, N, seed=90 + s), fr.latent(B, N, seed=100 + s), fr.latent(B, N, seed=110 + s),
            alpha=fr.uniform("ema.alpha%d" % s, (B, 1, 1), 0.0, 1.0))
    a, b = full.state_dict(), tr.state_dict()
    for part in ("G", "D"):
        for k, v in a[part].items():
            assert torch.equal(v, b[part][k]), (part, k)
    for k, v in a["ema"]["module"].items():
        if k in dict(full.G_ema.named_parameters()):
            assert torch.equal(v, b["ema"]["module"][k]), k
    for part in ("optG", "optD"):
        for k in ("m", "v"):
            assert torch.equal(a[part][k], b[part][k]), (part, k)
        assert a[part]["t"] == b[part]["t"] == 2 and a[part]["lr"] == b[part]["lr"]
    with pytest.raises(ValueError, match="EMA"):
        _train(None, steps=0)[0].load_state_dict(sd)
