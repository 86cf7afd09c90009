"""GPU: the generator EMA fused into G's Adam launch (spgan_adam_ema_step_dev / spgan_adam_ema_step / spgan_ema_update_dev) and the
bit-exact resume of a TrainStep.

  * the fused kernels leave p, m, v, g bit-identical to the plain Adam entry points; the three entry points produce bit-equal shadows;
    the shadow follows G22 (the reference's accumulate / exp_mov_avg, Common/network_utils.py:97-108) within 2 ulp per step;
  * TrainStep(ema_rate=...): graph replay == eager; G, D and both optimisers == the run without EMA; the shadow's host-side weight
    caches follow the replayed updates (all three operand modes);
  * resume: k steps + state_dict -> fresh objects -> load_state_dict -> k steps == 2k steps, bit for bit (in process, graph mode, and
    across processes through examples/train.py --restore);
  * data parallel: every rank's shadow is bit-identical without communication."""
import os
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

from helpers import golden
from oracle import spgan_oracle as orc
from spgan import fixture_rng as fr
from test_ema_cpu import ema_ulps
from test_parity_gpu import Opts, _load, sp  # noqa: F401  (sp is a fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G_FLAT = 585156          # the generator's flat buffer (2.34 MB)


def _bufs(n, tag, off=0):
    """p, g, m, v, e of n elements (starting `off` floats into their allocations: off = 1 takes the unaligned path)."""
    def mk(name, scale=1.0, pos=False):
        t = fr.normal("%s.%s" % (tag, name), (n + off,)) * scale
        return (t.abs() if pos else t).cuda()[off:]
    return dict(p=mk("p", 0.05), g=mk("g", 1e-2), m=mk("m", 1e-3), v=mk("v", 1e-5, pos=True), e=mk("e", 0.05))


@pytest.mark.parametrize("n,off", [(4, 0), (1000, 0), (1001, 1), (G_FLAT, 0)])
@pytest.mark.parametrize("warmup", [True, False])
def test_fused_adam_ema_bit_identical(sp, n, off, warmup):
    rate = 0.999
    base = _bufs(n, "emak%d" % n, off)
    plain = {k: v.clone() for k, v in base.items()}
    fused = {k: v.clone() for k, v in base.items()}
    host_plain = {k: v.clone() for k, v in base.items()}
    host_fused = {k: v.clone() for k, v in base.items()}
    alone_e = base["e"].clone()
    st_plain = torch.tensor([0.0, 0.0, 0.0, 1.0], device="cuda")
    st_fused = st_plain.clone()
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    for t in range(1, 4):
        gs = fr.normal("emak%d.gstep%d" % (n, t), (n,)).cuda() * 1e-2
        for d in (plain, fused, host_plain, host_fused):
            d["g"].copy_(gs)
        zg = t != 2
        sp.ops.adam_step_dev(plain["p"], plain["g"], plain["m"], plain["v"], st_plain, 1e-4, 0.5, 0.99, 1e-8, 0.5, zero_grad=zg)
        sp.ops.adam_ema_step_dev(fused["p"], fused["g"], fused["m"], fused["v"], fused["e"], st_fused, 1e-4, 0.5, 0.99, 1e-8, 0.5,
                                 zero_grad=zg, ema_rate=rate, ema_warmup=warmup)
        sp.ops.adam_step(host_plain["p"], host_plain["g"], host_plain["m"], host_plain["v"], t, 1e-4, 0.5, 0.99, 1e-8, 0.5)
        sp.ops.adam_ema_step(host_fused["p"], host_fused["g"], host_fused["m"], host_fused["v"], host_fused["e"], t, 1e-4, 0.5, 0.99,
                             1e-8, 0.5, ema_rate=rate, ema_warmup=warmup)
        sp.ops.ema_update_dev(alone_e, plain["p"], counter, ema_rate=rate, ema_warmup=warmup)
        torch.cuda.synchronize()
        for k in ("p", "g", "m", "v"):
            assert torch.equal(plain[k], fused[k]), (t, k)
        for k in ("p", "m", "v"):
            assert torch.equal(host_plain[k], host_fused[k]), (t, k)
        assert torch.equal(st_plain, st_fused)
        assert torch.equal(fused["e"], alone_e), t
        assert torch.equal(host_fused["e"], fused["e"]), t         # same t, same p (host and dev Adam agree here), same e
        if warmup and t == 1:
            assert torch.equal(fused["e"], fused["p"])             # exp_mov_avg at global_step 0: a copy
    assert int(counter.item()) == 3 and int(st_fused[:1].view(torch.int32).item()) == 3


@pytest.mark.parametrize("rule", ["acc", "ema"])
def test_ema_kernels_against_g22(sp, rule):
    d = golden("g22_ema.npz")
    warm, rate = rule == "ema", float(d["rate"])
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    prev = d["e0"]
    for t in range(1, d[rule].shape[0] + 1):
        e = torch.from_numpy(prev.copy()).cuda()
        p = torch.from_numpy(d["p"][t].copy()).cuda()
        sp.ops.ema_update_dev(e, p, counter, ema_rate=rate, ema_warmup=warm)
        ref = d[rule][t - 1]
        err = ema_ulps(e.cpu().numpy(), ref, prev, d["p"][t], t, rate, warm)
        assert err.max() <= 2.0, (rule, t, float(err.max()))
        if warm and t == 1:
            assert torch.equal(e, p)
        prev = ref


def _make(sp, ema_rate, graph, salt=8, warmup=True):
    o = Opts()
    G = _load(sp.Generator(o), fr.init_params(orc.generator_shapes(), salt=salt))
    D = _load(sp.Discriminator(o), fr.init_params(orc.discriminator_shapes(), salt=salt))
    return sp.TrainStep(G, D, gan="wgan", use_gp=True, lambda_gp=10.0, graph=graph, graph_warmup=2, ema_rate=ema_rate, ema_warmup=warmup)


def _steps(tr, first, count, B=4, N=256):
    x = _steps.__dict__.setdefault("x", fr.sphere_template(N)[None].repeat(B, 1, 1).cuda())
    for i in range(first, first + count):
        tr.step(x, fr.synthetic_real(B, N, seed=90 + i % 3).cuda(), fr.latent(B, N, seed=70 + i % 4).cuda(),
                fr.latent(B, N, seed=71 + i % 4).cuda(), alpha=fr.uniform("emag.alpha%d" % (i % 2), (B, 1, 1), 0.0, 1.0).cuda())
    torch.cuda.synchronize()


def _assert_same(a, b, what=""):
    """torch.equal over nested state dicts."""
    assert set(a) == set(b), what
    for k in a:
        if isinstance(a[k], dict):
            _assert_same(a[k], b[k], "%s.%s" % (what, k))
        elif isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), "%s.%s" % (what, k)
        else:
            assert a[k] == b[k], "%s.%s" % (what, k)


def test_trainstep_ema_graph_equals_eager_and_leaves_training_unchanged(sp):
    steps = 6
    eager, graph, plain = _make(sp, 0.999, False), _make(sp, 0.999, True), _make(sp, None, True)
    for tr in (eager, graph, plain):
        _steps(tr, 0, steps)
    assert graph._graph is not None and plain._graph is not None
    se, sg, sp_ = eager.state_dict(), graph.state_dict(), plain.state_dict()
    _assert_same(se, sg, "eager vs graph")
    assert graph.ema.t == steps
    del sg["ema"]
    _assert_same(sg, sp_, "with vs without EMA")
    assert not torch.equal(graph.ema.fp.flat, graph.optG.fp.flat)
    # rate 0.999 after 6 warm-up steps: a = 5/6 -- the shadow lags G but lies within its range of motion
    assert float((graph.ema.fp.flat - graph.optG.fp.flat).abs().max()) < 6e-4


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "f16"])
def test_ema_generator_weight_caches_follow_replayed_updates(sp, mode):
    """An eval forward of G_ema fills its weight-derived host caches; after further replayed steps (the shadow updated by the captured
    Adam launch) the same forward must equal a fresh Generator loaded from G_ema.state_dict()."""
    sp.ops.set_mfma_operands(mode)
    try:
        tr = _make(sp, 0.99, True)
        B, N = 4, 256
        x = fr.sphere_template(N)[None].repeat(B, 1, 1).cuda()
        z = fr.latent(B, N, seed=5).cuda()
        _steps(tr, 0, 4)
        tr.ema.copy_buffers()
        tr.G_ema.eval()
        with torch.no_grad():
            tr.G_ema(x, z)                                        # caches of the shadow's current weights
        _steps(tr, 4, 3)
        assert tr._graph is not None
        tr.ema.copy_buffers()
        with torch.no_grad():
            got = tr.G_ema(x, z).clone()
        fresh = sp.Generator(Opts()).cuda()
        fresh.load_state_dict(tr.G_ema.state_dict())
        fresh.eval()
        with torch.no_grad():
            ref = fresh(x, z)
        torch.cuda.synchronize()
        assert torch.equal(got, ref), float((got - ref).abs().max())
    finally:
        sp.ops.set_mfma_operands("f32")


def test_resume_in_process_graph_mode(sp):
    k = 5
    full = _make(sp, 0.999, True)
    _steps(full, 0, 2 * k)
    half = _make(sp, 0.999, True)
    _steps(half, 0, k)
    sd = half.state_dict()
    del half
    resumed = _make(sp, 0.999, True, salt=3)                       # different weights: replaced by the load
    _steps(resumed, 0, 3)                                          # ... and already captured: the load must keep its graph valid
    assert resumed._graph is not None
    graph_before = resumed._graph
    resumed.load_state_dict(sd)
    _steps(resumed, k, k)
    assert resumed._graph is graph_before
    a, b = full.state_dict(), resumed.state_dict()
    _assert_same(a, b, "2k vs k + resume + k")
    assert b["optG"]["t"] == b["optD"]["t"] == 2 * k and b["ema"]["t"] == 2 * k
    assert int(b["G"]["global_conv.1.num_batches_tracked"]) == int(a["G"]["global_conv.1.num_batches_tracked"]) > 0


def _run_example(out, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), "--synthetic", "64", "--np", "256", "--bs", "8",
                        "--gan", "wgan", "--gp", "--ema", "--out", out] + list(extra), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_example_restore_continues_bit_exactly(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _run_example(a, "--epochs", "2")
    _run_example(b, "--epochs", "1")
    log = _run_example(b, "--epochs", "2", "--restore", os.path.join(b, "0_chair"))
    assert "continuing at epoch 1" in log and "epoch 0:" not in log
    for suf in ("_G.pth", "_D.pth"):
        ca, cb = (torch.load(os.path.join(d, "1_chair" + suf), weights_only=False) for d in (a, b))
        _assert_same(ca, cb, suf)
    ck = torch.load(os.path.join(a, "1_chair_G.pth"), weights_only=False)
    assert set(ck) == {"G_model", "G_optimizer", "G_epoch", "G_ema_model"} and ck["G_optimizer"]["t"] == 16
    assert not torch.equal(ck["G_model"]["tail.4.weight"], ck["G_ema_model"]["tail.4.weight"])


def _dp_worker(rank, world, port, out):
    import test_dp_gpu as dpg
    dpg._setup_paths()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    import spgan
    from spgan import _lib
    _lib.load()
    torch.cuda.set_device(0)
    assert spgan.init_process_group_from_env("gloo") == rank
    G, D = dpg._models(100 + rank)                                  # different initial weights: sync_params() makes them rank 0's
    tr = spgan.TrainStep(G, D, gan="wgan", use_gp=True, distributed=True, graph=True, graph_warmup=2, ema_rate=0.99)
    x = spgan.shard_batch(dpg._inputs(0)[0], rank, world).contiguous().cuda()
    for s in range(4):
        _, real, z_d, z_g, alpha = [spgan.shard_batch(t, rank, world).contiguous().cuda() for t in dpg._inputs(s)]
        tr.step(x, real, z_d, z_g, alpha=alpha)
    torch.cuda.synchronize()
    torch.save({"ema": tr.ema.fp.flat.cpu(), "G": tr.optG.fp.flat.cpu(), "replayed": tr._graph is not None and tr.use_graph},
               os.path.join(out, "r%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_keep_identical_shadows(tmp_path):
    import test_dp_gpu as dpg
    mp.spawn(_dp_worker, args=(2, dpg._free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / ("r%d.pt" % r)) for r in range(2))
    assert r0["replayed"] and r1["replayed"]
    assert torch.equal(r0["G"], r1["G"]) and torch.equal(r0["ema"], r1["ema"])
    assert not torch.equal(r0["ema"], r0["G"])
