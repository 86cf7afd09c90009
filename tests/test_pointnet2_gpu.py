"""GPU: PointNet++ set abstraction / feature propagation (spgan.pointnet_util, HIP) against the vectors captured from the reference's
Common/pointnet_util.py:146-320 (golden G22, float32 and float64) and against the model of tests/pointnet2_model.py on odd shapes."""
import re

import numpy as np
import pytest
import torch

import pointnet2_model as pm
from helpers import check_bounded_by_reference_noise as check64, golden

pytestmark = pytest.mark.gpu
FLOOR = 8e-6          # the block tolerance of the other float32-vs-float64 golden checks (tests/test_benchsize_golden_gpu.py)


def _atol(name):
    # a conv bias in front of a train-mode BatchNorm: exactly zero gradient here, rounding noise in the reference
    return 2e-3 if re.search(r"(convs|conv_blocks)[.\d]*\.bias$", name) else 1e-7


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / max(float(b.double().norm()), 1e-30))


@pytest.fixture(scope="module")
def pu():
    from spgan import _lib, pointnet_util
    _lib.load()
    return pointnet_util


@pytest.fixture(scope="module")
def d():
    return golden("g22_pointnet2.npz")


def _module(pu, d, tag):
    kind, cargs, _ = pm.CASES[tag]
    m = getattr(pu, kind)(*cargs)
    m.load_state_dict(pm.case_state_dict(d, tag), strict=True)
    return m.cuda().train()


def _run(pu, d, tag, m):
    names = pm.CASES[tag][2]
    args = [a.cuda().requires_grad_(not n.startswith("xyz_nograd")) for a, n in zip(pm.case_inputs(d, tag), names)]
    kw = {} if tag.startswith("fp") else {"start": torch.from_numpy(d[tag + "|start"]).cuda()}
    outs = m(*args, **kw)
    outs = outs if isinstance(outs, tuple) else (outs,)
    sum((o * torch.from_numpy(d["%s|gout%d" % (tag, i)].astype(np.float32)).cuda()).sum() for i, o in enumerate(outs)).backward()
    return args, outs


# ---------------------------------------------------------------- three_nn / three_interpolate
def test_three_nn_golden(pu, d):
    x1, x2 = [t.transpose(1, 2).contiguous() for t in pm.case_inputs(d, "fp")[:2]]
    idx, w = pu.three_nn(x1.cuda(), x2.cuda())
    assert idx.dtype == torch.int64 and w.dtype == torch.float32
    # every point's 3rd / 4th nearest centre are >= 1e-4 apart and no two of the three nearest tie (asserted at capture): equality is well-defined
    assert np.array_equal(idx.cpu().numpy(), d["fp|nn_idx"].astype(np.int64))
    d32 = torch.from_numpy(d["fp|nn_dist4"][..., :3])
    r32 = 1.0 / (d32 + 1e-8)
    w32 = r32 / r32.sum(-1, keepdim=True)                                  # the reference's float32 weights (:305-307)
    _, w64, _ = pm.three_nn(x1.double(), x2.double())
    e_ref, e_own = _rel(w32, w64), _rel(w, w64)
    print("three_nn weights vs float64: own %.3e, reference float32 %.3e" % (e_own, e_ref))
    assert e_own <= max(1.5 * e_ref, FLOOR)
    # coincident points (xyz2 is an FPS subset of xyz1) get the reference's distances, hence its weights: bit for bit where the
    # float32 distances agree
    same = (w.cpu() == w32)
    print("three_nn weights bit-identical to the reference's float32: %.4f" % same.float().mean().item())


@pytest.mark.parametrize("B,N,S", [(2, 300, 77), (1, 1000, 513), (3, 65, 1), (3, 65, 2), (2, 257, 3)])
def test_three_nn_odd_shapes_vs_model(pu, B, N, S):
    g = torch.Generator().manual_seed(N + S)
    x1, x2 = torch.rand(B, N, 3, generator=g), torch.rand(B, S, 3, generator=g)
    idx, w = pu.three_nn(x1.cuda(), x2.cuda())
    ridx, rw, ds = pm.three_nn(x1.double(), x2.double())
    k = min(3, S)
    assert tuple(idx.shape) == (B, N, k)
    # tie-aware: a point whose k-th / (k+1)-th (or any two of its k nearest) centres are closer than float32 resolves may differ
    d = pm.sqdist(x1.double(), x2.double()).sort(-1)[0]
    gaps = (d[..., 1:min(S, 4)] - d[..., :min(S, 4) - 1]) if S > 1 else torch.ones(B, N, 1, dtype=torch.float64)
    clear = (gaps > 1e-5).all(-1) if S > 1 else torch.ones(B, N, dtype=torch.bool)
    assert clear.float().mean() > 0.95
    assert torch.equal(idx.cpu()[clear], ridx[clear])
    assert _rel(w.cpu()[clear], rw[clear]) < 1e-4
    assert torch.allclose(w.sum(-1).cpu(), torch.ones(B, N), atol=1e-5)


@pytest.mark.parametrize("D", [1, 3, 67])
def test_three_interpolate_forward_backward_vs_autograd(pu, D):
    B, N, S = 2, 333, 45
    g = torch.Generator().manual_seed(D)
    x1, x2 = torch.rand(B, N, 3, generator=g), torch.rand(B, S, 3, generator=g)
    p2 = torch.randn(B, S, D, generator=g)
    gout = torch.randn(B, N, D, generator=g)
    idx, w = pu.three_nn(x1.cuda(), x2.cuda())
    pg = p2.cuda().requires_grad_(True)
    out = pu.three_interpolate(pg, idx, w)
    (out * gout.cuda()).sum().backward()
    pr = p2.double().requires_grad_(True)
    ref = pm.three_interpolate(pr, idx.cpu(), w.cpu().double())
    (ref * gout.double()).sum().backward()
    assert _rel(out.detach(), ref.detach()) < 2e-7 and _rel(pg.grad, pr.grad) < 1e-6
    g1 = pg.grad.clone(); pg.grad = None
    (pu.three_interpolate(pg, idx, w) * gout.cuda()).sum().backward()
    assert torch.equal(g1, pg.grad)                                        # slot lists, no float atomics


@pytest.mark.parametrize("K", [8, 32, 128])
def test_group_max_and_backward_vs_torch(pu, K):
    Q, C = 37, 67
    g = torch.Generator().manual_seed(K)
    y = torch.randn(Q * K, C, generator=g)
    sc, sh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    mean, inv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    gpool = torch.randn(Q, C, generator=g)
    pooled, arg = pu._group_max(y.cuda(), Q, K, sc.cuda(), sh.cuda(), 0.0)
    z = torch.relu(y * sc + sh).view(Q, K, C)
    ref, rarg = z.max(1)
    # the kernel evaluates y*scale + shift as one fused multiply-add, torch in two roundings: one float32 ulp of |y*scale| <= 4.5 * 2^-23
    assert torch.allclose(pooled.cpu(), ref, rtol=0, atol=1e-6) and arg.dtype == torch.int32
    assert torch.allclose(torch.gather(z, 1, (arg.cpu().long() - torch.arange(Q).view(Q, 1) * K).unsqueeze(1)).squeeze(1), ref, rtol=0, atol=1e-6)
    gd, sums = pu._group_max_bwd(gpool.cuda(), pooled, arg, y.cuda(), mean.cuda(), inv.cuda(), 0.0, K)
    gv = gpool * (pooled.cpu() > 0)
    dense = torch.zeros(Q * K, C).scatter_(0, arg.cpu().long(), gv)
    assert torch.equal(gd.cpu(), dense)
    xh = (y - mean) * inv
    s0, s1 = dense.double().sum(0), (dense.double() * xh.double()).sum(0)
    assert _rel(sums[:C], s0) < 1e-5 and _rel(sums[C:], s1) < 1e-5


# ---------------------------------------------------------------- the modules against the reference
@pytest.mark.parametrize("tag", sorted(pm.CASES))
def test_module_train_mode_golden(pu, d, tag):
    m = _module(pu, d, tag)
    args, outs = _run(pu, d, tag, m)
    for i, o in enumerate(outs):
        check64(d, "%s|out%d" % (tag, i), "%s|out%d|f64" % (tag, i), o, floor=FLOOR, atol=1e-7)
    for k, p in m.named_parameters():
        check64(d, "%s|grad|%s" % (tag, k), "%s|grad|%s|f64" % (tag, k), p.grad, floor=FLOOR, atol=_atol(k))
    for a, n in zip(args, pm.CASES[tag][2]):
        if not n.startswith("xyz_nograd"):
            check64(d, "%s|gin|%s" % (tag, n), "%s|gin|%s|f64" % (tag, n), a.grad, floor=FLOOR, atol=1e-7)
    for k, v in m.named_buffers():
        if v.is_floating_point():
            check64(d, "%s|buf|%s" % (tag, k), "%s|buf|%s|f64" % (tag, k), v, floor=FLOOR)
        else:
            assert int(v) == int(d["%s|buf|%s" % (tag, k)]) == 1, k


@pytest.mark.parametrize("tag", sorted(pm.CASES))
def test_module_eval_mode_uses_running_statistics(pu, d, tag):
    m = _module(pu, d, tag)
    _run(pu, d, tag, m)
    m.eval()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    args = [a.cuda() for a in pm.case_inputs(d, tag)]
    kw = {} if tag.startswith("fp") else {"start": torch.from_numpy(d[tag + "|start"]).cuda()}
    with torch.no_grad():
        outs = m(*args, **kw)
    outs = outs if isinstance(outs, tuple) else (outs,)
    refs, _, _ = pm.run_model(d, tag, {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()},
                              [a.double() for a in pm.case_inputs(d, tag)], training=False)
    for o, r in zip(outs, refs):
        assert _rel(o, r) < 2e-6
    after = m.state_dict()
    assert all(torch.equal(after[k].cpu(), sd[k]) for k in sd)            # eval leaves every buffer (num_batches_tracked included) alone
    assert all(int(v) == 1 for k, v in after.items() if k.endswith("num_batches_tracked"))


@pytest.mark.parametrize("tag", ["sa", "msg", "fp"])
def test_two_identical_calls_are_bit_identical(pu, d, tag):
    res = []
    for _ in range(2):
        m = _module(pu, d, tag)
        args, outs = _run(pu, d, tag, m)
        res.append([o.detach() for o in outs] + [p.grad for p in m.parameters()] + [a.grad for a in args if a.grad is not None])
    assert len(res[0]) == len(res[1]) and all(torch.equal(a, b) for a, b in zip(*res))


def test_refusals(pu, d):
    fp = _module(pu, d, "fp")
    a = [t.cuda() for t in pm.case_inputs(d, "fp")]
    with pytest.raises(NotImplementedError, match="xyz1"):
        fp(a[0].clone().requires_grad_(True), a[1], a[2], a[3])
    with pytest.raises(NotImplementedError):
        fp(a[0], a[1].clone().requires_grad_(True), a[2], a[3])
    with pytest.raises(RuntimeError, match="no CPU"):
        fp(*pm.case_inputs(d, "fp"))
    with pytest.raises(RuntimeError, match="no CPU"):
        _module(pu, d, "sa")(*pm.case_inputs(d, "sa"))


def test_stack_inside_captured_body_equals_eager(pu):
    """SA -> SA -> FP -> FP, forward + backward, captured as one graph and replayed twice: bit-identical to the eager result."""
    import spgan
    B, N = 2, 256
    g = torch.Generator().manual_seed(5)
    xyz = torch.rand(B, 3, N, generator=g).cuda()
    feat = torch.randn(B, 4, N, generator=g).cuda()
    s1, s2 = torch.tensor([3, 7]).cuda(), torch.tensor([1, 2]).cuda()

    def build():
        torch.manual_seed(9)
        return torch.nn.ModuleList([pu.PointNetSetAbstraction(64, 0.25, 16, 7, [16, 32], False),
                                    pu.PointNetSetAbstraction(16, 0.5, 8, 35, [32, 64], False),
                                    pu.PointNetFeaturePropagation(96, [32]), pu.PointNetFeaturePropagation(36, [16, 8])]).cuda().train()

    def body_of(net):
        def body(x, f):
            for p in net.parameters():
                p.grad = None
            x1, f1 = net[0](x, f, start=s1)
            x2, f2 = net[1](x1, f1, start=s2)
            u1 = net[2](x1.detach(), x2.detach(), f1, f2)
            u0 = net[3](x.detach(), x1.detach(), f, u1)
            (u0 * u0).mean().backward()
            return (u0.detach(),) + tuple(p.grad for p in net.parameters())
        return body

    eager_net = build()
    eager = [t.clone() for t in body_of(eager_net)(xyz, feat.clone().requires_grad_(False))]
    net = build()
    cb = spgan.CapturedBody(body_of(net), modules=(net,), warmup=1)
    outs = None
    for _ in range(4):                      # 1 eager warm-up, 1 capture, 2 replays: same inputs, parameters untouched -> same result
        outs = [t.clone() for t in cb(xyz, feat)]
    torch.cuda.synchronize()
    assert not cb.eager, "the capture fell back to eager issue"
    assert len(outs) == len(eager) and all(torch.equal(a, b) for a, b in zip(outs, eager))
