"""GPU: spgan.pointconv_util (HIP) against the vectors captured from the reference's Common/pointconv_util.py (golden G24, float32 and
float64) and the kernels of csrc/pointconv.hip against the models of tests/pointconv_model.py on small and awkward sizes.

Tolerance rule for G24 (tests/test_pointnet2_gpu.py's): the build's rel-L2 error against the reference's float64 result may not exceed
1.5 x the reference's own float32 error against it (floor 8e-6); a conv / linear bias in front of a train-mode BatchNorm has an
exactly zero gradient here and rounding noise in the reference, hence the absolute bound 2e-3 for those.  The kernel-vs-model
bounds are those of float32 arithmetic on sums of K (or C) well-conditioned terms against a float64 model: 2e-6 forward, 1e-5 for
gradients; the kernel density is ill-conditioned in h and is bounded by the float32 model's own error instead (see its test)."""
import re

import numpy as np
import pytest
import torch

import pointconv_model as pcm
from helpers import check_bounded_by_reference_noise as check64, golden

pytestmark = pytest.mark.gpu
FLOOR = 8e-6


def _atol(name):
    return 2e-3 if re.search(r"(convs[.\d]*|(^|\.)linear)\.bias$", name) else 1e-7


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / max(float(b.double().norm()), 1e-30))


@pytest.fixture(scope="module")
def pc():
    from spgan import _lib, pointconv_util
    _lib.load()
    return pointconv_util


@pytest.fixture(scope="module")
def d():
    return golden("g24_pointconv.npz")


def _module(pc, d, tag):
    kind, cargs, _ = pcm.CASES[tag]
    m = getattr(pc, kind)(*cargs)
    m.load_state_dict(pcm.case_state_dict(d, tag), strict=True)
    return m.cuda().train()


def _run(pc, d, tag, m):
    args = [None if a is None else a.cuda().requires_grad_(True) for a in pcm.case_inputs(d, tag)]
    outs = m(*args)
    sum((o * torch.from_numpy(d["%s|gout%d" % (tag, i)].astype(np.float32)).cuda()).sum() for i, o in enumerate(outs)).backward()
    return args, outs


# ---------------------------------------------------------------- the narrow layers on the generic GEMM path
@pytest.mark.parametrize("cin,cout", [(1, 16), (16, 8), (8, 1), (3, 8), (8, 8), (8, 16)])
def test_narrow_layers_on_the_generic_gemm_path(cin, cout):
    """Input widths 1, 3, 8, 16 and output widths 1, 8, 16 at many rows: the DensityNet / WeightNet layer shapes on ops.gemm_nt (with the
    fused train-mode BatchNorm), ops.gemm_tn and ops.gemm_nt_bnbwd."""
    from spgan import ops
    M = 2 * 64 * 16 + 5
    g = torch.Generator().manual_seed(cin * 100 + cout)
    A, W, b = torch.randn(M, cin, generator=g), torch.randn(cout, cin, generator=g) * 0.5, torch.randn(cout, generator=g)
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    rm, rv = torch.zeros(cout).cuda(), torch.ones(cout).cuda()
    y, (sc, sh, inv, mu) = ops.gemm_nt(A.cuda(), W.cuda(), b.cuda(), bn=(gamma.cuda(), beta.cuda(), rm, rv))
    y64 = A.double() @ W.double().t() + b.double()
    assert _rel(y, y64) < 2e-6
    assert _rel(mu, y64.mean(0)) < 1e-5 and _rel(inv, 1.0 / torch.sqrt(y64.var(0, unbiased=False) + 1e-5)) < 1e-5
    assert _rel(rm, 0.1 * y64.mean(0)) < 1e-5
    psc, psh = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.1
    y2 = ops.gemm_nt(A.cuda(), W.cuda(), b.cuda(), pro=(psc.cuda(), psh.cuda(), 0.0))
    a64 = torch.relu(A.double() * psc.double() + psh.double())
    assert _rel(y2, a64 @ W.double().t() + b.double()) < 2e-6
    dy = torch.randn(M, cout, generator=g)
    assert _rel(ops.gemm_tn(dy.cuda(), A.cuda()), dy.double().t() @ A.double()) < 1e-5
    assert _rel(ops.gemm_tn(dy.cuda(), A.cuda(), pro=(psc.cuda(), psh.cuda(), 0.0)), dy.double().t() @ a64) < 1e-5
    pmu, pinv = torch.randn(cin, generator=g) * 0.1, torch.rand(cin, generator=g) + 0.5
    gg, s0, s1 = ops.gemm_nt_bnbwd(dy.cuda(), W.t().contiguous().cuda(), A.cuda(), psc.cuda(), psh.cuda(), pmu.cuda(), pinv.cuda(), 0.0)
    g64 = (dy.double() @ W.double()) * ((A.double() * psc.double() + psh.double()) > 0)
    assert _rel(gg, g64) < 2e-6
    assert _rel(s0, g64.sum(0)) < 1e-5 and _rel(s1, (g64 * ((A.double() - pmu.double()) * pinv.double())).sum(0)) < 1e-5


# ---------------------------------------------------------------- kernels against their models
def _kde_model(x, h, gd, gi, dtype):
    """The model's density, inverse density and the xyz gradient of <density, gd> + <1/density, gi> in `dtype`."""
    xx = x.detach().clone().to(dtype).requires_grad_(True)
    r = pcm.compute_density(xx, h)
    gdens, = torch.autograd.grad((r * gd.to(dtype)).sum(), xx, retain_graph=True)
    gboth, = torch.autograd.grad((r * gd.to(dtype)).sum() + ((1.0 / r) * gi.to(dtype)).sum(), xx)
    return r.detach(), gdens, gboth


@pytest.mark.parametrize("B,N,h", [(2, 300, 0.1), (1, 1000, 0.05), (3, 65, 0.2), (2, 256, 0.1), (1, 1, 0.1)])
def test_kde_density_and_gradient_vs_model(pc, B, N, h):
    """The expanded distance cancels: its float32 rounding error (about 2^-24 * (|a|^2 + |b|^2)) is divided by 2 h^2 in the exponent, so
    the attainable accuracy depends on h.  The bound is therefore the project's rule applied to the model: the kernel's error against
    the float64 model may not exceed 1.5 x the float32 model's own error against it (floors: 2e-6 forward, 1e-5 gradients)."""
    g = torch.Generator().manual_seed(N)
    x = torch.rand(B, N, 3, generator=g)
    gd, gi = torch.randn(B, N, generator=g), torch.randn(B, N, generator=g)
    r64, gdens64, gboth64 = _kde_model(x, h, gd, gi, torch.float64)
    r32, gdens32, gboth32 = _kde_model(x, h, gd, gi, torch.float32)
    xg = x.cuda().requires_grad_(True)
    dens = pc.compute_density(xg, h)
    assert tuple(dens.shape) == (B, N) and dens.dtype == torch.float32
    (dens * gd.cuda()).sum().backward()
    for what, own, m32, m64, floor in (("density", dens.detach(), r32, r64, 2e-6), ("dxyz", xg.grad, gdens32, gdens64, 1e-5)):
        e_own, e_ref = _rel(own, m64), _rel(m32, m64)
        print("kde %s B %d N %d h %g: own %.3e, float32 model %.3e" % (what, B, N, h, e_own, e_ref))
        assert e_own <= max(1.5 * e_ref, floor), what
    # both outputs of the launch (density and its inverse) with both gradients folded into one backward pass
    xg.grad = None
    dn, inv = pc._kde(xg, h)
    ((dn * gd.cuda()).sum() + (inv * gi.cuda()).sum()).backward()
    assert torch.equal(dn, dens) and _rel(inv.detach(), 1.0 / dn.detach().double()) < 2e-7
    e_own, e_ref = _rel(xg.grad, gboth64), _rel(gboth32, gboth64)
    print("kde dxyz (density and inverse) B %d N %d h %g: own %.3e, float32 model %.3e" % (B, N, h, e_own, e_ref))
    assert e_own <= max(1.5 * e_ref, 1e-5)
    g1 = xg.grad.clone(); xg.grad = None
    dn2, inv2 = pc._kde(xg, h)
    ((dn2 * gd.cuda()).sum() + (inv2 * gi.cuda()).sum()).backward()
    assert torch.equal(dn, dn2) and torch.equal(inv, inv2) and torch.equal(g1, xg.grad)


@pytest.mark.parametrize("B,N,S,K", [(2, 100, 7, 1), (2, 100, 7, 8), (3, 257, 33, 32), (2, 160, 1, 160), (1, 300, 5, 128)])
def test_group_density_scale_and_gradient_vs_model(pc, B, N, S, K):
    g = torch.Generator().manual_seed(N + K)
    inv = torch.rand(B, N, generator=g) + 0.5
    if K == N:
        idx = torch.arange(N).view(1, 1, N).expand(B, 1, N).contiguous()
    else:
        idx = torch.stack([torch.stack([torch.randperm(N, generator=g)[:K] for _ in range(S)]) for _ in range(B)])
    gout = torch.randn(B * S * K, 1, generator=g)
    ig = inv.cuda().requires_grad_(True)
    out = pc._density_scale(ig, idx.cuda())
    i64 = inv.double().requires_grad_(True)
    ref = pcm.density_scale(i64, idx).reshape(-1, 1)
    assert tuple(out.shape) == (B * S * K, 1) and _rel(out.detach(), ref.detach()) < 2e-7
    assert float(out.max()) == 1.0
    (out * gout.cuda()).sum().backward()
    (ref * gout.double()).sum().backward()
    # every slot's gradient is the difference of two terms of size |g| / m (they cancel exactly for K = 1, where the scale is the
    # constant 1): the error is measured against the size of those terms, not against the possibly vanishing result
    size = max(float(i64.grad.norm()), float((gout.double() / float(inv.min())).norm()))
    assert float((ig.grad.double().cpu() - i64.grad).norm()) <= 1e-5 * size
    g1 = ig.grad.clone(); ig.grad = None
    (pc._density_scale(ig, idx.cuda()) * gout.cuda()).sum().backward()
    assert torch.equal(g1, ig.grad)


@pytest.mark.parametrize("with_dens", [True, False])
@pytest.mark.parametrize("Q,K,C", [(5, 1, 16), (37, 8, 67), (9, 32, 128), (3, 128, 24), (2, 160, 32), (4, 33, 7), (3, 16, 200)])
def test_pointconv_aggregate_and_gradient_vs_model(pc, Q, K, C, with_dens):
    g = torch.Generator().manual_seed(Q * 1000 + K + C)
    F, Wt = torch.randn(Q * K, C, generator=g), torch.randn(Q * K, 16, generator=g)
    dens = torch.rand(Q * K, 1, generator=g) + 0.25 if with_dens else None
    gout = torch.randn(Q, 16 * C, generator=g)
    leaves = [t.cuda().requires_grad_(True) for t in (F, Wt)] + ([dens.cuda().requires_grad_(True)] if with_dens else [None])
    E = pc.pointconv_aggregate(leaves[0], leaves[1], leaves[2], K)
    refs = [t.double().requires_grad_(True) for t in (F, Wt)] + ([dens.double().requires_grad_(True)] if with_dens else [None])
    R = pcm.aggregate(refs[0], refs[1], refs[2], K)
    assert tuple(E.shape) == (Q, 16 * C) and _rel(E.detach(), R.detach()) < 2e-6
    # column order c*16 + w, element by element (an asymmetric pattern: a transposed tile would not pass)
    e0 = torch.einsum("kc,kw->cw", (F[:K] * (dens[:K] if with_dens else 1.0)).double(), Wt[:K].double())
    assert torch.allclose(E[0].view(C, 16).double().cpu(), e0, rtol=0, atol=1e-4 * float(e0.abs().max()))
    (E * gout.cuda()).sum().backward()
    (R * gout.double()).sum().backward()
    for a, b in zip(leaves, refs):
        if a is not None:
            assert a.grad.shape == a.shape and _rel(a.grad, b.grad) < 1e-5
    first = [E.detach()] + [a.grad.clone() for a in leaves if a is not None]
    for a in leaves:
        if a is not None:
            a.grad = None
    E2 = pc.pointconv_aggregate(leaves[0], leaves[1], leaves[2], K)
    (E2 * gout.cuda()).sum().backward()
    assert all(torch.equal(x, y) for x, y in zip(first, [E2.detach()] + [a.grad for a in leaves if a is not None]))


# ---------------------------------------------------------------- against the reference (golden G24)
def test_compute_density_golden(pc, d):
    x = pcm.case_inputs(d, "dsa")[0].transpose(1, 2).contiguous().cuda().requires_grad_(True)
    dens = pc.compute_density(x, pcm.BANDWIDTH)
    (dens * torch.from_numpy(d["kde|gout"].astype(np.float32)).cuda()).sum().backward()
    check64(d, "kde|density", "kde|density|f64", dens, floor=FLOOR)
    check64(d, "kde|gin|xyz", "kde|gin|xyz|f64", x.grad, floor=FLOOR)


@pytest.mark.parametrize("tag", ["dsa", "dsa_nopts", "sa"])
def test_sampling_and_grouping_indices_golden(pc, d, tag):
    kind, cargs, _ = pcm.CASES[tag]
    xyz = pcm.case_inputs(d, tag)[0].transpose(1, 2).contiguous().cuda()
    fps = pc.farthest_point_sample(xyz, cargs[0])
    assert fps.dtype == torch.int64 and np.array_equal(fps.cpu().numpy(), d[tag + "|fps0"].astype(np.int64))
    res = pc.sample_and_group(cargs[0], cargs[1], xyz, None, density_scale=torch.rand(xyz.shape[0], xyz.shape[1], 1).cuda())
    assert len(res) == 5 and len(pc.sample_and_group(cargs[0], cargs[1], xyz, None)) == 4
    new_xyz, new_points, gnorm, idx, gdens = res
    B, S, K = xyz.shape[0], cargs[0], cargs[1]
    assert tuple(new_xyz.shape) == (B, S, 3) and tuple(new_points.shape) == (B, S, K, 3) and tuple(gdens.shape) == (B, S, K, 1)
    # the K-th / (K+1)-th neighbours are >= 1e-4 apart and the float32 sets equal the float64 ones (asserted at capture): sets are well-defined
    assert np.array_equal(idx.sort(dim=-1)[0].cpu().numpy(), d[tag + "|knn0"].astype(np.int64))
    assert torch.equal(gnorm, pc.index_points(xyz, idx) - new_xyz.unsqueeze(2))


def test_sample_and_group_all_centres_on_the_mean(pc, d):
    xyz, pts = [t.transpose(1, 2).contiguous().cuda() for t in pcm.case_inputs(d, "dsa_all")]
    xg = xyz.clone().requires_grad_(True)
    dsc = torch.rand(xyz.shape[0], xyz.shape[1], 1).cuda()
    new_xyz, new_points, gxyz, gd = pc.sample_and_group_all(xg, pts, dsc)
    B, N, _ = xyz.shape
    assert tuple(new_xyz.shape) == (B, 1, 3) and tuple(new_points.shape) == (B, 1, N, 3 + pts.shape[2]) and tuple(gd.shape) == (B, 1, N, 1)
    assert _rel(new_xyz, xyz.mean(1, keepdim=True)) < 1e-6 and _rel(gxyz, (xyz - xyz.mean(1, keepdim=True)).unsqueeze(1)) < 1e-6
    assert torch.equal(new_points[..., 3:], pts.unsqueeze(1)) and len(pc.sample_and_group_all(xyz, None)) == 3
    w = torch.randn_like(gxyz)
    (gxyz * w).sum().backward()
    assert _rel(xg.grad, (w - w.mean(2, keepdim=True)).squeeze(1)) < 1e-5          # through the points and through the mean


@pytest.mark.parametrize("tag", sorted(pcm.CASES))
def test_module_train_mode_golden(pc, d, tag):
    """Every quantity is measured and logged before the test asserts.  Measured on an MI355X: the outputs, input gradients and ordinary
    parameter gradients of the three density cases land at 1e-6 .. 3e-6 where the reference's own float32 error is 1e-5 .. 3e-5 (the
    density's exponent is evaluated from a float64 distance here).  The weakest margin is the gradient of `densitynet.mlp_bns.2.weight`
    (2.2e-1 against a bound of 2.8e-1 in `dsa`): with beta = 0 the module's output does not depend on that weight's magnitude, so its
    exact gradient is a residue of order BatchNorm's eps and every float32 result, the reference's included, is rounding noise around it."""
    m = _module(pc, d, tag)
    args, outs = _run(pc, d, tag, m)
    missed = []

    def chk(name, t, **kw):          # every quantity is measured (and logged) before the test asserts
        try:
            check64(d, name, name + "|f64", t, floor=FLOOR, **kw)
        except AssertionError as e:
            missed.append(str(e))

    for i, o in enumerate(outs):
        chk("%s|out%d" % (tag, i), o, atol=1e-7)
    for k, p in m.named_parameters():
        chk("%s|grad|%s" % (tag, k), p.grad, atol=_atol(k))
        if _atol(k) == 2e-3:
            assert not p.grad.any(), k          # exactly zero
    for a, n in zip(args, pcm.CASES[tag][2]):
        if a is not None:
            chk("%s|gin|%s" % (tag, n), a.grad, atol=1e-7)
    for k, v in m.named_buffers():
        if v.is_floating_point():
            chk("%s|buf|%s" % (tag, k), v)
        else:
            assert int(v) == int(d["%s|buf|%s" % (tag, k)]) == 1, k
    assert not missed, "\n".join(missed)


@pytest.mark.parametrize("tag", sorted(pcm.CASES))
def test_module_eval_mode_uses_running_statistics(pc, d, tag):
    m = _module(pc, d, tag)
    _run(pc, d, tag, m)                 # one train step: the running statistics are no longer the initial ones
    m.eval()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    args = [None if a is None else a.cuda() for a in pcm.case_inputs(d, tag)]
    with torch.no_grad():
        outs = m(*args)
    refs, _, _ = pcm.run_model(d, tag, {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()},
                               [None if a is None else a.double() for a in pcm.case_inputs(d, tag)], training=False, idx=pcm.case_indices(d, tag))
    for o, r in zip(outs, refs):
        assert _rel(o, r) < 2e-6
    after = m.state_dict()
    assert all(torch.equal(after[k].cpu(), sd[k]) for k in sd)            # eval leaves every buffer (num_batches_tracked included) alone
    assert all(int(v) == 1 for k, v in after.items() if k.endswith("num_batches_tracked"))


def test_standalone_density_and_weight_nets_vs_model(pc):
    from pointnet2_model import _names, shared_mlp
    B, K, S = 2, 8, 19
    g = torch.Generator().manual_seed(3)
    for net, cin in ((pc.DensityNet(), 1), (pc.WeightNet(3, 16), 3)):
        net = net.cuda().train()
        sd = {k: v.detach().cpu().double() if v.is_floating_point() else v.cpu() for k, v in net.state_dict().items()}
        x = torch.rand(B, cin, K, S, generator=g)
        out = net(x.cuda())
        rows = x.double().permute(0, 3, 2, 1).reshape(B * S * K, cin)
        ref = shared_mlp(rows, 1, sd, _names(sd, "mlp_convs", "mlp_bns"), True, {}).view(B, S, K, -1).permute(0, 3, 2, 1)
        assert out.shape == ref.shape and _rel(out, ref) < 1e-5
        assert float(out.min()) >= 0.0                                    # ReLU behind the last layer too (no sigmoid)


@pytest.mark.parametrize("tag", ["dsa", "dsa_all"])
def test_two_identical_calls_are_bit_identical(pc, d, tag):
    res = []
    for _ in range(2):
        m = _module(pc, d, tag)
        args, outs = _run(pc, d, tag, m)
        res.append([o.detach() for o in outs] + [p.grad for p in m.parameters()] + [a.grad for a in args if a is not None])
    assert len(res[0]) == len(res[1]) and all(torch.equal(a, b) for a, b in zip(*res))


def test_refusals(pc, d):
    with pytest.raises(RuntimeError, match="no CPU"):
        _module(pc, d, "dsa")(*pcm.case_inputs(d, "dsa"))
    with pytest.raises(RuntimeError, match="no CPU"):
        pc.compute_density(torch.zeros(1, 4, 3), 0.1)
    with pytest.raises(ValueError, match="bandwidth"):
        pc.compute_density(torch.zeros(1, 4, 3).cuda(), 0.0)
    m = pc.PointConvSetAbstraction(4, 40, 3, [16], group_all=False).cuda()
    with pytest.raises(RuntimeError, match="knn_point"):                  # nsample > 32: spgan_knn_point's limit, passed on
        m(torch.rand(1, 3, 64).cuda(), None)
