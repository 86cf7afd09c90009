"""GPU: spgan.model_utils (csrc/point_losses.hip) against the numpy model tests/point_losses_model.py.

Exact clouds (coordinates multiples of 2^-6, radius 0.25 or 0.5: every d2, l1 and r*r is exact in float32): idx and val of group_nearest
equal the model bit for bit.  Random float32 clouds: idx is bit-equal to the float32-ordered model, losses and dpred are held to the
float64 model within the project's tolerance (tests/test_gan_layers_gpu.py): the same formulation composed from float32 torch ops on
the same GPU (the model's selected indices, gathered, measured, tail, mean, autograd) is evaluated against the float64 model -> e_ref;
the HIP result must lie within max(4 * e_ref, 8 * 2^-24 * scale), scale = the largest magnitude of the compared tensor, for dpred the
largest per-element sum of the contributions' magnitudes.  Every figure is appended to LOG (tools/point_losses_accuracy.py writes it to
profiles/point_losses_accuracy.json) together with the share of active tail terms, so that a test of zeros cannot pass unnoticed."""
import math

import numpy as np
import pytest
import torch

import point_losses_model as pm
import spgan
from spgan import _lib, model_utils as mu

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOG = []
METRICS = ("sq", "l1", "root")


def dev(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV).requires_grad_(grad)


def near(case, what, got, ref32, model, scale=None, active=None):
    got, ref32, model = (np.asarray(t, dtype=np.float64) for t in (got, ref32, model))
    scale = float(np.abs(model).max()) if scale is None else float(scale)
    e_ref = float(np.abs(ref32 - model).max())
    err = float(np.abs(got - model).max())
    bound = max(4 * e_ref, 8 * 2.0 ** -24 * scale)
    LOG.append({"case": case, "tensor": what, "err_hip": err, "e_ref": e_ref, "scale": scale, "bound": bound, "active_share": active})
    print("%s %s: hip %.3e  torch-f32 %.3e  bound %.3e  scale %.3e  active %s" % (case, what, err, e_ref, bound, scale, active))
    assert got.shape == model.shape and err <= bound, (case, what, err, e_ref, bound)


def check_selection(clouds, nsample, radius, metric, keep=5):
    val, idx = mu.group_nearest(dev(clouds), nsample, radius, metric, keep)
    midx, mval = pm.select_batch(clouds, nsample, radius, metric, keep)
    assert idx.dtype == torch.int32 and val.dtype == torch.float32 and tuple(idx.shape) == midx.shape
    assert np.array_equal(idx.cpu().numpy(), midx), (nsample, radius, metric)
    assert np.array_equal(val.cpu().numpy().view(np.uint32), mval.view(np.uint32)), (nsample, radius, metric)


# ------------------------------------------------------------------------------------------------------------ exact clouds
@pytest.mark.parametrize("nsample", [5, 20, 64, 65])
@pytest.mark.parametrize("N", [7, 64, 70, 130])
@pytest.mark.parametrize("radius", [0.25, 0.5, None])
def test_exact_clouds_bit_for_bit(radius, N, nsample):
    clouds = pm.exact_clouds(3, N, seed=1000 * N + nsample)
    for metric in METRICS:
        if radius is None and N < nsample:                   # kNN mode cannot fill its slots: refused, not skipped
            with pytest.raises(ValueError, match="N >= nsample"):
                mu.group_nearest(dev(clouds), nsample, None, metric)
            continue
        check_selection(clouds, nsample, radius, metric)
    if radius is None and N >= 6:
        check_selection(clouds, 6, None, "sq", keep=6)


# ------------------------------------------------------------------------------------------------------------ constructed clouds
CONSTRUCTED, CRADIUS = pm.constructed_clouds()


@pytest.mark.parametrize("nsample", [5, 8])
@pytest.mark.parametrize("knn", [False, True])
def test_constructed_clouds(knn, nsample):
    for metric in METRICS:
        check_selection(CONSTRUCTED, nsample, None if knn else CRADIUS, metric)
    check_selection(CONSTRUCTED, 6, None, "sq", keep=6)
    # the hazards' gradients: float64 model, all coordinates and distances exact
    for use_l1 in (False, True):
        x = dev(CONSTRUCTED, True)
        loss = mu.get_repulsion_loss(x, nsample, CRADIUS, knn, use_l1, h=0.05)
        loss.backward()
        m = pm.repulsion_loss(CONSTRUCTED, nsample, CRADIUS, knn, use_l1, h=0.05)
        assert abs(loss.item() - m["loss"]) <= 8 * 2.0 ** -24 * abs(m["loss"])
        assert np.max(np.abs(x.grad.cpu().numpy() - m["dpred"])) <= 8 * 2.0 ** -24 * m["scale"]
        if not knn:
            assert not x.grad[0, 13].any() and not x.grad[0, 20].any() and not x.grad[0, 21].any()      # alone in their balls: exactly 0
    last = mu.group_nearest(dev(CONSTRUCTED), nsample, None if knn else CRADIUS)[1][-1, -1].cpu().numpy()
    assert np.array_equal(last, pm.select(CONSTRUCTED[-1], nsample, None if knn else CRADIUS)[0][-1])     # the last query of the last cloud


# ------------------------------------------------------------------------------------------------------------ random float32 clouds
def torch32(clouds, m, tail):
    """The same formulation in float32 torch ops on the GPU over the model's selected indices -> (loss, dpred)."""
    x = dev(clouds, True)
    idx = torch.tensor(m["idx"], device=DEV)
    B = x.shape[0]
    d = x[:, :, None, :] - x[torch.arange(B, device=DEV)[:, None, None], idx]
    if m["metric"] == "l1":
        v = d.abs().sum(-1)
    else:
        v = (d * d).sum(-1)
        if m["metric"] == "root":
            v = torch.sqrt(v + 1e-12)
    loss = tail(v)
    loss.backward()
    return loss.item(), x.grad.cpu().numpy()


def hinge_tail(h):
    return lambda v: torch.relu(h - v[..., 1:]).mean()


def rep4_tail(radius):
    def f(v):
        v = v[..., 1:]
        w = torch.where(v > 1e-12, v, torch.full_like(v, 1e-12))
        return (radius - torch.sqrt(w) * torch.exp(-w / 0.03 ** 2)).mean()
    return f


def uniform_tail(v):
    return v.mean(2).var(dim=1, unbiased=False).sum() + v.var(dim=2, unbiased=False).sum()


def loss_cases(radius):
    """name -> (spgan call, model call, float32 tail): all four new-kernel losses, every flag combination."""
    cases = {}
    for knn in (False, True):
        for use_l1 in (False, True):
            h_rep = math.sqrt(0.001) * 2 if use_l1 else 0.001
            h_per = math.sqrt(0.001) * 2 if use_l1 else 0.01
            cases["repulsion knn=%d l1=%d" % (knn, use_l1)] = (
                lambda x, knn=knn, use_l1=use_l1: mu.get_repulsion_loss(x, 20, radius, knn, use_l1),
                lambda c, knn=knn, use_l1=use_l1: pm.repulsion_loss(c, 20, radius, knn, use_l1), hinge_tail(h_rep))
            cases["perulsion knn=%d l1=%d" % (knn, use_l1)] = (
                lambda x, knn=knn, use_l1=use_l1: mu.get_perulsion_loss(x, 15, radius, knn, 512, use_l1),
                lambda c, knn=knn, use_l1=use_l1: pm.perulsion_loss(c, 15, radius, knn, use_l1), hinge_tail(h_per))
    cases["repulsion4"] = (lambda x: mu.get_repulsion_loss4(x, 20, radius), lambda c: pm.repulsion_loss4(c, 20, radius), rep4_tail(radius))
    cases["uniform_knn"] = (mu.get_uniform_loss_knn, pm.uniform_loss_knn, uniform_tail)
    return cases


# radius 0.04 in a cloud of about 13 points per ball of radius 0.03: balls of some 30 points, so most overflow nsample 20 (index-order
# truncation), some pad; d2 < 0.0016 against h = 0.001 (sq), so the repulsion hinge is active on a majority but not on all values
RADIUS = 0.04
RANDOM200 = pm.random_clouds(2, 200, seed=7)


def run_loss_case(tag, clouds, name, case):
    fn, model, tail = case
    x = dev(clouds, True)
    loss = fn(x)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    m = model(clouds)
    l32, g32 = torch32(clouds, m, tail)
    near("%s %s" % (tag, name), "loss", loss.item(), l32, m["loss"], active=m["active"])
    near("%s %s" % (tag, name), "dpred", x.grad.cpu().numpy(), g32, m["dpred"], scale=m["scale"], active=m["active"])
    assert m["active"] > 0.5, (name, m["active"])            # a clear majority of the tail terms is active
    return m


@pytest.mark.parametrize("name", sorted(loss_cases(RADIUS)))
def test_random_clouds_losses(name):
    run_loss_case("N=200", RANDOM200, name, loss_cases(RADIUS)[name])


@pytest.mark.parametrize("knn", [False, True])
def test_random_clouds_indices(knn):
    for metric in METRICS:
        _, idx = mu.group_nearest(dev(RANDOM200), 20, None if knn else RADIUS, metric)
        assert np.array_equal(idx.cpu().numpy(), pm.select_batch(RANDOM200, 20, None if knn else RADIUS, metric)[0])


def test_random_clouds_2048():
    clouds = pm.random_clouds(2, 2048, seed=11)
    _, idx = mu.group_nearest(dev(clouds), 20, RADIUS)
    m = run_loss_case("N=2048", clouds, "repulsion knn=0 l1=0", loss_cases(RADIUS)["repulsion knn=0 l1=0"])
    assert np.array_equal(idx.cpu().numpy(), m["idx"])
    run_loss_case("N=2048", clouds, "repulsion4", loss_cases(RADIUS)["repulsion4"])


def test_group_nearest_gradient():
    """val's cotangent reaches pred through both ends of every selected pair."""
    g = np.random.RandomState(3).randn(2, 200, 5)
    for metric in METRICS:
        x = dev(RANDOM200, True)
        val, idx = mu.group_nearest(x, 20, RADIUS, metric)
        (val * dev(g)).sum().backward()
        dp, ab = pm.scatter_grad(RANDOM200, idx.cpu().numpy().astype(np.int64), g.astype(np.float32).astype(np.float64), metric)
        m = {"idx": idx.cpu().numpy().astype(np.int64), "metric": metric}
        _, g32 = torch32(RANDOM200, m, lambda v: (v * dev(g)).sum())
        near("group_nearest %s" % metric, "dpred", x.grad.cpu().numpy(), g32, dp, scale=ab.max())


# ------------------------------------------------------------------------------------------------------------ other checks
def test_two_calls_give_equal_bits():
    for name, (fn, _, _) in loss_cases(RADIUS).items():
        outs = []
        for _ in range(2):
            x = dev(RANDOM200, True)
            loss = fn(x)
            loss.backward()
            outs.append((loss.detach().clone(), x.grad.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), name


def test_backward_routes_agree(monkeypatch):
    """The reverse-CSR route and the table walk add the same terms: each against the model, each twice with equal bits."""
    m = pm.repulsion_loss(RANDOM200, 20, RADIUS)
    for route in ("csr", "table"):
        monkeypatch.setattr(mu, "BACKWARD_ROUTE", route)
        grads = []
        for _ in range(2):
            x = dev(RANDOM200, True)
            mu.get_repulsion_loss(x, 20, RADIUS).backward()
            grads.append(x.grad.clone())
        assert torch.equal(grads[0], grads[1]), route
        assert np.max(np.abs(grads[0].cpu().numpy() - m["dpred"])) <= 8 * 2.0 ** -24 * m["scale"], route
    # keep 6 and a cloud of more than one staged chunk of the table (N * keep > 4096)
    clouds = pm.random_clouds(1, 900, seed=13)
    g = np.random.RandomState(4).randn(1, 900, 6).astype(np.float32)
    for route in ("csr", "table"):
        monkeypatch.setattr(mu, "BACKWARD_ROUTE", route)
        x = dev(clouds, True)
        val, idx = mu.group_nearest(x, 12, None, "l1", 6)
        (val * dev(g)).sum().backward()
        dp, ab = pm.scatter_grad(clouds, idx.cpu().numpy().astype(np.int64), g.astype(np.float64), "l1")
        assert np.max(np.abs(x.grad.cpu().numpy() - dp)) <= 8 * 2.0 ** -24 * ab.max(), route


def test_captured_body_replays_the_eager_bits():
    def body(x):
        x = x.detach().requires_grad_(True)
        loss = mu.get_repulsion_loss(x, 20, RADIUS) + mu.get_repulsion_loss4(x, 20, RADIUS) + mu.get_uniform_loss_knn(x)
        (g,) = torch.autograd.grad(loss, x)
        return loss.detach(), g
    x = dev(RANDOM200)
    eager = [t.clone() for t in body(x)]
    cap = spgan.CapturedBody(body, modules=(), warmup=1)
    for _ in range(3):
        out = cap(x)
    torch.cuda.synchronize()
    assert not cap.eager and cap._graph is not None
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])


@pytest.mark.parametrize("threshold", [None, "on"])
def test_cd_compositions(threshold):
    rng = np.random.RandomState(5)
    pred, gt = rng.rand(2, 130, 3).astype(np.float32), rng.rand(2, 70, 3).astype(np.float32)
    df, db = pm.nn_dists64(gt, pred)
    p, g = dev(pred, True), dev(gt)
    f32, b32 = [t.cpu().numpy().astype(np.float64) for t in spgan.metrics.nn_distance(g, p.detach())]
    tol = lambda want: 8 * 2.0 ** -24 * abs(want) + 4 * max(np.abs(f32 - df).max(), np.abs(b32 - db).max())     # noqa: E731
    loss, none = mu.get_cd_loss(p, g, 0.5)
    assert none is None and abs(loss.item() - pm.cd_loss(df, db, 0.5)) <= tol(pm.cd_loss(df, db, 0.5))
    thr2 = None if threshold is None else 2.0                # twice the mean distance: drops a share of both directions
    want = pm.cd_loss2(df, db, 0.7, thr2)
    got = mu.get_cd_loss2(p, g, 0.5, 0.7, thr2)
    assert abs(got.item() - want) <= tol(want)
    if thr2 is not None:
        assert want < pm.cd_loss2(df, db, 0.7, None)
    thrh = None if threshold is None else float(np.median(df))
    want = pm.hausdorff_loss(df, db, 0.5, 0.7, thrh)
    got, none = mu.get_hausdorff_loss(p, g, 0.5, 0.7, thrh)
    assert none is None and abs(got.item() - want) <= tol(want) / 0.5
    (mu.get_cd_loss(p, g, 0.5)[0] + mu.get_cd_loss2(p, g, 0.5) + mu.get_hausdorff_loss(p, g, 0.5)[0]).backward()
    assert torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0


def test_inputs_and_c_entry_refusals():
    x = dev(RANDOM200)
    with pytest.raises(TypeError):
        mu.get_repulsion_loss(x.double())
    with pytest.raises(RuntimeError, match="GPU"):
        mu.get_repulsion_loss(x.cpu())
    xt = dev(np.ascontiguousarray(RANDOM200.transpose(0, 2, 1))).transpose(1, 2)      # non-contiguous view of the same cloud
    assert not xt.is_contiguous()
    assert torch.equal(mu.get_repulsion_loss(xt, 20, RADIUS), mu.get_repulsion_loss(x, 20, RADIUS))
    lib = _lib.load()
    B, N = 2, 200
    val = torch.empty(B, N, 5, device=DEV)
    idx = torch.empty(B, N, 5, dtype=torch.int32, device=DEV)
    part = torch.empty(lib.spgan_point_losses_partials(B, N), dtype=torch.float64, device=DEV)
    loss = torch.full((), 7.0, device=DEV)

    def f(nsample=20, radius=0.04, keep=5, knn=None):
        return lib.spgan_point_losses_fwd(x.data_ptr(), knn, B, N, nsample, radius, 0, keep, 1, 0.001, 0.0, val.data_ptr(), idx.data_ptr(),
                                          val.data_ptr(), part.data_ptr(), loss.data_ptr(), None)
    assert f(nsample=4) == -22 and f(nsample=257) == -22 and f(radius=0.0) == -22 and f(keep=9) == -22
    assert f(nsample=201, knn=idx.data_ptr()) == -22
    torch.cuda.synchronize()
    assert loss.item() == 7.0                                # refused before any launch: nothing was written
