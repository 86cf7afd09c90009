"""CPU: the numpy model of the point-distribution losses (tests/point_losses_model.py) against an independent brute-force float64 torch
formulation written straight from Common/model_utils.py -- a dense [N,N] matrix, a mask, the first-nsample rule by a stable sort of
indices, the five smallest, autograd for the gradient -- on the constructed clouds; the validation errors of spgan.model_utils; the
Chamfer / Hausdorff compositions' formulae on hand-made distance tensors; the header / binding agreement of the new C entries.

The five smallest are taken by a stable ascending sort, which is tf.nn.top_k's documented tie rule (lowest index first); torch.topk
leaves the order among equal values open, so it is held to the values only."""
import math
import os
import re

import numpy as np
import pytest
import torch

import point_losses_model as pm
import spgan
from spgan import _lib, model_utils as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("spgan_point_losses_partials", "spgan_point_losses_fwd", "spgan_point_losses_bwd")
CLOUDS, RADIUS = pm.constructed_clouds()


# ------------------------------------------------------------------------------------------------------------ the brute-force formulation
def brute_values(p, nsample, radius, knn, metric, keep=5):
    """p [N,3] float64 (requires grad) -> (val [N,keep], point index [N,keep]) as model_utils.py:160-176 computes them."""
    N = p.shape[0]
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    ar = torch.arange(N)
    if knn:
        idx = torch.sort(d2.detach(), dim=1, stable=True).indices[:, :nsample]
    else:
        mask = d2.detach() < radius * radius
        order = torch.sort(torch.where(mask, ar[None, :], N + ar[None, :]), dim=1, stable=True).indices[:, :min(nsample, N)]
        cnt = mask.sum(1).clamp(max=nsample)
        slot = torch.arange(nsample)[None, :].expand(N, nsample)
        idx = torch.gather(order, 1, torch.where(slot < cnt[:, None], slot, torch.zeros_like(slot)))
    grouped = p[idx] - p[:, None, :]
    if metric == "l1":
        dists = grouped.abs().sum(-1)
    else:
        dists = (grouped ** 2).sum(-1)
        if metric == "root":
            dists = torch.sqrt(dists + 1e-12)
    srt = torch.sort(dists, dim=1, stable=True)
    val, which = srt.values[:, :keep], srt.indices[:, :keep]
    top = -torch.topk(-dists, keep, dim=1).values
    assert torch.equal(top.detach(), val.detach())
    return val, torch.gather(idx, 1, which)


def brute_loss(clouds, fn):
    """-> (loss, dpred) with fn(p, b) -> per-cloud [N,4] terms; the mean over all B*N*4 terms."""
    ps = [torch.tensor(c, dtype=torch.float64, requires_grad=True) for c in clouds]
    terms = torch.stack([fn(p) for p in ps])
    loss = terms.mean()
    loss.backward()
    return loss.item(), np.stack([p.grad.numpy() for p in ps])


def hinge(h):
    return lambda v: torch.relu(h - v)


def rep4(radius):
    def f(v):
        w = torch.where(v > 1e-12, v, torch.full_like(v, 1e-12))
        return radius - torch.sqrt(w) * torch.exp(-w / 0.03 ** 2)
    return f


def close(a, b, scale):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) <= 1e-12 * max(scale, 1e-300)


# ------------------------------------------------------------------------------------------------------------ model against brute force
@pytest.mark.parametrize("nsample", [5, 8])
@pytest.mark.parametrize("knn", [False, True])
@pytest.mark.parametrize("metric", ["sq", "l1", "root"])
def test_model_selection_matches_brute_force(metric, knn, nsample):
    for c in CLOUDS:
        idx, val, _ = pm.select(c, nsample, None if knn else RADIUS, metric)
        bval, bidx = brute_values(torch.tensor(c, dtype=torch.float64), nsample, RADIUS, knn, metric)
        assert np.array_equal(idx, bidx.numpy())
        assert np.allclose(val, bval.numpy(), rtol=1e-6, atol=1e-7)           # the model's values are float32


@pytest.mark.parametrize("nsample", [5, 8])
@pytest.mark.parametrize("knn", [False, True])
@pytest.mark.parametrize("use_l1", [False, True])
def test_model_repulsion_and_perulsion(use_l1, knn, nsample):
    # h so large that the hinge is active on most of these coarse clouds, and once the reference's own default
    for h in (0.05, 0.001):
        m = pm.repulsion_loss(CLOUDS, nsample, RADIUS, knn, use_l1, h)
        h_eff = math.sqrt(h) * 2 if use_l1 else h
        metric = "l1" if use_l1 else "sq"
        loss, dp = brute_loss(CLOUDS, lambda p: hinge(h_eff)(brute_values(p, nsample, RADIUS, knn, metric)[0][:, 1:]))
        assert close(m["loss"], loss, abs(loss)) and close(m["dpred"], dp, m["scale"])
    m = pm.perulsion_loss(CLOUDS, nsample, RADIUS, knn, use_l1)
    metric = "root" if use_l1 else "sq"
    h_eff = math.sqrt(0.001) * 2 if use_l1 else 0.01
    loss, dp = brute_loss(CLOUDS, lambda p: hinge(h_eff)(brute_values(p, nsample, RADIUS, knn, metric)[0][:, 1:]))
    assert m["active"] > 0                                # some hinges are active: the gradient compared below is not all zeros
    assert close(m["loss"], loss, abs(loss)) and np.max(np.abs(m["dpred"] - dp)) <= 1e-9 * m["scale"]      # sqrt(d2 + 1e-12) near 0


@pytest.mark.parametrize("nsample", [5, 8])
def test_model_repulsion4_and_uniform(nsample):
    m = pm.repulsion_loss4(CLOUDS, nsample, RADIUS)
    loss, dp = brute_loss(CLOUDS, lambda p: rep4(RADIUS)(brute_values(p, nsample, RADIUS, False, "sq")[0][:, 1:]))
    assert close(m["loss"], loss, abs(loss)) and close(m["dpred"], dp, m["scale"])
    m = pm.uniform_loss_knn(CLOUDS)
    ps = [torch.tensor(c, dtype=torch.float64, requires_grad=True) for c in CLOUDS]
    total = 0.0
    for p in ps:
        var = brute_values(p, 6, None, True, "sq", keep=6)[0]
        total = total + var.mean(1).var(unbiased=False) + var.var(dim=1, unbiased=False).sum()
    total.backward()
    assert close(m["loss"], total.item(), abs(total.item()))
    assert close(m["dpred"], np.stack([p.grad.numpy() for p in ps]), m["scale"])


def test_constructed_hazards_are_what_they_claim():
    c = CLOUDS
    idx, val, slot = pm.select(c[0], 5, RADIUS, "sq")
    assert np.array_equal(idx[13], [13] * 5) and not val[13].any()                      # alone: five copies of itself
    assert np.array_equal(pm.group_slots(c[0], 5, RADIUS)[0], [0, 1, 2, 3, 4])          # truncation keeps the far ring, not 9..12
    assert set(pm.group_slots(c[0], 5, RADIUS)[14]) == {14, 15} and set(pm.group_slots(c[0], 5, RADIUS)[16]) == {16, 17, 18, 19}
    assert pm.group_slots(c[0], 5, RADIUS)[15][0] == 14 and list(pm.group_slots(c[0], 5, RADIUS)[15][2:]) == [14, 14, 14]
    assert set(pm.group_slots(c[0], 5, RADIUS)[20]) == {20} and set(pm.group_slots(c[0], 5, RADIUS)[21]) == {21}     # distance == radius
    idx8, val8, _ = pm.select(c[1], 8, RADIUS, "sq")
    assert list(idx8[5]) == [5, 2, 3, 4, 0] and val8[5][4] == np.float32(25 / 4096)     # 0, 1 and 6 tie for the fifth: the lowest slot
    idx6, _, _ = pm.select(c[1], 6, None, "sq", keep=6)
    assert list(idx6[5]) == [5, 2, 3, 4, 0, 1]
    assert (c.shape[0] * c.shape[1]) % 4 != 0


# ------------------------------------------------------------------------------------------------------------ validation
def test_validation_errors():
    x = torch.zeros(2, 32, 3)
    for bad in (4, 257, 0):
        with pytest.raises(ValueError, match="nsample"):
            mu.get_repulsion_loss(x, nsample=bad)
    with pytest.raises(ValueError, match="nsample"):
        mu.get_repulsion_loss(x, nsample=201, knn=True)
    with pytest.raises(ValueError, match="N >= nsample"):
        mu.get_perulsion_loss(x, nsample=33, knn=True)
    with pytest.raises(ValueError, match="N >= nsample"):
        mu.get_uniform_loss_knn(torch.zeros(1, 5, 3))
    for r in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius"):
            mu.get_repulsion_loss4(x, radius=r)
    with pytest.raises(ValueError, match="metric"):
        mu.group_nearest(x, 8, 0.1, metric="l2")
    with pytest.raises(ValueError, match="keep"):
        mu.group_nearest(x, 8, 0.1, keep=9)
    with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
        mu.get_repulsion_loss(torch.zeros(2, 32, 2))
    for fn in (mu.get_repulsion_loss, mu.get_repulsion_loss4, mu.get_perulsion_loss, mu.get_uniform_loss_knn):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(x)
    with pytest.raises(RuntimeError, match="GPU"):
        mu.get_cd_loss(x, x, 1.0)


def test_c_entries_refuse_bad_sizes_without_gpu():
    lib = _lib.load()
    X = 64          # never dereferenced: every call below is refused before a launch
    fwd, bwd = lib.spgan_point_losses_fwd, lib.spgan_point_losses_bwd

    def f(xyz=X, knn=None, B=2, n=64, nsample=20, radius=0.1, metric=0, keep=5, tail=1, h=0.001, val=X, idx=X, coef=X, partial=X, loss=X):
        return fwd(xyz, knn, B, n, nsample, radius, metric, keep, tail, h, 0.0, val, idx, coef, partial, loss, None)
    assert f(nsample=4) == -22 and f(nsample=257) == -22
    assert f(knn=X, nsample=201, n=512) == -22 and f(knn=X, nsample=65, n=64) == -22
    assert f(radius=0.0) == -22 and f(radius=-0.1) == -22 and f(radius=float("nan")) == -22
    assert f(metric=3) == -22 and f(metric=-1) == -22 and f(tail=3) == -22 and f(keep=1) == -22 and f(keep=9) == -22
    assert f(nsample=5, keep=6) == -22
    assert f(B=0) == -22 and f(n=0) == -22 and f(B=65536) == -22
    assert f(xyz=None) == -22 and f(val=None) == -22 and f(idx=None) == -22
    assert f(coef=None) == -22 and f(partial=None) == -22 and f(loss=None) == -22 and f(h=0.0) == -22
    assert bwd(None, X, X, None, 1.0, 1, 16, 5, 0, None, None, X, None) == -22
    assert bwd(X, X, X, None, 1.0, 1, 16, 5, 3, None, None, X, None) == -22
    assert bwd(X, X, X, None, 1.0, 1, 16, 1, 0, None, None, X, None) == -22
    assert bwd(X, X, X, None, 1.0, 1, 16, 5, 0, X, None, X, None) == -22               # rowptr without slots
    assert bwd(X, X, X, None, 1.0, 0, 16, 5, 0, None, None, X, None) == -22
    assert lib.spgan_point_losses_partials(2, 7) == 4 and lib.spgan_point_losses_partials(0, 7) == 0


# ------------------------------------------------------------------------------------------------------------ Chamfer / Hausdorff formulae
def test_cd_compositions_on_hand_made_distances(monkeypatch):
    df = torch.tensor([[1.0, 2.0, 3.0, 10.0], [0.5, 0.5, 0.5, 0.5]])                      # gt -> pred
    db = torch.tensor([[4.0, 0.0], [1.0, 3.0]])                                           # pred -> gt
    seen = []

    def fake(a, b):
        seen.append((a, b))
        return df, db
    monkeypatch.setattr(mu, "nn_distance", fake)
    pred, gt = torch.zeros(2, 2, 3), torch.ones(2, 4, 3)
    loss, none = mu.get_cd_loss(pred, gt, 2.0)
    assert none is None and seen[-1][0] is gt and seen[-1][1] is pred                     # the reference's argument order
    assert loss.item() == pytest.approx(((0.8 * 4.0 + 0.2 * 2.0) / 2 + (0.8 * 0.5 + 0.2 * 2.0) / 2) / 2)
    assert mu.get_cd_loss2(pred, gt, 2.0, threshold=None).item() == pytest.approx(((4.0 + 2.0) + (0.5 + 2.0)) / 2)
    # threshold 2: forward means 4 and 0.5 -> 10 survives no test at 8 (dropped), 0.5 < 1 kept; backward means 2 and 2 -> 4 dropped, 3 kept
    got = mu.get_cd_loss2(pred, gt, 2.0, forward_weight=0.5, threshold=2).item()
    assert got == pytest.approx(((0.5 * 6.0 / 4 + 0.0) + (0.5 * 0.5 + 2.0)) / 2)
    loss, none = mu.get_hausdorff_loss(pred, gt, 2.0)
    assert none is None and loss.item() == pytest.approx(max((10.0 + 4.0) / 2, (0.5 + 3.0) / 2))
    loss, _ = mu.get_hausdorff_loss(pred, gt, 2.0, forward_weight=2.0, threshold=3.5)
    assert loss.item() == pytest.approx(max((2 * 3.0 + 0.0) / 2, (2 * 0.5 + 3.0) / 2))
    d64, b64 = df.double().numpy(), db.double().numpy()
    assert pm.cd_loss(d64, b64, 2.0) == pytest.approx(mu.get_cd_loss(pred, gt, 2.0)[0].item())
    assert pm.cd_loss2(d64, b64, 0.5, 2) == pytest.approx(got)
    assert pm.hausdorff_loss(d64, b64, 2.0, 2.0, 3.5) == pytest.approx(loss.item())


# ------------------------------------------------------------------------------------------------------------ ABI
def test_symbols_declared_and_typed():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spgan_hip.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert s in _lib.SIGNATURES
    lib = _lib.load()
    for s in NEW:
        assert hasattr(lib, s)
    decl = re.search(r"int spgan_point_losses_fwd\((.*?)\);", txt, flags=re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["spgan_point_losses_fwd"][1])
    decl = re.search(r"int spgan_point_losses_bwd\((.*?)\);", txt, flags=re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["spgan_point_losses_bwd"][1])
    for name in ("model_utils", "get_repulsion_loss", "get_repulsion_loss4", "get_perulsion_loss", "get_uniform_loss_knn", "get_cd_loss",
                 "get_cd_loss2", "get_hausdorff_loss", "group_nearest"):
        assert hasattr(spgan, name) and name in spgan.__all__
