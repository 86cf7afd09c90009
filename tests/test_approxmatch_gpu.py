"""GPU: spgan.approxmatch (csrc/approxmatch.hip) against the float64 numpy model tests/approxmatch_model.py.

Tolerance: the project's rule max(4 * e_ref, 8 * 2^-24 * scale).  e_ref is the distance from the float64 model of the same formulation
written in float32 torch ops with dense [B,n,m] tensors on the same GPU (torch32 below); the scales are max(n,m) times the largest
pairwise distance for the cost, multiL / multiR for the two gradients, and the largest entry for the records and the plan.  Vectors are
compared in the max norm against their scale, not element by element: min and max(0, .) are kinks.  The gradients are those of the
definition with the plan held constant (the model's grad1 / grad2), not finite differences of the cost.

Every figure is appended to LOG; tools/approxmatch_accuracy.py writes it to profiles/approxmatch_accuracy.json."""
import numpy as np
import pytest
import torch

import approxmatch_model as am
import spgan
from spgan import _lib, approxmatch as ap, gan_metrics, metrics, model_utils as mu

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOG = []
_MODEL = {}                                              # (kind, B, n, m) -> (a, b, float64 model, torch32 results); computed once


def tile():
    return _lib.load().spgan_approxmatch_tile()


def shapes():
    """(B, n, m): one point; below / above one wave of rows; one more than the sweeps' LDS tile; n != m both ways; more pairs than a
    block row; exactly one tile of the backward."""
    return [(1, 1, 1), (3, 63, 63), (2, 65, 65), (2, 1025, 1025), (2, 64, 128), (2, 128, 64), (37, 32, 32), (4, 256, 256)]


def dev(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV).requires_grad_(grad)


def torch32(a, b):
    """The definition in float32 torch ops over dense [B,n,m] tensors -> dict of float64 numpy arrays."""
    a, b = dev(a), dev(b)
    B, n, m = a.shape[0], a.shape[1], b.shape[1]
    diff = a[:, :, None, :] - b[:, None, :, :]
    d2 = (diff * diff).sum(-1)
    dist = d2.sqrt()
    big = float(max(n, m))
    remain_l = torch.full((B, n), big / n, device=DEV)
    remain_r = torch.full((B, m), big / m, device=DEV)
    match = torch.zeros((B, n, m), device=DEV)
    rl, rr = [], []
    for j in am.LEVELS:
        e = torch.exp(am.level(j) * d2)
        ratio_l = remain_l / (1e-9 + (e * remain_r[:, None, :]).sum(2))
        sumr = remain_r * (e * ratio_l[:, :, None]).sum(1)
        ratio_r = torch.minimum(remain_r / (sumr + 1e-9), torch.ones_like(sumr)) * remain_r
        remain_r = (remain_r - sumr).clamp_min(0)
        w = e * ratio_l[:, :, None] * ratio_r[:, None, :]
        match = match + w
        remain_l = (remain_l - w.sum(2)).clamp_min(0)
        rl.append(ratio_l)
        rr.append(ratio_r)
    cost = (match * dist).sum((1, 2))
    unit = diff / dist.clamp_min(1e-20)[..., None]
    g1 = (match[..., None] * unit).sum(2)
    g2 = -(match[..., None] * unit).sum(1)
    out = dict(cost=cost, grad1=g1, grad2=g2, ratioL=torch.stack(rl, 1), ratioR=torch.stack(rr, 1), match=match.transpose(1, 2))
    return {k: v.double().cpu().numpy() for k, v in out.items()}


def case(kind, B, n, m):
    key = (kind, B, n, m)
    if key not in _MODEL:
        a, b = am.clouds(kind, B, n, m, seed=1)
        _MODEL[key] = (a, b, am.batch(a, b), torch32(a, b))
    return _MODEL[key]


def bound_of(ref32, model, scale):
    e_ref = float(np.abs(np.asarray(ref32, dtype=np.float64) - model).max())
    return max(4 * e_ref, 8 * 2.0 ** -24 * scale), e_ref


def near(name, what, got, ref32, model, scale):
    got, model = np.asarray(got, dtype=np.float64), np.asarray(model, dtype=np.float64)
    bound, e_ref = bound_of(ref32, model, scale)
    err = float(np.abs(got - model).max())
    LOG.append({"case": name, "tensor": what, "err_hip": err, "e_ref": e_ref, "scale": float(scale), "bound": bound,
                "ratio": err / bound if bound > 0 else 0.0})
    print("%s %s: hip %.3e  torch-f32 %.3e  bound %.3e  scale %.3e" % (name, what, err, e_ref, bound, scale))
    assert got.shape == model.shape and np.isfinite(got).all() and err <= bound, (name, what, err, e_ref, bound)
    return bound


def scales(model, n, m):
    return dict(cost=max(n, m) * model["dmax"], grad1=model["multiL"], grad2=model["multiR"], ratioL=float(np.abs(model["ratioL"]).max()),
                ratioR=float(np.abs(model["ratioR"]).max()), match=float(np.abs(model["match"]).max()))


@pytest.mark.parametrize("kind", am.KINDS)
@pytest.mark.parametrize("shape", shapes(), ids=lambda s: "%dx%dx%d" % s)
def test_against_the_float64_model(shape, kind):
    B, n, m = shape
    assert shapes()[3][1] == tile() + 1                      # case d follows the kernel's tile
    a, b, model, ref = case(kind, B, n, m)
    name = "%s-%dx%dx%d" % ((kind,) + shape)
    sc = scales(model, n, m)
    x, y = dev(a, True), dev(b, True)
    cost = ap.match_cost(x, y)
    w = torch.linspace(0.5, 1.5, B, device=DEV)              # a different cotangent per pair
    (cost * w).sum().backward()
    wn = w.double().cpu().numpy()[:, None, None]
    _, rl, rr = ap.approx_match_records(x, y)
    plan = ap.approx_match(x, y)
    assert plan.shape == (B, m, n) and rl.shape == (B, 10, n) and rr.shape == (B, 10, m) and cost.shape == (B,)
    bc = near(name, "cost", cost.detach().cpu().numpy(), ref["cost"], model["cost"], sc["cost"])
    b1 = near(name, "grad1", x.grad.cpu().numpy() / wn, ref["grad1"], model["grad1"], sc["grad1"])
    b2 = near(name, "grad2", y.grad.cpu().numpy() / wn, ref["grad2"], model["grad2"], sc["grad2"])
    near(name, "ratioL", rl.cpu().numpy(), ref["ratioL"], model["ratioL"], sc["ratioL"])
    near(name, "ratioR", rr.cpu().numpy(), ref["ratioR"], model["ratioR"], sc["ratioR"])
    near(name, "match", plan.cpu().numpy(), ref["match"], model["match"], sc["match"])
    # fused against dense: the cost of the written plan and its gradients
    x2, y2 = dev(a, True), dev(b, True)
    dense = ap.match_cost_dense(x2, y2, plan)
    (dense * w).sum().backward()
    near(name, "dense cost", dense.detach().cpu().numpy(), ref["cost"], model["cost"], sc["cost"])
    near(name, "dense grad1", x2.grad.cpu().numpy() / wn, ref["grad1"], model["grad1"], sc["grad1"])
    near(name, "dense grad2", y2.grad.cpu().numpy() / wn, ref["grad2"], model["grad2"], sc["grad2"])
    assert float((dense.detach() - cost.detach()).abs().max()) <= bc
    assert float(((x2.grad - x.grad).double().cpu().numpy() / wn).__abs__().max()) <= b1
    assert float(((y2.grad - y.grad).double().cpu().numpy() / wn).__abs__().max()) <= b2
    if kind == "far":
        assert float(np.abs(model["ratioL"]).max()) > 1e8            # the underflowed levels went through the 1e-9 path
    if kind in ("identical", "duplicates"):
        assert (model["match"] > 0).any() and torch.isfinite(x.grad).all() and torch.isfinite(y.grad).all()


def test_gradients_are_the_definitions_not_finite_differences():
    """With the plan held constant d cost / d xyz1 = sum_l match * unit vector; the cost's own finite difference also moves the plan."""
    a, b, model, _ = case("cube", 2, 65, 65)
    x = dev(a, True)
    ap.match_cost(x, dev(b)).sum().backward()
    h, gaps = 1e-3, []
    for i, c in ((5, 0), (7, 1), (20, 2)):
        up, down = a.astype(np.float64).copy(), a.astype(np.float64).copy()
        up[0, i, c] += h
        down[0, i, c] -= h
        fd = (am.approx_match(up[0], b[0])["cost"] - am.approx_match(down[0], b[0])["cost"]) / (2 * h)
        held = model["grad1"][0, i, c]
        assert abs(x.grad[0, i, c].item() - held) <= 1e-5
        gaps.append(abs(fd - held))
    assert max(gaps) > 0.05                                                      # they differ by construction (0.16 at point 20)


def test_results_repeat_bit_for_bit():
    a, b, _, _ = case("sphere", 4, 256, 256)
    outs = []
    for _ in range(2):
        x, y = dev(a, True), dev(b, True)
        c = ap.match_cost(x, y)
        c.sum().backward()
        outs.append((c.detach().clone(), x.grad.clone(), y.grad.clone(), ap.approx_match(x, y)))
    for u, v in zip(*outs):
        assert torch.equal(u, v)


def test_stride_zero_sample_equals_the_expanded_copy():
    a, b = am.clouds("cube", 1, 128, 128, seed=2)[0], am.clouds("sphere", 6, 128, 128, seed=2)[1]
    refs = dev(b)
    lazy, copied = dev(a, True), dev(np.repeat(a, 6, axis=0), True)
    view = lazy.expand(6, -1, -1)
    assert view.stride(0) == 0 and ap._batch_stride(view) == 0 and ap._batch_stride(copied) == 128 * 3
    c0, c1 = ap.match_cost(view, refs), ap.match_cost(copied, refs)
    assert torch.equal(c0, c1)
    assert torch.equal(ap.approx_match(view.detach(), refs), ap.approx_match(copied.detach(), refs))
    w = torch.linspace(1.0, 2.0, 6, device=DEV)
    g0 = torch.autograd.grad((c0 * w).sum(), view, retain_graph=True)[0]          # per pair, before autograd sums over the expansion
    g1 = torch.autograd.grad((c1 * w).sum(), copied)[0]
    assert torch.equal(g0, g1)
    (c0 * w).sum().backward()
    assert torch.equal(lazy.grad, g0.sum(0, keepdim=True))


def test_get_emd_loss_value_and_capture():
    a, b, model, ref = case("cube", 3, 63, 63)
    radius = torch.tensor([0.5, 1.0, 2.0], device=DEV)
    want = float(np.mean(model["cost"] / np.array([0.5, 1.0, 2.0]) / 63))
    got = mu.get_emd_loss(dev(a), dev(b), radius)
    assert got.dim() == 0 and abs(got.item() - want) <= max(4 * np.abs(ref["cost"] - model["cost"]).max(), 8 * 2.0 ** -24 * 63 * model["dmax"]) / 63 / 0.5
    assert abs(mu.get_emd_loss(dev(a), dev(b), 0.5).item() - float(np.mean(model["cost"] / 0.5 / 63))) <= 1e-5 * want

    def body(x, y):
        x, y = x.detach().requires_grad_(True), y.detach().requires_grad_(True)
        loss = mu.get_emd_loss(x, y, 0.7)
        gx, gy = torch.autograd.grad(loss, (x, y))
        return loss.detach(), gx, gy
    x, y = dev(a), dev(b)
    eager = [t.clone() for t in body(x, y)]
    cap = spgan.CapturedBody(body, modules=(), warmup=1)
    for _ in range(3):
        out = cap(x, y)
    torch.cuda.synchronize()
    assert not cap.eager and cap._graph is not None
    for u, v in zip(out, eager):
        assert torch.equal(u, v)


def test_fused_route_keeps_no_plan_in_memory():
    B, n = 4, 1024
    a, b = am.clouds("cube", B, n, n, seed=4)
    x, y = dev(a, True), dev(b, True)
    ap.match_cost(x, y).sum().backward()                                  # warm: code objects, allocator pools
    x.grad = y.grad = None
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    c = ap.match_cost(x, y)
    c.sum().backward()
    torch.cuda.synchronize()
    outputs = 2 * B * n * 3 * 4 + B * 4                                   # the two gradients and the cost
    extra = torch.cuda.max_memory_allocated() - base - outputs
    print("fused forward + backward at (4,1024,1024): %d bytes above inputs and outputs; one pair's plan: %d" % (extra, n * n * 4))
    assert extra < n * n * 4


def test_pairwise_driver_equals_the_separate_calls():
    s = dev(am.clouds("sphere", 5, 128, 128, seed=6)[0])
    r = dev(am.clouds("cube", 7, 128, 128, seed=6)[1])
    want = torch.stack([torch.cat([ap.emd_approx_match(s[i:i + 1], r[j:j + 1]) for j in range(7)]) for i in range(5)])
    for bs in (512, 3):
        assert torch.equal(metrics.pairwise_emd(s, r, batch_size=bs, emd="match_cost"), want)
    assert torch.equal(gan_metrics.pairwise_dists(s, r, 4, "EMD", emd="match_cost"), want)
    assert torch.equal(metrics.emd_approx(s, r[:5], emd="match_cost"), ap.match_cost(s, r[:5]) / 128)
    assert torch.equal(metrics.EMD_CD(s, r[:5], emd="match_cost", reduced=False)["MMD-EMD"], ap.match_cost(s, r[:5]) / 128)
    res = metrics.compute_all_metrics(s, r, emd="match_cost")                  # evaluation_metrics.py:193: the references are xyz1 there
    m_rs = metrics.pairwise_emd(r, s, emd="match_cost")
    assert torch.equal(res["lgan_mmd-EMD"], metrics.lgan_mmd_cov(m_rs.t())["lgan_mmd"])
    assert torch.equal(m_rs[2, 3:4], ap.emd_approx_match(r[2:3], s[3:4]))


def test_default_keyword_is_the_auction_bit_for_bit():
    s = dev(am.clouds("sphere", 4, 128, 128, seed=8)[0])
    r = dev(am.clouds("cube", 6, 128, 128, seed=8)[1])

    def old_emd_approx(x, y):
        dist, _ = metrics.emdFunction.apply(x, y, 0.005, 50)
        return dist.sqrt().mean(dim=1)

    def old_pairwise(a, b, batch_size=512):
        S, R = a.shape[0], b.shape[0]
        out = torch.empty((S * R,), dtype=torch.float32, device=a.device)
        si = torch.arange(S, device=a.device).repeat_interleave(R)
        ri = torch.arange(R, device=a.device).repeat(S)
        for lo in range(0, S * R, batch_size):
            out[lo:lo + batch_size] = old_emd_approx(a[si[lo:lo + batch_size]], b[ri[lo:lo + batch_size]])
        return out.view(S, R)
    assert torch.equal(metrics.emd_approx(s, r[:4]), old_emd_approx(s, r[:4]))
    assert torch.equal(metrics.emd_approx(s, r[:4], emd="auction"), old_emd_approx(s, r[:4]))
    assert torch.equal(metrics.pairwise_emd(s, r, 5), old_pairwise(s, r, 5))
    assert torch.equal(gan_metrics.pairwise_dists(s, r, 16, "EMD"), old_pairwise(s, r, 16))
    assert torch.equal(metrics.EMD_CD(s, r[:4], reduced=False)["MMD-EMD"], old_emd_approx(s, r[:4]))
    res = metrics.compute_all_metrics(s, r)
    old_rs = old_pairwise(r, s)
    assert torch.equal(res["lgan_mmd-EMD"], metrics.lgan_mmd_cov(old_rs.t())["lgan_mmd"])
    assert torch.equal(res["lgan_cov-EMD"], metrics.lgan_mmd_cov(old_rs.t())["lgan_cov"])
