"""GPU: the MST expansion penalty, minimum-density sampling and gather_operation (csrc/expansion.hip) against tests/expansion_model.py.

Exact cases (coordinates = small integers * 0.25, so squared lengths are exact and both sides round the same square roots): bit-equal
against the model in float32, which sums the edge lengths in the kernel's documented order (include/spgan_hip.h: per lane l the entries
l, 64+l, 128+l, .. in ascending order, then s_l += s_(l xor o) for o = 32, 16, 8, 4, 2, 1).  Random clouds: against the float64 model,
after asserting on the CPU that no discrete decision of the case is closer than float32 can resolve."""
import functools

import numpy as np
import pytest
import torch

import expansion_cases as ec
import expansion_model as em
import spgan

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def run(xyz, p, alpha, grad=None):
    x = torch.from_numpy(np.ascontiguousarray(xyz)).to(DEV).requires_grad_(grad is not None)
    dist, assignment, mml = spgan.expansionPenaltyModule()(x, p, alpha)
    out = dict(dist=dist.detach().cpu().numpy(), assignment=assignment.cpu().numpy(), mean_mst_length=mml.cpu().numpy())
    if grad is not None:
        assert not assignment.requires_grad and not mml.requires_grad
        (gx,) = torch.autograd.grad((dist * torch.from_numpy(grad).to(DEV)).sum(), x)
        out["grad"] = gx.cpu().numpy()
    return out


@pytest.mark.parametrize("name", sorted(ec.EXACT_CASES))
def test_exact_cases_are_bit_equal(name):
    xyz, p, alpha = ec.EXACT_CASES[name]
    want = em.expansion_forward(xyz, p, alpha, np.float32)
    got = run(xyz, p, alpha)
    assert got["assignment"].dtype == np.int32 and got["dist"].dtype == np.float32
    np.testing.assert_array_equal(got["assignment"], want["assignment"])
    assert np.array_equal(got["dist"].view(np.uint32), want["dist"].astype(np.float32).view(np.uint32))
    assert np.array_equal(got["mean_mst_length"].view(np.uint32), want["mean_mst_length"].astype(np.float32).view(np.uint32))
    assert (want["assignment"] >= 0).sum() == xyz.shape[1] - xyz.shape[1] // p          # alpha = 0.5: every tree edge is reported
    if name == "pair":
        np.testing.assert_array_equal(got["assignment"], [[-1, 0]])                      # the larger index owns the edge
    if name == "collinear512":
        assert want["rounds"] == 256


@functools.lru_cache(maxsize=None)
def reference(B, n, p, seed, alpha):
    xyz = ec.random_cloud(B, n, seed)
    return xyz, em.expansion_forward(xyz, p, alpha, np.float64)


@pytest.mark.parametrize("alpha", ec.ALPHAS)
@pytest.mark.parametrize("case", ec.RANDOM_CASES, ids=lambda c: "B%d-n%d-p%d" % c[:3])
def test_random_clouds_match_float64_model(case, alpha):
    B, n, p, seed = case
    xyz, want = reference(B, n, p, seed, alpha)
    # float32 cannot turn any discrete decision of this case: every Prim step's best and runner-up, and the chosen vertex's nearest and
    # second nearest tree vertex (which decides its parent), differ by more than 2e-6 relative; no owned edge lies within 1e-4 relative
    # of its threshold
    print("margins", case, alpha, want["step_gap"], want["parent_gap"], want["thr_margin"])
    assert want["step_gap"] > 2e-6 and want["parent_gap"] > 2e-6, (want["step_gap"], want["parent_gap"])
    assert want["thr_margin"] > 1e-4, want["thr_margin"]
    got = run(xyz, p, alpha)
    np.testing.assert_array_equal(got["assignment"], want["assignment"])
    assert p < 64 or (want["assignment"] >= 0).any()
    # an edge length: three products, two sums and a correctly rounded sqrt of float32 inputs
    np.testing.assert_allclose(got["dist"], want["dist"], rtol=2e-6, atol=0)
    # the mean: per lane a serial sum of at most 8 terms, then 6 butterfly levels -- at most 13 additions deep, 13 * 2^-24 = 7.8e-7 --
    # on terms within 2.4e-7 each, one division and (mean_mst_length) a second such sum over at most 8 primitive means and a division:
    # below 2e-6 in all
    np.testing.assert_allclose(got["mean_mst_length"], want["mean_mst_length"], rtol=2e-6, atol=0)


@pytest.mark.parametrize("case", [ec.RANDOM_CASES[1], ec.RANDOM_CASES[6], ec.RANDOM_CASES[7]], ids=lambda c: "B%d-n%d-p%d" % c[:3])
def test_random_cloud_is_bit_equal_to_the_float32_model(case):
    """The documented arithmetic -- every product, sum and square root rounded on its own, the sums in the stated order -- pins the
    outputs bit for bit wherever the float32 tree is the float64 one (asserted above for these cases), not only on lattices; in both
    kernel shapes (p <= 256: a wave per primitive, above: a workgroup per primitive)."""
    B, n, p, seed = case
    xyz = ec.random_cloud(B, n, seed)
    want = em.expansion_forward(xyz, p, 1.0, np.float32)
    np.testing.assert_array_equal(want["assignment"], reference(B, n, p, seed, 1.0)[1]["assignment"])
    got = run(xyz, p, 1.0)
    np.testing.assert_array_equal(got["assignment"], want["assignment"])
    assert np.array_equal(got["dist"].view(np.uint32), want["dist"].astype(np.float32).view(np.uint32))
    assert np.array_equal(got["mean_mst_length"].view(np.uint32), want["mean_mst_length"].astype(np.float32).view(np.uint32))


def test_large_alpha_reports_nothing():
    B, n, p, seed = ec.RANDOM_CASES[1]
    got = run(ec.random_cloud(B, n, seed), p, 100.0)
    assert np.all(got["dist"] == 0) and np.all(got["assignment"] == -1)
    np.testing.assert_allclose(got["mean_mst_length"], reference(B, n, p, seed, 1.0)[1]["mean_mst_length"], rtol=2e-6, atol=0)


@pytest.mark.parametrize("case", [ec.RANDOM_CASES[1], ec.RANDOM_CASES[3], ec.RANDOM_CASES[5]], ids=lambda c: "B%d-n%d-p%d" % c[:3])
def test_backward_is_the_closed_form_on_the_owners(case):
    B, n, p, seed = case
    xyz = ec.random_cloud(B, n, seed)
    g = np.random.default_rng(11).standard_normal((B, n)).astype(np.float32)
    got = run(xyz, p, 0.9, grad=g)
    want = em.expansion_backward(xyz, g, got["assignment"])
    own = got["assignment"] >= 0
    assert own.any() and (~own).any()
    assert np.all(got["grad"][~own] == 0)
    np.testing.assert_allclose(got["grad"], want, rtol=1e-6, atol=0)


def test_forward_and_backward_repeat_bit_for_bit():
    B, n, p, seed = ec.RANDOM_CASES[2]
    xyz = ec.random_cloud(B, n, seed)
    g = np.random.default_rng(12).standard_normal((B, n)).astype(np.float32)
    a, b = run(xyz, p, 1.0, grad=g), run(xyz, p, 1.0, grad=g)
    for k in ("dist", "mean_mst_length", "grad"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    np.testing.assert_array_equal(a["assignment"], b["assignment"])


def test_size_rules_raise():
    x = torch.zeros(1, 16, 3, device=DEV)
    for p in (1, 5, 513):
        with pytest.raises(ValueError):
            spgan.expansionPenaltyModule()(x, p, 1.5)
    with pytest.raises(ValueError):
        spgan.minimum_density_sample(x, 17, torch.ones(1, device=DEV))


@pytest.mark.parametrize("name", sorted(ec.MDS_CASES))
def test_minimum_density_sample(name):
    x, npoint, L, split = ec.mds_cloud(name)
    B, n, _ = x.shape
    out = spgan.minimum_density_sample(torch.from_numpy(x).to(DEV), npoint, torch.from_numpy(L).to(DEV), split=split)
    assert out.dtype == torch.int32 and tuple(out.shape) == (B, npoint)
    out = out.cpu().numpy()
    assert out.min() >= 0 and out.max() < n
    differ = 0
    for b in range(B):
        picks = out[b]
        assert picks[0] == 0 and len(set(picks.tolist())) == npoint
        # the float64 model along the kernel's own picks: each pick is a least-density point up to the float32 error of the densities.
        # Per term the argument of exp is off by at most (4A + 2) 2^-24, A = max d/t <= 80, and the weight is at most 2: 4e-5 per step.
        _, picked, least, A = em.mds(x[b], npoint, L[b], split=split, follow=picks)
        assert A <= 80, A
        j = np.arange(npoint)
        worst = float(np.max(picked[1:] - least[1:] - 4e-5 * j[1:])) if npoint > 1 else 0.0
        print("mds", name, b, "A", A, "worst excess over the bound", worst)
        assert np.all(picked[1:] <= least[1:] + 4e-5 * j[1:])
        own = em.mds(x[b], npoint, L[b], split=split)[0]
        differ += int(np.sum(own != picks))
        if name in ("default_split", "split100"):
            assert not np.array_equal(own, em.mds(x[b], npoint, L[b], split=n)[0]), "the weight does not change this sequence"
    assert differ <= 0.05 * B * npoint, differ
    if name == "all":
        assert sorted(out[0].tolist()) == list(range(n))


def test_minimum_density_sample_beyond_the_register_paths():
    """n = 16400 > 16384: the densities live in the workspace.  Same checks, few steps."""
    rng = np.random.default_rng(9)
    n, npoint, L = 16400, 6, np.float32(0.05)
    x = (rng.random((1, n, 3)) * 0.5).astype(np.float32)
    out = spgan.minimum_density_sample(torch.from_numpy(x).to(DEV), npoint, torch.full((1,), float(L), device=DEV)).cpu().numpy()[0]
    _, picked, least, A = em.mds(x[0], npoint, L, follow=out)
    assert A <= 80 and out[0] == 0 and len(set(out.tolist())) == npoint
    assert np.all(picked[1:] <= least[1:] + 4e-5 * np.arange(1, npoint))


@pytest.mark.parametrize("n", [8200, 13700])
def test_minimum_density_sample_lds_and_global_coordinates(n):
    """8192 < n <= 13600: coordinates in LDS; 13600 < n <= 16384: re-read from global memory."""
    rng = np.random.default_rng(n)
    npoint, L = 6, np.float32(0.05)
    x = (rng.random((2, n, 3)) * 0.5).astype(np.float32)
    out = spgan.minimum_density_sample(torch.from_numpy(x).to(DEV), npoint, torch.full((2,), float(L), device=DEV)).cpu().numpy()
    for b in range(2):
        _, picked, least, A = em.mds(x[b], npoint, L, follow=out[b])
        assert A <= 80 and out[b, 0] == 0 and len(set(out[b].tolist())) == npoint
        assert np.all(picked[1:] <= least[1:] + 4e-5 * np.arange(1, npoint))


def test_gather_operation():
    rng = np.random.default_rng(4)
    B, C, N, m = 3, 5, 37, 50
    f = torch.from_numpy(rng.standard_normal((B, C, N)).astype(np.float32)).to(DEV).requires_grad_(True)
    idx = torch.from_numpy(rng.integers(0, N, (B, m)).astype(np.int32)).to(DEV)          # m > N: duplicates
    out = spgan.gather_operation(f, idx)
    want = torch.gather(f.detach(), 2, idx.long()[:, None, :].expand(B, C, m))
    assert torch.equal(out, want)
    g = torch.from_numpy(rng.standard_normal((B, C, m)).astype(np.float32)).to(DEV)
    (df,) = torch.autograd.grad((out * g).sum(), f)
    ref = torch.zeros(B, C, N, dtype=torch.float64)
    for b in range(B):
        ref[b].index_add_(1, idx[b].long().cpu(), g[b].double().cpu())
    np.testing.assert_allclose(df.cpu().numpy(), ref.numpy(), rtol=1e-6, atol=1e-6)
    (df2,) = torch.autograd.grad((spgan.gather_operation(f, idx) * g).sum(), f)
    assert torch.equal(df, df2)
