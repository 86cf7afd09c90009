"""GPU: the evaluation-metric kernels (csrc/metrics.hip, csrc/emd.hip, the set statistics of csrc/local_cd.hip) at evaluation
scale and at their edges, against the numpy models of tests/metrics_model.py (pinned to the reference on the CPU by
tests/test_metrics_model_cpu.py) and the reference's own numbers at 300 x 277 (golden G25).

What runs here that no earlier test ran: second and third strides and blocks of every set-statistic kernel, ties between elements
owned by different threads, up to 576 selection rounds; chamfer_pairs_kernel with N != M, ragged sizes, the masked tail of its
4-queries pass and the 128 KB dynamic-LDS opt-in; the first-minimum rule of nn_distance_kernel across LDS chunks without any
mismatch allowance; a 1100-to-1 backward gather; the auction's multi-tile sweep and its cross-lane merge rule; exact occupancy
counters.

Every comparison is exact, or one float32 ulp of a single rounding, or a bound the project already uses for the same kernel
(pairwise_cd: rtol 2e-5, atol 1e-6 of test_cd_metrics_golden; Chamfer gradients: rtol 1e-4, atol 1e-5 of
test_chamfer_forward_backward; pairwise_simple: rtol 1e-5 of G23's l2 / l1 test).

Measured on an MI355X: largest relative error of pairwise_cd against float64 on the fixture_rng clouds, per (S, R, N, M) --
(3, 2, 300, 517): 7.3e-08; (2, 3, 1100, 1030): 4.8e-08; (2, 2, 2049, 2047): 1.5e-08; (1, 2, 5, 4096): 1.1e-07; (1, 1, 1, 1): 8.1e-08;
(2, 2, 4096, 4096): 1.1e-07 (bound: rtol 2e-5, atol 1e-6).  Every exact comparison held; no kernel needed a change.  The file takes
15 s; its longest test is the 4096-point case at 6.6 s, of which 4.4 s is the float64 model.
Oracle cost on an 8-core CPU: orc.emd_auction at B = 2, n = 1500, eps 0.005 takes 0.6 s for 3 iterations (its last step hands
out some 400 points per cloud by take_bids) and 2.8 s for 300 (about 45 points left); the n = 1100 lattice pair 1.2 s over its four
iteration counts; orc.entropy_of_occupancy_grid on 70 x 300 points 0.3 s / 2.1 s / 3.6 s at resolutions 16 / 28 / 32.
"""
import numpy as np
import pytest
import torch

import local_cd_model as lm
import metrics_model as mm
from helpers import golden
from oracle import spgan_oracle as orc
from spgan import fixture_rng as fr

pytestmark = pytest.mark.gpu

KS = (1, 2, 6, 7, 576)
FAMILIES = ("free", "ties", "dup")
REF_MEAN_RTOL = 1e-6          # the reference's own float32 means (see tests/test_metrics_model_cpu.py)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def g25():
    d = golden("g25_set_stats.npz")
    return dict(zip([str(k) for k in d["keys"]], d["values"]))


def within_one_ulp(got, model):
    """`got` (a float32 result) is one of the two float32 neighbours of the float64 model value: a sum in double, rounded once."""
    return abs(float(got) - model) <= abs(float(np.spacing(np.float32(model))))          # (the "ties" means are negative)


def _sqrt_blocks(blocks, sq):
    return [b - mm.SQRT_SHIFT for b in blocks] if sq else list(blocks)


def _vote(entry, blocks, k, sq):
    """The ABI entry point itself, so that the prediction vector is read too.  -> (out [9] or [1], pred [n0 + n1])."""
    from spgan import _lib
    xx, xy, yy = (dev(b) for b in blocks)
    n0, n1 = xx.shape[0], yy.shape[0]
    out = torch.full((9 if entry == "spgan_two_sample_knn" else 1,), float("nan"), device="cuda")
    pred = torch.full((n0 + n1,), -7, dtype=torch.int32, device="cuda")
    st = getattr(_lib.load(), entry)(xx.data_ptr(), xy.data_ptr(), yy.data_ptr(), n0, n1, k, int(sq), out.data_ptr(), pred.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    assert st == 0
    return out.cpu().numpy(), pred.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- set statistics
@pytest.mark.parametrize("family", FAMILIES)
def test_lgan_mmd_cov_three_blocks(family, g25):
    """[300, 530] and its transpose: three column blocks with a ragged last one, three strides per row, planted equal minima."""
    from spgan import gan_metrics as gm, metrics
    d = mm.mmd_matrix(family)
    for sfx, m in (("", d), ("T", np.ascontiguousarray(d.T))):
        mmd, cov, mmd_smp = mm.mmd_cov(m)
        res = metrics.lgan_mmd_cov(dev(m))
        assert res["lgan_cov"].item() == float(np.float32(cov)), (family, sfx)
        assert within_one_ulp(res["lgan_mmd"].item(), mmd) and within_one_ulp(res["lgan_mmd_smp"].item(), mmd_smp), (family, sfx)
        if family == "free":
            assert res["lgan_cov"].item() == g25["mmdcov|wide%s|lgan_cov" % sfx]
            np.testing.assert_allclose(res["lgan_mmd"].item(), g25["mmdcov|wide%s|lgan_mmd" % sfx], rtol=REF_MEAN_RTOL)
            np.testing.assert_allclose(res["lgan_mmd_smp"].item(), g25["mmdcov|wide%s|lgan_mmd_smp" % sfx], rtol=REF_MEAN_RTOL)
    for axis in (0, 1):
        cov, mmd = lm.cov_mmd(d, axis)
        assert gm.COV(dev(d), axis) == float(np.float32(cov)), (family, axis)
        assert within_one_ulp(gm.MMD(dev(d), axis), mmd), (family, axis)
        if family == "free":
            assert gm.COV(dev(d), axis) == float(np.float32(g25["COV|wide|axis%d" % axis]))
            np.testing.assert_allclose(gm.MMD(dev(d), axis), g25["MMD|wide|axis%d" % axis], rtol=REF_MEAN_RTOL)


@pytest.mark.parametrize("sq", [False, True], ids=["plain", "sqrt"])
@pytest.mark.parametrize("family", FAMILIES)
def test_two_sample_votes_at_577_clouds(family, sq, g25):
    """n0 = 300, n1 = 277: both vote kernels, k up to every other cloud; all outputs and the prediction vectors equal the models."""
    from spgan import gan_metrics as gm, metrics
    blocks = _sqrt_blocks(mm.set_stat_blocks(family), sq)
    t = [dev(b) for b in blocks]
    label = np.r_[-np.ones(mm.N0, np.int32), np.ones(mm.N1, np.int32)]
    for k in KS:
        want, want_pred = mm.two_sample_knn(*blocks, k, sqrt=sq)
        got = metrics.knn(t[0], t[1], t[2], k, sqrt=sq)
        for key, v in want.items():
            assert np.float32(got[key].item()) == v, (family, sq, k, key, got[key].item(), v)
        out, pred = _vote("spgan_two_sample_knn", blocks, k, sq)
        assert np.array_equal(pred, want_pred), (family, sq, k, np.flatnonzero(pred != want_pred)[:8])
        assert np.array_equal(out, np.array([want[key] for key in mm.KEYS], np.float32))
        _, pm_want = lm.knn_pm(*blocks, k, sqrt=sq, return_pred=True)
        acc_want = float(np.float32((pm_want == label).sum()) / np.float32(mm.N0 + mm.N1))
        assert gm.KNN(t[0], t[1], t[2], k, sqrt=sq) == acc_want, (family, sq, k)
        out, pm = _vote("spgan_two_sample_knn_pm", blocks, k, sq)
        assert np.array_equal(pm, pm_want), (family, sq, k, np.flatnonzero(pm != pm_want)[:8])
        assert float(out[0]) == acc_want
        if family == "free":
            for key in mm.KEYS:
                assert np.float32(got[key].item()) == np.float32(g25["knn|k%d|sqrt%d|%s" % (k, sq, key)]), (k, sq, key)
            assert acc_want == g25["KNN|k%d|sqrt%d" % (k, sq)]


@pytest.mark.parametrize("n0,n1", [(1, 300), (300, 1)])
def test_two_sample_votes_with_a_single_cloud_on_one_side(n0, n1):
    label = np.r_[-np.ones(n0, np.int32), np.ones(n1, np.int32)]
    for family in ("free", "ties"):
        for sq in (False, True):
            blocks = _sqrt_blocks(mm.set_stat_blocks(family, n0, n1), sq)
            for k in (1, 2, 7, 300):
                want, want_pred = mm.two_sample_knn(*blocks, k, sqrt=sq)
                out, pred = _vote("spgan_two_sample_knn", blocks, k, sq)
                assert np.array_equal(pred, want_pred) and np.array_equal(out, np.array([want[key] for key in mm.KEYS], np.float32))
                _, pm_want = lm.knn_pm(*blocks, k, sqrt=sq, return_pred=True)
                out, pm = _vote("spgan_two_sample_knn_pm", blocks, k, sq)
                assert np.array_equal(pm, pm_want)
                assert out[0] == np.float32((pm_want == label).sum()) / np.float32(n0 + n1)


@pytest.mark.parametrize("S,R,D", [(37, 29, 1), (37, 29, 16), (5, 300, 33)])
def test_pairwise_simple_over_several_blocks(S, R, D):
    from spgan import gan_metrics as gm
    a, b = fr.normal("ps.a.%d.%d" % (S, D), (S, D)).numpy(), fr.normal("ps.b.%d.%d" % (R, D), (R, D)).numpy()
    df = a.astype(np.float64)[:, None, :] - b.astype(np.float64)[None, :, :]
    np.testing.assert_allclose(gm.pairwise_simple(dev(a), dev(b), 16, "l2").cpu().numpy(), (df ** 2).sum(-1), rtol=1e-5)
    np.testing.assert_allclose(gm.pairwise_simple(dev(a), dev(b), 16, "l1").cpu().numpy(), np.abs(df).sum(-1), rtol=1e-5)


# ------------------------------------------------------------------------------------------------------------------ pairwise_cd
def _pairwise_cd_case(S, R, N, M):
    from spgan import metrics
    tag = "%d.%d.%d.%d" % (S, R, N, M)
    # lattice clouds: exact integer sums, so a dropped, duplicated or clamped-but-counted point changes the result
    A, B = mm.lattice_clouds("pcd.la." + tag, (S, N, 3)), mm.lattice_clouds("pcd.lb." + tag, (R, M, 3))
    got = metrics.pairwise_cd(dev(A), dev(B))
    np.testing.assert_array_equal(got.cpu().numpy(), mm.pairwise_cd_exact(A, B))
    if N != M:
        assert torch.equal(got, metrics.pairwise_cd(dev(B), dev(A)).t())
    # fixture_rng clouds against float64
    A = (fr.normal("pcd.a." + tag, (S, N, 3)) * 0.5).numpy()
    B = (fr.normal("pcd.b." + tag, (R, M, 3)) * 0.5 + 0.1).numpy()
    got = metrics.pairwise_cd(dev(A), dev(B))
    want = mm.pairwise_cd_f64(A, B)
    err = float((np.abs(got.cpu().numpy() - want) / np.abs(want)).max())
    print("pairwise_cd (S, R, N, M) = (%d, %d, %d, %d): largest relative error against float64 %.3e" % (S, R, N, M, err))
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=2e-5, atol=1e-6)
    if N != M:
        np.testing.assert_allclose(metrics.pairwise_cd(dev(B), dev(A)).t().cpu().numpy(), want, rtol=2e-5, atol=1e-6)


@pytest.mark.parametrize("S,R,N,M", [(3, 2, 300, 517), (2, 3, 1100, 1030), (2, 2, 2049, 2047), (1, 2, 5, 4096), (1, 1, 1, 1)])
def test_pairwise_cd_ragged_and_unequal_sizes(S, R, N, M):
    """N != M, sizes that are no multiple of 256, the masked tail of the 4-queries pass (1100, 1030, 2049), one point."""
    _pairwise_cd_case(S, R, N, M)


def test_pairwise_cd_with_128_kb_of_dynamic_lds():
    """N + M = 8192: the only configuration that needs the opt-in above 64 KB of dynamic LDS (beside the static red[4]).  Its own
    test function: a refused launch is reported here as a status by check, not met in the middle of another test."""
    _pairwise_cd_case(2, 2, 4096, 4096)


def test_pairwise_cd_rejects_more_than_4096_points():
    from spgan import metrics
    a, b = torch.zeros((1, 4097, 3), device="cuda"), torch.zeros((1, 16, 3), device="cuda")
    with pytest.raises(RuntimeError, match="chamfer_pairs"):
        metrics.pairwise_cd(a, b)
    with pytest.raises(RuntimeError, match="chamfer_pairs"):
        metrics.pairwise_cd(b, a)


# ------------------------------------------------------------------------------------------- Chamfer index rule and backward
def test_chamfer_first_minimum_across_lds_chunks():
    """Lattice clouds with duplicated points (tests/test_metrics_model_cpu.py: no row is ambiguous in float32): indices exactly the
    first minimum, distances bit-equal, no mismatch allowance."""
    from spgan import metrics
    a, b = mm.chamfer_tie_clouds()
    d1, d2, i1, i2 = metrics.ChamferDistance()(dev(a), dev(b))
    for i in range(a.shape[0]):
        rmin, ridx, cmin, cidx = mm.nn_minima(a[i], b[i])
        np.testing.assert_array_equal(i1[i].cpu().numpy(), ridx)
        np.testing.assert_array_equal(i2[i].cpu().numpy(), cidx)
        np.testing.assert_array_equal(d1[i].cpu().numpy(), rmin.astype(np.float32))
        np.testing.assert_array_equal(d2[i].cpu().numpy(), cmin.astype(np.float32))
    assert i1.dtype == torch.int32 and (i1[:, :6] == 7).all() and (i2[:, 519] == 0).all()


def test_chamfer_backward_many_to_one():
    """All 1100 points of b (three chunks of the gather) choose a[0]; gradients against float64 autograd, bit-identical twice."""
    from spgan import metrics
    an, bn = mm.many_to_one_clouds()
    B, Na, Nb = an.shape[0], an.shape[1], bn.shape[1]
    w1 = fr.normal("m2o.w1", (B, Na))
    w2 = fr.uniform("m2o.w2", (B, Nb), 0.5, 1.5)
    grads = []
    for _ in range(2):
        a, b = dev(an).requires_grad_(True), dev(bn).requires_grad_(True)
        d1, d2, i1, i2 = metrics.ChamferDistance()(a, b)
        ((d1 * w1.cuda()).sum() + (d2 * w2.cuda()).sum()).backward()
        grads.append((a.grad.clone(), b.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    assert (i2 == 0).all()
    ac, bc = torch.from_numpy(an).double().requires_grad_(True), torch.from_numpy(bn).double().requires_grad_(True)
    d = ((ac[:, :, None, :] - bc[:, None, :, :]) ** 2).sum(-1)
    # a -> b is a search among clustered points from far away: any index whose float64 distance is within float32 rounding of the
    # minimum is a first minimum of the float32 search; the model's gradient is routed through the kernel's choice
    i1c = i1.cpu().long()
    r1 = torch.gather(d, 2, i1c[:, :, None]).squeeze(2)
    assert (r1.detach() <= d.detach().min(2)[0] * (1 + 1e-6)).all()
    assert (i1c == d.detach().argmin(2)).float().mean() > 0.99
    r2 = d.min(1)[0]
    np.testing.assert_allclose(d1.detach().cpu().numpy(), r1.detach().numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(d2.detach().cpu().numpy(), r2.detach().numpy(), rtol=1e-5, atol=1e-7)
    ((r1 * w1.double()).sum() + (r2 * w2.double()).sum()).backward()
    np.testing.assert_allclose(grads[0][0].cpu().numpy(), ac.grad.numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(grads[0][1].cpu().numpy(), bc.grad.numpy(), rtol=1e-4, atol=1e-5)
    assert np.abs(ac.grad[:, 0].numpy()).min() > 50                                  # the 1100-term sums are what is compared


# -------------------------------------------------------------------------------------------------------------------------- EMD
def _emd_equals_oracle(a, b, eps, iters):
    from spgan import metrics
    dist, assign = metrics.emdModule()(dev(a), dev(b), eps, iters)
    od, oa = orc.emd_auction(a, b, eps, iters)
    assert np.array_equal(assign.cpu().numpy(), oa), (a.shape, eps, iters, int((assign.cpu().numpy() != oa).sum()))
    np.testing.assert_array_equal(dist.cpu().numpy(), od)
    return oa


@pytest.mark.parametrize("iters", [3, 300])
def test_emd_two_tiles_equals_the_oracle(iters):
    """n = 1500: two EMD_TILEs, the second ragged.  3 iterations end in take_bids over some 400 unassigned points, 300 leave few."""
    a, b = mm.emd_sets(2, 1500)
    oa = _emd_equals_oracle(a, b, 0.005, iters)
    assert (oa >= 0).all() and (oa >= 1024).any()


def test_emd_merge_rule_on_a_lattice():
    """n = 1100 on a 5^3 lattice: for every bidder several objects share the best value, on different lanes and in both tiles;
    with one iteration the assignment IS each bidder's first best object (merge's lowest-index rule, take_bids)."""
    a, b = mm.emd_lattice_pair()
    for iters in (1, 2, 10, 40):
        oa = _emd_equals_oracle(a, b, 0.005, iters)
        if iters == 1:
            same = (a[:, :, None, :] == b[:, None, :, :]).all(-1)
            has = same.any(2)
            assert np.array_equal(oa[has], same.argmax(2)[has])


@pytest.mark.parametrize("n", [1, 63])
def test_emd_fewer_objects_than_lanes(n):
    a, b = mm.emd_sets(2, 64)
    a, b = np.ascontiguousarray(a[:, :n]), np.ascontiguousarray(b[:, :n])
    for iters in (1, 2, 50):
        _emd_equals_oracle(a, b, 0.005, iters)


# --------------------------------------------------------------------------------------------------------------- occupancy grid
@pytest.mark.parametrize("res,sphere", mm.OCCUPANCY_CASES)
def test_occupancy_counters_are_exact(res, sphere):
    """Points a quarter spacing at most from their cell centre (unambiguous in float32 and float64:
    tests/test_metrics_model_cpu.py): the counters equal the oracle's exactly, the Bernoulli entropy to 1e-12.  Five cells are
    hit by all 70 clouds, 70 by exactly one, many several times by one cloud."""
    from spgan import gan_metrics as gm, metrics
    grid, spacing = orc.unit_cube_grid_point_cloud(res, sphere)
    pts, cell = mm.grid_clouds("occ.%d" % res, grid, spacing, mm.OCC_S, mm.OCC_N)
    ent, cnt = metrics.entropy_of_occupancy_grid(dev(pts), res, sphere)
    o_ent, o_cnt = orc.entropy_of_occupancy_grid(pts, res, sphere)
    np.testing.assert_array_equal(cnt.cpu().numpy(), o_cnt)
    assert abs(ent.item() - o_ent) <= 1e-12, (ent.item(), o_ent)
    assert np.array_equal(o_cnt, np.bincount(cell.ravel(), minlength=len(o_cnt)))
    np.testing.assert_array_equal(gm.voxel_counts(dev(pts)).cpu().numpy(), lm.voxel_counts(pts))
