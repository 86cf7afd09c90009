"""CPU: the numpy models of the evaluation-metric kernels (tests/metrics_model.py, local_cd_model.knn_pm) against the reference's
own numbers -- G11, G23 and G25 (tests/golden/make_golden_set_stats.py: the reference's knn / lgan_mmd_cov / KNN / COV / MMD on
tie-free 300 x 277 and 300 x 530 matrices) -- and against the oracle, and the properties of the seeded inputs that
tests/test_metrics_scale_gpu.py relies on (no rounding ambiguity where it asserts exact indices).  The GPU tests then hold the
kernels to these models."""
import numpy as np
import pytest
import torch

import local_cd_model as lm
import metrics_model as mm
from helpers import golden
from oracle import spgan_oracle as orc

KS = (1, 2, 6, 7, 576)
# The reference takes its means in float32 over 277 to 530 values of (0, 1); a float32 sum of n terms added pairwise is off by up to
# about log2(n) * 2^-24 = 5.4e-7 of the sum.  The models' float64 means are compared with its numbers to 1e-6.
REF_MEAN_RTOL = 1e-6


@pytest.fixture(scope="module")
def g25():
    d = golden("g25_set_stats.npz")
    return dict(zip([str(k) for k in d["keys"]], d["values"]))


def _sqrt_blocks(blocks, sq):
    return [b - mm.SQRT_SHIFT for b in blocks] if sq else list(blocks)


def test_models_reproduce_g11():
    d = golden("g11_chamfer_metrics.npz")
    mmd, cov, mmd_smp = mm.mmd_cov(d["M_rs"].T)
    np.testing.assert_allclose(mmd, float(d["mmdcov|lgan_mmd"]), rtol=REF_MEAN_RTOL)
    np.testing.assert_allclose(mmd_smp, float(d["mmdcov|lgan_mmd_smp"]), rtol=REF_MEAN_RTOL)
    assert np.float32(cov) == d["mmdcov|lgan_cov"]
    out, pred = mm.two_sample_knn(d["M_rr"], d["M_rs"], d["M_ss"], 1)
    for k in ("acc_t", "acc_f", "acc"):
        assert out[k] == d["1nn|" + k], k
    assert pred.shape == (11,)


def test_models_reproduce_g23():
    g23 = golden("g23_local_cd.npz")
    xx, xy, yy = g23["knn_xx"], g23["knn_xy"], g23["knn_yy"]
    for k in (1, 3, 6):
        for sq, key in ((False, "knn_k%d"), (True, "knn_sqrt_k%d")):
            acc, pred = lm.knn_pm(xx - 0.5 if sq else xx, xy, yy, k, sqrt=sq, return_pred=True)
            assert np.float32(acc) == g23[key % k]
            label = np.r_[-np.ones(5, np.int32), np.ones(4, np.int32)]
            assert np.float32((pred == label).sum()) / np.float32(9) == g23[key % k]
    acc, pred = lm.knn_pm(g23["tie_xx"], g23["tie_xy"], g23["tie_yy"], 6, return_pred=True)
    assert acc == g23["tie_k6"] == 0.0 and np.array_equal(pred, [1, 1, 1, 1, -1, -1, -1])
    # the 0/1 vote on the same matrices: a 3-3 tie predicts the first set, so every sample is right and every reference wrong
    out, pred = mm.two_sample_knn(g23["tie_xx"], g23["tie_xy"], g23["tie_yy"], 6)
    assert np.array_equal(pred, [1] * 7) and out["acc_t"] == 1.0 and out["acc_f"] == 0.0
    for dist in ("CD", "CD_M", "CD_C"):
        sr = g23["pd_%s_sr_64" % dist]
        mmd, cov, _ = mm.mmd_cov(sr)
        assert cov == g23["cam_%s_COV_64" % dist]
        np.testing.assert_allclose(mmd, g23["cam_%s_MMD_64" % dist], rtol=1e-7)          # `.mean().float()` there
        np.testing.assert_allclose(mm.mmd_cov(sr.T)[0], g23["camt_%s_MMD_t_64" % dist], rtol=1e-7)


def test_free_matrices_are_tie_free_and_asymmetric():
    xx, xy, yy = mm.set_stat_blocks("free")
    assert xx.shape == (300, 300) and xy.shape == (300, 277) and yy.shape == (277, 277)
    assert not np.array_equal(xx, xx.T) and not np.array_equal(yy, yy.T)
    for sq in (False, True):
        assert mm.columns_tie_free(mm.joint_f32(*_sqrt_blocks((xx, xy, yy), sq), sqrt=sq))
    assert (xx - mm.SQRT_SHIFT).min() < 0
    wide = mm.mmd_matrix("free")
    assert wide.shape == (300, 530) and mm.columns_tie_free(wide) and mm.columns_tie_free(wide.T)
    # and the other two families are not: equal minima in different strides, equal k-th neighbours
    assert not mm.columns_tie_free(mm.joint_f32(*mm.set_stat_blocks("ties")))
    assert not mm.columns_tie_free(mm.joint_f32(*mm.set_stat_blocks("dup")))
    t = mm.mmd_matrix("ties")
    assert np.flatnonzero(t[0] == t[0].min()).tolist() == [3, 259, 515] and np.flatnonzero(t[1] == t[1].min()).tolist() == [515]


@pytest.mark.parametrize("sq", [False, True])
def test_vote_models_agree_with_the_oracle_and_each_other(sq):
    blocks = _sqrt_blocks(mm.set_stat_blocks("free"), sq)
    t = [torch.from_numpy(np.sqrt(np.abs(b)) if sq else b) for b in blocks]          # the oracle has no sqrt switch
    for k in KS:
        out, pred = mm.two_sample_knn(*blocks, k, sqrt=sq)
        want = orc.one_nn_accuracy(t[0], t[1], t[2], k)
        for key in ("acc_t", "acc_f", "acc"):
            assert out[key] == np.float32(want[key].item()), (k, key)
        assert out["tp"] + out["fn"] == 300 and out["fp"] + out["tn"] == 277
        # the +-1 vote differs from the 0/1 vote only in who wins an even split
        acc, pm = lm.knn_pm(*blocks, k, sqrt=sq, return_pred=True)
        idx = mm.neighbour_order(mm.joint_f32(*blocks, sqrt=sq), k)
        votes = (idx < 300).sum(0)
        assert np.array_equal(pm == -1, 2 * votes > k) and np.array_equal(pred == 1, 2 * votes >= k)


def test_mmd_cov_model_agrees_with_the_oracle_and_cov_mmd():
    for d in (mm.set_stat_blocks("free")[1], mm.mmd_matrix("free")):
        for m in (d, np.ascontiguousarray(d.T)):
            mmd, cov, mmd_smp = mm.mmd_cov(m)
            want = orc.lgan_mmd_cov(torch.from_numpy(m))
            np.testing.assert_allclose(mmd, want["lgan_mmd"].item(), rtol=REF_MEAN_RTOL)
            np.testing.assert_allclose(mmd_smp, want["lgan_mmd_smp"].item(), rtol=REF_MEAN_RTOL)
            assert np.float32(cov) == np.float32(want["lgan_cov"].item())
            assert lm.cov_mmd(m, 1) == (cov, mmd) and lm.cov_mmd(m, 0) == (mm.mmd_cov(m.T)[1], mmd_smp)


def test_models_reproduce_the_reference_at_evaluation_size(g25):
    blocks = mm.set_stat_blocks("free")
    label = np.r_[-np.ones(300, np.int32), np.ones(277, np.int32)]
    for sq in (False, True):
        b = _sqrt_blocks(blocks, sq)
        for k in KS:
            out, _ = mm.two_sample_knn(*b, k, sqrt=sq)
            for key, v in out.items():
                assert v == np.float32(g25["knn|k%d|sqrt%d|%s" % (k, sq, key)]), (k, sq, key)
            acc, pm = lm.knn_pm(*b, k, sqrt=sq, return_pred=True)
            assert float(np.float32((pm == label).sum()) / np.float32(577)) == g25["KNN|k%d|sqrt%d" % (k, sq)] == float(np.float32(acc))
    for tag, d in (("xy", blocks[1]), ("wide", mm.mmd_matrix("free"))):
        for sfx, m in (("", d), ("T", d.T)):
            mmd, cov, mmd_smp = mm.mmd_cov(m)
            np.testing.assert_allclose(mmd, g25["mmdcov|%s%s|lgan_mmd" % (tag, sfx)], rtol=REF_MEAN_RTOL)
            np.testing.assert_allclose(mmd_smp, g25["mmdcov|%s%s|lgan_mmd_smp" % (tag, sfx)], rtol=REF_MEAN_RTOL)
            assert np.float32(cov) == np.float32(g25["mmdcov|%s%s|lgan_cov" % (tag, sfx)])
        for axis in (0, 1):
            cov, mmd = lm.cov_mmd(d, axis)
            assert cov == g25["COV|%s|axis%d" % (tag, axis)]
            np.testing.assert_allclose(mmd, g25["MMD|%s|axis%d" % (tag, axis)], rtol=REF_MEAN_RTOL)


def test_lattice_chamfer_model():
    """pairwise_cd_exact is pairwise_cd_f64 rounded the kernel's way; on lattice inputs float32 distances are the float64 ones."""
    A, B = mm.lattice_clouds("cdmodel.a", (2, 37, 3)), mm.lattice_clouds("cdmodel.b", (3, 50, 3))
    assert np.abs(A).max() <= 1.0 and np.array_equal(A * 16, np.rint(A * 16))
    ex, f64 = mm.pairwise_cd_exact(A, B), mm.pairwise_cd_f64(A, B)
    assert ex.dtype == np.float32 and ex.shape == (2, 3)
    np.testing.assert_allclose(ex, f64, rtol=2e-7)
    C = mm.lattice_clouds("cdmodel.c", (2, 50, 3))                          # the oracle's pairwise_cd needs N == M
    np.testing.assert_allclose(mm.pairwise_cd_f64(C, B), orc.pairwise_cd(torch.from_numpy(C).double(), torch.from_numpy(B).double()).numpy(),
                               rtol=1e-12, atol=1e-12)
    with pytest.raises(AssertionError, match="lattice"):
        mm.pairwise_cd_exact(A + np.float32(0.001), B)
    # chunked search = one-shot search, first occurrence kept across chunks
    r1 = mm.nn_minima(A[0], B[0], chunk_bytes=8 * 50 * 5)
    r2 = mm.nn_minima(A[0], B[0])
    assert all(np.array_equal(x, y) for x, y in zip(r1, r2))


def test_chamfer_tie_inputs_have_no_ambiguous_row():
    """Where the GPU test asserts exact indices, float32 rounding decides nothing: every float32 distance (in the kernels' operation
    order, and in any other) equals the float64 one, so the only ties are exact ones and the first-minimum rule settles them."""
    a, b = mm.chamfer_tie_clouds()
    assert a.shape == (2, 300, 3) and b.shape == (2, 1100, 3)
    d32 = lm.d2_f32(a, b)
    d64 = ((a.astype(np.float64)[:, :, None, :] - b.astype(np.float64)[:, None, :, :]) ** 2).sum(-1)
    assert np.array_equal(d32.astype(np.float64), d64)
    for i in range(2):
        rmin, ridx, cmin, cidx = mm.nn_minima(a[i], b[i])
        assert np.array_equal(ridx, d64[i].argmin(1)) and np.array_equal(cidx, d64[i].argmin(0))
        assert ridx[0] == 7 and d64[i][0, 7] == d64[i][0, 519] == 0.0                 # equal candidates in chunks 0 and 1: the first
        assert (ridx[:6] == 7).all() and ridx[20] <= 100 and d64[i][20, 100] == d64[i][20, 1030] == 0.0
        assert cidx[7] == 0 and cidx[519] == 0
        ties_a = ((d64[i] == rmin[:, None]).sum(1) > 1).sum()
        ties_b = ((d64[i] == cmin[None, :]).sum(0) > 1).sum()
        assert ties_a >= 20 and ties_b >= 60, (ties_a, ties_b)                          # plenty of rows where the rule decides


def test_many_to_one_inputs():
    a, b = mm.many_to_one_clouds()
    for i in range(2):
        rmin, ridx, cmin, cidx = mm.nn_minima(a[i], b[i])
        assert (cidx == 0).all()
        d = ((a[i].astype(np.float64)[:, None, :] - b[i].astype(np.float64)[None, :, :]) ** 2).sum(-1)
        two_b = np.sort(d, axis=0)[:2]
        assert (two_b[1] > 4 * two_b[0]).all()          # b -> a: a[0] by a wide margin, nothing for float32 rounding to decide
        # a -> b is a search among 1100 clustered points from far away: near-ties exist there (the GPU test accepts any index whose
        # float64 distance is within float32 rounding of the minimum, and routes the model's gradient through it)
        assert len(np.unique(ridx)) > 30


def test_emd_lattice_inputs_tie_across_lanes_and_tiles():
    a, b = mm.emd_lattice_pair()
    assert a.shape == (2, 1100, 3)
    for i in range(2):
        same = (a[i][:, None, :] == b[i][None, :, :]).all(-1)                           # objects at the bidder's own place: value 3
        many = same.sum(1) >= 2
        assert many.mean() > 0.9
        first = same.argmax(1)
        last = 1099 - same[:, ::-1].argmax(1)
        assert (many & (first < 1024) & (last >= 1024)).sum() > 100                      # equal best objects in both tiles
        assert (many & ((first % 64) != (last % 64))).sum() > 500                        # and on different lanes


@pytest.mark.parametrize("res,sphere", mm.OCCUPANCY_CASES)
def test_occupancy_inputs_are_unambiguous(res, sphere):
    """Cell centres plus at most a quarter of the spacing per axis: the nearest kept cell is the constructed one in float32 and in
    float64 alike (the nearest other cell is at least 0.5 spacing^2 farther), so exact counters can be demanded of the kernel."""
    grid, spacing = orc.unit_cube_grid_point_cloud(res, sphere)
    axis = orc.unit_cube_grid_point_cloud(res, False)[0][:, 0, 0, 0]
    pts, cell = mm.grid_clouds("occ.%d" % res, grid, spacing, mm.OCC_S, mm.OCC_N)
    assert pts.shape == (70, 300, 3) and pts.dtype == np.float32
    assert np.array_equal(mm.nearest_cells(pts, grid, axis, np.float32), cell.ravel())
    assert np.array_equal(mm.nearest_cells(pts, grid, axis, np.float64), cell.ravel())
    G = grid.reshape(-1, 3).shape[0]
    clouds_per_cell = np.zeros(G, np.int64)
    for s in range(70):
        clouds_per_cell[np.unique(cell[s])] += 1
    assert (clouds_per_cell == 70).sum() >= 5 and (clouds_per_cell == 1).sum() >= 70
    assert (np.bincount(cell.ravel(), minlength=G) > clouds_per_cell).any()          # cells hit several times by one cloud
    if res == 16:                                                                     # the oracle's search finds the same cells
        ent, cnt = orc.entropy_of_occupancy_grid(pts, res, sphere)
        assert np.array_equal(cnt, np.bincount(cell.ravel(), minlength=G))
        p = clouds_per_cell[clouds_per_cell > 0] / 70.0
        q = 1.0 - p
        h = -(p * np.log(p) + np.where(q > 0, q * np.log(np.where(q > 0, q, 1.0)), 0.0))
        assert abs(ent - h.sum() / G) <= 1e-12
