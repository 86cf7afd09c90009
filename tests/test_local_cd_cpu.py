"""CPU: the float64 model of the local-shape Chamfer and the GAN_metrics pieces (tests/local_cd_model.py) against G23, the
reference's own functions (tests/golden/make_golden_local_cd.py).  The GPU tests then hold the kernels to this model."""
import numpy as np
import pytest
import torch

import local_cd_model as lm
from helpers import golden


@pytest.fixture(scope="module")
def g23():
    return golden("g23_local_cd.npz")


def test_lattice_knn_order(g23):
    """Exact ties on a lattice with duplicated points: ascending distance, the lower index first."""
    lat = g23["lat"]
    for K in (8, 20, 32):
        idx = lm.knn_idx(lat, lat, K)
        np.testing.assert_array_equal(idx, g23["lat_idx_k%d" % K])
        grouped = lat[0][idx[0]].transpose(2, 0, 1)[None]
        np.testing.assert_array_equal(grouped, g23["lat_grouped_k%d" % K])
    # the query itself comes first; a duplicated point's first neighbour is its lower-index twin
    np.testing.assert_array_equal(lm.knn_idx(lat, lat, 1)[0, :, 0], np.r_[np.arange(64), np.arange(8)])


def test_get_local_pair_matches_reference(g23):
    p1, p2 = (torch.from_numpy(g23[k]).double().transpose(1, 2).contiguous() for k in ("glp_pt1", "glp_pt2"))
    m, c = lm.local_pair(p1, p2, 20)
    np.testing.assert_allclose(m.item(), g23["glp_mu_64"], rtol=1e-10)
    np.testing.assert_allclose(c.item(), g23["glp_var_64"], rtol=1e-10)
    # the reference's float32 run differs from float64 by its own rounding only
    np.testing.assert_allclose(g23["glp_mu_32"], g23["glp_mu_64"], rtol=1e-3)


def test_get_local_pair_gradients_match_reference(g23):
    p1 = torch.from_numpy(g23["glp_pt1"]).double().transpose(1, 2).contiguous().requires_grad_(True)
    p2 = torch.from_numpy(g23["glp_pt2"]).double().transpose(1, 2).contiguous().requires_grad_(True)
    m, c = lm.local_pair(p1, p2, 20)
    for val, tag in ((m, "gmu"), (c, "gvar")):
        g1, g2 = torch.autograd.grad(val, (p1, p2), retain_graph=True)
        for got, key in ((g1, "glp_%s_pt1" % tag), (g2, "glp_%s_pt2" % tag)):
            want = g23[key].transpose(0, 2, 1)
            err = np.abs(got.numpy() - want).max() / max(np.abs(want).max(), 1e-30)
            assert err < 1e-3, (key, err)


def test_chamfer_and_local_cd_match_reference(g23):
    for D in (3, 9):
        x, y = torch.from_numpy(g23["cl_x%d" % D]).double(), torch.from_numpy(g23["cl_y%d" % D]).double()
        np.testing.assert_allclose(lm.chamfer(x, y)[0].item(), g23["cl%d_64" % D], rtol=1e-10)
    a, b = torch.from_numpy(g23["lcd_pt1"]).double(), torch.from_numpy(g23["lcd_pt2"]).double()
    m, c = lm.local_pair(a, b, 8)
    np.testing.assert_allclose(m.item(), g23["lcd_mu_64"], rtol=1e-10)
    np.testing.assert_allclose(c.item(), g23["lcd_var_64"], rtol=1e-10)


def test_pairwise_matrix_and_chunk_sum_quirk(g23):
    mat = lm.pairwise_local(g23["pw_sample"], g23["pw_ref"], 8)
    for t, dist in enumerate(("CD_M", "CD_C")):
        np.testing.assert_allclose(mat[..., t], g23["plcd_%s_bs1_64" % dist], rtol=1e-10)
        quirk = g23["plcd_%s_bs4_64" % dist]
        assert quirk.shape == (8, 3)                                   # ceil(10 / 4) chunk sums, not [S,R]
        np.testing.assert_allclose(lm.chunk_sums(mat[..., t], 4), quirk, rtol=1e-10)


def test_cov_mmd_from_reference_matrices(g23):
    for dist in ("CD", "CD_M", "CD_C"):
        sr = g23["pd_%s_sr_64" % dist]
        cov, mmd = lm.cov_mmd(sr)
        assert cov == g23["cam_%s_COV_64" % dist]
        # the reference rounds the mean to float32 (`.mean().float()`)
        np.testing.assert_allclose(mmd, g23["cam_%s_MMD_64" % dist], rtol=1e-7)
        np.testing.assert_allclose(lm.cov_mmd(sr.T)[1], g23["camt_%s_MMD_t_64" % dist], rtol=1e-7)


def f32(x):
    return float(np.float32(x))                                       # the reference's accuracy is a float32 mean


def test_knn_pm_vote(g23):
    for k in (1, 3, 6):
        assert f32(lm.knn_pm(g23["knn_xx"], g23["knn_xy"], g23["knn_yy"], k)) == g23["knn_k%d" % k]
        assert f32(lm.knn_pm(g23["knn_xx"] - 0.5, g23["knn_xy"], g23["knn_yy"], k, sqrt=True)) == g23["knn_sqrt_k%d" % k]
    # 4 samples, 3 references, k = 6 = every other cloud: each sample's vote is a 3-3 tie, which predicts "reference", and each
    # reference sees 4 samples against 2 references; so no cloud is classified correctly (the 0/1-label vote of
    # spgan.metrics.knn would call every sample correctly instead)
    got = lm.knn_pm(g23["tie_xx"], g23["tie_xy"], g23["tie_yy"], 6)
    assert f32(got) == g23["tie_k6"]
    assert got == 0.0


def test_jsd_point_count_histogram(g23):
    c1 = lm.voxel_counts(g23["jsd_c1"])
    np.testing.assert_allclose(c1 / c1.sum(), g23["voxel_c1"], rtol=0, atol=0)
    assert c1.sum() < g23["jsd_c1"].shape[0] * g23["jsd_c1"].shape[1]         # some points lie outside the cube
    np.testing.assert_allclose(lm.jsd(g23["jsd_c1"], g23["jsd_c2"]), g23["jsd"], rtol=1e-12)


def test_voxel_bins_are_half_open():
    e = -0.5 + np.arange(29) * (1.0 / 28)
    pts = np.array([[e[3], e[5], e[27]], [np.nextafter(np.float32(e[4]), np.float32(-1)), 0.0, 0.0], [0.5, 0.0, 0.0], [-0.5, -0.5, -0.5]],
                   np.float32)
    c = lm.voxel_counts(pts[None])
    assert c.sum() == 3                                                          # x = 0.5 lies outside
    assert c[0, 0, 0] == 1
