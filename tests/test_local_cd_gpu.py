"""GPU: the local-shape Chamfer kernels (csrc/local_cd.hip) and the GAN_metrics drivers (spgan/gan_metrics.py).

  * knn_moments: indices equal the CPU model (tests/local_cd_model.py) exactly, on tie-free inputs and on a lattice with duplicated
    points; the moments agree with the model to float32 rounding;
  * ChamferLoss (3-D, 9-D), local_CD and get_local_pair against G23 (the reference's own functions), at ten times the reference's
    own float32-vs-float64 gap recorded in G23; gradients against float64 autograd of the model given the same indices/argmins;
  * forward values and gradients are bit-identical across runs;
  * pairwise_local_cd equals a local_CD loop pair by pair, its ss diagonal is exactly 0, s != r is asymmetric; full size 64x64x2048;
  * the drivers, KNN's +-1 vote and the JSD histogram against G23."""
import numpy as np
import pytest
import torch

import local_cd_model as lm
from helpers import golden
from spgan import gan_metrics as gm
from spgan import losses, metrics

pytestmark = pytest.mark.gpu
GAP_FACTOR = 10.0          # tolerance = GAP_FACTOR x |reference float32 - reference float64| / |float64| (floored at 1e-6)


@pytest.fixture(scope="module")
def g23():
    return golden("g23_local_cd.npz")


def _tol(g23, key):
    v32, v64 = float(g23[key + "_32"]), float(g23[key + "_64"])
    return GAP_FACTOR * max(abs(v32 - v64) / abs(v64), 1e-6)


def _close(got, g23, key):
    want = float(g23[key + "_64"])
    rel = abs(float(got) - want) / abs(want)
    assert rel <= _tol(g23, key), (key, float(got), want, rel, _tol(g23, key))


def _rand(shape, seed, scale=0.3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale)


@pytest.mark.parametrize("K", [1, 8, 20, 32])
def test_knn_moments_indices_and_moments(K):
    q, c = _rand((3, 300, 3), 1), _rand((3, 517, 3), 2)
    idx, mu, cov = metrics.knn_moments(q.cuda(), c.cuda(), K)
    want = lm.knn_idx(q.numpy(), c.numpy(), K)
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
    m64, c64 = lm.moments(c.double(), want)
    np.testing.assert_allclose(mu.cpu().double().numpy(), m64.numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(cov.cpu().double().numpy(), c64.numpy(), rtol=1e-4, atol=1e-8)
    # self query: the point itself first
    idx_s, _, _ = metrics.knn_moments(c.cuda(), c.cuda(), K)
    assert (idx_s[:, :, 0].cpu() == torch.arange(517)).all()


@pytest.mark.parametrize("K", [8, 20, 32])
def test_knn_moments_lattice_ties(g23, K):
    lat = torch.from_numpy(g23["lat"])
    two = torch.cat([lat, lat.flip(1)], 0).contiguous()                  # B = 2, the second in reverse order
    idx, _, _ = metrics.knn_moments(two.cuda(), two.cuda(), K)
    np.testing.assert_array_equal(idx[0].cpu().numpy(), g23["lat_idx_k%d" % K][0])
    np.testing.assert_array_equal(idx.cpu().numpy(), lm.knn_idx(two.numpy(), two.numpy(), K))


def test_chamfer_loss_against_reference(g23):
    for D in (3, 9):
        x, y = torch.from_numpy(g23["cl_x%d" % D]).cuda(), torch.from_numpy(g23["cl_y%d" % D]).cuda()
        _close(metrics.ChamferLoss()(x, y), g23, "cl%d" % D)


def test_local_cd_and_get_local_pair_against_reference(g23):
    m, c = metrics.local_CD(torch.from_numpy(g23["lcd_pt1"]).cuda(), torch.from_numpy(g23["lcd_pt2"]).cuda())
    _close(m, g23, "lcd_mu")
    _close(c, g23, "lcd_var")
    m, c = losses.get_local_pair(torch.from_numpy(g23["glp_pt1"]).cuda(), torch.from_numpy(g23["glp_pt2"]).cuda())
    _close(m, g23, "glp_mu")
    _close(c, g23, "glp_var")


def _glp_grads(p1, p2):
    a, b = p1.cuda().requires_grad_(True), p2.cuda().requires_grad_(True)
    m, c = losses.get_local_pair(a, b)
    gm_ = torch.autograd.grad(m, (a, b), retain_graph=True)
    gc_ = torch.autograd.grad(c, (a, b))
    return m.detach(), c.detach(), gm_, gc_


def test_get_local_pair_gradients(g23):
    p1, p2 = torch.from_numpy(g23["glp_pt1"]), torch.from_numpy(g23["glp_pt2"])
    m, c, gmu, gvar = _glp_grads(p1, p2)
    # float64 model with the kernels' neighbour indices and Chamfer argmins
    q, c2 = p1.transpose(1, 2).contiguous(), p2.transpose(1, 2).contiguous()
    idx1, mu1, cv1 = metrics.knn_moments(q.cuda(), q.cuda(), 20)
    idx2, mu2, cv2 = metrics.knn_moments(q.cuda(), c2.cuda(), 20)
    from spgan.local_cd import _nn_dim
    _, ia, _, ib = _nn_dim(mu1, mu2, 3)
    _, ja, _, jb = _nn_dim(cv1, cv2, 6)
    args = tuple(t.long().cpu() for t in (ia, ib, ja, jb))
    qd, cd = q.double().requires_grad_(True), c2.double().requires_grad_(True)
    wm, wc = lm.local_pair(qd, cd, 20, idx1.cpu().numpy(), idx2.cpu().numpy(), args)
    np.testing.assert_allclose(m.item(), wm.item(), rtol=1e-5)
    np.testing.assert_allclose(c.item(), wc.item(), rtol=1e-4)
    for val, got in ((wm, gmu), (wc, gvar)):
        want = torch.autograd.grad(val, (qd, cd), retain_graph=True)
        for g_, w_ in zip(got, want):
            w_ = w_.transpose(1, 2)
            err = (g_.cpu().double() - w_).abs().max() / w_.abs().max()
            assert err < 1e-4, err
    # against the reference's own float32 autograd (its torch.min may route a tie elsewhere; none occur on this input)
    for got, tag in ((gmu, "gmu"), (gvar, "gvar")):
        for g_, key in zip(got, ("glp_%s_pt1" % tag, "glp_%s_pt2" % tag)):
            w_ = g23[key]
            assert np.abs(g_.cpu().numpy() - w_).max() / np.abs(w_).max() < 1e-3, key


def test_determinism(g23):
    p1, p2 = torch.from_numpy(g23["glp_pt1"]), torch.from_numpy(g23["glp_pt2"])
    r1, r2 = _glp_grads(p1, p2), _glp_grads(p1, p2)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])
    for a, b in zip(r1[2] + r1[3], r2[2] + r2[3]):
        assert torch.equal(a, b)
    s = torch.from_numpy(g23["pw_sample"]).cuda()
    assert torch.equal(metrics.pairwise_local_cd(s, s), metrics.pairwise_local_cd(s, s))


def test_pairwise_equals_local_cd_loop(g23):
    s, r = torch.from_numpy(g23["pw_sample"]).cuda(), torch.from_numpy(g23["pw_ref"]).cuda()
    out = metrics.pairwise_local_cd(s, r)
    assert out.shape == (8, 10, 2)
    for i in range(8):
        for j in range(10):
            m, c = metrics.local_CD(s[i:i + 1], r[j:j + 1])
            assert out[i, j, 0].item() == m.item() and out[i, j, 1].item() == c.item(), (i, j)
    ss = metrics.pairwise_local_cd(s, s)
    assert (ss.diagonal(0, 0, 1) == 0).all()
    assert not torch.equal(ss[0, 1], ss[1, 0])
    np.testing.assert_allclose(out.cpu().double().numpy(), lm.pairwise_local(g23["pw_sample"], g23["pw_ref"]), rtol=1e-4)


def test_pairwise_local_CD_chunk_sum_quirk(g23):
    s, r = torch.from_numpy(g23["pw_sample"]).cuda(), torch.from_numpy(g23["pw_ref"]).cuda()
    for dist in ("CD_M", "CD_C"):
        for bs in (1, 4):
            got = gm.pairwise_local_CD(s, r, bs, dist).cpu().numpy()
            want = g23["plcd_%s_bs%d_64" % (dist, bs)]
            assert got.shape == want.shape
            np.testing.assert_allclose(got, want, rtol=1e-4)


@pytest.mark.parametrize("dist", ["CD", "CD_M", "CD_C"])
def test_drivers_against_reference(g23, dist):
    s, r = torch.from_numpy(g23["pw_sample"]).cuda(), torch.from_numpy(g23["pw_ref"]).cuda()
    np.testing.assert_allclose(gm.pairwise_dists(s, r, 1, dist).cpu().numpy(), g23["pd_%s_sr_64" % dist], rtol=1e-4)
    res = gm.compute_all_metrics(s, r, 1, dist)
    assert sorted(res) == sorted(["JSD", "COV", "MMD", "1NN", "6NN", "FPD"])
    for k, v in res.items():
        np.testing.assert_allclose(v, g23["cam_%s_%s_64" % (dist, k)], rtol=1e-4, atol=1e-9, err_msg=k)
    res = gm.compute_all_metrics_train(s, r, None, 1, dist)
    assert sorted(res) == sorted(["JSD", "COV", "MMD", "MMD_t", "1NN", "FPD"])
    for k, v in res.items():
        np.testing.assert_allclose(v, g23["camt_%s_%s_64" % (dist, k)], rtol=1e-4, atol=1e-9, err_msg=k)


def test_l2_features_and_emd_dispatch(g23):
    fs, fr = torch.from_numpy(g23["pw_fs"]).cuda(), torch.from_numpy(g23["pw_fr"]).cuda()
    np.testing.assert_allclose(gm.pairwise_dists(fs, fr, 4, "l2").cpu().numpy(), g23["pd_l2_sr_64"], rtol=1e-5)
    np.testing.assert_allclose(gm.pairwise_simple(fs, fr, 4, "l1").cpu().numpy(), g23["ps_l1_sr_64"], rtol=1e-5)
    res = gm.compute_all_metrics_train(fs, fr, None, 4, "l2")
    for k, v in res.items():
        np.testing.assert_allclose(v, g23["camt_l2_%s_64" % k], rtol=1e-5, err_msg=k)
    with pytest.raises(NotImplementedError, match="evaluation.pointnet"):
        gm.compute_all_metrics(fs, fr, 4, "l2")
    with pytest.raises(NotImplementedError, match="evaluation.pointnet"):
        gm.compute_all_metrics_train(torch.from_numpy(g23["pw_sample"]).cuda(), torch.from_numpy(g23["pw_ref"]).cuda(), None, 1, "CD", True)
    s, r = torch.from_numpy(g23["pw_sample"][:3]).cuda(), torch.from_numpy(g23["pw_ref"][:2]).cuda()
    assert torch.equal(gm.pairwise_dists(s, r, 4, "EMD"), metrics.pairwise_emd(s, r, 4))


def test_knn_vote_and_jsd(g23):
    t = lambda k: torch.from_numpy(np.ascontiguousarray(g23[k])).cuda()    # noqa: E731
    for k in (1, 3, 6):
        assert gm.KNN(t("knn_xx"), t("knn_xy"), t("knn_yy"), k) == float(g23["knn_k%d" % k])
        assert gm.KNN(t("knn_xx") - 0.5, t("knn_xy"), t("knn_yy"), k, sqrt=True) == float(g23["knn_sqrt_k%d" % k])
    assert gm.KNN(t("tie_xx"), t("tie_xy"), t("tie_yy"), 6) == float(g23["tie_k6"]) == 0.0
    # the existing 0/1-label vote calls every sample correct on the same matrices
    assert metrics.knn(t("tie_xx"), t("tie_xy"), t("tie_yy"), 6)["acc_t"].item() == 1.0
    counts = gm.voxel_counts(t("jsd_c1")).cpu().numpy()
    np.testing.assert_array_equal(counts, lm.voxel_counts(g23["jsd_c1"]))
    np.testing.assert_array_equal(gm.get_voxel_occ_dist(t("jsd_c1")).cpu().numpy(), g23["voxel_c1"])
    np.testing.assert_allclose(gm.JSD(t("jsd_c1"), t("jsd_c2")), g23["jsd"], rtol=1e-10)
    e = -0.5 + np.arange(29) * (1.0 / 28)
    pts = np.array([[e[3], e[5], e[27]], [np.nextafter(np.float32(e[4]), np.float32(-1)), 0.0, 0.0], [0.5, 0.0, 0.0]], np.float32)
    np.testing.assert_array_equal(gm.voxel_counts(torch.from_numpy(pts).cuda()).cpu().numpy(), lm.voxel_counts(pts[None]))


def test_full_size_pairwise():
    S, N = 64, 2048
    base = _rand((1, N, 3), 5)
    s = (base + _rand((S, N, 3), 6, 0.02)).cuda()
    out = metrics.pairwise_local_cd(s, s)
    assert out.shape == (S, S, 2) and torch.isfinite(out).all()
    assert (out.diagonal(0, 0, 1) == 0).all()
    for i, j in ((0, 1), (5, 63), (40, 7), (63, 0)):
        m, c = metrics.local_CD(s[i:i + 1], s[j:j + 1])
        assert out[i, j, 0].item() == m.item() and out[i, j, 1].item() == c.item(), (i, j)
        assert out[i, j, 0].item() > 0
