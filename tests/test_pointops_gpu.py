"""GPU: the pointops family (spgan.pointops, csrc/pointops.hip) against its numpy / torch model (tests/pointops_model.py).  B = 2 with
different clouds per batch entry throughout.  Index ops and forwards are compared bit for bit: distances have one fixed rounding order,
gathers move bits.  Gradients are compared with float64 autograd of the plain torch composition; the bound is 4 times the float32 torch
composition's own distance from float64 on the same inputs (the summation orders differ), see `_check_grads`."""
import numpy as np
import pytest
import torch

import pointops_model as pm
from spgan import _lib, pointops

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = np.float32(2.0 ** -4)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rand_cloud(rng, B, n):
    return rng.random((B, n, 3), dtype=np.float32)


def _knn_both(nsample, xyz, new_xyz):
    idx, d2 = pointops.knn_with_dist2(nsample, _t(xyz), _t(new_xyz))
    return idx.cpu().numpy(), d2.cpu().numpy()


def _assert_knn(nsample, xyz, new_xyz):
    idx, d2 = _knn_both(nsample, xyz, new_xyz)
    ridx, rd2 = pm.knnquery(nsample, xyz, new_xyz)
    assert idx.dtype == np.int32 and d2.dtype == np.float32
    np.testing.assert_array_equal(idx, ridx)
    np.testing.assert_array_equal(d2.view(np.uint32), rd2.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------------------
# kNN
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 257])
def test_knn_lattice_ties_and_padding(n):
    """Lattice coordinates times 2^-4: every d2 is exact and ties abound; nsample > n pads with index 0 and +inf."""
    rng = np.random.default_rng(100 + n)
    xyz = pm.lattice_cloud(rng, 2, n)
    for m in (1, 3, 70):
        new_xyz = pm.lattice_cloud(rng, 2, m)
        new_xyz[:, 0] = xyz[:, n // 2]                         # one query is a cloud point: it is its own nearest neighbour (with its twins)
        for nsample in (1, 2, 32, 33, 64, 65, 200):
            _assert_knn(nsample, xyz, new_xyz)


def test_knn_past_the_register_capacity():
    """Clouds of capacity + 1 and of more than two chunks: the winners so far join the next chunk's candidates."""
    cap = _lib.load().spgan_pointops_knn_capacity()
    rng = np.random.default_rng(7)
    for n in (cap, cap + 1, 2 * cap + 37):
        xyz = pm.lattice_cloud(rng, 2, n, side=6)
        new_xyz = pm.lattice_cloud(rng, 2, 3, side=6)
        for nsample in (1, 33, 200):
            _assert_knn(nsample, xyz, new_xyz)


def test_knn_random_clouds_bit_equal():
    rng = np.random.default_rng(11)
    cap = _lib.load().spgan_pointops_knn_capacity()
    for n, m, nsample in ((300, 70, 20), (1000, 9, 64), (cap + 500, 5, 200)):
        xyz, new_xyz = _rand_cloud(rng, 2, n), _rand_cloud(rng, 2, m)
        _assert_knn(nsample, xyz, new_xyz)
    x = _t(_rand_cloud(rng, 2, 50))
    assert torch.equal(pointops.knnquery(4, x), pointops.knnquery(4, x, x))
    assert torch.equal(pointops.knnquery_naive(4, x, x), pointops.knnquery(4, x, x))
    assert torch.equal(pointops.knnquery_exclude(4, x, x), pointops.knnquery(5, x, x)[:, :, 1:])
    assert pointops.knnquery(4, x).dtype == torch.int32 and not pointops.knnquery(4, x).requires_grad


def test_nsample_above_200_raises():
    """Deliberate difference: the reference overruns its 200-entry arrays."""
    x = _t(_rand_cloud(np.random.default_rng(0), 2, 300))
    with pytest.raises(ValueError, match="nsample"):
        pointops.knnquery(201, x, x)
    with pytest.raises(ValueError, match="nsample"):
        pointops.QueryAndGroup(None, 201)(x, x, None)
    i = torch.empty((2, 300, 201), dtype=torch.int32, device=DEV)
    d = torch.empty((2, 300, 201), device=DEV)
    assert _lib.load().spgan_pointops_knnquery(x.data_ptr(), x.data_ptr(), 2, 300, 300, 201, i.data_ptr(), d.data_ptr(), None) == -22


@pytest.mark.parametrize("m", [1, 2, 3, 64])
def test_nearestneighbor(m):
    rng = np.random.default_rng(20 + m)
    known, unknown = pm.lattice_cloud(rng, 2, m), pm.lattice_cloud(rng, 2, 37)
    dist, idx = pointops.nearestneighbor(_t(unknown), _t(known))
    rdist, ridx = pm.nearestneighbor(unknown, known)
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
    np.testing.assert_array_equal(dist.cpu().numpy().view(np.uint32), rdist.view(np.uint32))       # the square root is applied
    if m < 3:
        assert np.all(np.isinf(rdist[:, :, m:])) and np.all(ridx[:, :, m:] == 0)
    known, unknown = _rand_cloud(rng, 2, m), _rand_cloud(rng, 2, 37)
    dist, idx = pointops.nearestneighbor(_t(unknown), _t(known))
    rdist, ridx = pm.nearestneighbor(unknown, known)
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
    np.testing.assert_array_equal(dist.cpu().numpy().view(np.uint32), rdist.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------------------
# ball query, label statistics, feature distribute
# ------------------------------------------------------------------------------------------------------------------------------------
def _ball_case():
    """Query 0 of each shape sits at a lattice point p; the cloud holds p + (3,4,0)*2^-4 (exactly at r = 5*2^-4), close points before and
    after it, and lattice filler.  Query 1 is far from everything.  The two shapes differ."""
    rng = np.random.default_rng(5)
    n = 70
    xyz = np.empty((2, n, 3), dtype=np.float32)
    new_xyz = np.empty((2, 3, 3), dtype=np.float32)
    for b in range(2):
        p = np.array([8 + b, 8, 8], dtype=np.float32)
        pts = rng.integers(0, 17, size=(n, 3)).astype(np.float32)
        pts[2] = p + (3, 4, 0)                                  # d == r: outside
        pts[3 + b] = p + (1, 0, 0)                              # the first hit, unless the filler has one earlier
        pts[40] = p + (0, 0, 4)
        pts[41] = p + (2, 2, 1)
        pts[66] = p                                             # crosses the first 64-candidate step
        xyz[b] = pts * S
        new_xyz[b, 0] = p * S
        new_xyz[b, 1] = (np.array([300, 300, 300], dtype=np.float32)) * S
        new_xyz[b, 2] = (p + (1, 1, 1)) * S
    return xyz, new_xyz, np.float32(5) * S


def test_ballquery_strict_padding_truncation_empty():
    xyz, new_xyz, r = _ball_case()
    hits = pm.dist2(new_xyz, xyz) < r * r
    assert hits[:, 0].sum(axis=1).min() >= 4 and not hits[:, 1].any()
    for nsample in (1, 3, 64, 100):
        idx = pointops.ballquery(float(r), nsample, _t(xyz), _t(new_xyz))
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (2, 3, nsample)
        idx = idx.cpu().numpy()
        np.testing.assert_array_equal(idx, pm.ballquery(r, nsample, xyz, new_xyz))
        for b in range(2):
            h = np.flatnonzero(hits[b, 0])
            assert 2 not in idx[b, 0]                              # the point at distance exactly r
            np.testing.assert_array_equal(idx[b, 0, :min(nsample, h.size)], h[:nsample])      # truncation keeps the lowest indices
            assert np.all(idx[b, 0, h.size:] == h[0])             # padding uses the first hit
            assert np.all(idx[b, 1] == 0)                          # an empty ball
    r2 = np.nextafter(r, np.float32(1))                            # one ulp more and the boundary point is inside
    idx = pointops.ballquery(float(r2), 100, _t(xyz), _t(new_xyz)).cpu().numpy()
    assert 2 in idx[0, 0] and 2 in idx[1, 0]
    rng = np.random.default_rng(6)
    for n in (5, 64, 65, 300):
        c, q = pm.lattice_cloud(rng, 2, n, side=8), pm.lattice_cloud(rng, 2, 9, side=8)
        for nsample in (1, 4, 70):
            got = pointops.ballquery(float(3 * S), nsample, _t(c), _t(q)).cpu().numpy()
            np.testing.assert_array_equal(got, pm.ballquery(3 * S, nsample, c, q))


@pytest.mark.parametrize("nclass", [1, 13, 40, 300])
def test_label_statistics(nclass):
    """nclass 300 goes past the classes a lane keeps in registers."""
    xyz, new_xyz, r = _ball_case()
    rng = np.random.default_rng(nclass)
    ls = rng.integers(1, 7, size=(2, xyz.shape[1], nclass)).astype(np.int32)
    nsample = 3                                                    # the ball of query 0 holds more
    full = pointops.labelstat_ballrange(float(r), _t(xyz), _t(new_xyz), _t(ls))
    part, idx = pointops.labelstat_and_ballquery(float(r), nsample, _t(xyz), _t(new_xyz), _t(ls))
    assert full.dtype == torch.int32 and part.dtype == torch.int32 and idx.dtype == torch.int32
    rpart, ridx = pm.labelstat_and_ballquery(r, nsample, xyz, new_xyz, ls)
    np.testing.assert_array_equal(full.cpu().numpy(), pm.labelstat_ballrange(r, xyz, new_xyz, ls))
    np.testing.assert_array_equal(part.cpu().numpy(), rpart)
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
    assert not torch.equal(full[:, 0], part[:, 0])                 # the scan that stops at nsample hits sums fewer rows
    assert torch.equal(full[:, 1], torch.zeros_like(full[:, 1]))
    by_idx = pointops.labelstat_idx(nsample, _t(ls), idx)
    np.testing.assert_array_equal(by_idx.cpu().numpy(), pm.labelstat_idx(ls, ridx))
    big, bidx = pointops.labelstat_and_ballquery(float(r), 100, _t(xyz), _t(new_xyz), _t(ls))
    assert torch.equal(big, full)                                  # nsample above every ball: the two agree
    rng2 = np.random.default_rng(nclass + 1)
    c, q = pm.lattice_cloud(rng2, 2, 130, side=8), pm.lattice_cloud(rng2, 2, 9, side=8)
    ls2 = rng2.integers(-3, 9, size=(2, 130, nclass)).astype(np.int32)
    got, gidx = pointops.labelstat_and_ballquery(float(4 * S), 5, _t(c), _t(q), _t(ls2))
    want, widx = pm.labelstat_and_ballquery(4 * S, 5, c, q, ls2)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(gidx.cpu().numpy(), widx)
    np.testing.assert_array_equal(pointops.labelstat_ballrange(float(4 * S), _t(c), _t(q), _t(ls2)).cpu().numpy(),
                                  pm.labelstat_ballrange(4 * S, c, q, ls2))


def test_featuredistribute_ties_far_clouds_and_featuregather():
    rng = np.random.default_rng(9)
    for n in (1, 64, 200):
        max_xyz, xyz = pm.lattice_cloud(rng, 2, n, side=3), pm.lattice_cloud(rng, 2, 45, side=3)
        got = pointops.featuredistribute(_t(max_xyz), _t(xyz))
        assert got.dtype == torch.int32 and tuple(got.shape) == (2, 45)
        np.testing.assert_array_equal(got.cpu().numpy(), pm.featuredistribute(max_xyz, xyz))     # ties: the lowest index
    feat = torch.randn(2, 6, 200, device=DEV, requires_grad=True)
    out = pointops.featuregather(feat, got)
    ref = torch.gather(feat, 2, got.long()[:, None, :].expand(2, 6, 45))
    assert torch.equal(out, ref)
    g = torch.randn_like(out)
    (d_ours,) = torch.autograd.grad(out, feat, g)
    (d_ref,) = torch.autograd.grad(ref.double(), feat, g.double())
    torch.testing.assert_close(d_ours, d_ref.float(), rtol=1e-5, atol=1e-6)
    far = pointops.featuredistribute(_t(max_xyz + np.float32(400)), _t(xyz))
    assert torch.equal(far, torch.full_like(far, -1))              # no point nearer than 100000: the reference's starting value
    with pytest.raises(IndexError):
        pointops.featuregather(feat, far)                          # deliberate difference: the reference reads out of bounds


# ------------------------------------------------------------------------------------------------------------------------------------
# grouping and its gradient
# ------------------------------------------------------------------------------------------------------------------------------------
GRAD_FIGURES = []


def _check_grads(ours, t32, t64, what):
    """max |ours - f64| <= 4 * max |torch f32 - f64|, both over all gradient tensors of the case and relative to max |f64|.
    Measured on the MI355X over this file's cases: see `test_grouping_backward_against_float64`."""
    scale = max(float(g.abs().max()) for g in t64)
    e_ours = max(float((a.double() - c).abs().max()) for a, c in zip(ours, t64)) / scale
    e_t32 = max(float((a.double() - c).abs().max()) for a, c in zip(t32, t64)) / scale
    GRAD_FIGURES.append((what, e_ours, e_t32))
    print("%s: ours %.3e, torch float32 %.3e of the float64 gradient" % (what, e_ours, e_t32))
    assert e_ours <= 4.0 * e_t32, (what, e_ours, e_t32)


def _padded_ball_idx(rng, n, m, K):
    """Ball-query indices on a random cloud: small balls, so most slots repeat the first hit."""
    xyz, new_xyz = _rand_cloud(rng, 2, n), _rand_cloud(rng, 2, m)
    return _t(xyz), _t(new_xyz), pointops.ballquery(0.2, K, _t(xyz), _t(new_xyz))


def test_grouping_forward_bit_equal_and_repeatable():
    rng = np.random.default_rng(31)
    xyz, new_xyz, idx = _padded_ball_idx(rng, 150, 40, 16)
    assert (idx[:, :, 1:] == idx[:, :, :1]).float().mean() > 0.3             # heavy duplication
    feat = torch.randn(2, 7, 150, device=DEV)
    out = pointops.grouping(feat, idx)
    assert torch.equal(out, pm.grouping(feat, idx)) and torch.equal(out, pointops.grouping(feat, idx))
    ints = torch.randint(-5, 1 << 40, (2, 3, 150), device=DEV)
    assert torch.equal(pointops.grouping_int(ints, idx), pm.grouping(ints, idx))
    knn_idx = pointops.knnquery(9, xyz, new_xyz)
    assert torch.equal(pointops.grouping(feat, knn_idx), pm.grouping(feat, knn_idx))


def test_grouping_backward_against_float64():
    """Heavily duplicated indices (ball-query padding), forward and backward twice, bit for bit.
    Measured (MI355X, this case): ours 2.07e-07, torch float32 1.68e-07 of the largest float64 gradient entry; the bound is 4 x the
    latter.  Over the module cases below: ours 6.2e-08 .. 1.5e-07, torch float32 4.6e-08 .. 2.7e-07 (torch's sums use atomics, so its
    figure moves a little from run to run)."""
    rng = np.random.default_rng(32)
    _, _, idx = _padded_ball_idx(rng, 150, 40, 16)
    feat = torch.randn(2, 7, 150, device=DEV, requires_grad=True)
    g = torch.randn(2, 7, 40, 16, device=DEV)
    runs = []
    for _ in range(2):
        out = pointops.grouping(feat, idx)
        runs.append((out.detach().clone(), torch.autograd.grad(out, feat, g)[0]))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    (t32,) = torch.autograd.grad(pm.grouping(feat, idx), feat, g)
    f64 = feat.detach().double().requires_grad_(True)
    (t64,) = torch.autograd.grad(pm.grouping(f64, idx), f64, g.double())
    _check_grads([runs[0][1]], [t32], [t64], "grouping")


MODULE_CASES = [
    # (class, radius, use_xyz, features, inject idx)
    ("QueryAndGroup", 0.25, True, True, False),
    ("QueryAndGroup", None, True, True, False),
    ("QueryAndGroup", 0.25, False, True, False),
    ("QueryAndGroup", None, True, False, False),
    ("QueryAndGroup", None, True, True, True),
    ("QueryAndGroup_Dilate", None, True, True, False),
    ("QueryAndGroup_Dilate", 0.3, True, False, False),
    ("Le_QueryAndGroup", 0.25, True, True, False),
    ("Le_QueryAndGroup", None, True, False, False),
    ("Le_QueryAndGroup_SameSize", None, True, True, False),
    ("Le_QueryAndGroup_SameSize", 0.25, False, True, True),
    ("Le_QueryAndGroup_OnlyFeature", 0.25, True, True, False),
    ("Le_QueryAndGroup_OnlyFeature", None, False, True, True),
    ("Gen_QueryAndGroupXYZ", 0.25, True, False, False),
    ("Gen_QueryAndGroupXYZ", None, True, False, False),
]


def _module_model(name, use_xyz, xyz, new_xyz, feat, idx):
    """The reference's forward of each module in plain torch on a given idx -> tuple of outputs."""
    gx = pm.query_and_group(xyz, new_xyz, None, idx)
    if name in ("QueryAndGroup", "QueryAndGroup_Dilate"):
        return (pm.query_and_group(xyz, new_xyz, feat, idx, use_xyz=use_xyz),)
    if name in ("Le_QueryAndGroup", "Le_QueryAndGroup_SameSize"):
        return (gx, pm.grouping(feat, idx) if feat is not None else gx)
    if name == "Le_QueryAndGroup_OnlyFeature":
        return (pm.grouping(feat, idx),)
    return (pm.query_and_group(xyz, new_xyz, None, idx, subtract=False),)


@pytest.mark.parametrize("name,radius,use_xyz,with_feat,inject", MODULE_CASES)
def test_modules_forward_and_gradients(name, radius, use_xyz, with_feat, inject):
    rng = np.random.default_rng(200 + MODULE_CASES.index((name, radius, use_xyz, with_feat, inject)))
    n, K, C = 150, 8, 5
    m = n if name == "Le_QueryAndGroup_SameSize" else 40
    xyz = _t(_rand_cloud(rng, 2, n)).requires_grad_(True)
    new_xyz = _t(_rand_cloud(rng, 2, m)).requires_grad_(True)
    feat = torch.randn(2, C, n, device=DEV, requires_grad=True) if with_feat else None
    mod = getattr(pointops, name)(radius, K, use_xyz)
    dilate = name == "QueryAndGroup_Dilate"
    ask = 2 * K if dilate else K
    query = pointops.ballquery(radius, ask, xyz, new_xyz) if radius is not None else pointops.knnquery(ask, xyz, new_xyz)
    if inject:
        query = torch.flip(query, dims=[2]).contiguous()            # something the module would not have computed itself
    args = (xyz, new_xyz) if name == "Gen_QueryAndGroupXYZ" else (xyz, new_xyz, feat, query if inject else None)
    np.random.seed(1234)
    out = mod(*args)
    out = out if isinstance(out, tuple) else (out,)
    idx = query
    if dilate:
        np.random.seed(1234)                                        # the same draw as the module's
        cols = np.arange(2 * K)
        np.random.shuffle(cols)
        idx = query[:, :, torch.from_numpy(cols[:K]).to(DEV)].contiguous()
    ref = _module_model(name, use_xyz, xyz, new_xyz, feat, idx)
    assert len(out) == len(ref)
    for a, b in zip(out, ref):
        assert a.is_contiguous() and a.shape == b.shape and torch.equal(a, b)
    leaves = [t for t in (xyz, new_xyz, feat) if t is not None]
    gs = [torch.randn_like(o) for o in out]

    def grads(outs, leaves_, gs_):
        got = torch.autograd.grad(list(outs), leaves_, gs_, allow_unused=True)
        return [torch.zeros_like(l) if g is None else g for g, l in zip(got, leaves_)]

    ours = grads(out, leaves, gs)
    t32 = grads(ref, leaves, gs)
    l64 = [t.detach().double().requires_grad_(True) for t in leaves]
    x64, q64 = l64[0], l64[1]
    f64 = l64[2] if with_feat else None
    t64 = grads(_module_model(name, use_xyz, x64, q64, f64, idx), l64, [g.double() for g in gs])
    np.random.seed(1234)
    again = mod(*args)
    again = again if isinstance(again, tuple) else (again,)
    ours2 = grads(again, leaves, gs)
    assert all(torch.equal(a, b) for a, b in zip(out, again)) and all(torch.equal(a, b) for a, b in zip(ours, ours2))
    if name == "Le_QueryAndGroup_OnlyFeature" or (with_feat and not use_xyz and name.startswith("QueryAndGroup")):
        assert not ours[0].any() and not ours[1].any()              # the coordinates do not reach the output
    elif name != "Gen_QueryAndGroupXYZ":
        assert ours[0].any() and ours[1].any()                      # gradients reach xyz and new_xyz
    if with_feat:
        assert ours[2].any()
    _check_grads(ours, t32, t64, "%s r=%s use_xyz=%s feat=%s idx=%s" % (name, radius, use_xyz, with_feat, inject))


def test_new_xyz_defaults_to_xyz():
    """new_xyz = None means xyz in every module -- also in Le_QueryAndGroup_SameSize, where the reference dereferences None first
    (deliberate difference)."""
    rng = np.random.default_rng(41)
    xyz = _t(_rand_cloud(rng, 2, 60))
    feat = torch.randn(2, 4, 60, device=DEV)
    for name in ("QueryAndGroup", "Le_QueryAndGroup", "Le_QueryAndGroup_SameSize", "Le_QueryAndGroup_OnlyFeature"):
        mod = getattr(pointops, name)(None, 6)
        a, b = mod(xyz, None, feat), mod(xyz, xyz, feat)
        a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
        assert all(torch.equal(p, q) for p, q in zip(a, b)), name
    g = pointops.Gen_QueryAndGroupXYZ(None, 6)
    assert torch.equal(g(xyz), g(xyz, xyz))
    with pytest.raises(AssertionError):
        pointops.Le_QueryAndGroup_SameSize(None, 6)(xyz, xyz[:, :10].contiguous(), feat)


def test_only_feature_without_features_raises():
    """Deliberate difference: the reference dies on an undefined name."""
    xyz = _t(_rand_cloud(np.random.default_rng(42), 2, 30))
    with pytest.raises(ValueError, match="needs features"):
        pointops.Le_QueryAndGroup_OnlyFeature(None, 4)(xyz, xyz, None)
    with pytest.raises(AssertionError):
        pointops.QueryAndGroup(None, 4, use_xyz=False)(xyz, xyz, None)


def test_group_all_and_both_group_routes():
    rng = np.random.default_rng(43)
    xyz, new_xyz = _t(_rand_cloud(rng, 2, 50)), _t(_rand_cloud(rng, 2, 11))
    feat = torch.randn(2, 4, 50, device=DEV)
    out = pointops.GroupAll()(xyz, None, feat)
    assert tuple(out.shape) == (2, 7, 1, 50) and torch.equal(out[:, :3, 0], xyz.transpose(1, 2)) and torch.equal(out[:, 3:, 0], feat)
    assert tuple(pointops.GroupAll(False)(xyz, None, feat).shape) == (2, 4, 1, 50) and tuple(pointops.GroupAll()(xyz, None).shape) == (2, 3, 1, 50)
    mod = pointops.QueryAndGroup(0.3, 8)
    fused = mod(xyz, new_xyz, feat)
    try:
        pointops.GROUP_ROUTE = "composed"
        composed = mod(xyz, new_xyz, feat)
    finally:
        pointops.GROUP_ROUTE = "fused"
    assert torch.equal(fused, composed)


# ------------------------------------------------------------------------------------------------------------------------------------
# layout edges of spgan_pointops_group_cm
# ------------------------------------------------------------------------------------------------------------------------------------
def _stage_limit():
    return _lib.load().spgan_pointops_group_stage_limit()


@pytest.mark.parametrize("K", [1, 20])
@pytest.mark.parametrize("C", [1, 3, 67])
def test_group_cm_layout_edges(C, K):
    """m*K is no multiple of 64; n below, at and just past the LDS-staging limit; a slice with c0 > 0 leaves its neighbours alone."""
    lib = _lib.load()
    lim = _stage_limit()
    m = 7
    assert (m * K) % 64 != 0
    g = torch.Generator(device=DEV).manual_seed(C * 100 + K)
    for n in (50, lim // 3 + 5, lim, lim + 1):
        feat = torch.randn(2, C, n, device=DEV, generator=g)
        idx = torch.randint(0, n, (2, m, K), device=DEV, generator=g, dtype=torch.int32)
        idx[0, 0, 0], idx[1, -1, -1] = n - 1, 0
        assert torch.equal(pointops.grouping(feat, idx), pm.grouping(feat, idx)), n
        c0, Ctot = 2, C + 5
        buf = torch.full((2, Ctot, m, K), -7.0, device=DEV)
        assert lib.spgan_pointops_group_cm(feat.data_ptr(), 0, None, idx.data_ptr(), 2, C, n, m, K, c0, Ctot, buf.data_ptr(), None,
                                           torch.cuda.current_stream().cuda_stream) == 0
        assert torch.equal(buf[:, c0:c0 + C], pm.grouping(feat, idx)), n
        assert bool((buf[:, :c0] == -7.0).all()) and bool((buf[:, c0 + C:] == -7.0).all())
        if C == 3:                                                   # the point-major source with its centre, at the same sizes
            xyz = feat.transpose(1, 2).contiguous()
            ctr = torch.randn(2, m, 3, device=DEV, generator=g)
            got = pointops._GroupSlices.apply(xyz, ctr, None, idx)
            assert torch.equal(got, pm.query_and_group(xyz, ctr, None, idx)), n


def test_group_cm_bad_index_writes_zero_and_flags():
    feat = torch.randn(2, 3, 20, device=DEV)
    idx = torch.randint(0, 20, (2, 4, 5), device=DEV, dtype=torch.int32)
    idx[1, 2, 3] = 20
    idx[0, 0, 0] = -1
    out = torch.full((2, 3, 4, 5), 9.0, device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert _lib.load().spgan_pointops_group_cm(feat.data_ptr(), 0, None, idx.data_ptr(), 2, 3, 20, 4, 5, 0, 3, out.data_ptr(), bad.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream) == 0
    assert int(bad.item()) == 1 and not out[1, :, 2, 3].any() and not out[0, :, 0, 0].any()
    ok = idx.clamp(0, 19)
    keep = torch.ones(2, 1, 4, 5, dtype=torch.bool, device=DEV)
    keep[1, 0, 2, 3] = keep[0, 0, 0, 0] = False
    assert torch.equal(out * keep, pm.grouping(feat, ok) * keep)


# ------------------------------------------------------------------------------------------------------------------------------------
# the ops built on launches that existed before
# ------------------------------------------------------------------------------------------------------------------------------------
def test_furthestsampling_gathering_interpolation_pairwise():
    rng = np.random.default_rng(51)
    pts = _rand_cloud(rng, 2, 200)
    idx = pointops.furthestsampling(_t(pts), 16)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (2, 16)
    want = np.zeros((2, 16), dtype=np.int64)
    for b in range(2):
        d = np.full(200, np.inf)
        for j in range(1, 16):
            d = np.minimum(d, ((pts[b].astype(np.float64) - pts[b, want[b, j - 1]]) ** 2).sum(1))
            want[b, j] = int(np.argmax(d))
    np.testing.assert_array_equal(idx.cpu().numpy(), want)          # starts at point 0
    feat = torch.randn(2, 6, 200, device=DEV, requires_grad=True)
    out = pointops.gathering(feat, idx)
    assert torch.equal(out, torch.gather(feat, 2, idx.long()[:, None, :].expand(2, 6, 16)))
    (dg,) = torch.autograd.grad(out, feat, torch.ones_like(out))
    assert float(dg.sum()) == 2 * 6 * 16
    unknown, known = _t(_rand_cloud(rng, 2, 90)), _t(pts)
    dist, nidx = pointops.nearestneighbor(unknown, known)
    w = 1.0 / (dist + 1e-8)
    w = (w / w.sum(dim=2, keepdim=True)).contiguous()
    o = pointops.interpolation(feat, nidx, w)
    assert torch.equal(o, pm.interpolation(feat, nidx, w)) and torch.equal(o, pointops.interpolation(feat, nidx, w))
    g = torch.randn_like(o)
    (ours,) = torch.autograd.grad(o, feat, g)
    (ours2,) = torch.autograd.grad(pointops.interpolation(feat, nidx, w), feat, g)
    (t32,) = torch.autograd.grad(pm.interpolation(feat, nidx, w), feat, g)
    f64 = feat.detach().double().requires_grad_(True)
    (t64,) = torch.autograd.grad(pm.interpolation(f64, nidx, w.double()), f64, g.double())
    assert torch.equal(ours, ours2)
    _check_grads([ours], [t32], [t64], "interpolation")
    x, y = torch.randn(30, 3, device=DEV), torch.randn(20, 3, device=DEV)
    torch.testing.assert_close(pointops.pairwise_distances(x, y), ((x[:, None] - y[None]) ** 2).sum(-1), rtol=1e-4, atol=1e-5)
    assert float(pointops.pairwise_distances(x).min()) >= 0.0
