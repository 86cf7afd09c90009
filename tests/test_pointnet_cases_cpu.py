"""CPU: the cases of tests/pointnet_cases.py are what they claim to be -- no GPU needed.

* the threshold: which float32 `thr` makes `d > thr` equal torch's `sqrdists > radius ** 2` for every float32 d (the reference's mask,
  Common/pointnet_util.py:102) -- float32(radius ** 2) rounded to nearest, not its round-down, not a comparison in double;
* exactness: on every lattice case the float64 model equals the oracle's float32 torch expressions bit for bit;
* the cases bite: tie cases have equal distances at the deciding rank, boundary cases have a point with d == r^2, the radius cases have
  their special point exactly where the two thresholds differ.
Where torch leaves a tie choice open (torch.max in the sampling loop, topk in knn_point) the model's rule is the kernel's documented one; what
CPU torch happens to choose is printed, nothing depends on it.
"""
import numpy as np
import pytest
import torch

import pointnet_cases as pc
from oracle import spgan_oracle as orc

F = np.float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ----------------------------------------------------------------------------------------------------------------------- the threshold
@pytest.mark.parametrize("r", pc.RADII_HIGH + pc.RADII_LOW + (0.3, 0.15, 0.02, pc.R5))
def test_threshold_is_float32_of_the_double_square_rounded_to_nearest(r):
    thr = pc.ball_threshold(r)
    lo, hi = np.nextafter(thr, F(0)), np.nextafter(thr, F(2))
    d = torch.tensor([lo, thr, hi])
    got = (d > r ** 2).tolist()                                  # the reference's expression: float32 tensor against a Python double
    assert got == (d > torch.tensor(thr)).tolist() == [False, False, True]
    in_double = (d.double() > r ** 2).tolist()
    print("r %.17g: r**2 %.17g, thr %.17g; a comparison in double would give %s" % (r, r ** 2, float(thr), in_double))
    if r ** 2 < float(thr):                                      # thr was rounded UP: round-down or a double comparison would put d == thr outside
        assert in_double == [False, True, True] and got[1] is False


def test_squaring_the_float32_radius_is_off_by_one_ulp_for_the_usual_radii():
    def ulps(r):
        return int(F(F(r) * F(r)).view(np.int32)) - int(pc.ball_threshold(r).view(np.int32))
    assert [ulps(r) for r in pc.RADII_HIGH] == [1] * 5 and [ulps(r) for r in pc.RADII_LOW] == [-1] * 4
    assert [ulps(r) for r in (0.3, 0.15, 0.02, pc.R5, pc.R_TILE)] == [0] * 5          # the golden radii and the lattice radii agree
    assert sum(ulps(i / 100) != 0 for i in range(1, 101)) == 36


def test_the_wrappers_threshold_is_the_models():
    """spgan.pointnet_util.ball_threshold (what the wrapper hands to the C entry) against the model's, over the two-decimal radii."""
    from spgan import pointnet_util as pu
    for r in [i / 100 for i in range(1, 101)] + [pc.R5, pc.R_TILE, float(np.nextafter(F(pc.R5), F(0)))]:
        assert pu.ball_threshold(r) == float(pc.ball_threshold(r))


# ----------------------------------------------------------------------------------------------------------------------- square distance
@pytest.mark.parametrize("B,N,M,C", pc.SQDIST_SHAPES)
def test_square_distance_is_exact(B, N, M, C):
    a, b = pc.sqdist_case(B, N, M, C)
    ref = orc.square_distance(_t(a), _t(b))
    assert ref.dtype == torch.float32
    np.testing.assert_array_equal(ref.double().numpy(), pc.square_distance(a, b))
    diff = ((a.astype(np.float64)[:, :, None] - b.astype(np.float64)[:, None]) ** 2).sum(-1)
    np.testing.assert_array_equal(diff, pc.square_distance(a, b))


# ----------------------------------------------------------------------------------------------------------------------- farthest point sampling
def _assert_fps_rule(xyz, start, picks):
    """Every pick is the lowest index among the maxima of the float32 running minimum (the oracle's expressions, the kernel's tie rule)."""
    x = _t(xyz)
    B, N, _ = x.shape
    ties = 0
    for b in range(B):
        dist = torch.full((N,), 1e10)
        assert picks[b, 0] == start[b]
        for i in range(picks.shape[1] - 1):
            dist = torch.minimum(dist, torch.sum((x[b] - x[b, picks[b, i]]) ** 2, -1))
            top = torch.nonzero(dist == dist.max()).view(-1)
            assert picks[b, i + 1] == int(top[0])
            ties += int(top.numel() > 1)
    return ties


@pytest.mark.parametrize("kind", ["side3", "triple"])
@pytest.mark.parametrize("N", pc.FPS_N)
def test_fps_cases(N, kind):
    xyz, start, exp = pc.fps_case(N, kind)
    assert start[0] == N - 1 and xyz.shape == (2, N, 3)
    full = exp[N]
    ties = _assert_fps_rule(xyz, start, full)
    for p, e in exp.items():
        np.testing.assert_array_equal(e, full[:, :p])
    agree = np.array_equal(orc.farthest_point_sample(_t(xyz), N, _t(start)).numpy(), full)
    print("N %d %s: %d of %d picks decided among equal maxima; CPU torch.max agrees: %s" % (N, kind, ties, 2 * (N - 1), agree))
    if N >= 63:
        assert ties >= (N - 1) // 2, "the cloud does not tie"
    if kind == "triple" and N >= 63:                             # once every distinct position is taken all distances are 0: index 0 repeats
        distinct = len({tuple(p) for p in xyz[0].tolist()})
        assert distinct < N and (full[0, distinct:] == 0).all()


def test_fps_tie_clouds():
    for I in pc.FPS_TIE_SETS:
        xyz = pc.fps_tie_cloud([I])
        got = pc.farthest_point_sample(xyz, 3, np.zeros(1, dtype=np.int64))
        assert got[0].tolist() == [0, min(I), 0]                 # second pick min(I); then every distance is 0 except nothing: index 0
        _assert_fps_rule(xyz, np.zeros(1, dtype=np.int64), got)
    lanes = [(i % 512, (i % 512) // 64) for I in pc.FPS_TIE_SETS for i in I]           # (thread, wave) of a 512-thread block striding by 512
    assert lanes[0][0] == lanes[1][0]                                                   # 517, 5: one thread
    assert lanes[2][1] == lanes[3][1] and lanes[2][0] != lanes[3][0]                    # 70, 69: one wave
    assert lanes[4][1] != lanes[5][1]                                                   # 200, 70: two waves
    assert lanes[8][1] < lanes[9][1]                                                    # 513 (wave 0) against 100 (wave 1): the lower index in the later wave


# ----------------------------------------------------------------------------------------------------------------------- ball query
def _oracle_ball(r, ns, xyz, q):
    return orc.query_ball_point(r, ns, _t(xyz), _t(q)).numpy()


@pytest.mark.parametrize("C", [3, 2])
@pytest.mark.parametrize("N", pc.BALL_N)
def test_ball_cases(N, C):
    on_sphere = 0
    for S in pc.BALL_S:
        xyz, q = pc.ball_case(N, S, C)
        d = pc.square_distance(q, xyz)
        np.testing.assert_array_equal(orc.square_distance(_t(q), _t(xyz)).double().numpy(), d)
        on_sphere += int((d == pc.R5 ** 2).sum())
        for ns in pc.BALL_NSAMPLE + [N + 5]:
            exp = pc.query_ball_point(pc.R5, ns, xyz, q)
            assert exp.shape == (2, S, ns)
            # nsample > N: the reference raises an IndexError (its group_first has nsample columns, its sorted row N); the oracle's
            # restatement returns the N columns of the row.  The kernel's own definition: those N columns, then the first hit again.
            ref = _oracle_ball(pc.R5, ns, xyz, q)
            assert ref.shape == (2, S, min(ns, N))
            np.testing.assert_array_equal(exp[:, :, :N], ref)
            np.testing.assert_array_equal(exp[:, :, N:], np.repeat(exp[:, :, :1], max(ns - N, 0), axis=2))
    if N >= 255:
        assert on_sphere >= 20, "no cloud point exactly on the sphere"


def test_ball_boundary_case():
    xyz, q, where = pc.ball_boundary_case()
    d = pc.square_distance(q, xyz)
    r_in = float(np.nextafter(F(pc.R5), F(0)))
    for b, i in enumerate(where):
        assert d[b, 0, i] == pc.R5 ** 2 and (np.delete(d[b, 0], i) > 0.5).all()
    assert pc.query_ball_point(pc.R5, 4, xyz, q).tolist() == [[[3] * 4], [[300] * 4]]                 # `>`: on the sphere is inside
    assert pc.query_ball_point(r_in, 4, xyz, q).tolist() == [[[301] * 4], [[301] * 4]]                # one ulp less: outside, empty
    for r in (pc.R5, r_in):
        np.testing.assert_array_equal(pc.query_ball_point(r, 4, xyz, q), _oracle_ball(r, 4, xyz, q))


def test_ball_tile_case():
    xyz, q, hits = pc.ball_tile_case()
    N = xyz.shape[1]
    d = pc.square_distance(q, xyz)
    for b in range(2):
        for j, h in enumerate(hits[b]):
            assert np.flatnonzero(~(d[b, j] > pc.R_TILE ** 2)).tolist() == sorted(h)
    assert hits[0][0] == [255, 256] and min(hits[0][1]) >= 512 and len(hits[0][2]) == 70 and hits[0][3] == []
    for ns in (1, 2, 5, 64, 80):
        exp = pc.query_ball_point(pc.R_TILE, ns, xyz, q)
        np.testing.assert_array_equal(exp, _oracle_ball(pc.R_TILE, ns, xyz, q))
        assert (exp[:, 3] == N).all()                                                                   # the empty ball: every slot N
        assert exp[0, 2].tolist() == (sorted(hits[0][2])[:ns] + [hits[0][2][0]] * max(0, ns - 70))      # truncation keeps the lowest, padding repeats the first


@pytest.mark.parametrize("r", pc.RADII_HIGH)
def test_radius_case_high(r):
    xyz, q, where = pc.radius_case_high(r)
    d = orc.square_distance(_t(q), _t(xyz)).numpy()
    thr = pc.ball_threshold(r)
    for b, i in enumerate(where):
        assert d[b, 0, i] == F(F(r) * F(r)) == np.nextafter(thr, F(2))        # on the squared float32 radius, one ulp above the reference's threshold
    exp = _oracle_ball(r, 40, xyz, q)
    np.testing.assert_array_equal(exp, pc.query_ball_point(r, 40, xyz, q, d=d))
    assert all(i not in exp[b] for b, i in enumerate(where))


@pytest.mark.parametrize("r", pc.RADII_LOW)
def test_radius_case_low(r):
    case = pc.radius_case_low(r)
    assert case is not None, "the bounded search found no point with d == float32(r ** 2)"
    xyz, q, where = case
    d = orc.square_distance(_t(q), _t(xyz)).numpy()
    thr = pc.ball_threshold(r)
    x, y = pc.radius_point_low(r)
    assert float(y) * 16 == round(float(y) * 16)                               # y*y is exact: contraction cannot change the sum
    assert F(np.float64(x) * np.float64(x) + np.float64(y) * np.float64(y)) == thr      # one rounding (fused) gives the same value
    for b, i in enumerate(where):
        assert d[b, 0, i] == thr == np.nextafter(F(F(r) * F(r)), F(2))         # on the reference's threshold, one ulp above the squared float32 radius
    exp = _oracle_ball(r, 40, xyz, q)
    np.testing.assert_array_equal(exp, pc.query_ball_point(r, 40, xyz, q, d=d))
    assert all(i in exp[b] for b, i in enumerate(where))


# ----------------------------------------------------------------------------------------------------------------------- kNN
@pytest.mark.parametrize("kind", ["side3", "triple"])
@pytest.mark.parametrize("k", pc.KNN_K)
def test_knn_cases(k, kind):
    tie_rows = rows = agree = cases = 0
    for N in pc.knn_ns(k):
        for S in pc.KNN_S:
            xyz, q, exp = pc.knn_case(k, N, S, kind)
            d = orc.square_distance(_t(q), _t(xyz))
            np.testing.assert_array_equal(d.double().numpy(), pc.square_distance(q, xyz))
            # the oracle's topk, re-sorted by (distance, index): the same distances rank by rank; which of the equals it took is torch's choice
            ref = orc.knn_point(k, _t(xyz), _t(q))
            rd = torch.gather(d, 2, ref)
            ed = torch.gather(d, 2, _t(exp))
            assert torch.equal(torch.sort(rd, dim=-1)[0], ed)
            key = rd.double() * (1 << 20) + ref.double()                       # d is a multiple of 2^-8 below 2^4: an exact (distance, index) key
            resorted = torch.gather(ref, 2, torch.argsort(key, dim=-1))
            agree += int(torch.equal(resorted, _t(exp))); cases += 1
            # the model's own rule: ascending (distance, index), and nothing left out has a smaller key than the last one taken
            ekey = ed.double() * (1 << 20) + _t(exp).double()
            assert bool((ekey[..., 1:] > ekey[..., :-1]).all())
            allkey = d.double() * (1 << 20) + torch.arange(N).double()
            assert torch.equal(torch.sort(allkey, dim=-1)[0][..., :k], ekey)
            if N > k:
                sd = torch.sort(d, dim=-1)[0]
                tie_rows += int((sd[..., k - 1] == sd[..., k]).sum()); rows += 2 * S
    print("k %d %s: a tie decides the k-th place in %d of %d rows; CPU topk re-sorted agrees in %d of %d cases" % (k, kind, tie_rows, rows, agree, cases))
    assert tie_rows >= rows // 4


# ----------------------------------------------------------------------------------------------------------------------- gathers
@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("D", pc.GATHER_D)
@pytest.mark.parametrize("C", pc.GATHER_C)
def test_gather_cases(C, D, dims):
    xyz, feat, centre, idx = pc.gather_case(C, D, dims)
    N = xyz.shape[1]
    assert idx[1].max() == N - 1 and idx[1].min() == 0 and (idx.size * C) % 256 and (idx.size * (C + D)) % 256
    np.testing.assert_array_equal(pc.index_points(xyz, idx), orc.index_points(_t(xyz), _t(idx)).numpy())
    if dims == 3:
        g = orc.index_points(_t(xyz), _t(idx)) - _t(centre)[:, :, None, :]
        ref = g if feat is None else torch.cat([g, orc.index_points(_t(feat), _t(idx))], dim=-1)
        np.testing.assert_array_equal(pc.group_concat(xyz, centre, feat, idx), ref.numpy())


def test_group_is_the_oracles():
    xyz, feat = pc.cloud(2, 50, tag=90), pc.integer_cotangent((2, 50, 4), tag=91)
    idx = pc.knn_point(7, xyz, xyz)
    ref, ref_gx = orc.group(7, _t(xyz), _t(feat), idx=_t(idx))
    np.testing.assert_array_equal(pc.group_concat(xyz, xyz, feat, idx), ref.numpy())
    np.testing.assert_array_equal(pc.group_concat(xyz, xyz, None, idx), ref_gx.numpy())


# ----------------------------------------------------------------------------------------------------------------------- CSR and adjoints
@pytest.mark.parametrize("N", pc.CSR_N)
def test_csr_cases(N):
    idx = pc.csr_case(N)
    B, S = idx.shape
    assert B == 3 and 0 <= idx.min() and idx.max() < N
    rowptr, src, valid = pc.gather_csr(idx, N)
    assert (valid == S).all() and src.min() >= 0
    deg = (rowptr[:, 1] - rowptr[:, 0]).reshape(B, N)
    for b in range(B):
        for n in {0, N // 2, N - 1}:                              # a segment lists exactly the slots that hold the point, ascending
            seg = src[rowptr[b * N + n, 0]:rowptr[b * N + n, 1]] - b * S
            assert seg.tolist() == np.flatnonzero(idx[b] == n).tolist()
    if N > 1:
        assert deg[1, N // 2] == pc.HUB_DEGREE and deg[1].sum() == S
        assert deg[2, N - 1] == 0 and (deg[2] == 0).sum() >= N // 2
    else:
        assert S == pc.HUB_DEGREE
    # the adjoint model is the transpose of the gather: <gather(p), w> == <p, scatter(w)> on integers
    w = pc.integer_cotangent((B * S, 4), tag=N)
    p = pc.integer_cotangent((B, N, 2), tag=N + 1).astype(np.float64)
    lhs = (pc.index_points(p, idx).reshape(B * S, 2) * w[:, 1:3]).sum()
    assert lhs == (p.reshape(B * N, 2) * pc.scatter_slots(w, 1, 2, idx, N)).sum()


def test_csr_drops_bad_indices():
    idx = pc.csr_case(1025)[:2].copy()
    idx[0, 5], idx[1, 3000] = -1, 1025
    rowptr, src, valid = pc.gather_csr(idx, 1025)
    assert valid.tolist() == [3000, 3000] and (src[[3000, 6001]] == -1).all()
    assert 5 not in src[:3000] and 3001 + 3000 not in src[3001:6001]


@pytest.mark.parametrize("N,k", [(33, 1), (33, 10), (300, 20)])
def test_edge_graphs_and_adjoint_model(N, k):
    idx = pc.edge_graph(N, k)
    assert (idx[1, :, 0] == N // 2).all() and (idx[2] != N - 1).all()
    C = 2
    x = pc.integer_cotangent((3, C, N), tag=5).astype(np.float64)
    dE = pc.integer_cotangent((3, 2 * C, N, k), tag=6)
    xt = torch.from_numpy(x).requires_grad_(True)
    ee = orc.get_edge_features(xt, k, idx=_t(idx).reshape(3, N * k))
    (ee * _t(dE).double()).sum().backward()
    np.testing.assert_array_equal(xt.grad.numpy(), pc.edge_features_cm_bwd(dE, idx, k))
