"""GPU: the kernels of csrc/pointnet.hip (spgan.pointnet_util) on exact clouds, against the numpy model of tests/pointnet_cases.py.

Lattice clouds (integer coordinates times 2^-4) make every distance exact in float32, so every index output has one right answer and is
compared with assert_array_equal: no row, element or case is left out, and there is no tolerance anywhere in this file.  The adjoint
kernels get small-integer cotangents: every sum is then exact in float32 whatever its order and must equal the float64 sum bit for bit.
B >= 2 with different clouds per batch entry throughout.  tests/test_pointnet_cases_cpu.py proves the cases (model == oracle, ties and
boundary points really present).
"""
import numpy as np
import pytest
import torch

import pointnet_cases as pc
from oracle import spgan_oracle as orc
from spgan import _lib, ops
from spgan import pointnet_util as pu

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.detach().cpu().numpy()


def _ball(r, ns, xyz, q):
    got = pu.query_ball_point(r, ns, _t(xyz), _t(q))
    assert got.dtype == torch.int64
    return _n(got)


# ----------------------------------------------------------------------------------------------------------------------- square distance
@pytest.mark.parametrize("B,N,M,C", pc.SQDIST_SHAPES)
def test_square_distance_lattice(B, N, M, C):
    a, b = pc.sqdist_case(B, N, M, C)
    got = pu.square_distance(_t(a), _t(b))
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, N, M)
    np.testing.assert_array_equal(_n(got).astype(np.float64), pc.square_distance(a, b))


# ----------------------------------------------------------------------------------------------------------------------- farthest point sampling
@pytest.mark.parametrize("kind", ["side3", "triple"])
@pytest.mark.parametrize("N", pc.FPS_N)
def test_fps_lattice(N, kind):
    """Lattice side 3 (maximal distances tie at almost every step) and a cloud with every position three times (npoint = N is above the
    number of distinct positions: once all distances are 0, index 0 repeats).  start differs per batch entry and includes N - 1."""
    xyz, start, exp = pc.fps_case(N, kind)
    for npoint, e in exp.items():
        got = pu.farthest_point_sample(_t(xyz), npoint, _t(start))
        assert got.dtype == torch.int64
        np.testing.assert_array_equal(_n(got), e)


def test_fps_constructed_ties():
    """N 1025 (three strides of the 512-thread block), start 0: every point at the origin except a set I at (1,0,0) -- the second pick is
    min(I), whether the two live in one thread (517, 5), one wave, two waves, or with the lower index in the later wave (513, 100)."""
    xyz = pc.fps_tie_cloud(pc.FPS_TIE_SETS)
    B = len(pc.FPS_TIE_SETS)
    start = np.zeros(B, dtype=np.int64)
    exp = pc.farthest_point_sample(xyz, 4, start)
    assert exp[:, 1].tolist() == [min(I) for I in pc.FPS_TIE_SETS]
    np.testing.assert_array_equal(_n(pu.farthest_point_sample(_t(xyz), 4, _t(start))), exp)
    for b, I in enumerate(pc.FPS_TIE_SETS):                                           # and each cloud on its own (one workgroup)
        np.testing.assert_array_equal(_n(pu.farthest_point_sample(_t(xyz[b:b + 1]), 4, _t(start[:1]))), exp[b:b + 1])


# ----------------------------------------------------------------------------------------------------------------------- ball query
@pytest.mark.parametrize("C", [3, 2])
@pytest.mark.parametrize("N", pc.BALL_N)
def test_ball_lattice(N, C):
    """Radius 5 * 2^-4 on [0,16] * 2^-4 lattice clouds: points at offsets like (3,4,0) lie exactly on the sphere and are inside (the mask
    is `>`).  C = 2 runs the second instantiation of the kernel against the same model."""
    for S in pc.BALL_S:
        xyz, q = pc.ball_case(N, S, C)
        for ns in pc.BALL_NSAMPLE:
            np.testing.assert_array_equal(_ball(pc.R5, ns, xyz, q), pc.query_ball_point(pc.R5, ns, xyz, q))


@pytest.mark.parametrize("N", pc.BALL_N)
def test_ball_more_slots_than_points(N):
    """nsample > N, where the reference raises an IndexError: all nsample slots are filled like any short row -- the hits (at most N),
    then the first hit again, or N throughout in an empty ball."""
    xyz, q = pc.ball_case(N, 257)
    ns = N + 5
    exp = pc.query_ball_point(pc.R5, ns, xyz, q)
    assert exp.shape == (2, 257, ns)
    np.testing.assert_array_equal(_ball(pc.R5, ns, xyz, q), exp)


def test_ball_boundary_point_is_inside():
    xyz, q, where = pc.ball_boundary_case()
    assert _ball(pc.R5, 4, xyz, q).tolist() == [[[where[0]] * 4], [[where[1]] * 4]]
    r_in = float(np.nextafter(F(pc.R5), F(0)))
    N = xyz.shape[1]
    assert _ball(r_in, 4, xyz, q).tolist() == [[[N] * 4], [[N] * 4]]


def test_ball_tile_edges_truncation_padding_and_the_empty_ball():
    """Hits at 255 and 256 (and 254 / 255 in the second batch entry) straddle the 256-candidate tile; hits only in the last tile; 70 hits
    of which the lowest nsample are kept; fewer hits than slots: the first hit repeats.

    The empty ball: every slot is N, as in the reference.  Only the index tensor is asserted -- it is NOT gathered through:
    index_points and group_concat do not bounds-check in the forward, by the design stated at ops.index_check_flag (the reference would
    raise an IndexError there).  Changing that is not this test's business."""
    xyz, q, hits = pc.ball_tile_case()
    N = xyz.shape[1]
    for ns in (1, 2, 5, 64, 80):
        got = _ball(pc.R_TILE, ns, xyz, q)
        np.testing.assert_array_equal(got, pc.query_ball_point(pc.R_TILE, ns, xyz, q))
        assert (got[:, 3] == N).all()
    got = _ball(pc.R_TILE, 5, xyz, q)
    assert got[0, 0].tolist() == [255, 256, 255, 255, 255] and got[1, 0].tolist() == [254, 255, 254, 254, 254]
    assert got[0, 1].tolist() == [512, 599, 512, 512, 512]
    assert got[0, 2].tolist() == sorted(hits[0][2])[:5]


@pytest.mark.parametrize("r", pc.RADII_HIGH)
def test_ball_radius_rounding_high(r):
    """float32(r) * float32(r) rounds one ulp above float32(r ** 2), the threshold the reference's `sqrdists > radius ** 2` compares with:
    the cloud point (float32(r), 0, 0) seen from the origin has exactly that distance and is OUTSIDE for the reference.  Expected
    indices: the oracle's expression on the CPU."""
    xyz, q, where = pc.radius_case_high(r)
    exp = orc.query_ball_point(r, 40, torch.from_numpy(xyz), torch.from_numpy(q)).numpy()
    assert all(i not in exp[b] for b, i in enumerate(where))
    np.testing.assert_array_equal(_ball(r, 40, xyz, q), exp)


@pytest.mark.parametrize("r", pc.RADII_LOW)
def test_ball_radius_rounding_low(r):
    """float32(r) * float32(r) rounds one ulp below float32(r ** 2): a cloud point whose float32 distance from the origin equals
    float32(r ** 2) is INSIDE for the reference (pointnet_cases.radius_point_low finds one for each of these four radii)."""
    xyz, q, where = pc.radius_case_low(r)
    exp = orc.query_ball_point(r, 40, torch.from_numpy(xyz), torch.from_numpy(q)).numpy()
    assert all(i in exp[b] for b, i in enumerate(where))
    np.testing.assert_array_equal(_ball(r, 40, xyz, q), exp)


# ----------------------------------------------------------------------------------------------------------------------- kNN
@pytest.mark.parametrize("kind", ["side3", "triple"])
@pytest.mark.parametrize("k", pc.KNN_K)
def test_knn_point_lattice(k, kind):
    """k at and next to the template breaks (10 | 11, 20 | 21, 32), N = k (nsample == N), N around the 256-candidate tile and three tiles;
    lattice side 3 and a triplicated cloud: zero-distance and equal-distance ties decide the k-th place in most rows."""
    for N in pc.knn_ns(k):
        for S in pc.KNN_S:
            xyz, q, exp = pc.knn_case(k, N, S, kind)
            got = pu.knn_point(k, _t(xyz), _t(q))
            assert got.dtype == torch.int64
            np.testing.assert_array_equal(_n(got), exp, err_msg="k %d N %d S %d" % (k, N, S))


def test_knn_point_refusals():
    xyz = _t(pc.cloud(2, 40))
    out = torch.empty((2, 40, 64), dtype=torch.int64, device=DEV)
    lib = _lib.load()
    for ns, n in ((33, 40), (21, 20), (2, 1)):                                        # nsample 33; nsample > N
        assert lib.spgan_knn_point(ns, xyz.data_ptr(), xyz.data_ptr(), 2, n, n, 3, out.data_ptr(), None) == -22
    with pytest.raises(RuntimeError, match="knn_point"):
        pu.knn_point(33, xyz, xyz)
    with pytest.raises(RuntimeError, match="knn_point"):
        pu.knn_point(21, xyz[:, :20].contiguous(), xyz)


# ----------------------------------------------------------------------------------------------------------------------- gathers, forward
@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("D", pc.GATHER_D)
@pytest.mark.parametrize("C", pc.GATHER_C)
def test_index_points_and_group_concat_forward(C, D, dims):
    xyz, feat, centre, idx = pc.gather_case(C, D, dims)
    got = pu.index_points(_t(xyz), _t(idx))
    np.testing.assert_array_equal(_n(got), orc.index_points(torch.from_numpy(xyz), torch.from_numpy(idx)).numpy())
    if D:
        np.testing.assert_array_equal(_n(pu.index_points(_t(feat), _t(idx))), pc.index_points(feat, idx))
    idx3 = idx if dims == 3 else idx[:, :, None]                                      # [B,S] as groups of one
    got = pu._group_concat_raw(_t(xyz), _t(centre), None if feat is None else _t(feat), _t(idx3))
    np.testing.assert_array_equal(_n(got), pc.group_concat(xyz, centre, feat, idx3))


# ----------------------------------------------------------------------------------------------------------------------- gather CSR
def _csr(idx, N, bad=None):
    B, S = idx.shape
    rowptr = torch.full((B * N, 2), -1, dtype=torch.int32, device=DEV)
    src = torch.full((B * S,), -1, dtype=torch.int32, device=DEV)
    st = _lib.load().spgan_gather_csr(_t(idx).data_ptr(), B, S, N, rowptr.data_ptr(), src.data_ptr(), None if bad is None else bad.data_ptr(), None)
    torch.cuda.synchronize()
    return st, _n(rowptr), _n(src)


@pytest.mark.parametrize("N", pc.CSR_N)
def test_gather_csr(N):
    """Three shapes with different patterns (random; one hub of 2048 slots, the insertion sort's worst customer; points of degree 0),
    N at the 1024-thread block, at the > 64 KB LDS opt-in (8177) and at the limit (16384): rowptr and src equal the numpy CSR."""
    idx = pc.csr_case(N)
    exp_rowptr, exp_src, _ = pc.gather_csr(idx, N)
    rowptr, src = pu.gather_csr(_t(idx), N)
    np.testing.assert_array_equal(_n(rowptr), exp_rowptr)
    np.testing.assert_array_equal(_n(src), exp_src)
    st, rowptr, src = _csr(idx, N)
    assert st == 0
    np.testing.assert_array_equal(rowptr, exp_rowptr)
    np.testing.assert_array_equal(src, exp_src)


def test_gather_csr_refuses_16385_points():
    idx = np.zeros((2, 8), dtype=np.int64)
    st, rowptr, src = _csr(idx, 16385)
    assert st == -22 and (rowptr == -1).all() and (src == -1).all()


def test_gather_csr_bad_indices_set_the_flag_and_own_no_slot():
    N = 1025
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    for where in ([(0, 5, -1)], [(1, 3000, N)], [(0, 5, -1), (1, 3000, N)]):          # each bad value in a call of its own, then both
        idx = pc.csr_case(N)[:2].copy()
        for b, e, v in where:
            idx[b, e] = v
        exp_rowptr, exp_src, valid = pc.gather_csr(idx, N)
        bad.zero_()
        st, rowptr, src = _csr(idx, N, bad)
        S = idx.shape[1]
        assert st == 0 and int(bad.item()) == 1
        assert sorted(valid.tolist()) == ([S - 1, S] if len(where) == 1 else [S - 1, S - 1])
        np.testing.assert_array_equal(rowptr, exp_rowptr)
        for b in range(2):                                                            # the unused tail of each shape's range is not compared
            np.testing.assert_array_equal(src[b * S:b * S + valid[b]], exp_src[b * S:b * S + valid[b]])
    bad.zero_()
    assert _csr(pc.csr_case(N), N, bad)[0] == 0 and int(bad.item()) == 0


# ----------------------------------------------------------------------------------------------------------------------- adjoint kernels
@pytest.mark.parametrize("C", pc.GATHER_C)
def test_scatter_slots_column_window(C):
    """A window [col0, col0 + C) of wider rows (ld > C, col0 > 0), over the hub / degree-0 patterns of the CSR cases."""
    N = 1025
    idx = pc.csr_case(N)
    B, S = idx.shape
    rowptr, src = pu.gather_csr(_t(idx), N)
    for col0, ld in ((2, C + 5), (0, C)):
        dout = pc.integer_cotangent((B * S, ld), tag=C)
        got = pu._scatter_slots(_t(dout), col0, C, rowptr, src, (B, N, C))
        np.testing.assert_array_equal(_n(got).astype(np.float64).reshape(B * N, C), pc.scatter_slots(dout, col0, C, idx, N))


@pytest.mark.parametrize("K", [1, 33, 160])
def test_group_center_bwd(K):
    Q, C, ld = 2 * 37, 3, 8
    dout = pc.integer_cotangent((Q * K, ld), tag=K)
    d = _t(dout)
    out = torch.empty((Q, C), dtype=torch.float32, device=DEV)
    assert _lib.load().spgan_group_center_bwd(d.data_ptr(), ld, Q, K, C, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_n(out).astype(np.float64), pc.group_center_bwd(dout, K, C))


@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("N", [33, 300])
@pytest.mark.parametrize("k", [1, 10, 20])
def test_edge_features_cm_bwd_built_graphs(k, N, C):
    """Three graphs: random, a hub gathered by every point (in-degree >= N), a point gathered by none."""
    idx = pc.edge_graph(N, k)
    dE = pc.integer_cotangent((3, 2 * C, N, k), tag=100 * k + C)
    got = ops.edge_features_cm_bwd(_t(dE), _t(idx.reshape(3, N * k)), k)
    np.testing.assert_array_equal(_n(got).astype(np.float64), pc.edge_features_cm_bwd(dE, idx, k))


# ----------------------------------------------------------------------------------------------------------------------- end to end
def _grads(fn, inputs, cots):
    outs = fn(*inputs)
    outs = outs if isinstance(outs, tuple) else (outs,)
    return torch.autograd.grad([o for o in outs], inputs, [c.to(o) for o, c in zip(outs, cots)])


def test_gather_gradients_equal_float64_autograd():
    """index_points, group and sample_and_group with integer cotangents on a lattice cloud: gradients equal the oracle's float64 autograd
    exactly, and two runs give identical bits."""
    B, N, S, K, D = 2, 300, 40, 12, 4
    xyz = pc.cloud(B, N, tag=95)
    feat = pc.integer_cotangent((B, N, D), tag=96)
    start = np.array([N - 1, 7], dtype=np.int64)

    def both(fn_gpu, fn_ref, arrays, cots):
        g_in = [_t(a).requires_grad_(True) for a in arrays]
        r_in = [torch.from_numpy(a).double().requires_grad_(True) for a in arrays]
        got = _grads(fn_gpu, g_in, [_t(c) for c in cots])
        again = _grads(fn_gpu, g_in, [_t(c) for c in cots])
        ref = _grads(fn_ref, r_in, [torch.from_numpy(c) for c in cots])
        for g, g2, r in zip(got, again, ref):
            np.testing.assert_array_equal(_n(g).astype(np.float64), r.numpy())
            assert torch.equal(g, g2)

    # index_points, 3-D idx with the repeats of a padded ball query, and 2-D idx
    idx3 = pc.query_ball_point(pc.R5, K, xyz, xyz[:, :S])
    both(lambda f: pu.index_points(f, _t(idx3)), lambda f: orc.index_points(f, torch.from_numpy(idx3)), [feat], [pc.integer_cotangent((B, S, K, D), tag=1)])
    idx2 = np.ascontiguousarray(idx3[:, :, -1])
    both(lambda f: pu.index_points(f, _t(idx2)), lambda f: orc.index_points(f, torch.from_numpy(idx2)), [feat], [pc.integer_cotangent((B, S, D), tag=2)])
    # group: xyz in the gathered and in the centre role, and the features
    knn = pc.knn_point(K, xyz, xyz)
    np.testing.assert_array_equal(_n(pu.knn_point(K, _t(xyz), _t(xyz))), knn)
    cots = [pc.integer_cotangent((B, N, K, 3 + D), tag=3), pc.integer_cotangent((B, N, K, 3), tag=4)]
    both(lambda x, f: pu.group(K, x, f), lambda x, f: orc.group(K, x, f, idx=torch.from_numpy(knn)), [xyz, feat], cots)
    # sample_and_group: FPS centres, ball query, centred grouping.  The reference side is the oracle's composition (sample_and_group's
    # body) around the MODEL's centres: the oracle's own sampling loop picks among equal maxima by torch.max, whose choice is unspecified.
    fps = pc.farthest_point_sample(xyz, S, start)
    np.testing.assert_array_equal(_n(pu.farthest_point_sample(_t(xyz), S, _t(start))), fps)

    def ref_sag(x, f):
        new_xyz = orc.index_points(x, torch.from_numpy(fps))
        idx = orc.query_ball_point(pc.R5, K, x, new_xyz)
        gx = orc.index_points(x, idx) - new_xyz.view(B, S, 1, 3)
        return new_xyz, torch.cat([gx, orc.index_points(f, idx)], dim=-1)

    cots = [pc.integer_cotangent((B, S, 3), tag=5), pc.integer_cotangent((B, S, K, 3 + D), tag=6)]
    both(lambda x, f: pu.sample_and_group(S, pc.R5, K, x, f, start=_t(start)), ref_sag, [xyz, feat], cots)
    nx, npts = pu.sample_and_group(S, pc.R5, K, _t(xyz), _t(feat), start=_t(start))
    rx, rpts = ref_sag(torch.from_numpy(xyz), torch.from_numpy(feat))
    np.testing.assert_array_equal(_n(nx), rx.numpy())
    np.testing.assert_array_equal(_n(npts), rpts.numpy())
