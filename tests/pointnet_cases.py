"""A numpy model of the ball-query / grouping kernels of csrc/pointnet.hip (spgan.pointnet_util) and the clouds they are tested on.
Shared by tests/test_pointnet_edges_gpu.py (the kernels) and tests/test_pointnet_cases_cpu.py (the cases themselves).

Clouds are lattice clouds: integer coordinates times 2^-4 (pointops_model.lattice_cloud; side 17 gives [0, 16], side 3 gives {0, 1, 2}
so that distances tie constantly).  On them every product, sum and difference of the expanded form -2ab + |a|^2 + |b|^2 and of the
difference form sum((a-b)^2) is a multiple of 2^-8 far below 2^24 of them: exact in float32 in any order, with or without contraction.
The model therefore works in float64, and an index output has exactly one right answer.

The model's rules are the ones the kernels document:
    farthest point sampling   the lowest index among equal (maximal) distances
    knn_point                 ascending (distance, index)
    query_ball_point          hits are the points with not (d > thr), ascending index, the first `nsample`, padded with the first hit;
                              no hit at all: every slot is N.  thr is float32(radius ** 2): what torch compares a float32 distance with
                              when the reference writes `sqrdists > radius ** 2` (ball_threshold; test_pointnet_cases_cpu.py shows it).
    gather CSR                per point the global slot numbers b*S + e that hold it, ascending (a stable sort of the slots by index)
"""
import functools

import numpy as np

import pointops_model as pm

F = np.float32
U = F(2.0 ** -4)                        # the lattice unit
R5 = 5 * 2.0 ** -4                      # the boundary radius: (3,4,0) and (5,0,0) lattice offsets lie exactly on this sphere


# ----------------------------------------------------------------------------------------------------------------------- the model
def ball_threshold(radius):
    """float32(radius ** 2), round to nearest: `d > radius ** 2` with a float32 tensor d casts the Python double to float32."""
    return F(float(radius) ** 2)


def square_distance(src, dst):
    """[B,N,C], [B,M,C] -> float64 [B,N,M] in the expanded form."""
    a, b = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    d = -2.0 * np.einsum("bnc,bmc->bnm", a, b)
    d = d + (a * a).sum(-1)[:, :, None]
    return d + (b * b).sum(-1)[:, None, :]


def query_ball_point(radius, nsample, xyz, new_xyz, d=None):
    """-> int64 [B,S,nsample] (nsample > N, where the reference raises an IndexError: the hits, then the first hit, like any short row).
    d: the distances [B,S,N] to use instead of the model's own (for clouds that are not lattice clouds)."""
    thr = np.float64(ball_threshold(radius))
    d = square_distance(new_xyz, xyz) if d is None else np.asarray(d, dtype=np.float64)
    B, S, N = d.shape
    out = np.full((B, S, nsample), N, dtype=np.int64)
    for b in range(B):
        for s in range(S):
            h = np.flatnonzero(~(d[b, s] > thr))[:nsample]
            if h.size:
                out[b, s, :] = h[0]
                out[b, s, :h.size] = h
    return out


def knn_point(nsample, xyz, new_xyz):
    """-> int64 [B,S,nsample], ascending (distance, index)."""
    d = square_distance(new_xyz, xyz)
    return np.argsort(d, axis=2, kind="stable")[:, :, :nsample].astype(np.int64)


def farthest_point_sample(xyz, npoint, start):
    """-> int64 [B,npoint]: the difference form, running minimum from 1e10, the first maximum (np.argmax) = the lowest index."""
    x = np.asarray(xyz, dtype=np.float64)
    B, N, _ = x.shape
    out = np.zeros((B, npoint), dtype=np.int64)
    for b in range(B):
        dist = np.full(N, 1e10)
        far = int(start[b])
        for i in range(npoint):
            out[b, i] = far
            dist = np.minimum(dist, ((x[b] - x[b, far]) ** 2).sum(-1))
            far = int(np.argmax(dist))
    return out


def index_points(points, idx):
    B = points.shape[0]
    return np.stack([points[b][idx[b]] for b in range(B)])


def group_concat(xyz, center, feat, idx):
    """-> [B,S,K,C+D] = [xyz[idx] - center | feat[idx]]."""
    g = index_points(xyz, idx) - center[:, :, None, :]
    return g if feat is None else np.concatenate([g, index_points(feat, idx)], axis=-1)


def gather_csr(idx, N):
    """idx int64 [B,S] -> (rowptr int32 [B*N,2], src int32 [B*S], valid [B]): indices outside [0,N) own no slot; the tail
    src[b*S + valid[b] : (b+1)*S] is unused (left at -1 here)."""
    idx = np.asarray(idx).reshape(idx.shape[0], -1)
    B, S = idx.shape
    rowptr = np.zeros((B * N, 2), dtype=np.int32)
    src = np.full(B * S, -1, dtype=np.int32)
    valid = np.zeros(B, dtype=np.int64)
    for b in range(B):
        ok = np.flatnonzero((idx[b] >= 0) & (idx[b] < N))
        order = ok[np.argsort(idx[b][ok], kind="stable")]
        deg = np.bincount(idx[b][ok], minlength=N)
        end = np.cumsum(deg)
        rowptr[b * N:(b + 1) * N, 0] = b * S + end - deg
        rowptr[b * N:(b + 1) * N, 1] = b * S + end
        src[b * S:b * S + ok.size] = b * S + order
        valid[b] = ok.size
    return rowptr, src, valid


def scatter_slots(dout2d, col0, C, idx, N):
    """float64 [B*N, C]: dpoints[b*N + idx[b,e]] += dout2d[b*S + e, col0:col0+C]."""
    idx = np.asarray(idx).reshape(idx.shape[0], -1)
    B, S = idx.shape
    out = np.zeros((B * N, C))
    np.add.at(out, (np.arange(B)[:, None] * N + idx).reshape(-1), np.asarray(dout2d, dtype=np.float64)[:, col0:col0 + C])
    return out


def group_center_bwd(dout2d, K, C):
    d = np.asarray(dout2d, dtype=np.float64)
    return -d[:, :C].reshape(-1, K, C).sum(1)


def edge_features_cm_bwd(dE, idx, k):
    """dE [B,2C,N,k], idx [B,N,k] -> float64 dx [B,C,N] of E = [central | x[idx] - central]."""
    dE = np.asarray(dE, dtype=np.float64)
    B, C2, N, _ = dE.shape
    C = C2 // 2
    dx = dE[:, :C].sum(-1) - dE[:, C:].sum(-1)
    for b in range(B):
        for c in range(C):
            np.add.at(dx[b, c], idx[b].reshape(-1), dE[b, C + c].reshape(-1))
    return dx


# ----------------------------------------------------------------------------------------------------------------------- clouds
def _rng(*key):
    return np.random.default_rng([20261020] + [int(k) for k in key])


def cloud(B, n, side=17, tag=0):
    return pm.lattice_cloud(_rng(1, B, n, side, tag), B, n, side)


def triplicated(B, n, side=17, tag=0):
    """Every position occurs three times (n rounded up: the last copies are cut), interleaved so that twins are far apart in index."""
    m = -(-n // 3)
    base = pm.lattice_cloud(_rng(2, B, n, side, tag), B, m, side)
    return np.ascontiguousarray(np.concatenate([base, base, base], axis=1)[:, :n])


def integer_cotangent(shape, tag=0, lo=-4, hi=5):
    """Small integers as float32: every partial sum of them is an integer below 2^24, so a float32 sum is exact in any order."""
    return _rng(3, tag, *shape).integers(lo, hi, size=shape).astype(F)


# ----------------------------------------------------------------------------------------------------------------------- square distance
SQDIST_SHAPES = [(1, 1, 1, 3), (2, 5, 257, 3), (2, 3, 256, 1), (1, 2, 300, 7)]            # (B, N, M, C)


def sqdist_case(B, N, M, C):
    r = _rng(4, B, N, M, C)
    return (r.integers(0, 17, size=(B, N, C)).astype(F) * U).astype(F), (r.integers(0, 17, size=(B, M, C)).astype(F) * U).astype(F)


# ----------------------------------------------------------------------------------------------------------------------- farthest point sampling
FPS_N = [1, 2, 63, 64, 65, 511, 512, 513, 1025]


def fps_npoints(N):
    return sorted({1, min(N, 40), N})


@functools.lru_cache(maxsize=None)
def fps_case(N, kind):
    """kind 'side3': lattice side 3 (maximal distances tie constantly); 'triple': every position three times, side 17.
    -> (xyz [2,N,3], start [2] with N-1 in it, {npoint: expected})."""
    xyz = cloud(2, N, side=3, tag=10) if kind == "side3" else triplicated(2, N, side=17, tag=11)
    start = np.array([N - 1, N // 3], dtype=np.int64)
    full = farthest_point_sample(xyz, N, start)                           # a shorter run is a prefix of a longer one
    return xyz, start, {p: np.ascontiguousarray(full[:, :p]) for p in fps_npoints(N)}


FPS_TIE_N = 1025
FPS_TIE_SETS = [(517, 5), (70, 69), (200, 70), (600, 520), (513, 100), (1024, 517)]


def fps_tie_cloud(sets):
    """Batch entry b: every point at the origin except the set sets[b] at (1,0,0).  From start 0 the second pick is min(sets[b])."""
    xyz = np.zeros((len(sets), FPS_TIE_N, 3), dtype=F)
    for b, I in enumerate(sets):
        xyz[b, list(I), 0] = 1.0
    return xyz


# ----------------------------------------------------------------------------------------------------------------------- ball query
BALL_N = [1, 255, 256, 257, 513]
BALL_S = [1, 256, 257]


BALL_NSAMPLE = [1, 3, 64]                 # and N + 5: more slots than points


@functools.lru_cache(maxsize=None)
def ball_case(N, S, C=3):
    """Lattice cloud and queries ([0,16] * 2^-4; C = 2 drops z): radius R5 puts many cloud points exactly on the sphere."""
    xyz, q = cloud(2, N, tag=20 + S)[..., :C].copy(), cloud(2, S, tag=40 + N)[..., :C].copy()
    q[:, 0] = xyz[:, N // 2]                                              # one query is a cloud point
    return np.ascontiguousarray(xyz), np.ascontiguousarray(q)


def ball_boundary_case():
    """Query (8,8,8)*2^-4; cloud point 3 at offset (3,4,0)*2^-4: d == R5^2 exactly.  Everything else is far away (two corners).
    Batch entry 1 has the boundary point at index 300 (second tile) and the query elsewhere."""
    N = 301
    xyz = np.zeros((2, N, 3), dtype=F)
    xyz[:, 1::2] = 16 * U
    q = np.zeros((2, 1, 3), dtype=F)
    q[0, 0] = (8 * U, 8 * U, 8 * U)
    q[1, 0] = (6 * U, 9 * U, 7 * U)
    xyz[0, 3] = q[0, 0] + np.array([3, 4, 0], dtype=F) * U
    xyz[1, 300] = q[1, 0] + np.array([0, -3, 4], dtype=F) * U
    return xyz, q, [3, 300]


def ball_tile_case():
    """N 600, three 256-candidate tiles; all points far from the queries except a chosen hit set per query.
    query 0: hits 255 and 256 (straddle the tile edge); query 1: hits only in the last tile (512, 599); query 2: 70 hits spread over all
    tiles (truncation keeps the lowest); query 3: no hit at all.  Batch entry 1: the same with every hit index shifted by -1 (254/255, ...)."""
    N = 600
    hits = [[255, 256], [512, 599], list(range(3, 600, 8))[:70], []]
    xyz = np.zeros((2, N, 3), dtype=F)
    q = np.zeros((2, 4, 3), dtype=F)
    for b in range(2):
        xyz[b, :, 2] = 16 * U                                             # far plane z = 1
        for j, h in enumerate(hits):
            centre = np.array([4 * j + 1, 2 + b, 0], dtype=F) * U         # queries 4 lattice units apart in x: balls of radius 2 are disjoint
            q[b, j] = centre
            for t, i in enumerate(h):
                xyz[b, i - b] = centre + np.array([(t % 3) - 1, (t // 3) % 2, 0], dtype=F) * U
    return xyz, q, [[[i - b for i in h] for h in hits] for b in range(2)]


R_TILE = 2 * 2.0 ** -4

RADII_HIGH = (0.05, 0.1, 0.2, 0.4, 0.8)        # float32(r) * float32(r) is one ulp ABOVE float32(r ** 2)
RADII_LOW = (0.35, 0.45, 0.7, 0.9)             # ... one ulp BELOW


def _filler(n, tag):
    """Lattice points around the special one: their distances are multiples of 2^-8, exact, on either side of the thresholds."""
    return cloud(1, n, tag=tag)[0]


def radius_case_high(r):
    """Query at the origin; cloud point 7 is (float32(r), 0, 0): its float32 distance is float32(r)^2 rounded, one ulp above the reference's
    threshold float32(r ** 2) -> outside for the reference, inside for a kernel that squares the float32 radius.  -> (xyz [2,N,3], q, index)."""
    N = 40
    xyz = np.stack([_filler(N, 60), _filler(N, 61)])
    xyz[0, 7] = (F(r), 0, 0)
    xyz[1, 33] = (0, F(r), 0)
    return xyz, np.zeros((2, 1, 3), dtype=F), [7, 33]


def radius_point_low(r):
    """A point (x, m*2^-4, 0) whose float32 squared norm equals float32(r ** 2) exactly: m*m*2^-8 is exact, so fl(fl(x*x) + y*y) is the
    same with and without contraction.  A bounded search over m and the float32 neighbours of sqrt(thr - y^2); None if there is none."""
    thr = ball_threshold(r)
    for m in range(0, 17):
        y = F(m) * U
        rest = np.float64(thr) - np.float64(y) ** 2
        if rest <= 0:
            break
        x = F(np.sqrt(rest))
        for _ in range(8):
            x = np.nextafter(x, F(0))
        for _ in range(17):
            if F(F(x * x) + F(y * y)) == thr:
                return x, y
            x = np.nextafter(x, F(2))
    return None


def radius_case_low(r):
    """As radius_case_high with a point exactly ON the reference's threshold (inside: the mask is `>`); a kernel that squares the float32
    radius has its threshold one ulp lower and leaves the point out."""
    pt = radius_point_low(r)
    if pt is None:
        return None
    N = 40
    xyz = np.stack([_filler(N, 62), _filler(N, 63)])
    xyz[0, 5] = (pt[0], pt[1], 0)
    xyz[1, 38] = (0, pt[1], pt[0])
    return xyz, np.zeros((2, 1, 3), dtype=F), [5, 38]


# ----------------------------------------------------------------------------------------------------------------------- kNN
KNN_K = [1, 10, 11, 20, 21, 32]
KNN_S = [1, 257]


def knn_ns(k):
    return sorted({k, 255, 256, 257, 600})


@functools.lru_cache(maxsize=None)
def knn_case(k, N, S, kind):
    xyz = cloud(2, N, side=3, tag=70 + k) if kind == "side3" else triplicated(2, N, side=17, tag=71 + k)
    q = cloud(2, S, side=3 if kind == "side3" else 17, tag=72 + N)
    q[:, 0] = xyz[:, N - 1]
    return xyz, q, knn_point(k, xyz, q)


# ----------------------------------------------------------------------------------------------------------------------- gathers
GATHER_C = [1, 3, 67]
GATHER_D = [0, 5]


def gather_case(C, D, dims):
    """xyz [2,N,C], feat [2,N,D] | None, centre [2,S,C], idx [2,S] or [2,S,K]; element counts no multiple of 256; 0 and N-1 in the last entry."""
    N, S, K = 37, 9, 7
    r = _rng(5, C, D, dims)
    xyz = (r.integers(0, 17, size=(2, N, C)).astype(F) * U).astype(F)
    feat = (r.integers(-8, 9, size=(2, N, D)).astype(F) * U).astype(F) if D else None
    centre = (r.integers(0, 17, size=(2, S, C)).astype(F) * U).astype(F)
    idx = r.integers(0, N, size=(2, S, K) if dims == 3 else (2, S)).astype(np.int64)
    idx[1].reshape(-1)[-1] = N - 1
    idx[1].reshape(-1)[-2] = 0
    return xyz, feat, centre, idx


# ----------------------------------------------------------------------------------------------------------------------- gather CSR
CSR_N = [1, 1023, 1024, 1025, 8176, 8177, 16384]
CSR_SLOTS = 3001
HUB_DEGREE = 2048          # one thread insertion-sorts a segment: the work grows with the square of the degree


@functools.lru_cache(maxsize=None)
def csr_case(N):
    """idx int64 [3, S]: entry 0 random; entry 1 one hub (point N // 2) holding HUB_DEGREE slots, scattered among random ones; entry 2 only
    every third point is ever gathered (degree 0 elsewhere, the last point included when N > 1)."""
    r = _rng(6, N)
    S = CSR_SLOTS
    idx = r.integers(0, N, size=(3, S)).astype(np.int64)
    if N > 1:
        hub = N // 2
        other = r.integers(0, N - 1, size=S)
        idx[1] = np.where(other >= hub, other + 1, other)                 # never the hub ...
        idx[1, r.permutation(S)[:HUB_DEGREE]] = hub                       # ... except in exactly HUB_DEGREE scattered slots
        idx[2] = (idx[2] // 3) * 3
        idx[2][idx[2] == N - 1] = 0
    else:
        idx = idx[:, :HUB_DEGREE]                                         # N 1: the one point holds every slot
    return idx


# ----------------------------------------------------------------------------------------------------------------------- edge-feature graphs
def edge_graph(N, k):
    """idx int64 [3,N,k]: entry 0 random; entry 1 every point gathers the hub N // 2 in slot 0; entry 2 nobody gathers point N - 1."""
    r = _rng(7, N, k)
    idx = r.integers(0, N, size=(3, N, k)).astype(np.int64)
    idx[1, :, 0] = N // 2
    idx[2][idx[2] == N - 1] = 0
    return idx
