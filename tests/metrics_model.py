"""Plain numpy models of the evaluation-metric kernels (csrc/metrics.hip, the set statistics at the end of csrc/local_cd.hip):
float64 where the kernel rounds, exact integers or explicit float32 steps where the kernel's result is fully determined.  No GPU.

Also the seeded inputs that the CPU tests, the GPU tests and tests/golden/make_golden_set_stats.py share: the matrices are
regenerated from spgan.fixture_rng names wherever they are needed, so no golden file has to carry them.
"""
import numpy as np

from spgan import fixture_rng as fr

f32 = np.float32

N0, N1 = 300, 277            # clouds per side of the set-statistic tests: n = 577 = 2 * 256 + 65, three strides, the last ragged
MMD_S, MMD_R = 300, 530      # lgan_mmd_cov matrix: 530 columns = three 256-column blocks, the last ragged


# ---------------------------------------------------------------------------------------------------------------- set statistics
def mmd_cov(d):
    """(lgan_mmd, lgan_cov, lgan_mmd_smp) of a [samples, references] matrix (evaluation_metrics.py:161-173): float64 means of
    the column and the row minima; coverage from the first argmin of every row."""
    d = np.asarray(d, np.float64)
    return float(d.min(0).mean()), len(np.unique(d.argmin(1))) / float(d.shape[1]), float(d.min(1).mean())


def joint_f32(Mxx, Mxy, Myy, sqrt=False):
    """[[Mxx, Mxy], [Mxy^T, Myy]] in float32 with an infinite diagonal; sqrt: sqrt(|v|) rounded to float32, as the kernels and
    the reference (torch float32) take it -- two float32 values may share a float32 root, which a float64 root would separate."""
    Mxx, Mxy, Myy = (np.asarray(x, f32) for x in (Mxx, Mxy, Myy))
    M = np.block([[Mxx, Mxy], [Mxy.T, Myy]]).astype(f32)
    if sqrt:
        M = np.sqrt(np.abs(M)).astype(f32)
    np.fill_diagonal(M, np.inf)
    return M


def neighbour_order(M, k):
    """[k, n]: for every column of M its k nearest rows, ordered by (distance, index)."""
    return np.argsort(M, axis=0, kind="stable")[:k]


KEYS = ("tp", "fp", "fn", "tn", "precision", "recall", "acc_t", "acc_f", "acc")


def two_sample_knn(Mxx, Mxy, Myy, k, sqrt=False):
    """evaluation_metrics.knn (:129-158) with labels 1 (first set) / 0: pred = 2 * votes >= k over the k nearest other clouds.
    -> ({the nine result keys: np.float32}, pred int32 [n0 + n1]).  The ratios are float32 arithmetic on the float32 counts
    with 1e-10f in the denominators, the operations two_sample_final_kernel performs."""
    n0, n1 = np.asarray(Mxx).shape[0], np.asarray(Myy).shape[0]
    idx = neighbour_order(joint_f32(Mxx, Mxy, Myy, sqrt), k)
    votes = (idx < n0).sum(0)
    pred = (2 * votes >= k).astype(np.int32)
    tp, fp = f32(pred[:n0].sum()), f32(pred[n0:].sum())
    fn, tn = f32(n0 - int(tp)), f32(n1 - int(fp))
    e = f32(1e-10)
    out = (tp, fp, fn, tn, tp / ((tp + fp) + e), tp / ((tp + fn) + e), tp / ((tp + fn) + e), tn / ((tn + fp) + e), (tp + tn) / f32(n0 + n1))
    return {name: f32(v) for name, v in zip(KEYS, out)}, pred


# ------------------------------------------------------------------------------------------------------------ seeded matrices
def _quarters(name, shape):
    return (np.floor(fr.uniform(name, shape, 0.0, 5.0).numpy()).clip(0, 4) / 4.0).astype(f32)


def _distinct(name, shapes):
    """float32 arrays of the given shapes that together hold a seeded permutation of {1, ..., T} * 2^-18 (T < 2^18): values in
    (0, 1), all different, 64 float32 steps or more apart."""
    sizes = [int(np.prod(s)) for s in shapes]
    total = sum(sizes)
    assert total < 2 ** 18
    perm = np.argsort(fr.uniform(name, (total,), 0.0, 1.0).numpy(), kind="stable")
    vals = ((perm + 1) * 2.0 ** -18).astype(f32)
    return [vals[lo:lo + n].reshape(s).copy() for lo, n, s in zip(np.cumsum([0] + sizes[:-1]), sizes, shapes)]


SQRT_SHIFT = f32(0.3)        # sqrt=True inputs are the blocks minus this: negative entries, so that sqrt(|v|) is exercised


def set_stat_blocks(family, n0=N0, n1=N1):
    """(Mxx [n0,n0], Mxy [n0,n1], Myy [n1,n1]) float32.
      "free":  a seeded permutation of distinct values in (0, 1); Mxx / Myy asymmetric, as the CD_M / CD_C matrices are;
      "ties":  entries from {0, 1/4, ..., 1}: equal minima and equal k-th neighbours on indices of different threads and strides;
      "dup":   "free" with blocks of exact zeros off the diagonal (memorised references: duplicated clouds)."""
    tag = "setstat.%s.%d.%d." % (family, n0, n1)
    shapes = ((n0, n0), (n0, n1), (n1, n1))
    if family == "ties":
        return tuple(_quarters(tag + s, shp) for s, shp in zip(("xx", "xy", "yy"), shapes))
    xx, xy, yy = _distinct(tag + "all", shapes)
    if family == "dup":
        a, b = min(40, n0), min(40, n1)
        xy[:a, :b] = 0.0                                  # samples 0..39 are copies of references 0..39 (and of each other)
        xx[:a, :a] = 0.0
        yy[:b, :b] = 0.0
        if n0 > 256 and n1 > 270:
            xy[256:n0, 258:270] = 0.0                     # a second block whose rows and columns lie in later strides
    elif family != "free":
        raise ValueError(family)
    return xx, xy, yy


def mmd_matrix(family, S=MMD_S, R=MMD_R):
    """[S,R] float32 for lgan_mmd_cov / COV / MMD, the families of set_stat_blocks.  "ties" also carries planted rows: row 0's
    minimum -1 sits at columns 3, 259 and 515 (one thread, three strides), row 1's at 515 only, row 2's at 255 and 256
    (neighbouring threads 255 and 0), row 3's at R - 1 and 4, rows 4 and 5 have theirs at 256 and at 513 only (the first
    column of the second and the third stride)."""
    tag = "mmd.%s.%d.%d" % (family, S, R)
    if family == "ties":
        d = _quarters(tag, (S, R))
        if R > 515 and S > 3:
            d[0, [3, 259, 515]] = -1.0
            d[1, 515] = -1.0
            d[2, [255, 256]] = -1.0
            d[3, [R - 1, 4]] = -1.0
            d[4, 256] = -1.0
            d[5, 513] = -1.0
        return d
    d, = _distinct(tag, ((S, R),))
    if family == "dup":
        d[10:50, 260:300] = 0.0
    elif family != "free":
        raise ValueError(family)
    return d


def columns_tie_free(M):
    """No column of M holds a finite value twice (so a top-k without a tie rule, the reference's, is well defined on it)."""
    s = np.sort(np.asarray(M), axis=0)
    return bool((s[1:] > s[:-1])[np.isfinite(s[1:])].all())


# ----------------------------------------------------------------------------------------------------------------- Chamfer pairs
def lattice_clouds(name, shape):
    """float32 clouds with coordinates k/16, |k| <= 16: every squared distance is an integer multiple of 1/256 <= 12, exact in
    float32 whatever the evaluation order or contraction."""
    return (np.rint(fr.uniform(name, shape, -16.49, 16.49).numpy()) / 16.0).astype(f32)


def nn_minima(a, b, chunk_bytes=64 << 20):
    """float64 (min_j |a_i - b_j|^2 [N], first argmin [N], min_i [M], first argmin [M]) by brute force, in row chunks of at
    most chunk_bytes."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    N, M = a.shape[0], b.shape[0]
    rows = max(1, chunk_bytes // (8 * M))
    rmin, ridx = np.empty(N), np.empty(N, np.int64)
    cmin, cidx = np.full(M, np.inf), np.zeros(M, np.int64)
    for lo in range(0, N, rows):
        x = a[lo:lo + rows]
        d = (x[:, None, 0] - b[None, :, 0]) ** 2
        d += (x[:, None, 1] - b[None, :, 1]) ** 2
        d += (x[:, None, 2] - b[None, :, 2]) ** 2
        ridx[lo:lo + rows] = d.argmin(1)
        rmin[lo:lo + rows] = d.min(1)
        ci = d.argmin(0)
        cv = d[ci, np.arange(M)]
        better = cv < cmin                                  # strict: an earlier chunk keeps an equal minimum (first occurrence)
        cmin[better], cidx[better] = cv[better], ci[better] + lo
    return rmin, ridx, cmin, cidx


def _pairs(A, B, fn, dtype):
    A, B = np.asarray(A), np.asarray(B)
    out = np.empty((A.shape[0], B.shape[0]), dtype)
    for s in range(A.shape[0]):
        for r in range(B.shape[0]):
            rmin, _, cmin, _ = nn_minima(A[s], B[r])
            out[s, r] = fn(rmin, cmin)
    return out


def pairwise_cd_exact(A, B):
    """[S,R] float32 for lattice clouds: the two sums of minima are exact integers of 1/256 (below 2^24 of them), so the kernel's
    result is fl32(fl32(fl32(sum1) / N) + fl32(fl32(sum2) / M)) whatever its summation order: comparable bit for bit."""
    def fn(rmin, cmin):
        s1, s2 = rmin.sum(), cmin.sum()
        assert s1 * 256 == int(s1 * 256) < 2 ** 24 and s2 * 256 == int(s2 * 256) < 2 ** 24, "not a lattice input"
        return f32(f32(s1) / f32(len(rmin))) + f32(f32(s2) / f32(len(cmin)))
    return _pairs(A, B, fn, f32)


def pairwise_cd_f64(A, B):
    """[S,R] float64: mean_i min_j + mean_j min_i for arbitrary float32 clouds."""
    return _pairs(A, B, lambda rmin, cmin: rmin.mean() + cmin.mean(), np.float64)


# ------------------------------------------------------------------------------------------------------------- occupancy grid
def grid_clouds(name, grid, spacing, S, N, common=5):
    """[S,N,3] float32 clouds of grid-cell centres plus a jitter of at most 0.25 * spacing per axis, and the cell of every point
    [S,N].  Cells 0..common-1 of a fixed shuffle are hit by every cloud, the next S by exactly one cloud each (cloud s: one
    point), the rest are drawn with replacement from the remaining cells, so a cloud hits many cells several times."""
    grid = np.asarray(grid, f32).reshape(-1, 3)
    G = grid.shape[0]
    perm = np.argsort(fr.uniform(name + ".perm", (G,), 0.0, 1.0).numpy(), kind="stable")
    pool = perm[common + S:]
    pick = np.floor(fr.uniform(name + ".pick", (S, N), 0.0, 1.0).numpy().astype(np.float64) * len(pool)).astype(np.int64).clip(0, len(pool) - 1)
    cell = pool[pick]
    cell[:, :common] = perm[:common][None, :]
    cell[:, common] = perm[common:common + S]
    jit = fr.uniform(name + ".jit", (S, N, 3), -0.25, 0.25).numpy() * f32(spacing)
    return (grid[cell] + jit).astype(f32), cell


def nearest_cells(points, grid, axis, dtype):
    """[P] first argmin over the grid cells of ((dx*dx + dy*dy) + dz*dz) with every operation rounded to `dtype` (float32: the
    kernel's arithmetic without contraction; float64: the oracle's).  The grid's coordinates are values of `axis` (ascending), so
    the distances are assembled from per-axis tables of (p - axis value)^2: the same operations as the direct form."""
    p, g = np.asarray(points, dtype).reshape(-1, 3), np.asarray(grid, dtype).reshape(-1, 3)
    ax, res = np.asarray(axis, dtype), len(axis)
    ci, cj, ck = (np.searchsorted(ax, g[:, c]) for c in range(3))
    assert np.array_equal(ax[ci], g[:, 0]) and np.array_equal(ax[cj], g[:, 1]) and np.array_equal(ax[ck], g[:, 2])
    cij, full = ci * res + cj, len(g) == res ** 3
    out = np.empty(len(p), np.int64)
    for lo in range(0, len(p), 512):
        t = (p[lo:lo + 512, None, :] - ax[None, :, None]) ** 2
        sxy = (t[:, :, None, 0] + t[:, None, :, 1]).reshape(t.shape[0], -1)
        d = (sxy[:, :, None] + t[:, None, :, 2]).reshape(t.shape[0], -1) if full else sxy[:, cij] + t[:, ck, 2]
        assert d.dtype == dtype
        out[lo:lo + 512] = d.argmin(1)
    return out


OCCUPANCY_CASES = ((16, True), (28, True), (32, False))      # (resolution, in_sphere); S = 70 clouds of N = 300 each
OCC_S, OCC_N = 70, 300


# ------------------------------------------------------------------------------------- Chamfer index rule, backward, auction
def chamfer_tie_clouds(B=2, N=300, M=1100):
    """Lattice clouds a [B,N,3], b [B,M,3] with planted exact ties: b[7] = b[512 + 7] is a corner point that nothing precedes,
    and a[0..5] sit on and next to it (their equal nearest candidates lie in the first two 512-candidate chunks); b[100] =
    b[1030] (chunks 0 and 2) with a[20] on it; a[7] = a[263].  The random lattice points tie in many more places."""
    a, b = lattice_clouds("cdtie.a", (B, N, 3)), lattice_clouds("cdtie.b", (B, M, 3))
    corner = np.array([17, 17, 17], f32) / 16
    b[:, 7] = corner
    b[:, 512 + 7] = corner
    off = np.array([[0, 0, 0], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [-1, -1, 0], [-2, 0, -1]], f32) / 16
    a[:, :6] = corner + off
    b[:, 1030] = b[:, 100]
    a[:, 20] = b[:, 100]
    a[:, 263] = a[:, 7]
    return a, b


def many_to_one_clouds(B=2, Na=300, Nb=1100):
    """a [B,Na,3], b [B,Nb,3] float32: every point of b lies within 0.6 of a[0] and at least 1.4 from every other point of a
    (those lie on shells of radius 2 to 3), so all Nb = 1100 points (three chunks of the backward gather) choose a[0]."""
    a = fr.normal("m2o.a", (B, Na, 3)).numpy().astype(np.float64)
    a *= (fr.uniform("m2o.r", (B, Na, 1), 2.0, 3.0).numpy() / np.linalg.norm(a, axis=-1, keepdims=True))
    a[:, 0] = (0.1, -0.05, 0.2)
    b = a[:, :1] + np.array([0.15, 0.1, -0.1]) + fr.uniform("m2o.b", (B, Nb, 3), -0.2, 0.2).numpy()
    return a.astype(f32), b.astype(f32)


def emd_sets(B, n):
    """The auction inputs of tests/test_oracle_golden.py::_emd_sets at any size (clouds in the unit cube)."""
    a = np.stack([(fr.synthetic_real(1, n, seed=800 + i)[0].numpy() * 0.5 + 0.5) for i in range(B)]).astype(f32)
    b = np.stack([(fr.synthetic_real(1, n, seed=900 + i)[0].numpy() * 0.45 + 0.5) for i in range(B)]).astype(f32)
    return a, b


def emd_lattice_pair(B=2, n=1100):
    """Both clouds on the 5 x 5 x 5 lattice {0, 1/4, ..., 1}^3: about nine copies of every object, spread over the 64 lanes and
    both 1024-object tiles, tie exactly in value for every bidder."""
    def lat(name):
        return (np.floor(fr.uniform(name, (B, n, 3), 0.0, 5.0).numpy()).clip(0, 4) / 4.0).astype(f32)
    return lat("emdlat.a"), lat("emdlat.b")
