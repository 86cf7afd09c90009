"""Numpy model of spgan.model_utils' point-distribution losses (csrc/point_losses.hip).

Group membership and the selection run in float32 in the kernel's operation order -- dx = p_i - p_j, d2 = (dx*dx + dy*dy) + dz*dz,
l1 = (|dx| + |dy|) + |dz|, every operation rounded on its own; keys (float bits of the slot value, slot), the `root` metric keyed on d2 --
so the selected indices are the kernel's bit for bit.  The selected values, the tails, the losses and dpred are then computed in
float64 from the selected indices.
"""
import math

import numpy as np

F = np.float32
U = 1.0 / 64.0
KEEP = 5


# ---------------------------------------------------------------------------------------------------------------- float32: which slots
def _diffs32(cloud):
    c = np.asarray(cloud, dtype=F)
    d = c[:, None, :] - c[None, :, :]                      # query i - candidate j, float32
    return d[..., 0], d[..., 1], d[..., 2]


def group_slots(cloud, nsample, radius=None):
    """cloud [N,3] -> j int64 [N,nsample]: the point in every slot.  radius None: the nsample nearest by (d2, index); else the first
    nsample indices with d2 < radius*radius (a float32 product, strict), further slots repeat the first hit, an empty ball holds point 0."""
    dx, dy, dz = _diffs32(cloud)
    d2 = (dx * dx + dy * dy) + dz * dz
    N = d2.shape[0]
    if radius is None:
        assert N >= nsample
        return np.argsort(d2, axis=1, kind="stable")[:, :nsample].astype(np.int64)
    r2 = F(radius) * F(radius)
    j = np.zeros((N, nsample), dtype=np.int64)
    for i in range(N):
        hits = np.flatnonzero(d2[i] < r2)[:nsample]
        if hits.size:
            j[i, :hits.size] = hits
            j[i, hits.size:] = hits[0]
    return j


def select(cloud, nsample, radius=None, metric="sq", keep=KEEP):
    """-> (idx int64 [N,keep], val float32 [N,keep], slot int64 [N,keep]): the keep smallest slots by (value bits, slot), ascending."""
    j = group_slots(cloud, nsample, radius)
    dx, dy, dz = _diffs32(cloud)
    rows = np.arange(j.shape[0])[:, None]
    gx, gy, gz = dx[rows, j], dy[rows, j], dz[rows, j]
    if metric == "l1":
        m = (np.abs(gx) + np.abs(gy)) + np.abs(gz)
    else:
        m = (gx * gx + gy * gy) + gz * gz
    assert m.dtype == F
    key = (m.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(nsample, dtype=np.uint64)[None, :]
    slot = np.argsort(key, axis=1, kind="stable")[:, :keep]
    mv = m[rows, slot]
    val = np.sqrt(mv + F(1e-12)).astype(F) if metric == "root" else mv
    assert val.dtype == F
    return j[rows, slot], val, slot.astype(np.int64)


def select_batch(clouds, nsample, radius=None, metric="sq", keep=KEEP):
    out = [select(c, nsample, radius, metric, keep) for c in clouds]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ---------------------------------------------------------------------------------------------------------------- float64: what they are worth
def values64(clouds, idx, metric):
    """clouds [B,N,3], idx [B,N,keep] -> (v float64 [B,N,keep], d float64 [B,N,keep,3] = p_i - p_idx)."""
    c = np.asarray(clouds, dtype=np.float64)
    B = c.shape[0]
    nb = c[np.arange(B)[:, None, None], idx]
    d = c[:, :, None, :] - nb
    if metric == "l1":
        v = np.abs(d).sum(-1)
    else:
        v = (d * d).sum(-1)
        if metric == "root":
            v = np.sqrt(v + 1e-12)
    return v, d


def _g(d, metric):
    if metric == "sq":
        return 2.0 * d
    if metric == "l1":
        return np.sign(d)
    return d / np.sqrt((d * d).sum(-1, keepdims=True) + 1e-12)


def scatter_grad(clouds, idx, cval, metric):
    """dL/dval = cval [B,N,keep] -> (dpred float64 [B,N,3], the per-element sum of the contributions' magnitudes)."""
    _, d = values64(clouds, idx, metric)
    contrib = cval[..., None] * _g(d, metric)               # to the query; the selected point takes the negative
    dp = contrib.sum(2)
    ab = np.abs(contrib).sum(2)
    B = idx.shape[0]
    bi = np.broadcast_to(np.arange(B)[:, None, None], idx.shape)
    np.add.at(dp, (bi, idx), -contrib)
    np.add.at(ab, (bi, idx), np.abs(contrib))
    return dp, ab


def tail_hinge(v, h):
    t = h - v
    return np.maximum(t, 0.0), np.where(t > 0.0, -1.0, 0.0)


def tail_rep4(v, radius, h=0.03):
    w = np.maximum(v, 1e-12)
    s, e = np.sqrt(w), np.exp(-w / h ** 2)
    return radius - s * e, np.where(v > 1e-12, s * e / h ** 2 - e / (2.0 * s), 0.0)


def _loss(clouds, idx, metric, tail):
    """mean of the tail over the winners 1.. -> dict(loss, dpred, scale, active)."""
    v, _ = values64(clouds, idx, metric)
    term, dterm = tail(v[..., 1:])
    count = term.size
    cval = np.zeros_like(v)
    cval[..., 1:] = dterm / count
    dp, ab = scatter_grad(clouds, idx, cval, metric)
    return {"loss": float(term.sum() / count), "dpred": dp, "scale": float(ab.max()), "active": float((dterm != 0).mean()), "idx": idx}


def repulsion_loss(clouds, nsample=20, radius=0.07, knn=False, use_l1=False, h=0.001):
    metric = "l1" if use_l1 else "sq"
    idx, _ = select_batch(clouds, nsample, None if knn else radius, metric)
    h_eff = math.sqrt(h) * 2 if use_l1 else h
    out = _loss(clouds, idx, metric, lambda v: tail_hinge(v, h_eff))
    out["metric"] = metric
    return out


def repulsion_loss4(clouds, nsample=20, radius=0.07):
    idx, _ = select_batch(clouds, nsample, radius, "sq")
    out = _loss(clouds, idx, "sq", lambda v: tail_rep4(v, radius))
    out["metric"] = "sq"
    return out


def perulsion_loss(clouds, nsample=15, radius=0.07, knn=False, use_l1=False):
    metric = "root" if use_l1 else "sq"
    idx, _ = select_batch(clouds, nsample, None if knn else radius, metric)
    h_eff = math.sqrt(0.001) * 2 if use_l1 else 0.01
    out = _loss(clouds, idx, metric, lambda v: tail_hinge(v, h_eff))
    out["metric"] = metric
    return out


def uniform_loss_knn(clouds):
    idx, _ = select_batch(clouds, 6, None, "sq", keep=6)
    v, _ = values64(clouds, idx, "sq")
    B, N, K = v.shape
    m = v.mean(2)
    loss = m.var(1).sum() + v.var(2).sum()
    cval = (2.0 * (m - m.mean(1, keepdims=True)) / N)[..., None] / K + 2.0 * (v - m[..., None]) / K
    dp, ab = scatter_grad(clouds, idx, cval, "sq")
    return {"loss": float(loss), "dpred": dp, "scale": float(ab.max()), "active": 1.0, "idx": idx, "metric": "sq"}


# ---------------------------------------------------------------------------------------------------------------- Chamfer / Hausdorff
def cd_loss(df, db, radius):
    """df [B,Ngt] (gt -> pred), db [B,Npred], float64."""
    return float(((0.8 * df.mean(1) + 0.2 * db.mean(1)) / radius).mean())


def cd_loss2(df, db, forward_weight=1.0, threshold=100):
    if threshold is not None:
        df = np.where(df < df.mean(1, keepdims=True) * threshold, df, 0.0)
        db = np.where(db < db.mean(1, keepdims=True) * threshold, db, 0.0)
    return float((forward_weight * df.mean(1) + db.mean(1)).mean())


def hausdorff_loss(df, db, radius, forward_weight=1.0, threshold=None):
    if threshold is not None:
        df = np.where(df < threshold, df, 0.0)
        db = np.where(db < threshold, db, 0.0)
    return float(((forward_weight * df.max(1) + db.max(1)) / radius).max())


def nn_dists64(gt, pred):
    g, p = np.asarray(gt, np.float64), np.asarray(pred, np.float64)
    d = ((g[:, :, None, :] - p[:, None, :, :]) ** 2).sum(-1)
    return d.min(2), d.min(1)


# ---------------------------------------------------------------------------------------------------------------- clouds
def exact_clouds(B, N, seed):
    """Coordinates are multiples of 2^-6 in [0,1): every d2, l1 and r*r (r = 0.25, 0.5) is exact in float32."""
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 64, size=(B, N, 3)).astype(F) * F(U)).astype(F)


def constructed_clouds():
    """[3,22,3], radius 0.25, coordinates multiples of 2^-6; one hazard per group of points (66 queries: no multiple of the four
    queries of a workgroup, so the last query of the last cloud sits in a partly filled one).

    cloud 0:  0        a hub whose ball holds 13 points: 1..8 at distance 13/64 come first in index order, 9..12 at distance 2/64 are the
                       nearest and fall to the index-order truncation at nsample 5 and 8
              13       a point whose ball holds only itself (all values 0, gradient exactly 0)
              14, 15   a ball with 2 hits;  16..19  a ball with 4 hits (padding duplicates enter the five)
              15, 17.. queries whose first hit has a lower index than they have
              20, 21   two points at exactly distance radius (excluded: each is alone)
    cloud 1:  5        a centre with 0, 1, 6 at one distance (25 units), 2, 3, 4 nearer, 7, 8 farther: at nsample 8 the tie sits at the fifth /
                       sixth / seventh position, at kNN 6 at the sixth / seventh
              9..21    a line with spacing 4/64: left and right neighbours tie everywhere, balls overflow nsample 5
    cloud 2:           a dense lattice scatter: every ball overflows, ties abound; holds the last query."""
    c = np.zeros((3, 22, 3), dtype=np.float64)
    hub = np.array([32, 32, 32])
    ring = [(13, 0, 0), (-13, 0, 0), (0, 13, 0), (0, -13, 0), (0, 0, 13), (0, 0, -13), (12, 5, 0), (-12, -5, 0)]
    near = [(2, 0, 0), (0, 2, 0), (0, 0, 2), (-2, 0, 0)]
    c[0, 0] = hub
    for k, o in enumerate(ring):
        c[0, 1 + k] = hub + o
    for k, o in enumerate(near):
        c[0, 9 + k] = hub + o
    c[0, 13] = (1, 1, 1)
    c[0, 14], c[0, 15] = (58, 6, 6), (58, 8, 6)
    c[0, 16], c[0, 17], c[0, 18], c[0, 19] = (6, 58, 6), (7, 58, 6), (6, 60, 6), (6, 58, 9)
    c[0, 20], c[0, 21] = (6, 6, 58), (22, 6, 58)
    ctr = np.array([32, 32, 32])
    offs = [(5, 0, 0), (0, 5, 0), (2, 0, 0), (0, 3, 0), (0, 0, 4), (0, 0, 0), (0, 0, -5), (-6, 0, 0), (0, -6, 0)]
    for k, o in enumerate(offs):
        c[1, k] = ctr + o
    for k in range(13):
        c[1, 9 + k] = (4 * k, 0, 0)
    for k in range(22):
        c[2, k] = (20 + k % 11, 20 + (5 * k + 3) % 16, 20 + (11 * k + 1) % 16)
    assert len({tuple(p) for p in c[2]}) == 22
    return (c * U).astype(F), 0.25


def random_clouds(B, N, seed, density=200 / 0.12 ** 3):
    """float32 points uniform in a cube whose side keeps `density` points per unit volume: about 13 points per ball of radius 0.03."""
    rng = np.random.RandomState(seed)
    side = (N / density) ** (1.0 / 3.0)
    return (rng.rand(B, N, 3) * side).astype(F)
