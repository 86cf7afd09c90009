"""A numpy model of the pointops family (spgan.pointops, csrc/pointops.hip), written from the stated semantics:
float32 distances in the stated rounding order d2 = (dx*dx + dy*dy) + dz*dz with dx = query - candidate, a stable argsort on (d2, index)
for the neighbour orders, plain integer sums for the label statistics, and torch float64 autograd for the grouping gradients."""
import numpy as np
import torch

F = np.float32


def dist2(query, cloud):
    """query [B,m,3], cloud [B,n,3] float32 -> [B,m,n] float32, every operation rounded on its own."""
    q = np.asarray(query, dtype=F)[:, :, None, :]
    c = np.asarray(cloud, dtype=F)[:, None, :, :]
    d = (q - c).astype(F)
    sq = (d * d).astype(F)
    return ((sq[..., 0] + sq[..., 1]).astype(F) + sq[..., 2]).astype(F)


def knnquery(nsample, xyz, new_xyz=None):
    """-> (idx int32 [B,m,nsample], dist2 float32): ascending d2, the lower index first on equal d2; slots past n: index 0, +inf."""
    new_xyz = xyz if new_xyz is None else new_xyz
    d = dist2(new_xyz, xyz)
    B, m, n = d.shape
    order = np.argsort(d, axis=2, kind="stable")          # stable: equal d2 keep ascending index
    k = min(nsample, n)
    idx = np.zeros((B, m, nsample), dtype=np.int32)
    out = np.full((B, m, nsample), np.inf, dtype=F)
    idx[:, :, :k] = order[:, :, :k]
    out[:, :, :k] = np.take_along_axis(d, order[:, :, :k], axis=2)
    return idx, out


def nearestneighbor(unknown, known):
    idx, d2 = knnquery(3, known, unknown)
    return np.sqrt(d2).astype(F), idx


def _ball_hits(radius, xyz, new_xyz):
    r2 = F(F(radius) * F(radius))
    return dist2(new_xyz, xyz) < r2                         # strict


def ballquery(radius, nsample, xyz, new_xyz):
    hits = _ball_hits(radius, xyz, new_xyz)
    B, m, n = hits.shape
    idx = np.zeros((B, m, nsample), dtype=np.int32)
    for b in range(B):
        for j in range(m):
            h = np.flatnonzero(hits[b, j])[:nsample]
            if h.size:
                idx[b, j, :] = h[0]
                idx[b, j, :h.size] = h
    return idx


def labelstat_ballrange(radius, xyz, new_xyz, label_stat):
    hits = _ball_hits(radius, xyz, new_xyz)
    return np.einsum("bjk,bkc->bjc", hits.astype(np.int64), np.asarray(label_stat, dtype=np.int64)).astype(np.int32)


def labelstat_and_ballquery(radius, nsample, xyz, new_xyz, label_stat):
    hits = _ball_hits(radius, xyz, new_xyz)
    first = np.cumsum(hits, axis=2) <= nsample             # the scan ends at nsample hits
    kept = hits & first
    stat = np.einsum("bjk,bkc->bjc", kept.astype(np.int64), np.asarray(label_stat, dtype=np.int64)).astype(np.int32)
    return stat, ballquery(radius, nsample, xyz, new_xyz)


def labelstat_idx(label_stat, idx):
    B = idx.shape[0]
    ls = np.asarray(label_stat, dtype=np.int64)
    return np.stack([ls[b][idx[b]].sum(axis=1) for b in range(B)]).astype(np.int32)


def featuredistribute(max_xyz, xyz):
    d = dist2(xyz, max_xyz)
    best = np.argmin(d, axis=2)                             # the first minimum: the lowest index among equals
    near = np.take_along_axis(d, best[..., None], axis=2)[..., 0] < F(100000.0)
    return np.where(near, best, -1).astype(np.int32)


def grouping(features, idx):
    """torch: features [B,C,n], idx [B,m,K] (any integer dtype) -> [B,C,m,K] by torch.gather."""
    B, C, n = features.shape
    _, m, K = idx.shape
    flat = idx.reshape(B, 1, m * K).long().expand(B, C, m * K)
    return torch.gather(features, 2, flat).reshape(B, C, m, K)


def query_and_group(xyz, new_xyz, features, idx, use_xyz=True, subtract=True):
    """The reference's composition in plain torch: transpose, gather, in-place subtraction, concatenation."""
    grouped_xyz = grouping(xyz.transpose(1, 2).contiguous(), idx)
    if subtract:
        grouped_xyz = grouped_xyz - new_xyz.transpose(1, 2).unsqueeze(-1)
    if features is None:
        return grouped_xyz
    grouped = grouping(features, idx)
    return torch.cat([grouped_xyz, grouped], dim=1) if use_xyz else grouped


def interpolation(features, idx, weight):
    """features [B,C,m], idx / weight [B,n,3] -> [B,C,n] = (w0*f0 + w1*f1) + w2*f2 in the tensors' dtype."""
    B, C, m = features.shape
    n = idx.shape[1]
    f = torch.gather(features, 2, idx.reshape(B, 1, n * 3).long().expand(B, C, n * 3)).reshape(B, C, n, 3)
    t = f * weight.unsqueeze(1)
    return (t[..., 0] + t[..., 1]) + t[..., 2]


def lattice_cloud(rng, B, n, side=4):
    """Integer lattice coordinates in [0, side) times 2^-4: every distance is exact in float32 and ties abound.  Different per b."""
    return (rng.integers(0, side, size=(B, n, 3)).astype(F) * F(2.0 ** -4)).astype(F)
