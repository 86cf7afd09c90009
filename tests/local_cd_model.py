"""CPU model of the local-shape Chamfer and the GAN_metrics pieces (csrc/local_cd.hip, spgan/local_cd.py, spgan/gan_metrics.py).

Neighbour indices come from float32 squared distances evaluated in the kernels' order, ((dx*dx + dy*dy) + dz*dz) with each
operation rounded to float32 (numpy's float32 arithmetic), then a stable sort: ascending distance, the lower index first on ties.
So they equal the kernels' indices exactly.  Everything after the indices is float64.
"""
import numpy as np
import torch


def d2_f32(query: np.ndarray, cloud: np.ndarray) -> np.ndarray:
    """[B,M,3] x [B,N,3] float32 -> [B,M,N] float32 in the fixed rounding order."""
    q = np.asarray(query, np.float32)[:, :, None, :]
    c = np.asarray(cloud, np.float32)[:, None, :, :]
    dx, dy, dz = q[..., 0] - c[..., 0], q[..., 1] - c[..., 1], q[..., 2] - c[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def knn_idx(query, cloud, k: int) -> np.ndarray:
    """int64 [B,M,k]: pointops knnquery order."""
    return np.argsort(d2_f32(query, cloud), axis=-1, kind="stable")[..., :k].astype(np.int64)


def moments(cloud: torch.Tensor, idx) -> tuple:
    """float64 (mu [B,M,3], cov6 [B,M,6]) of cloud[b, idx[b,m,:]] (differentiable in cloud)."""
    idx = torch.as_tensor(np.asarray(idx), dtype=torch.int64)
    B, M, K = idx.shape
    g = cloud[torch.arange(B)[:, None, None], idx]                 # [B,M,K,3]
    mu = g.mean(dim=2)
    t = g - mu[:, :, None, :]
    c = torch.einsum("bmka,bmkc->bmac", t, t) / K
    cov6 = torch.stack([c[..., 0, 0], c[..., 0, 1], c[..., 0, 2], c[..., 1, 1], c[..., 1, 2], c[..., 2, 2]], dim=-1)
    return mu, cov6


def full9(cov6: torch.Tensor) -> torch.Tensor:
    xx, xy, xz, yy, yz, zz = cov6.unbind(-1)
    return torch.stack([xx, xy, xz, xy, yy, yz, xz, yz, zz], dim=-1)


def chamfer(a: torch.Tensor, b: torch.Tensor, ia=None, ib=None):
    """sum_i min_j |a_i - b_j|^2 + sum_j min_i (over the batch), float64; with ia / ib given, those argmins are used (the
    gradient then routes exactly as the kernels route it).  -> (value, ia, ib)."""
    d = ((a[:, :, None, :] - b[:, None, :, :]) ** 2).sum(-1)
    if ia is None:
        ia = d.detach().argmin(dim=2)
        ib = d.detach().argmin(dim=1)
    ia, ib = torch.as_tensor(ia, dtype=torch.int64), torch.as_tensor(ib, dtype=torch.int64)
    va = torch.gather(d, 2, ia[:, :, None]).squeeze(2)
    vb = torch.gather(d, 1, ib[:, None, :]).squeeze(1)
    return va.sum() + vb.sum(), ia, ib


def local_pair(q: torch.Tensor, c2: torch.Tensor, k: int, idx1=None, idx2=None, args=None):
    """(mean term, covariance term) of local_CD / get_local_pair for query cloud q [B,M,3] and second cloud c2, float64.
    idx1 / idx2: the neighbour indices (default: knn_idx of the float32 values); args: the Chamfer argmins (ia, ib) x 2."""
    qn, cn = q.detach().float().numpy(), c2.detach().float().numpy()
    idx1 = knn_idx(qn, qn, k) if idx1 is None else idx1
    idx2 = knn_idx(qn, cn, k) if idx2 is None else idx2
    mu1, cv1 = moments(q, idx1)
    mu2, cv2 = moments(c2, idx2)
    a = args or (None, None, None, None)
    n = float(q.shape[1])
    lm, _, _ = chamfer(mu1, mu2, a[0], a[1])
    lc, _, _ = chamfer(full9(cv1), full9(cv2), a[2], a[3])
    return lm / n, lc / n


def pairwise_local(sample: np.ndarray, ref: np.ndarray, k: int = 8) -> np.ndarray:
    """[S,R,2] float64 per-pair matrix."""
    S, R = sample.shape[0], ref.shape[0]
    out = np.zeros((S, R, 2))
    for s in range(S):
        for r in range(R):
            m, c = local_pair(torch.from_numpy(sample[s:s + 1]).double(), torch.from_numpy(ref[r:r + 1]).double(), k)
            out[s, r] = (m.item(), c.item())
    return out


def chunk_sums(mat: np.ndarray, batch_size: int) -> np.ndarray:
    """The reference pairwise_local_CD's [S, ceil(R/batch_size)] chunk sums of an [S,R] matrix."""
    return np.stack([mat[:, lo:lo + batch_size].sum(1) for lo in range(0, mat.shape[1], batch_size)], axis=1)


def knn_pm(Mxx, Mxy, Myy, k: int, sqrt: bool = False, return_pred: bool = False):
    """GAN_metrics.KNN: labels -1 / +1, k nearest other clouds by (distance, index), a vote >= 0 predicts +1.  The matrices are
    float32, and with `sqrt` so are the roots (as in the reference and the kernel: two float32 values may share a float32 root).
    -> the accuracy; with return_pred also the +-1 predictions (int32 [n0 + n1])."""
    Mxx, Mxy, Myy = (np.asarray(x, np.float32) for x in (Mxx, Mxy, Myy))
    n0, n1 = Mxx.shape[0], Myy.shape[0]
    M = np.block([[Mxx, Mxy], [Mxy.T, Myy]])
    if sqrt:
        M = np.sqrt(np.abs(M)).astype(np.float32)
    M = M.astype(np.float64) + np.diag(np.full(n0 + n1, np.inf))
    label = np.concatenate([-np.ones(n0), np.ones(n1)])
    idx = np.argsort(M, axis=0, kind="stable")[:k]
    pred = np.where(label[idx].sum(0) >= 0, 1.0, -1.0)
    acc = float((pred == label).mean())
    return (acc, pred.astype(np.int32)) if return_pred else acc


def voxel_counts(clouds, res: int = 28) -> np.ndarray:
    """int64 [res,res,res]: half-open float64 bins -0.5 + arange(res+1) * (1/res), points outside not counted."""
    p = np.asarray(clouds, np.float32).reshape(-1, 3)
    e = -0.5 + np.arange(res + 1) * (1.0 / res)
    ijk = []
    for c in range(3):
        x = p[:, c].astype(np.float64)[None, :]
        inb = (e[:res, None] <= x) & (x < e[1:, None])
        ijk.append(np.where(inb.any(0), inb.argmax(0), -1))
    ok = (ijk[0] >= 0) & (ijk[1] >= 0) & (ijk[2] >= 0)
    out = np.zeros((res, res, res), np.int64)
    np.add.at(out, (ijk[0][ok], ijk[1][ok], ijk[2][ok]), 1)
    return out


def _entropy2(p: np.ndarray) -> float:
    p = p / p.sum()
    nz = p[p > 0]
    return float(-(nz * np.log(nz)).sum() / np.log(2.0))


def jsd(c1, c2) -> float:
    d1 = voxel_counts(c1).astype(np.float64).ravel()
    d2 = voxel_counts(c2).astype(np.float64).ravel()
    d1, d2 = d1 / d1.sum(), d2 / d2.sum()
    return _entropy2((d1 + d2) / 2.0) - 0.5 * (_entropy2(d1) + _entropy2(d2))


def cov_mmd(d: np.ndarray, axis: int = 1):
    """(COV, MMD) of GAN_metrics.py:458-463 (first index on ties)."""
    d = np.asarray(d, np.float64)
    cov = len(np.unique(d.argmin(axis))) / float(d.shape[axis])
    mmd = float(d.min((axis + 1) % 2).mean())
    return cov, mmd
