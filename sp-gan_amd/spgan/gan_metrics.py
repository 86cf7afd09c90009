"""The evaluation drivers of Common/GAN_metrics.py, with its names (which do not clash with spgan.metrics.compute_all_metrics, the
port of metrics/evaluation_metrics.py).

  pairwise_dists, pairwise_simple,      GAN_metrics.py:548-593: the [S,R] distance matrices ("CD", "CD_M", "CD_C", "EMD", "l2";
  pairwise_local_CD                     "l1" through pairwise_simple), and :628-656 with its chunk-sum quirk (below)
  COV, MMD, KNN, JSD,                   GAN_metrics.py:411-482: coverage, minimum matching distance, the +-1-label k-NN accuracy,
  get_voxel_occ_dist                    and the JSD of 28^3 point-count histograms over [-0.5, 0.5)
  compute_all_metrics,                  GAN_metrics.py:762-832 (the reference's result keys)
  compute_all_metrics_train

Differences from the module in the metrics family (spgan.metrics): KNN votes with labels -1 / +1 and a tied vote predicts the
second set (the reference clouds), which changes 6NN; MMD_t is its own entry; JSD compares point counts in a 28^3 cube, not
per-cloud occupancy of grid cells in the sphere.

The chunk-sum quirk.  The reference's pairwise_local_CD calls local_CD on a sample expanded against `batch_size` reference clouds
at once, and local_CD sums over that batch, so it returns [S, ceil(R / batch_size)] chunk sums, not an [S,R] matrix (batch_size = 1
gives the matrix).  pairwise_local_CD here reproduces that; pairwise_dists, and with it both drivers, use the per-pair matrix.

FPD (spgan.fpd: float64 MFMA kernels) is opt-in.  The pretrained feature network `evaluation.pointnet` is not part of the reference
tree and is not provided, so by default compute_all_metrics on 2-D inputs and compute_all_metrics_train(use_FPD_JSD=True) raise
NotImplementedError as before.  compute_all_metrics(..., fpd=True) on 2-D feature rows runs the reference's branch (l2 distances over
the features, FPD filled in); compute_all_metrics_train(..., model=<module>, use_FPD_JSD=True) takes the caller's network, computes its
activations, JSD and FPD (the reference computes the activations and leaves its FPD line commented out, so its FPD stays 0).
"EMD" dispatches to spgan.metrics.pairwise_emd, not the reference's emd_approx of this module (300 iterations, mean of the squared
distances over a whole chunk): with emd="auction" (the default) the tree's auction, mean over the points of sqrt(dist); with
emd="match_cost" the approxmatch EMD of StructuralLosses.match_cost (spgan.approxmatch), divided by the point count.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from . import _lib
from .fpd import FPD, extract_acts_with_model
from .local_cd import pairwise_local_cd
from .metrics import _entropy, _matrix, lgan_mmd_cov, pairwise_cd, pairwise_emd
from .ops import _f32, _p, _s, check

Tensor = torch.Tensor

_NO_POINTNET = ("FPD needs PointNet activations from `evaluation.pointnet` (PointNetCls), which the reference tree does not "
                "contain; it is not available here (pass fpd=True with feature rows, or model=<your network> with use_FPD_JSD=True)")


def _dev(x) -> Tensor:
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    return x


def pairwise_simple(sample_pcs: Tensor, ref_pcs: Tensor, batch_size: int = 16, dist_type: str = "l2") -> Tensor:
    """GAN_metrics.py:562-593: feature rows sample [S,D], ref [R,D] -> [S,R] of sum (s - r)^2 ("l2") or sum |s - r| ("l1").
    batch_size only chunks the reference's loop and does not change the result."""
    if dist_type not in ("l2", "l1"):
        raise ValueError("dist_type must be 'l2' or 'l1', got %r" % (dist_type,))
    a, b = _matrix(_dev(sample_pcs), "sample_pcs"), _matrix(_dev(ref_pcs), "ref_pcs")
    if a.shape[1] != b.shape[1]:
        raise ValueError("feature sizes differ: %d and %d" % (a.shape[1], b.shape[1]))
    S, D = a.shape
    R = b.shape[0]
    out = torch.empty((S, R), dtype=torch.float32, device=a.device)
    check(_lib.load().spgan_pairwise_simple(_p(a), _p(b), S, R, D, 1 if dist_type == "l1" else 0, _p(out), _s()), "pairwise_simple",
          S=S, R=R, D=D)
    return out


def _local_term(dist_type: str) -> int:
    if dist_type not in ("CD_M", "CD_C"):
        raise ValueError("dist_type must be 'CD_M' or 'CD_C', got %r" % (dist_type,))
    return 0 if dist_type == "CD_M" else 1


def pairwise_local_CD(sample_pcs: Tensor, ref_pcs: Tensor, batch_size: int, dist_type: str) -> Tensor:
    """GAN_metrics.py:628-656 as written: [S, ceil(R / batch_size)], entry (s, c) = the sum over the references of chunk c of
    local_CD(sample[s], ref[r]) ("CD_M": the mean term, "CD_C": the covariance term).  batch_size = 1 gives the [S,R] matrix."""
    term = _local_term(dist_type)
    m = pairwise_local_cd(_dev(sample_pcs), _dev(ref_pcs))[..., term]
    R = m.shape[1]
    return torch.stack([m[:, lo:lo + batch_size].sum(dim=1) for lo in range(0, R, batch_size)], dim=1)


def pairwise_dists(sample_pcs: Tensor, ref_pcs: Tensor, batch_size: int, dist_type: str = "l2", emd: str = "auction") -> Tensor:
    """GAN_metrics.py:548-559: the [S,R] matrix for "CD" (mean_i min_j + mean_j min_i), "CD_M" / "CD_C" (the local terms, per pair;
    see the module note), "EMD" (spgan.metrics.pairwise_emd with its `emd` route) and anything else as "l2" on feature rows."""
    sample_pcs, ref_pcs = _dev(sample_pcs), _dev(ref_pcs)
    if dist_type == "CD":
        return pairwise_cd(sample_pcs, ref_pcs)
    if dist_type in ("CD_M", "CD_C"):
        return pairwise_local_cd(sample_pcs, ref_pcs)[..., _local_term(dist_type)].contiguous()
    if dist_type == "EMD":
        return pairwise_emd(sample_pcs, ref_pcs, batch_size, emd=emd)
    return pairwise_simple(sample_pcs, ref_pcs, batch_size, "l2")


def _oriented(dists: Tensor, axis: int) -> Tensor:
    if axis not in (0, 1):
        raise ValueError("axis must be 0 or 1, got %r" % (axis,))
    d = _matrix(_dev(dists), "dists")
    return d if axis == 1 else d.t().contiguous()


def COV(dists: Tensor, axis: int = 1) -> float:
    """GAN_metrics.py:458-459: the fraction of the entries along `axis` that are the nearest of some entry of the other axis (the
    first one on ties)."""
    return float(lgan_mmd_cov(_oriented(dists, axis))["lgan_cov"])


def MMD(dists: Tensor, axis: int = 1) -> float:
    """GAN_metrics.py:462-463: the mean, over the entries along `axis`, of their smallest distance to the other axis."""
    return float(lgan_mmd_cov(_oriented(dists, axis))["lgan_mmd"])


def KNN(Mxx: Tensor, Mxy: Tensor, Myy: Tensor, k: int, sqrt: bool = False) -> float:
    """GAN_metrics.py:466-481: leave-one-out k-NN accuracy on the joint matrix [[Mxx, Mxy], [Mxy^T, Myy]]; the k nearest other
    clouds vote with labels -1 (first set) and +1 (second set), a vote >= 0 predicts +1.  Distance ties: the lower index first."""
    xx, xy, yy = _matrix(_dev(Mxx), "Mxx"), _matrix(_dev(Mxy), "Mxy"), _matrix(_dev(Myy), "Myy")
    n0, n1 = xx.shape[0], yy.shape[0]
    if xx.shape != (n0, n0) or yy.shape != (n1, n1) or xy.shape != (n0, n1):
        raise ValueError("expected Mxx [n0,n0], Mxy [n0,n1], Myy [n1,n1]; got %s %s %s" % (tuple(xx.shape), tuple(xy.shape), tuple(yy.shape)))
    if not 0 < int(k) < n0 + n1:
        raise ValueError("k must lie in [1, n0 + n1), got %d" % k)
    out = torch.empty((1,), dtype=torch.float32, device=xx.device)
    pred = torch.empty((n0 + n1,), dtype=torch.int32, device=xx.device)
    check(_lib.load().spgan_two_sample_knn_pm(_p(xx), _p(xy), _p(yy), n0, n1, int(k), 1 if sqrt else 0, _p(out), _p(pred), _s()),
          "two_sample_knn_pm", n0=n0, n1=n1, k=k)
    return float(out[0])


def voxel_counts(clouds: Tensor, res: int = 28) -> Tensor:
    """int32 [res,res,res]: the points of all clouds ([S,N,3]) per half-open cell of the cube [-0.5, 0.5)^3 (float64 edges
    -0.5 + i/res, as numpy builds them); points outside the cube are not counted."""
    pc = _dev(clouds)
    _f32(pc, "clouds")
    if pc.shape[-1] != 3:
        raise ValueError("clouds must end in a dimension of 3, got %s" % (tuple(pc.shape),))
    pc = pc.contiguous()
    counts = torch.zeros((res, res, res), dtype=torch.int32, device=pc.device)
    npts = pc.numel() // 3
    if npts:
        check(_lib.load().spgan_voxel_counts(_p(pc), npts, int(res), _p(counts), _s()), "voxel_counts", npts=npts, res=res)
    return counts


def get_voxel_occ_dist(all_clouds: Tensor, clouds_flag: str = "gen", res: int = 28, bound: float = 0.5, bs: int = 128,
                       warning: bool = True) -> Tensor:
    """GAN_metrics.py:411-447: the float64 [res,res,res] distribution of the points over the cells (counts / total).  The
    reference's bound / bs / warning arguments only steer its printing and batching."""
    c = voxel_counts(all_clouds, res).double()
    return c / c.sum()


def JSD(clouds1: Tensor, clouds2: Tensor, clouds1_flag: str = "gen", clouds2_flag: str = "ref", warning: bool = True) -> float:
    """GAN_metrics.py:450-455: Jensen-Shannon divergence (base 2) of the two sets' 28^3 point distributions."""
    d1 = get_voxel_occ_dist(clouds1).flatten()
    d2 = get_voxel_occ_dist(clouds2).flatten()
    return float(_entropy((d1 + d2) / 2.0, 2) - 0.5 * (_entropy(d1, 2) + _entropy(d2, 2)))


def _three(sample_pcs, ref_pcs, batch_size, dist_type):
    ss = pairwise_dists(sample_pcs, sample_pcs, batch_size, dist_type)
    rr = pairwise_dists(ref_pcs, ref_pcs, batch_size, dist_type)
    sr = pairwise_dists(sample_pcs, ref_pcs, batch_size, dist_type)
    return ss, rr, sr


def compute_all_metrics(sample_pcs: Tensor, ref_pcs: Tensor, batch_size: int = 16, dist_type: str = "CD", fpd: bool = False) -> Dict[str, float]:
    """GAN_metrics.py:796-831 -> {"JSD", "COV", "MMD", "1NN", "6NN", "FPD"} (FPD 0.0 on clouds, as there).  2-D inputs are feature
    rows: with fpd=True the reference's branch (:815-816) runs -- the distances over the features, JSD 0.0 and FPD(sample, ref);
    without it they are refused."""
    sample_pcs, ref_pcs = _dev(sample_pcs), _dev(ref_pcs)
    if sample_pcs.dim() == 2:
        if not fpd:
            raise NotImplementedError(_NO_POINTNET)
        ss, rr, sr = _three(sample_pcs, ref_pcs, batch_size, dist_type)
        return {"JSD": 0.0, "COV": COV(sr), "MMD": MMD(sr), "1NN": KNN(ss, sr, rr, 1), "6NN": KNN(ss, sr, rr, 6), "FPD": FPD(sample_pcs, ref_pcs)}
    ss, rr, sr = _three(sample_pcs, ref_pcs, batch_size, dist_type)
    return {"JSD": JSD(sample_pcs, ref_pcs, "gen", "ref", False), "COV": COV(sr), "MMD": MMD(sr), "1NN": KNN(ss, sr, rr, 1),
            "6NN": KNN(ss, sr, rr, 6), "FPD": 0.0}


def compute_all_metrics_train(sample_pcs: Tensor, ref_pcs: Tensor, model=None, batch_size: int = 16, dist_type: str = "CD",
                              use_FPD_JSD: bool = False) -> Dict[str, float]:
    """GAN_metrics.py:762-793 -> {"JSD", "COV", "MMD", "MMD_t", "1NN", "FPD"}; JSD and FPD stay 0 unless use_FPD_JSD, which needs
    `model` (a module whose forward returns (_, activations)): then JSD of the clouds and FPD of the model's activations are filled
    in (the reference computes the activations and stops there: its FPD line is commented out)."""
    if use_FPD_JSD and model is None:
        raise NotImplementedError(_NO_POINTNET)
    ss, rr, sr = _three(sample_pcs, ref_pcs, batch_size, dist_type)
    fpd, jsd = 0, 0
    if use_FPD_JSD:
        sample_pcs, ref_pcs = _dev(sample_pcs), _dev(ref_pcs)
        sample_buf, ref_buf = extract_acts_with_model([sample_pcs, ref_pcs], model, batch_size=batch_size)
        fpd = FPD(sample_buf, ref_buf)
        jsd = JSD(sample_pcs, ref_pcs, "gen", "ref", False)
    return {"JSD": jsd, "COV": COV(sr), "MMD": MMD(sr), "MMD_t": MMD(sr.t()), "1NN": KNN(ss, sr, rr, 1), "FPD": fpd}


__all__ = ["pairwise_dists", "pairwise_simple", "pairwise_local_CD", "COV", "MMD", "KNN", "JSD", "get_voxel_occ_dist", "voxel_counts",
           "compute_all_metrics", "compute_all_metrics_train"]
