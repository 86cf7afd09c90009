"""The Frechet point-cloud distance of Common/GAN_metrics.py (FPD, :537-545), on the device in float64 (csrc/frechet.hip).

  get_activations, extract_acts_with_model   GAN_metrics.py:50-105, 190-200: the caller's feature network over batches of clouds
  ActivationStatistics, activation_statistics the mean and covariance of [n,d] activations, chunk by chunk (np.mean / np.cov)
  calculate_frechet_distance                  GAN_metrics.py:484-535: |mu1 - mu2|^2 + tr(S1 + S2 - 2 sqrt(S1 S2))
  FPD                                         GAN_metrics.py:537-545

The reference copies the activations to the host and calls scipy.linalg.sqrtm.  Here tr sqrt(S1 S2) is the nuclear norm of
sqrt(S1) sqrt(S2): two square roots by the coupled Newton-Schulz iteration and one polar iteration, all float64 MFMA products,
each stage stopped on the device; one distance costs one host read (the result).  The pretrained feature networks
(`evaluation.pointnet`, `evaluation.AutoEncoder`) are not part of the reference tree and are not provided: `model` is any module
whose forward returns `(_, activations)`.

Three deliberate differences from the reference:
  1. means are float64 (np.mean of float32 activations is float32, which costs 4e-3 of the result on features of mean 1000);
  2. mismatched shapes and sets of fewer than 2 rows raise ValueError (the reference asserts, or divides by zero);
  3. eps is used only if the result is not finite (the reference's fallback branch).
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .ops import _p, _s, check

Tensor = torch.Tensor
MAX_DIM = 2048


def get_activations(pointclouds: Tensor, model, batch_size: int = 100, dims: int = 512) -> Tensor:
    """GAN_metrics.py:50-105: model.eval(); batches of `batch_size` clouds in input order, the partial last batch kept;
    `_, actv = model(batch)` under no_grad, `actv.squeeze(1)`; the rows concatenated, on the model's device.  `dims` is unused, as there."""
    model.eval()
    n = pointclouds.size(0)
    acts = []
    for start in range(0, n, batch_size):
        batch = pointclouds[start:min(start + batch_size, n)]
        with torch.no_grad():
            _, actv = model(batch)
        acts.append(actv.squeeze(1))
    return torch.cat(acts, dim=0)


def extract_acts_with_model(pcs: Sequence[Tensor], model, batch_size: int = 16) -> List[Tensor]:
    """GAN_metrics.py:190-200: get_activations for every set of clouds in `pcs`."""
    with torch.no_grad():
        return [get_activations(pc, model, batch_size=batch_size) for pc in pcs]


def _acts(acts, name: str) -> Tensor:
    if isinstance(acts, np.ndarray):
        acts = torch.from_numpy(np.ascontiguousarray(acts, dtype=np.float32)).cuda()
    if not isinstance(acts, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor or a numpy array" % name)
    if not acts.is_cuda:
        raise RuntimeError("%s must live on the GPU (spgan has no CPU path); got device %s" % (name, acts.device))
    if acts.dim() != 2:
        raise ValueError("%s must be [n, d] activations, got shape %s" % (name, tuple(acts.shape)))
    if not 2 <= acts.shape[1] <= MAX_DIM:
        raise ValueError("%s: the feature size must lie in [2, %d], got %d" % (name, MAX_DIM, acts.shape[1]))
    return acts.detach().float().contiguous()


class ActivationStatistics:
    """Running (count, pivot [d], sum [d], M2 [d,d]) of activation rows in float64 on the device.  update() adds a chunk [n,d] of
    float32 rows: its column sums and centred Gram matrix come from one launch sequence and are merged by the pairwise update, so the
    5000 activation rows of an evaluation never have to be resident at once.  The sums are taken of x - pivot (the first row seen),
    so that a large common mean does not round them.  mean = pivot + sum / count, cov = M2 / (count - 1) (np.cov)."""

    def __init__(self):
        self.count = 0
        self._sum = None
        self._m2 = None

    def update(self, acts) -> "ActivationStatistics":
        x = _acts(acts, "acts")
        n, d = x.shape
        if n == 0:
            return self
        if self._sum is None:
            self._sum = torch.empty((2, d), dtype=torch.float64, device=x.device)       # pivot, sums of x - pivot
            self._m2 = torch.empty((d, d), dtype=torch.float64, device=x.device)
        elif self._sum.shape[1] != d:
            raise ValueError("feature size changed between chunks: %d, then %d" % (self._sum.shape[1], d))
        lib = _lib.load()
        nbytes = lib.spgan_fpd_moments_ws_bytes(n, d)
        ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=x.device)
        check(lib.spgan_fpd_moments_update(_p(x), n, d, self.count, _p(self._sum), _p(self._m2), _p(ws), nbytes, _s()), "fpd_moments_update",
              n=n, d=d, count=self.count)
        self.count += n
        return self

    def _need(self, k: int, what: str):
        if self.count < k:
            raise ValueError("%s needs at least %d activation rows, got %d" % (what, k, self.count))

    @property
    def mean(self) -> Tensor:
        self._need(1, "mean")
        return self._sum[0] + self._sum[1] / self.count

    @property
    def cov(self) -> Tensor:
        self._need(2, "cov")
        return self._m2 / (self.count - 1)

    def state_dict(self) -> Dict[str, object]:
        return {"count": self.count, "sum": None if self._sum is None else self._sum.clone(), "m2": None if self._m2 is None else self._m2.clone()}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        self.count = int(state["count"])
        self._sum = None if state["sum"] is None else state["sum"].detach().clone().double()
        self._m2 = None if state["m2"] is None else state["m2"].detach().clone().double()

    def save(self, path) -> None:
        """An .npz with the keys of the precomputed-statistics files FID tools exchange: m (mean), s (covariance)."""
        np.savez(path, m=self.mean.cpu().numpy(), s=self.cov.cpu().numpy())

    @staticmethod
    def load(path) -> Tuple[np.ndarray, np.ndarray]:
        """(m, s) of a file written by save(), as float64 numpy arrays for calculate_frechet_distance."""
        with np.load(path) as f:
            return np.asarray(f["m"], dtype=np.float64), np.asarray(f["s"], dtype=np.float64)


def activation_statistics(acts) -> Tuple[Tensor, Tensor]:
    """(mean [d], covariance [d,d]) of [n,d] activations: float64 tensors on the device (np.mean in float64, np.cov)."""
    st = ActivationStatistics().update(acts)
    if st.count < 2:
        raise ValueError("a covariance needs at least 2 activation rows, got %d" % st.count)
    return st.mean, st.cov


def _f64(x, name: str) -> Tensor:
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
    if not isinstance(x, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor or a numpy array" % name)
    if not x.is_cuda:
        raise RuntimeError("%s must live on the GPU (spgan has no CPU path); got device %s" % (name, x.device))
    return x.detach().double().contiguous()


def frechet_distance_device(mu1: Tensor, sigma1: Tensor, mu2: Tensor, sigma2: Tensor) -> Tensor:
    """float64 [5] on the device: (distance, iterations of sqrt(sigma1), of sqrt(sigma2), of the polar stage, tr sqrt(sigma1 sigma2));
    no host read."""
    d = mu1.shape[0]
    lib = _lib.load()
    nbytes = lib.spgan_fpd_distance_ws_bytes(d)
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=mu1.device)
    out = torch.empty((5,), dtype=torch.float64, device=mu1.device)
    check(lib.spgan_fpd_distance(_p(mu1), _p(sigma1), _p(mu2), _p(sigma2), d, _p(out), _p(ws), nbytes, _s()), "fpd_distance", d=d)
    return out


def frechet_distance_info(mu1, sigma1, mu2, sigma2, eps: float = 1e-6) -> Dict[str, object]:
    """calculate_frechet_distance with its iteration counts: {"distance", "iterations": (sqrt(sigma1), sqrt(sigma2), polar),
    "tr_covmean", "used_eps"}."""
    mu1, mu2 = _f64(mu1, "mu1").reshape(-1), _f64(mu2, "mu2").reshape(-1)
    sigma1, sigma2 = _f64(sigma1, "sigma1"), _f64(sigma2, "sigma2")
    if sigma1.dim() < 2:
        sigma1, sigma2 = sigma1.reshape(1, -1), sigma2.reshape(1, -1)           # np.atleast_2d
    if mu1.shape != mu2.shape:
        raise ValueError("the mean vectors have different lengths: %s and %s" % (tuple(mu1.shape), tuple(mu2.shape)))
    if sigma1.shape != sigma2.shape:
        raise ValueError("the covariances have different dimensions: %s and %s" % (tuple(sigma1.shape), tuple(sigma2.shape)))
    d = mu1.shape[0]
    if sigma1.shape != (d, d):
        raise ValueError("expected covariances [%d,%d] for means [%d], got %s" % (d, d, d, tuple(sigma1.shape)))
    if not 2 <= d <= MAX_DIM:
        raise ValueError("the feature size must lie in [2, %d], got %d" % (MAX_DIM, d))
    out = frechet_distance_device(mu1, sigma1, mu2, sigma2).cpu()                 # the one host read
    used_eps = False
    if not bool(torch.isfinite(out[0])):
        off = torch.eye(d, dtype=torch.float64, device=mu1.device) * eps
        out = frechet_distance_device(mu1, sigma1 + off, mu2, sigma2 + off).cpu()
        used_eps = True
    return {"distance": float(out[0]), "iterations": (int(out[1]), int(out[2]), int(out[3])), "tr_covmean": float(out[4]), "used_eps": used_eps}


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps: float = 1e-6) -> float:
    """GAN_metrics.py:484-535 for device tensors or numpy arrays (float32 or float64) -> a Python float.  eps is added to both
    diagonals only if the first result is not finite."""
    return frechet_distance_info(mu1, sigma1, mu2, sigma2, eps)["distance"]


def FPD(pc1_acts, pc2_acts) -> float:
    """GAN_metrics.py:537-545: the Frechet distance between the Gaussians fitted to two sets of activations [n1,d], [n2,d]."""
    a, b = _acts(pc1_acts, "pc1_acts"), _acts(pc2_acts, "pc2_acts")
    if a.shape[1] != b.shape[1]:
        raise ValueError("feature sizes differ: %d and %d" % (a.shape[1], b.shape[1]))
    m1, s1 = activation_statistics(a)
    m2, s2 = activation_statistics(b)
    return calculate_frechet_distance(m1, s1, m2, s2)


__all__ = ["get_activations", "extract_acts_with_model", "ActivationStatistics", "activation_statistics", "calculate_frechet_distance",
           "frechet_distance_info", "frechet_distance_device", "FPD"]
