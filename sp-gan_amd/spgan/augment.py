"""Device-side batch augmentation over the HIP kernels of csrc/augment.hip: the point-cloud transforms of Common/data_utils.py,
Common/provider.py and Common/point_operation.py for a whole batch in two launches, with the project's own counter-based random
stream (Philox4x32-10; the draw assignment is stated in include/spgan_hip.h).

    aug = BatchAugment(seed=7, permute=True, rotate="axis", scale=(0.8, 1.25))        # H5DataLoader's pair
    batch, params = aug(data [S,P,C], index int64 [B], n=2048, layout="bnc")          # [B,n,C] (or "bcn": [B,C,n]), [B,16]
    gt2 = aug.apply(params, gt)                                                       # the same A, t on a paired cloud (*_and_gt)

Stages run in one fixed order -- gather, permutation, rotation, rotation perturbation, scale, translation, jitter, dropout -- each on
or off.  Every call that draws advances a device-resident 64-bit counter by one, in the kernel: nothing synchronises with the host, so a
call replays inside spgan.CapturedBody with fresh draws per replay (create the object with `device=` or call it once before capturing,
so that the counter exists), and (seed, step) is the whole resume state.  Results repeat bit for bit.

The reference-named wrappers below go through the same kernel.  Unlike the reference they RETURN A NEW TENSOR and leave their argument
untouched, draw from this module's stream instead of numpy's / torch's, and permute every cloud on its own.  No gradients flow through
any of this.  Importing this module does not load the shared library or touch the GPU.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

Tensor = torch.Tensor
MAX_POINTS = 8192            # spgan_augment_max_points
PURPOSE_EPOCH = 4            # host-side stream of DeviceDataset's epoch order


# ------------------------------------------------------------------------------------------ host Philox (epoch order only)
def philox_words(seed: int, purpose: int, slot: int, step: int, n: int) -> np.ndarray:
    """The first n words of the stream of (purpose, slot) at `step` (include/spgan_hip.h), on the host: uint32 [n]."""
    m32 = np.uint64(0xFFFFFFFF)
    e = np.arange((n + 3) // 4, dtype=np.uint64)
    c0, c1 = e, np.full_like(e, (purpose << 24) | slot)
    c2, c3 = np.full_like(e, step & 0xFFFFFFFF), np.full_like(e, (step >> 32) & 0xFFFFFFFF)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack([c0, c1, c2, c3], axis=1).reshape(-1)[:n].astype(np.uint32)


def epoch_order(seed: int, epoch: int, count: int) -> np.ndarray:
    """A uniformly random order of `count` items for `epoch`: ascending (draw << 32) | index, as the kernel's permutation."""
    w = philox_words(seed, PURPOSE_EPOCH, 0, epoch, count).astype(np.uint64)
    return np.argsort((w << np.uint64(32)) | np.arange(count, dtype=np.uint64), kind="stable")


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class AugmentGenerator:
    """A seed and the device-resident call counter `step` (int64 [1]); the counter is created on first use on a device."""

    def __init__(self, seed: int = 0, device=None):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._step: Optional[Tensor] = None
        self._pending = 0
        if device is not None:
            self.step_tensor(torch.device(device))

    def step_tensor(self, device) -> Tensor:
        if self._step is None or self._step.device != device:
            self._pending = self.step
            self._step = torch.tensor([self._pending], dtype=torch.int64, device=device)
        return self._step

    @property
    def step(self) -> int:
        """The counter's value (reads it back from the device: a host synchronisation)."""
        return self._pending if self._step is None else int(self._step.item()) & 0xFFFFFFFFFFFFFFFF

    def get_state(self) -> dict:
        return {"seed": self.seed, "step": self.step}

    def set_state(self, state: dict) -> None:
        self.seed = int(state["seed"]) & 0xFFFFFFFFFFFFFFFF
        step = int(state["step"]) & 0xFFFFFFFFFFFFFFFF
        self._pending = step
        if self._step is not None:
            self._step.fill_(step - (1 << 64) if step >= (1 << 63) else step)


default_generator = AugmentGenerator(0)


def manual_seed(seed: int) -> None:
    """Seed the stream of the reference-named wrappers that are not given a generator, and rewind its counter."""
    default_generator.set_state({"seed": seed, "step": 0})


def _pair(v) -> Tuple[float, float]:
    a, b = v
    return float(a), float(b)


class BatchAugment:
    """One configuration of the pipeline.
      permute            per-cloud random point order (np.random.shuffle of the rows)
      rotate             None | "axis" (about `axis` by U[0, 2pi)) | "xyz" (Rz Ry Rx of three such angles)
      transpose          False: xyz @ R (provider, point_operation); True: xyz @ R.T (data_utils.angle_axis callers)
      perturb            None | (sigma, clip): Rz Ry Rx of three clipped normal angles
      scale              None | (lo, hi); scale_per_axis: one factor per axis
      translate          None | range; translate_scalar: one offset added to all three axes (PointcloudTranslate)
      jitter             None | (sigma, clip)
      dropout            None | max_ratio: rows with u <= u_cloud * max_ratio take the final value of row 0
    """

    def __init__(self, seed: int = 0, permute: bool = False, rotate: Optional[str] = None, axis: Sequence[float] = (0.0, 1.0, 0.0),
                 transpose: bool = False, perturb=None, scale=None, scale_per_axis: bool = False, translate=None,
                 translate_scalar: bool = False, jitter=None, dropout=None, device=None, generator: Optional[AugmentGenerator] = None):
        if rotate not in (None, "axis", "xyz"):
            raise ValueError("rotate must be None, 'axis' or 'xyz', got %r" % (rotate,))
        ax = np.asarray(axis, dtype=np.float64).reshape(-1)
        if ax.shape != (3,) or not np.isfinite(ax).all() or np.linalg.norm(ax) == 0:
            raise ValueError("axis must be a non-zero 3-vector")
        ax = ax / np.linalg.norm(ax)
        cfg = _lib.AugmentCfg()
        cfg.permute = int(bool(permute))
        cfg.rotate = {None: 0, "axis": 1, "xyz": 2}[rotate]
        cfg.axis[0], cfg.axis[1], cfg.axis[2] = float(ax[0]), float(ax[1]), float(ax[2])
        cfg.transpose = int(bool(transpose))
        if perturb is not None:
            cfg.perturb = 1
            cfg.perturb_sigma, cfg.perturb_clip = _pair(perturb)
        if scale is not None:
            cfg.scale = 2 if scale_per_axis else 1
            cfg.scale_lo, cfg.scale_hi = _pair(scale)
        if translate is not None:
            cfg.translate = 2 if translate_scalar else 1
            cfg.translate_range = float(translate)
        if jitter is not None:
            cfg.jitter = 1
            cfg.jitter_sigma, cfg.jitter_clip = _pair(jitter)
            if not cfg.jitter_clip > 0:
                raise ValueError("jitter clip must be positive")
        if dropout is not None:
            if not 0.0 <= float(dropout) < 1.0:
                raise ValueError("dropout max_ratio must lie in [0, 1)")
            cfg.dropout = 1
            cfg.dropout_max = float(dropout)
        self.cfg = cfg
        self.generator = generator if generator is not None else AugmentGenerator(seed, device)
        self._arange = {}

    # ------------------------------------------------------------------ state
    @property
    def seed(self) -> int:
        return self.generator.seed

    def get_state(self) -> dict:
        """{'seed', 'step'}: the whole state of the stream (reading the step synchronises with the device)."""
        return self.generator.get_state()

    def set_state(self, state: dict) -> None:
        self.generator.set_state(state)

    # ------------------------------------------------------------------ launch
    def _launch(self, cfg, data: Tensor, index: Tensor, n: Optional[int], layout: str, keys, params):
        if not isinstance(data, torch.Tensor) or data.dim() != 3:
            raise ValueError("data must be a [S, P, C] tensor")
        if not data.is_cuda:
            raise ValueError("data must live on the GPU (spgan has no CPU path); got device %s" % data.device)
        if data.dtype != torch.float32:
            raise ValueError("data must be float32, got %s" % data.dtype)
        S, P, C = data.shape
        if C not in (3, 6):
            raise ValueError("data must have 3 (xyz) or 6 (xyz + normal) channels, got %d" % C)
        if S < 1 or P < 1:
            raise ValueError("data is empty: %s" % (tuple(data.shape),))
        n = P if n is None else int(n)
        if n < 1 or n > P:
            raise ValueError("n must lie in 1 .. P = %d, got %d" % (P, n))
        if n > MAX_POINTS:
            raise ValueError("at most %d points per cloud (spgan_augment_max_points), got n = %d" % (MAX_POINTS, n))
        if layout not in ("bnc", "bcn"):
            raise ValueError("layout must be 'bnc' or 'bcn', got %r" % (layout,))
        if not isinstance(index, torch.Tensor) or index.dim() != 1 or index.dtype != torch.int64 or index.device != data.device:
            raise ValueError("index must be an int64 [B] tensor on the data's device")
        B = index.numel()
        if B < 1 or B > 65535:
            raise ValueError("1 .. 65535 clouds per call, got %d" % B)
        dev = data.device
        data, index = data.contiguous(), index.contiguous()
        if keys is not None:
            if not isinstance(keys, torch.Tensor) or tuple(keys.shape) != (B, n) or keys.device != dev:
                raise ValueError("keys must be [B, n] = %s on the data's device" % ((B, n),))
            if keys.dtype == torch.int64:
                keys = ((keys + (1 << 31)) % (1 << 32) - (1 << 31)).to(torch.int32)           # values 0 .. 2^32-1 -> their bit patterns
            elif keys.dtype not in (torch.int32, torch.uint32):
                raise ValueError("keys must be uint32 (or int32 bit patterns, or int64 values below 2^32), got %s" % keys.dtype)
            keys = keys.contiguous()
        if params is not None:
            if not isinstance(params, torch.Tensor) or tuple(params.shape) != (B, 16) or params.dtype != torch.float32 or params.device != dev:
                raise ValueError("params must be float32 [B, 16] = %s on the data's device" % ((B, 16),))
            params = params.contiguous()
        permute = bool(cfg.permute) or keys is not None
        if permute != bool(cfg.permute):
            c2 = _lib.AugmentCfg.from_buffer_copy(cfg)
            c2.permute = int(permute)
            cfg = c2
        draws = (permute and keys is None) or bool(cfg.jitter) or bool(cfg.dropout) or (
            params is None and bool(cfg.rotate or cfg.perturb or cfg.scale or cfg.translate))
        step = self.generator.step_tensor(dev)
        out = torch.empty((B, n, C) if layout == "bnc" else (B, C, n), dtype=torch.float32, device=dev)
        rec = torch.empty((B, 16), dtype=torch.float32, device=dev)
        perm = torch.empty((B, n), dtype=torch.int32, device=dev) if permute else None
        st = _lib.load().spgan_augment_batch(_p(data), S, P, C, _p(index), B, n, 0 if layout == "bnc" else 1, cfg, self.generator.seed,
                                             _p(step), int(draws), _p(keys), _p(params), _p(perm), _p(out), _p(rec), _stream())
        if st == -22:
            raise ValueError("augment_batch refused its sizes: S=%d P=%d C=%d B=%d n=%d (n <= %d)" % (S, P, C, B, n, MAX_POINTS))
        _lib.check(st, "augment_batch", S=S, P=P, C=C, B=B, n=n)
        return out, rec

    def __call__(self, data: Tensor, index: Tensor, n: Optional[int] = None, layout: str = "bnc", keys: Optional[Tensor] = None,
                 params: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """-> (batch [B,n,C] or [B,C,n], parameter record [B,16]).  keys uint32 [B,n] replaces the permutation draws (and turns the
        permutation on for this call); params [B,16] replaces stages 3-6 (apply-only mode)."""
        return self._launch(self.cfg, data, index, n, layout, keys, params)

    def _rows(self, B: int, dev) -> Tensor:
        key = (B, dev)
        if key not in self._arange:
            self._arange[key] = torch.arange(B, dtype=torch.int64, device=dev)
        return self._arange[key]

    def transform(self, pts: Tensor, layout: str = "bnc") -> Tuple[Tensor, Tensor]:
        """The pipeline on a batch that is already gathered: pts [B,N,C] -> (new tensor, parameter record)."""
        if not isinstance(pts, torch.Tensor) or pts.dim() != 3:
            raise ValueError("pts must be a [B, N, C] tensor")
        return self._launch(self.cfg, pts, self._rows(pts.shape[0], pts.device), None, layout, None, None)

    def apply(self, params: Tensor, pts: Tensor, layout: str = "bnc") -> Tensor:
        """xyz A + t of a parameter record on another batch [B,N,C] (the `gt` of the reference's *_and_gt functions): no permutation,
        no jitter, no dropout, no draw; the counter stays."""
        if not isinstance(pts, torch.Tensor) or pts.dim() != 3:
            raise ValueError("pts must be a [B, N, C] tensor")
        return self._launch(_lib.AugmentCfg(), pts, self._rows(pts.shape[0], pts.device), None, layout, None, params)[0]

    @staticmethod
    def params_from(angle_y: Optional[Tensor] = None, scale: Optional[Tensor] = None, translate: Optional[Tensor] = None,
                    batch: Optional[int] = None, device=None) -> Tensor:
        """A parameter record [B,16] from given values: xyz @ Ry(angle_y) (point_operation's matrix), * scale ([B] or [B,3]),
        + translate ([B,3]); each optional."""
        given = [t for t in (angle_y, scale, translate) if t is not None]
        if given:
            B, dev = given[0].shape[0], given[0].device
        elif batch is not None:
            B, dev = int(batch), torch.device(device if device is not None else "cuda")
        else:
            raise ValueError("params_from needs a value or `batch`")
        A = torch.zeros((B, 3, 3), dtype=torch.float32, device=dev)
        if angle_y is not None:
            c, s = torch.cos(angle_y.float()), torch.sin(angle_y.float())
            A[:, 0, 0] = c; A[:, 0, 2] = s; A[:, 1, 1] = 1.0; A[:, 2, 0] = -s; A[:, 2, 2] = c
        else:
            A[:, 0, 0] = 1.0; A[:, 1, 1] = 1.0; A[:, 2, 2] = 1.0
        if scale is not None:
            sc = scale.float().to(dev)
            A = A * (sc.view(B, 1, 1) if sc.dim() == 1 else sc.view(B, 1, 3))
        rec = torch.zeros((B, 16), dtype=torch.float32, device=dev)
        rec[:, :9] = A.reshape(B, 9)
        if translate is not None:
            rec[:, 9:12] = translate.float().to(dev).view(B, 3)
        return rec


# ------------------------------------------------------------------------------------------ reference-named wrappers
class _Wrapper:
    """A reference transform as a callable on a device batch [B,N,C]: returns a new tensor (the reference writes in place)."""

    def __init__(self, seed: Optional[int] = None, **options):
        gen = default_generator if seed is None else AugmentGenerator(seed)
        self.aug = BatchAugment(generator=gen, **options)

    def __call__(self, pc: Tensor) -> Tensor:
        return self.aug.transform(pc)[0]


class PointcloudRotate_batch(_Wrapper):
    def __init__(self, axis=(0.0, 1.0, 0.0), seed: Optional[int] = None):
        super().__init__(seed, rotate="axis", axis=axis, transpose=True)


class PointcloudRotatePerturbation_batch(_Wrapper):
    def __init__(self, angle_sigma: float = 0.06, angle_clip: float = 0.18, seed: Optional[int] = None):
        super().__init__(seed, perturb=(angle_sigma, angle_clip), transpose=True)


class PointcloudScale_batch(_Wrapper):
    def __init__(self, scale_low: float = 2. / 3., scale_high: float = 3. / 2., seed: Optional[int] = None):
        super().__init__(seed, scale=(scale_low, scale_high), scale_per_axis=True)


class PointcloudTranslate_batch(_Wrapper):
    def __init__(self, translate_range: float = 0.2, seed: Optional[int] = None):
        super().__init__(seed, translate=translate_range)


class PointcloudScaleAndTranslate(_Wrapper):
    def __init__(self, scale_low: float = 2. / 3., scale_high: float = 3. / 2., translate_range: float = 0.2, seed: Optional[int] = None):
        super().__init__(seed, scale=(scale_low, scale_high), scale_per_axis=True, translate=translate_range)


class PointcloudJitter_batch(_Wrapper):
    def __init__(self, std: float = 0.01, clip: float = 0.05, seed: Optional[int] = None):
        super().__init__(seed, jitter=(std, clip))


class PointcloudRandomInputDropout_batch(_Wrapper):
    def __init__(self, max_dropout_ratio: float = 0.875, seed: Optional[int] = None):
        super().__init__(seed, dropout=max_dropout_ratio)


class PointcloudRotatebyAngle(_Wrapper):
    """__call__(pc, rotation_angle): xyz (and normals) @ Ry(angle), one angle for the batch."""

    def __init__(self, rotation_angle: float = 0.0, seed: Optional[int] = None):
        super().__init__(seed)
        self.rotation_angle = rotation_angle

    def __call__(self, pc: Tensor, rotation_angle: Optional[float] = None) -> Tensor:
        if rotation_angle is not None:
            self.rotation_angle = rotation_angle
        angle = torch.full((pc.shape[0],), float(self.rotation_angle), dtype=torch.float32, device=pc.device)
        return self.aug.apply(BatchAugment.params_from(angle_y=angle), pc)


def _fn(pc: Tensor, generator: Optional[AugmentGenerator], **options) -> Tensor:
    return BatchAugment(generator=generator if generator is not None else default_generator, **options).transform(pc)[0]


def rotate_point_cloud(batch_data: Tensor, generator: Optional[AugmentGenerator] = None) -> Tensor:
    """provider.py:32-50: every cloud @ Ry(U[0, 2pi))."""
    return _fn(batch_data, generator, rotate="axis", axis=(0.0, 1.0, 0.0))


def rotate_point_cloud_z(batch_data: Tensor, generator: Optional[AugmentGenerator] = None) -> Tensor:
    """provider.py:52-70: the matrix there, [c s 0; -s c 0; 0 0 1], is Rz transposed."""
    return _fn(batch_data, generator, rotate="axis", axis=(0.0, 0.0, 1.0), transpose=True)


def rotate_perturbation_point_cloud(batch_data: Tensor, angle_sigma: float = 0.06, angle_clip: float = 0.18,
                                    generator: Optional[AugmentGenerator] = None) -> Tensor:
    return _fn(batch_data, generator, perturb=(angle_sigma, angle_clip))


def jitter_point_cloud(batch_data: Tensor, sigma: float = 0.01, clip: float = 0.05, generator: Optional[AugmentGenerator] = None) -> Tensor:
    return _fn(batch_data, generator, jitter=(sigma, clip))


def shift_point_cloud(batch_data: Tensor, shift_range: float = 0.1, generator: Optional[AugmentGenerator] = None) -> Tensor:
    return _fn(batch_data, generator, translate=shift_range)


def random_scale_point_cloud(batch_data: Tensor, scale_low: float = 0.8, scale_high: float = 1.25,
                             generator: Optional[AugmentGenerator] = None) -> Tensor:
    return _fn(batch_data, generator, scale=(scale_low, scale_high))


def random_point_dropout(batch_pc: Tensor, max_dropout_ratio: float = 0.875, generator: Optional[AugmentGenerator] = None) -> Tensor:
    return _fn(batch_pc, generator, dropout=max_dropout_ratio)


def shuffle_points(batch_data: Tensor, generator: Optional[AugmentGenerator] = None) -> Tensor:
    """provider.py:20-30 draws one order for the whole batch; here every cloud gets its own."""
    return _fn(batch_data, generator, permute=True)


def augment_batch_data(batch_data: Tensor, use_normal: bool = False, generator: Optional[AugmentGenerator] = None) -> Tensor:
    """provider.py:249-262 in one call: rotation about y, rotation perturbation, scale, shift, jitter and the point shuffle (which runs
    first here: the stage order is fixed, and the distribution is the same).  Normals (use_normal, C = 6) are rotated only."""
    if use_normal != (batch_data.shape[-1] == 6):
        raise ValueError("use_normal = %s needs %d channels, got %d" % (use_normal, 6 if use_normal else 3, batch_data.shape[-1]))
    return _fn(batch_data, generator, permute=True, rotate="axis", perturb=(0.06, 0.18), scale=(0.8, 1.25), translate=0.1,
               jitter=(0.01, 0.05))


def reference_transform(which: str = "ref", seed: int = 0, device=None) -> BatchAugment:
    """'ref': what H5DataLoader.__getitem__ applies with augment (point shuffle, rotation about y, one scale in [0.8, 1.25]);
    'full': the reference's point_transform (H5DataLoader.py:21-31: rotation, rotation perturbation, scale, scalar translation,
    jitter, and the input dropout it lists) on top of the shuffle."""
    if which == "ref":
        return BatchAugment(seed, permute=True, rotate="axis", scale=(0.8, 1.25), device=device)
    if which == "full":
        return BatchAugment(seed, permute=True, rotate="axis", transpose=True, perturb=(0.06, 0.18), scale=(0.8, 1.25), translate=0.1,
                            translate_scalar=True, jitter=(0.01, 0.05), dropout=0.875, device=device)
    raise ValueError("unknown transform set %r" % (which,))


__all__ = ["BatchAugment", "AugmentGenerator", "default_generator", "manual_seed", "philox_words", "epoch_order", "reference_transform",
           "PointcloudRotate_batch", "PointcloudRotatePerturbation_batch", "PointcloudScale_batch", "PointcloudTranslate_batch",
           "PointcloudScaleAndTranslate", "PointcloudJitter_batch", "PointcloudRandomInputDropout_batch", "PointcloudRotatebyAngle",
           "rotate_point_cloud", "rotate_point_cloud_z", "rotate_perturbation_point_cloud", "jitter_point_cloud", "shift_point_cloud",
           "random_scale_point_cloud", "random_point_dropout", "shuffle_points", "augment_batch_data"]
