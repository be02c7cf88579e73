"""Point augmentation of the training recipe and the test-time-augmentation views, for the device data stage.

The reference augments every training sample in its voxel datasets (semantickitti_voxel_ms.py:90-100, nuscenes_voxel_ms.py:91-101,
semantickitti_voxel.py:89-99) with `aug_points_ms` / `aug_points` (R/tools/utils/common/seg_utils.py:43-166): a random rotation
about z, a scale drawn from SCALE_AUG_RANGE, one of four x/y flips and a Gaussian translation, applied jointly to the current
scan and the fused multi-scan cloud BEFORE the clamp and both voxelisations.  Under `TTA: True` it builds ten views per scan the
same way (:102-119): rotation `TTA_ANGLES[vote] * pi / 8`, a random scale, no flip, no translation.

Split between host and device the way the work splits:

  host    the random draws, in the reference's order and with the reference's calls on a `np.random.RandomState` - the same seed
          gives the same augmentation as `np.random.seed(seed)` gives the reference - and cos / sin of the angle in float64
          (`AugParams`, `draw_train_params`, `draw_tta_params`);
  device  the per-point arithmetic (ts_stage_augment, csrc/stage.hip): float64 in the reference's order, one rounding to float32,
          switched-off steps skipped (`augment_points`; the stage functions of data/stage.py and data/nuscenes.py take `aug=`).

LaserMix / PolarMix, which the recipe applies before this augmentation, are in data/mix.py.  The KD variant `aug_points_ms_gt`
(seg_utils.py:168-239: the same draws and arithmetic on three clouds) is this kernel with the sample's record on the teacher's
rows too (data/kd.py).  The TIAF variant `aug_points_rgb_ms` (seg_utils.py:241-313: the same draws and arithmetic on the current
scan, the fused cloud and the FOV cloud) and the image flip are in data/tiaf.py; the image-side colour jitter is not built.
"""
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

__all__ = ["AugParams", "TTA_ANGLES", "draw_train_params", "draw_tta_params", "pack_params", "augment_points"]

# seg_utils.py:58,118: the rotation of TTA vote v is TTA_ANGLES[v] * pi / 8
TTA_ANGLES = (0, 1, -1, 2, -2, 6, -6, 7, -7, 8)

ROTATE, SCALE, FLIP, TRANSLATE, SCALE_F32 = 1, 2, 4, 8, 16        # the enable bits of a ts_stage_augment record


@dataclass(frozen=True)
class AugParams:
    """One sample's augmentation: c = cos(theta), s = sin(theta) (float64, np.cos / np.sin as the reference computes them), scale,
    flip type 0 .. 3 (1: x -> -x, 2: y -> -y, 3: both), translation, and which of the four steps run at all.  A step that is off
    is SKIPPED by the kernel, so `AugParams()` leaves a cloud bit for bit as it is."""
    c: float = 1.0
    s: float = 0.0
    scale: float = 1.0
    flip: int = 0
    translate: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    rotate_on: bool = False
    scale_on: bool = False
    flip_on: bool = False
    translate_on: bool = False
    theta: float = 0.0             # the drawn angle (c and s are what the device uses)

    @property
    def bits(self) -> int:
        b = ROTATE * self.rotate_on + SCALE * self.scale_on + FLIP * self.flip_on + TRANSLATE * self.translate_on
        # seg_utils.py:136: `xyz * scale_factor` - after the rotation xyz is float64 (np.dot with the float64 matrix); without it
        # xyz is still the float32 cloud and numpy multiplies a float32 array by a Python float in float32
        if self.scale_on and not self.rotate_on:
            b += SCALE_F32
        return b

    def record(self) -> List[float]:
        """the TS_AUG_RECORD doubles of include/taseg_hip.h: c, s, scale, tx, ty, tz, bits, flip"""
        return [self.c, self.s, self.scale, self.translate[0], self.translate[1], self.translate[2], float(self.bits),
                float(self.flip)]


def _rotation(theta: float) -> Tuple[float, float]:
    return float(np.cos(theta)), float(np.sin(theta))


def draw_train_params(rng: np.random.RandomState, flip: bool = True, scale: bool = True,
                      scale_range: Sequence[float] = (0.9, 1.1), jitter: bool = True, rotate: bool = True) -> AugParams:
    """The training augmentation of one sample (seg_utils.py:115-164 with if_tta False), consuming `rng` exactly as the reference
    consumes numpy's global generator: uniform(0, 2 pi), uniform(lo, hi), choice(4, 1), three normal(0, 0.1, 1) - each only when
    its switch (ROTATE_AUG, SCALE_AUG, FLIP_AUG, TRANSFORM_AUG) is on."""
    theta, c, s, factor, flip_type, noise = 0.0, 1.0, 0.0, 1.0, 0, (0.0, 0.0, 0.0)
    if rotate:
        theta = float(rng.uniform(0, 2 * np.pi))
        c, s = _rotation(theta)
    if scale:
        factor = float(rng.uniform(scale_range[0], scale_range[1]))
    if flip:
        flip_type = int(rng.choice(4, 1)[0])
    if jitter:
        noise = (float(rng.normal(0, 0.1, 1)[0]), float(rng.normal(0, 0.1, 1)[0]), float(rng.normal(0, 0.1, 1)[0]))
    return AugParams(c=c, s=s, scale=factor, flip=flip_type, translate=noise, rotate_on=bool(rotate), scale_on=bool(scale),
                     flip_on=bool(flip), translate_on=bool(jitter), theta=theta)


def draw_tta_params(rng: np.random.RandomState, vote: int, scale_range: Sequence[float] = (0.9, 1.1)) -> AugParams:
    """TTA view `vote` (semantickitti_voxel_ms.py:102-119): the table's rotation, a random scale, no flip, no translation.  The
    scale comes from SCALE_AUG_RANGE: the reference's `scale_aug_range = [0.95, 1.05]` assignment names an attribute nothing reads."""
    theta = TTA_ANGLES[vote] * np.pi / 8.0
    c, s = _rotation(theta)
    factor = float(rng.uniform(scale_range[0], scale_range[1]))
    return AugParams(c=c, s=s, scale=factor, rotate_on=True, scale_on=True, theta=float(theta))


def pack_params(params: Union[AugParams, Sequence[AugParams], np.ndarray]) -> np.ndarray:
    """float64 [B, 8]: one ts_stage_augment record per sample (a packed array passes through)"""
    if isinstance(params, np.ndarray):
        if params.dtype != np.float64 or params.ndim != 2 or params.shape[1] != 8:
            raise TypeError("packed augmentation parameters are float64 [B, 8]")
        return params
    if isinstance(params, AugParams):
        params = [params]
    if not len(params) or not all(isinstance(p, AugParams) for p in params):
        raise TypeError("aug must be AugParams records, one per sample")
    return np.array([p.record() for p in params], dtype=np.float64)


def augment_points(points, params, sample_idx=None, out: Optional["torch.Tensor"] = None):   # noqa: F821
    """points [n, F >= 3] float32 on the device with the xyz columns augmented (the other columns untouched), in one launch.
    params: an AugParams, a list of them (row i uses params[sample_idx[i]], sample_idx [n] int32; None = all rows params[0]) or
    the packed float64 [B, 8] records, on the host or already on the device.  out: None = a new tensor, `points` = in place."""
    import torch
    from .. import backend as B
    if not isinstance(params, torch.Tensor):
        params = torch.from_numpy(pack_params(params)).to(points.device, non_blocking=True)
    return B.stage_augment(points, params, sample_idx, out)
