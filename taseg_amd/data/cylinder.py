"""The cylinder data stage on the device: what Cylinder_TS's dataset does per sample in numpy
(R/pcseg/data/dataset/semantickitti/semantickitti_cylinder.py:104-219 `get_single_sample`, `voxelize_with_label`, `collate_batch`,
`collate_batch_tta`), for a whole batch of resident scans in one chain of launches.

  augmentation (aug=)   ts_stage_augment     `aug_points` (seg_utils.py:43-100) on the xyz columns, stored back into the float32 rows
                                             (:115): the arithmetic and draws of data/augment.py, one record per sample
  polar cells           ts_cylinder_cells    rho, phi in degrees (float32), clip + floor in float64 (:144-153), the voxel centres
                                             and the 5 + F feature columns (:156-160), `point_coord` as int64 - one lane per row
  voxels + labels       ts_cylinder_voxels   sparse_quantize's order and first-occurrence representative, the inverse map local to
                                             each sample, the majority vote of :38-43 (label 67 not counted, lowest class on a tie,
                                             class 0 for a voxel of ignored points) - one stable sort, no table, no atomics
  voxel rows            index_select         voxel_coord / voxel_feature = rows `inds` of the point arrays (:156-157: a voxel's
                                             centre and its representative's come from the same integers)

Reproduced bit for bit against the real dataset code (tests/golden/cylinder_stage.npz), with ONE stated difference: numpy's float32
`arctan2` is not correctly rounded (up to ~2.3 ulp from the float64 value); the device takes `(float)atan2((double)y, (double)x)`,
so the `phi_deg` feature column can differ from the reference's by a few float32 ulp.  The cells never did on the fixtures.

One host read per batch: the per-sample voxel counts, their total and the error words, in one copy.  A label that is neither
`ignore_label` nor in [0, num_classes) (an IndexError in the reference) and a non-finite coordinate (a NaN handed to astype(int)
there) raise ValueError at that read.

Not built: the `augmented_*` / `flag*` keys (`get_single_sample` never produces them; the collate functions only pass them on), the
nuScenes and Waymo dataset files (the same stage; rows of 5 columns are covered).  PolarMix / LaserMix clouds (data/mix.py
`polarmix_points` / `lasermix_points`) are device clouds that can be fed in as `points`.

Both batches feed the evaluation on the device as they are: `pcseg.eval.evaluate(model, batches, num_class, on_device=True)` over
`build_cylinder_batch`'s (validation, predictions=True) and, with tta_votes=V, over `build_cylinder_tta_batch`'s - the votes of one
scan as the V scenes of a batch, equal point counts, which is what `DeviceEvalTail.run_points` sums.  Every point's cell is a voxel
of the batch here, so the tail's "no voxel row" flag cannot rise on them.
"""
from dataclasses import dataclass
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from .. import backend as B
from .augment import augment_points, draw_tta_params
from .stage import _aug_records, rows_index32

__all__ = ["CylinderGrid", "build_cylinder_batch", "build_cylinder_tta_batch"]

FLAG_NONFINITE, FLAG_LABEL, FLAG_RANGE = 1, 2, 4        # include/taseg_hip.h TS_CYL_FLAG_*


def _numbers(values, name) -> Tuple:
    out = tuple(v.item() if isinstance(v, np.generic) else v for v in values)
    if len(out) != 3 or not all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in out):
        raise TypeError(f"{name} must hold three numbers")
    return out


@dataclass(frozen=True)
class CylinderGrid:
    """CYLINDER_SPACE_MIN / CYLINDER_SPACE_MAX / CYLINDER_GRID_SIZE of the recipe (rho in metres, phi in degrees, z in metres).  The
    numbers are kept as given - integers from a YAML file stay integers - and turned into numpy arrays where the reference does it
    (:75-77), so `intervals` are the reference's doubles."""
    space_min: Tuple
    space_max: Tuple
    grid_size: Tuple

    def __post_init__(self):
        for name in ("space_min", "space_max", "grid_size"):
            object.__setattr__(self, name, _numbers(getattr(self, name), name))
        if not all(isinstance(g, int) and g >= 2 for g in self.grid_size):
            raise ValueError("grid_size must hold three integers >= 2")
        if not all(np.isfinite(self.space()).tolist()) or not all((self.intervals > 0).tolist()):
            raise ValueError("the space needs finite bounds with space_min < space_max on every axis")

    @property
    def intervals(self) -> np.ndarray:
        """semantickitti_cylinder.py:149-151: crop_range / (grid_size - 1), float64 [3]"""
        max_bound, min_bound = np.array(self.space_max), np.array(self.space_min)
        crop_range = max_bound - min_bound
        return crop_range / (np.array(self.grid_size) - 1)

    def space(self) -> np.ndarray:
        """the 9 doubles ts_cylinder_cells takes: min, max (the bounds as numpy promotes them against the float32 polar array in
        np.clip, :153) and the intervals"""
        return np.concatenate([np.array(self.space_min, dtype=np.float64), np.array(self.space_max, dtype=np.float64),
                               self.intervals.astype(np.float64)])


def _check_scans(scans):
    if not scans:
        raise ValueError("build_cylinder_batch: no scans")
    if len(scans) > 1024:
        raise ValueError("build_cylinder_batch: coordinate outside the supported range (0 <= batch < 1024, -2^17 <= x,y,z < 2^17)")
    f = None
    for s in scans:
        p, lab = s["points"], s["labels"]
        B.L.require_device(p, lab)
        if p.dtype != torch.float32 or p.ndim != 2 or p.shape[1] < 4:
            raise TypeError("points must be a float32 [n, F >= 4] tensor (x, y, z, intensity, ...)")
        if f is not None and p.shape[1] != f:
            raise ValueError("every scan of a batch must have the same number of columns")
        f = p.shape[1]
        if lab.shape != (p.shape[0],):
            raise ValueError("labels must hold one class per point")


def _finish(flags: int):
    if flags & FLAG_RANGE:
        raise ValueError("build_cylinder_batch: coordinate outside the supported range (0 <= batch < 1024, -2^17 <= x,y,z < 2^17)")
    if flags & FLAG_NONFINITE:
        raise ValueError("build_cylinder_batch: a point has a non-finite coordinate (the reference would hand astype(int) a NaN)")
    if flags & FLAG_LABEL:
        raise ValueError("build_cylinder_batch: a label is neither ignore_label nor in [0, num_classes) (an IndexError in the reference)")


def _build(points, labels, sample32, n_points: Sequence[int], names: List, grid: CylinderGrid, rec, num_classes, ignore_label,
           fresh) -> Dict:
    """rows of all samples one after the other (sample32 ascending) -> the batch dictionary; rec: float64 [B, 8] records or None;
    fresh: `points` is a copy this call made (augmented in place) and not a resident scan"""
    dev, nb = points.device, len(n_points)
    if rec is not None:
        points = augment_points(points, torch.from_numpy(rec).to(dev, non_blocking=True), sample32, out=points if fresh else None)
    # counts [B + 1] and the three error words in ONE tensor: one fill, one copy to the host
    state = torch.zeros(nb + 1 + B.CYL_FLAG_WORDS, dtype=torch.int32, device=dev)
    counts, flags = state[:nb + 1], state[nb + 1:]
    cells, point_coord, point_feature, _ = B.cylinder_cells(points, grid.space(), sample32, flags)
    index, inverse, voxel_label, _, _ = B.cylinder_voxels(cells, labels, nb, num_classes, ignore_label, counts, flags)
    host = state.cpu().numpy()                                    # the one host read of the batch
    _finish(int(host[nb + 1]) | int(host[nb + 2]) | int(host[nb + 3]))
    m = int(host[nb])
    inds = index[:m].long()
    return {"point_coord": point_coord, "voxel_coord": point_coord.index_select(0, inds),
            "point_feature": point_feature, "voxel_feature": point_feature.index_select(0, inds),
            "point_label": labels, "voxel_label": voxel_label[:m], "inverse_map": inverse,
            "num_points": torch.tensor(list(n_points), dtype=torch.int64),
            "offset": torch.from_numpy(np.cumsum(host[:nb]).astype(np.int32)).to(dev, non_blocking=True), "name": names}


def build_cylinder_batch(scans: List[Dict], grid: CylinderGrid, aug=None, num_classes: int = 20, ignore_label: int = 67) -> Dict:
    """scans[b] = dict(points = float32 [n, F >= 4] on the device (x, y, z, intensity, ...), labels = [n] integer classes, name).
    Returns `collate_batch`'s dictionary (semantickitti_cylinder.py:176-203) with its dtypes, ready for Cylinder_TS.forward:
    point_coord / voxel_coord int64 [., 4] (x, y, z, b), point_feature / voxel_feature float32 [., 5 + F], point_label / voxel_label
    / inverse_map int64 (inverse_map local to its sample), num_points int64 [B] on the host, offset int32 [B], name.
    aug: one AugParams per sample (`draw_train_params(rng, flip, scale, scale_range, jitter, rotate)`, called once per sample as
    `get_single_sample` calls `aug_points`) or None - None issues no augment launch, and the resident scans are never written.
    One ts_stage_augment at most, one ts_cylinder_cells, one ts_cylinder_voxels chain, ONE host read."""
    _check_scans(scans)
    nb = len(scans)
    rec = None if aug is None else _aug_records(aug, nb)
    n_points = [int(s["points"].shape[0]) for s in scans]
    dev = scans[0]["points"].device
    points = scans[0]["points"].contiguous() if nb == 1 else torch.cat([s["points"] for s in scans], 0)
    labels = scans[0]["labels"].long().contiguous() if nb == 1 else torch.cat([s["labels"] for s in scans], 0).long()
    return _build(points, labels, rows_index32(n_points, dev), n_points, [s.get("name", "") for s in scans], grid, rec, num_classes,
                  ignore_label, fresh=nb > 1)


def build_cylinder_tta_batch(scan: Dict, votes_min: int, votes_max: int, rng, grid: CylinderGrid,
                             scale_range: Sequence[float] = (0.95, 1.05), num_classes: int = 20, ignore_label: int = 67) -> Dict:
    """The reference's `__getitem__` under `TTA: True` + `collate_batch_tta` (semantickitti_cylinder.py:92-99, :126-142, :221-249): the
    scan `votes_max - votes_min` times as batch entries, entry i rotated by TTA_ANGLES[votes_min + i] * pi / 8 and scaled by a draw
    from `rng` (np.random.RandomState) out of `scale_range` = SCALE_AUG_RANGE - the `scale_aug_range` assignment at :129 names an
    attribute nothing reads - no flip, no translation; the draws in view order.  The scan's rows are repeated once per
    view and that copy is augmented in place, every row with its view's record; the resident scan is not written."""
    _check_scans([scan])
    votes = list(range(votes_min, votes_max))
    if not votes:
        raise ValueError("build_cylinder_tta_batch: no views")
    rec = _aug_records([draw_tta_params(rng, v, scale_range) for v in votes], len(votes))
    n, f = scan["points"].shape
    points = scan["points"].contiguous().unsqueeze(0).expand(len(votes), n, f).reshape(len(votes) * n, f)
    labels = scan["labels"].long().contiguous().repeat(len(votes))
    n_points = [n] * len(votes)
    return _build(points, labels, rows_index32(n_points, points.device), n_points, [scan.get("name", "")] * len(votes), grid, rec,
                  num_classes, ignore_label, fresh=len(votes) > 1)
