"""Moving-object augmentation of the SMSA recipe for the device data stage.

`tools/cfgs/voxel/semantic_kitti_ms/minkunet_mk34_cr10_smsa.yaml` (`DATASET: 'semantickitti_ms_ms'`, MinkUNetMs, 26 classes) trains
on `SemantickittiMsMsDataset` (R/pcseg/data/dataset/semantickitti/semantickitti_ms_ms.py), which is `semantickitti_ms.py` plus

  * the 26-class label map of semantickitti_utils_ms_ms.py: the six moving classes 252 / 253 / 254 / 255 / 259 / 258 become
    classes 20 .. 25 of their own instead of folding onto their static twins;
  * 14 PolarMix instance classes (:15; `INSTANCE_CLASSES["semantickitti_ms_ms"]` of data/mix.py);
  * `static2moving` (:305-351) and `moving2static` (:353-384), called on the sample (:152-163) and on its mix partner
    (:198-207 / :248-257) with the current scan, its FULL uint32 labels and the pose-fused, UN-FILTERED history rows, before the
    class-step mask is applied (:165), before the mix and before `aug_points_ms`.

`static2moving` picks parked trucks (raw class 18) and other-vehicles (20), slides each history scan of the object by an amount
proportional to the scan's age and relabels it moving-truck (258) / moving-other-vehicle (259); `moving2static` collapses moving
bicyclists (253) and motorcyclists (255) onto the spot of the current scan and relabels them 31 / 32.  The same split as
data/mix.py and data/augment.py:

  device  per-instance statistics of the un-shifted clouds (ts_stage_moving_stats, csrc/moving.hip: counts, extents, numpy's
          float32 means in numpy's summation order) - both passes touch disjoint rows (an instance is a FULL label), so one table
          serves both - and the per-row shifts and the relabelling (ts_stage_moving_apply);
  host    the random draws, in the reference's order and with its calls on a `np.random.RandomState` (`draw_moving_params`,
          `draw_smsa_sample`), the branch decisions on the float32 statistics, the float32 subtraction of two means.

What the reference does, reproduced and not repaired: `np.random.choice(MAUG_PROB, 1)` is drawn for every candidate, before its
rows are counted; an instance without a history row at frame offset -1 gets a NaN shift in `moving2static` (the mean of nothing):
its history rows become NaN and fall to the clamp; the class-step filter enumerates FLEXIBLE_STEPS, 20 entries for 26 classes
(:441), so classes 20 .. 25 are never taken from history.
"""
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import mix as M

__all__ = ["LEARNING_MAP", "LEARNING_MAP_INV", "CLASS_NAMES", "NUM_CLASSES", "LABEL_TABLE", "CANONICAL_CLASS", "STATIC_CLASSES",
           "MOVING_CLASSES", "NONE", "S2M_X", "S2M_Y", "M2S", "RECORD", "MovingTable", "MovingRecord", "MovingParams",
           "pairwise_sum", "numpy_mean", "draw_moving_params", "draw_smsa_sample", "pack_moving", "pad_steps"]

# the published semantic-kitti label definition with the moving classes kept apart (semantic-kitti-all.yaml's idea; the reference's
# copy is semantickitti_utils_ms_ms.py): raw id -> training class, class -> canonical raw id
LEARNING_MAP = {0: 0, 1: 0, 10: 1, 11: 2, 13: 5, 15: 3, 16: 5, 18: 4, 20: 5, 30: 6, 31: 7, 32: 8, 40: 9, 44: 10, 48: 11, 49: 12,
                50: 13, 51: 14, 52: 0, 60: 9, 70: 15, 71: 16, 72: 17, 80: 18, 81: 19, 99: 0,
                252: 20, 253: 21, 254: 22, 255: 23, 256: 5, 257: 5, 258: 25, 259: 24}
LEARNING_MAP_INV = {0: 0, 1: 10, 2: 11, 3: 15, 4: 18, 5: 20, 6: 30, 7: 31, 8: 32, 9: 40, 10: 44, 11: 48, 12: 49, 13: 50, 14: 51,
                    15: 70, 16: 71, 17: 72, 18: 80, 19: 81, 20: 252, 21: 253, 22: 254, 23: 255, 24: 259, 25: 258}
# semantickitti_voxel_ms_ms.py:27-33
CLASS_NAMES = ("unlabeled", "car", "bicycle", "motorcycle", "truck", "other-vehicle", "person", "bicyclist", "motorcyclist", "road",
               "parking", "sidewalk", "other-ground", "building", "fence", "vegetation", "trunk", "terrain", "pole", "traffic-sign",
               "moving-car", "moving-bicyclist", "moving-person", "moving-motorcyclist", "moving-other-vehicle", "moving-truck")
NUM_CLASSES = len(CLASS_NAMES)

LABEL_TABLE = np.zeros(260, dtype=np.int64)              # raw class -> training class (the lut of ts_stage_moving_apply)
for _k, _v in LEARNING_MAP.items():
    LABEL_TABLE[_k] = _v
CANONICAL_CLASS = np.full(260, -1, dtype=np.int64)       # raw class -> class whose canonical id it is (else -1): the pseudo class
for _c, _raw in LEARNING_MAP_INV.items():
    CANONICAL_CLASS[_raw] = _c

STATIC_CLASSES = {18: 258, 20: 259}                      # static2moving: raw class -> the raw class it becomes (:346-349)
MOVING_CLASSES = {253: 31, 255: 32}                      # moving2static (:379-382)
NONE, S2M_X, S2M_Y, M2S = 0, 1, 2, 3
RECORD = 8                                               # TS_MOVING_RECORD of include/taseg_hip.h
_CHUNK, _LEAF = 8192, 128


@dataclass
class MovingTable:
    """The per-instance statistics of one cloud, read back from the device (`stage.moving_tables`): labels int64 [k] the
    candidates - the distinct full labels of the current rows with raw class 18, 20, 253 or 255, ascending; counts int32 [k, 3]
    (rows in the current scan, in the history, at frame offset -1); stats float32 [k, 9] (min x, max x, min y, max y of the history
    rows, mean history y, mean x / y at frame offset -1, mean current x / y); n_history: the cloud's history rows (0: the frame has
    no predecessor, neither pass runs)."""
    labels: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int64))
    counts: np.ndarray = field(default_factory=lambda: np.zeros((0, 3), dtype=np.int32))
    stats: np.ndarray = field(default_factory=lambda: np.zeros((0, 9), dtype=np.float32))
    n_history: int = 0


@dataclass(frozen=True)
class MovingRecord:
    """One instance that moves.  label: its full label; kind S2M_X / S2M_Y / M2S; center: the signed centre shift added to y
    (S2M_X; 0.0: none); shift: shift_x / shift_y of static2moving (float64); shift_x, shift_y: the float32 shifts of moving2static;
    new_class: the raw class its rows get."""
    label: int
    kind: int
    center: float = 0.0
    shift: float = 0.0
    shift_x: float = 0.0
    shift_y: float = 0.0
    new_class: int = 0


@dataclass(frozen=True)
class MovingParams:
    """The moving-object augmentation of one cloud: the instances that move, ascending by label (`records`), and what was drawn for
    every candidate, in order: (pass 0 / 1, label, the `choice(MAUG_PROB, 1)` value, the `rand()` values that followed)."""
    records: Tuple[MovingRecord, ...] = ()
    draws: Tuple[tuple, ...] = ()


def pairwise_sum(a: Sequence[float]) -> np.float32:
    """numpy's pairwise sum of float32 terms (`pairwise_sum` of numpy's loops_utils.h.src), in plain Python: fewer than 8 terms
    sequentially from 0; up to 128 eight running sums over groups of 8, combined ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)),
    the remainder sequentially; above that split at n / 2 rounded down to a multiple of 8."""
    n = len(a)
    f = np.float32
    if n < 8:
        res = f(0.0)
        for v in a:
            res = f(res + f(v))
        return res
    if n <= _LEAF:
        r = [f(a[j]) for j in range(8)]
        top = n - n % 8
        for i in range(8, top, 8):
            for j in range(8):
                r[j] = f(r[j] + f(a[i + j]))
        res = f(f(f(r[0] + r[1]) + f(r[2] + r[3])) + f(f(r[4] + r[5]) + f(r[6] + r[7])))
        for i in range(top, n):
            res = f(res + f(a[i]))
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return f(pairwise_sum(a[:n2]) + pairwise_sum(a[n2:]))


def numpy_mean(a: Sequence[float]) -> np.float32:
    """`column.mean()` of a strided float32 column as numpy evaluates it - the rule of ts_stage_moving_stats: the rows in pieces
    of 8192, each summed by `pairwise_sum`, the pieces' sums added in order, the total divided by float32(n) (NaN for n = 0)."""
    a = np.asarray(a, dtype=np.float32)
    total = np.float32(0.0)
    for c in range(0, len(a), _CHUNK):
        total = np.float32(total + pairwise_sum(a[c:c + _CHUNK]))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(total / np.float32(len(a)))


def draw_moving_params(rng: np.random.RandomState, table: Optional[MovingTable], maug_prob: int = 4, shift_x_range: float = 4.0,
                       shift_y_range: float = 4.0) -> MovingParams:
    """The moving-object augmentation of one cloud, consuming `rng` exactly as one `static2moving` + `moving2static` call pair
    consumes numpy's global generator (semantickitti_ms_ms.py:152-163, :305-384).  Per candidate of the pass's classes, ascending by
    full label (np.unique): `choice(maug_prob, 1)` always; on a 1 and with history rows, static2moving draws `rand()` for the centre
    shift (only along x, only for center_y > 4 or < -2) and `rand()` for the shift; moving2static draws nothing more.  table: the
    cloud's MovingTable (None or one without history rows: no pass runs, nothing is drawn)."""
    if table is None or table.n_history <= 0 or len(table.labels) == 0:
        return MovingParams()
    records, draws = [], []
    raw = table.labels & 0xFFFF
    for which, classes in ((0, STATIC_CLASSES), (1, MOVING_CLASSES)):
        # (:152 / :158: the pass runs when the current scan has a row of its classes - when it has a candidate)
        for k in [i for i in range(len(table.labels)) if int(raw[i]) in classes]:
            label, (n_cur, n_hist, _) = int(table.labels[k]), (int(v) for v in table.counts[k])
            coin = int(rng.choice(maug_prob, 1)[0])
            drawn = []
            st = table.stats[k]
            if coin == 1 and n_hist > 0 and which == 0:
                if np.float32(st[1] - st[0]) > np.float32(st[3] - st[2]):        # :320, float32 extents, strict
                    center_y, center = st[4], 0.0
                    if center_y > 4 or center_y < -2:
                        drawn.append(float(rng.rand()))
                        center = 2 + drawn[-1] * 3
                        center = -center if center_y > 4 else center
                    drawn.append(float(rng.rand()))
                    records.append(MovingRecord(label, S2M_X, center=float(center), shift=drawn[-1] * shift_x_range + 0.5,
                                                new_class=classes[int(raw[k])]))
                else:
                    drawn.append(float(rng.rand()))
                    records.append(MovingRecord(label, S2M_Y, shift=drawn[-1] * shift_y_range + 0.5, new_class=classes[int(raw[k])]))
            if coin == 1 and n_hist > 0 and n_cur >= 20 and which == 1:
                with np.errstate(invalid="ignore"):
                    sx, sy = np.float32(st[5] - st[7]), np.float32(st[6] - st[8])   # :369-370, float32
                records.append(MovingRecord(label, M2S, shift_x=float(sx), shift_y=float(sy), new_class=classes[int(raw[k])]))
            draws.append((which, label, coin, tuple(drawn)))
    return MovingParams(tuple(sorted(records, key=lambda r: r.label)), tuple(draws))


def draw_smsa_sample(rng: np.random.RandomState, omega: Sequence[float], table: Optional[MovingTable],
                     partner_table: Optional[MovingTable] = None, augment: str = "GlobalAugment_LP", training: bool = True,
                     degrees: bool = False, maug_prob: int = 4, shift_x_range: float = 4.0, shift_y_range: float = 4.0):
    """(MovingParams, MixParams, the partner's MovingParams) of one SMSA training sample, in the reference's order
    (semantickitti_ms_ms.py:152-289): the sample's static2moving and moving2static draws, the mix coin, - when the sample is
    mixed - the PARTNER's two passes, then the strategy draw or the three PolarMix draws.  Follow with `draw_train_params` on the
    same `rng`.  Outside training nothing moves and nothing is mixed; the coin is still drawn."""
    kw = dict(maug_prob=maug_prob, shift_x_range=shift_x_range, shift_y_range=shift_y_range)
    moving = draw_moving_params(rng, table, **kw) if training else MovingParams()
    prob = M.draw_coin(rng)
    mixed = training and augment == "GlobalAugment_LP"
    partner = draw_moving_params(rng, partner_table, **kw) if mixed else MovingParams()
    mix = M.draw_mix_after_coin(rng, prob, omega, augment=augment, training=training, dataset="semantickitti_ms_ms", degrees=degrees)
    return moving, mix, partner


def pack_moving(params: Sequence[Optional[MovingParams]]):
    """(rec_labels int64 [R], rec_start int32 [C + 1], records float64 [R, RECORD]) of ts_stage_moving_apply for the clouds of a
    call, one MovingParams (or None) per cloud"""
    labels, start, rows = [], [0], []
    for p in params:
        for r in sorted(p.records, key=lambda r: r.label) if p is not None else ():
            labels.append(r.label)
            rows.append([r.kind, r.center, r.shift, r.shift_x, r.shift_y, r.new_class, 0.0, 0.0])
        start.append(len(labels))
    return (np.asarray(labels, dtype=np.int64), np.asarray(start, dtype=np.int32),
            np.asarray(rows, dtype=np.float64).reshape(-1, RECORD))


def pad_steps(steps: Sequence[int]) -> List[int]:
    """FLEXIBLE_STEPS for all 26 classes: the recipe lists 20 and the reference enumerates the list (:441) - a class past its end
    is never taken from history, as with step 0"""
    steps = [int(s) for s in steps]
    return steps + [0] * max(NUM_CLASSES - len(steps), 0)
