"""Scan mixing of the training recipe - PolarMix and LaserMix - for the device data stage.

Under `AUGMENT: 'GlobalAugment_LP'` the reference mixes every training sample with a second, randomly paired scan BEFORE
`aug_points_ms`, the clamp and both voxelisations (R/pcseg/data/dataset/semantickitti/semantickitti_ms.py:151-237 with
PolarMix_semantickitti.py and LaserMix_semantickitti.py; nuscenes/nuscenes_ms.py:132-214 with the nuScenes twins).  The same
split as data/augment.py:

  host    the random draws, in the reference's order and with the reference's calls on a `np.random.RandomState`
          (`draw_omega`, `draw_mix_params`), cos / sin of the two paste angles in float64, the LaserMix thresholds;
  device  the per-row work (ts_stage_mix, csrc/mix.hip): a segment id per row, a deterministic stable partition, the scatter
          with the two rotated copies of the instance rows (`mix_points`, `polarmix_points`, `lasermix_points`; the stage
          functions of data/stage.py take `mix=` / `partners=`).

What the reference does, reproduced and not repaired:

  * `prob = np.random.choice(2, 1)` is drawn for every sample, mix or not;
  * LaserMix (`prob == 1`) calls `lasermix_aug`, which compares an inclination in RADIANS with thresholds written in degrees
    (`-6.7 / np.pi * 180` is about -384): band 1 takes every row of the first cloud and the branch is the identity.  It still
    consumes its strategy draw.  `lasermix_aug_` of the same file (inclination in degrees) mixes for real: `degrees=True` here;
  * PolarMix (`prob == 0`): alpha, the swap draw and the paste draw (`np.random.random() < 1.0`: always true, still consumed);
    the SemanticKITTI file copies every column after xyz into the rotated copies, the nuScenes file only column 3 (the others
    stay 0);
  * `Omega` is drawn once, when the dataset module is imported.

The yaw of the device is `(float)(-atan2((double)y, (double)x))`, compared with `(float)alpha` and `(float)beta`; numpy's float32
arctan2 is a SIMD approximation that is not correctly rounded, so a row whose yaw lies within a few float32 ulps of a bound may
land on the other side than in the reference - the only permitted difference (and the float64 inclination of `degrees=True`
likewise at a band threshold).
"""
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

__all__ = ["MixParams", "NONE", "LASER", "POLAR", "STRATEGIES", "LASER_THRESHOLDS", "LASER_THRESHOLDS_NUSCENES", "INSTANCE_CLASSES", "MAX_CLASSES", "RECORD",
           "draw_omega", "draw_mix_params", "draw_coin", "draw_mix_after_coin", "laser_thresholds", "pack_mix", "mix_capacity",
           "mix_points", "polarmix_points", "lasermix_points"]

NONE, LASER, POLAR = 0, 1, 2
# LaserMix_semantickitti.py:29 - the list np.random.choice draws from - and the band thresholds of each strategy (:34-107)
STRATEGIES = ("inc3phi1", "inc4phi1", "inc5phi1", "inc6phi1")
LASER_THRESHOLDS = ((-6.7, -13.4), (-5.0, -10.0, -15.0), (-4.0, -8.0, -12.0, -16.0), (-3.3, -6.6, -9.9, -13.2, -16.5))
# LaserMix_nuscenes.py:116-201: the nuScenes file's `lasermix_aug_` has its own bands, no inc6phi1, and draws its strategy from the
# one-element list ['inc3phi1'] (:135); its `lasermix_aug` (:11-114) is the SemanticKITTI file's
LASER_THRESHOLDS_NUSCENES = ((0.0, -10.0), (4.0, -2.0, -10.0), (4.0, 0.0, -4.0, -12.0))
STRATEGIES_NUSCENES_DEGREES = ("inc3phi1",)
# semantickitti_ms.py:13, nuscenes_ms.py:15, semantickitti_ms_ms.py:15 (the SMSA recipe: the six moving classes too)
INSTANCE_CLASSES = {"semantickitti": tuple(range(1, 9)), "nuscenes": tuple(range(1, 11)),
                    "semantickitti_ms_ms": tuple(range(1, 9)) + tuple(range(20, 26))}
MAX_CLASSES = 16          # TS_MIX_MAX_CLASSES of include/taseg_hip.h
RECORD = 24               # TS_MIX_RECORD


@dataclass(frozen=True)
class MixParams:
    """One sample's mix.  kind NONE / LASER / POLAR; strategy 0 .. 3 (STRATEGIES) and `degrees` (False: the reference's
    `lasermix_aug`, the identity; True: `lasermix_aug_`) for LASER; alpha, beta, swap, paste, omega (the two paste angles),
    instance_classes and tail_all (True: the rotated copies carry every column after xyz, SemanticKITTI; False: only column 3,
    nuScenes) for POLAR.  prob is the drawn coin, partner the drawn partner index (nuScenes draws it, SemanticKITTI shuffles a
    list once).  dataset picks the band thresholds of a LASER record with `degrees` (`laser_thresholds`): "nuscenes" takes
    LaserMix_nuscenes.py's, which has no inc6phi1 (ValueError); everything else SemanticKITTI's."""
    kind: int = NONE
    strategy: int = 0
    degrees: bool = False
    alpha: float = 0.0
    beta: float = 0.0
    swap: bool = False
    paste: bool = False
    omega: Tuple[float, float] = (0.0, 0.0)
    instance_classes: Tuple[int, ...] = INSTANCE_CLASSES["semantickitti"]
    tail_all: bool = True
    prob: int = -1
    partner: Optional[int] = None
    dataset: str = "semantickitti"

    def __post_init__(self):
        if self.kind not in (NONE, LASER, POLAR) or not 0 <= self.strategy < len(STRATEGIES):
            raise ValueError("MixParams: bad kind / strategy")
        if self.dataset not in INSTANCE_CLASSES:
            raise ValueError("MixParams: dataset must be one of %s" % sorted(INSTANCE_CLASSES))
        if self.kind == LASER:
            laser_thresholds(self.strategy, self.degrees, self.dataset)      # (inc6phi1 under the nuScenes `lasermix_aug_`)
        cls = tuple(int(c) for c in self.instance_classes)
        if len(cls) > MAX_CLASSES or len(set(cls)) != len(cls):
            raise ValueError("MixParams: at most %d instance classes, each once" % MAX_CLASSES)
        object.__setattr__(self, "instance_classes", cls)
        object.__setattr__(self, "omega", (float(self.omega[0]), float(self.omega[1])))


def draw_omega(rng: np.random.RandomState) -> Tuple[float, float]:
    """semantickitti_ms.py:14 / nuscenes_ms.py:16: the two paste angles, two `random()` draws, once per process"""
    return (float(rng.random_sample() * np.pi * 2 / 3), float((rng.random_sample() + 1) * np.pi * 2 / 3))


def draw_mix_params(rng: np.random.RandomState, omega: Sequence[float], augment: str = "GlobalAugment_LP", training: bool = True,
                    dataset: str = "semantickitti", degrees: bool = False, n_partners: Optional[int] = None) -> MixParams:
    """The mix of one sample, consuming `rng` exactly as the reference's `__getitem__` consumes numpy's global generator
    (semantickitti_ms.py:151-237, nuscenes_ms.py:132-214): `choice(2, 1)` always; LaserMix (prob 1): `choice(strategies, size=1)`;
    PolarMix (prob 0): `random()` for alpha, `random()` for the swap, `random()` for the paste.  Under `degrees=True,
    dataset="nuscenes"` the strategy draw is LaserMix_nuscenes.py:135-136's `choice(['inc3phi1'], size=1)`.  nuScenes honours
    GlobalAugment_L / GlobalAugment_P (:135,:168) and draws the partner with `choice(len(infos))` right after the coin (:133) -
    pass `n_partners=len(infos)` to replay that draw (None: not drawn).  Follow with `draw_train_params` on the same `rng`."""
    if dataset not in INSTANCE_CLASSES:
        raise ValueError("dataset must be one of %s" % sorted(INSTANCE_CLASSES))
    return draw_mix_after_coin(rng, draw_coin(rng), omega, augment, training, dataset, degrees, n_partners)


def draw_coin(rng: np.random.RandomState) -> int:
    """`prob = np.random.choice(2, 1)`, drawn for every sample (semantickitti_ms.py:151)"""
    return int(rng.choice(2, 1)[0])


def draw_mix_after_coin(rng: np.random.RandomState, prob: int, omega: Sequence[float], augment: str = "GlobalAugment_LP",
                        training: bool = True, dataset: str = "semantickitti", degrees: bool = False,
                        n_partners: Optional[int] = None) -> MixParams:
    """draw_mix_params from the coin on: the SMSA recipe draws its partner's moving-object augmentation between the coin and the
    rest (data/moving.py `draw_smsa_sample`)"""
    if dataset not in INSTANCE_CLASSES:
        raise ValueError("dataset must be one of %s" % sorted(INSTANCE_CLASSES))
    partner = None
    if dataset == "nuscenes":
        if n_partners is not None:
            partner = int(rng.choice(int(n_partners)))
        laser_on, polar_on = augment in ("GlobalAugment_LP", "GlobalAugment_L"), augment in ("GlobalAugment_LP", "GlobalAugment_P")
    else:
        laser_on = polar_on = augment == "GlobalAugment_LP"
    common = dict(prob=prob, partner=partner, omega=tuple(omega), instance_classes=INSTANCE_CLASSES[dataset],
                  tail_all=dataset != "nuscenes", dataset=dataset)
    if training and laser_on and prob == 1:
        pool = STRATEGIES_NUSCENES_DEGREES if dataset == "nuscenes" and degrees else STRATEGIES
        return MixParams(kind=LASER, strategy=int(rng.choice(len(pool), 1)[0]), degrees=bool(degrees), **common)
    if training and polar_on and prob == 0:
        alpha = float((rng.random_sample() - 1) * np.pi)
        swap = bool(rng.random_sample() < 0.5)
        paste = bool(rng.random_sample() < 1.0)
        return MixParams(kind=POLAR, alpha=alpha, beta=float(alpha + np.pi), swap=swap, paste=paste, **common)
    return MixParams(kind=NONE, **common)


def laser_thresholds(strategy: int, degrees: bool, dataset: str = "semantickitti") -> List[float]:
    """the band thresholds as the reference writes them: `-6.7` against degrees (`lasermix_aug_`), `-6.7 / np.pi * 180` against
    radians (`lasermix_aug`, LaserMix_semantickitti.py:34).  dataset="nuscenes": `lasermix_aug_` of LaserMix_nuscenes.py:138-194
    has bands of its own (LASER_THRESHOLDS_NUSCENES) and no inc6phi1; its `lasermix_aug` is the SemanticKITTI file's."""
    if dataset == "nuscenes" and degrees:
        if strategy >= len(LASER_THRESHOLDS_NUSCENES):
            raise ValueError("%s does not exist in the nuScenes lasermix_aug_" % STRATEGIES[strategy])
        return [float(t) for t in LASER_THRESHOLDS_NUSCENES[strategy]]
    return [float(t) if degrees else float(t / np.pi * 180) for t in LASER_THRESHOLDS[strategy]]


def pack_mix(params: Sequence[MixParams], n1: Sequence[int], n2: Sequence[int]):
    """(records float64 [J, RECORD], classes int32 [J, MAX_CLASSES], blocks) of ts_stage_mix for jobs whose rows are
    concatenated job-major, cloud 1 before cloud 2 (include/taseg_hip.h)"""
    rec = np.zeros((len(params), RECORD), dtype=np.float64)
    cls = np.full((len(params), MAX_CLASSES), -1, dtype=np.int32)
    row = blk = 0
    for j, (p, a, b) in enumerate(zip(params, n1, n2)):
        a, b = int(a), int(b)
        r = rec[j]
        r[0], r[1], r[2], r[3], r[4] = p.kind, p.alpha, p.beta, p.swap, p.paste
        r[5], r[6], r[7], r[8] = np.cos(p.omega[0]), np.sin(p.omega[0]), np.cos(p.omega[1]), np.sin(p.omega[1])
        r[9], r[10] = p.tail_all, p.degrees
        if p.kind == LASER:
            thr = laser_thresholds(p.strategy, p.degrees, p.dataset)
            r[11] = len(thr)
            r[12:12 + len(thr)] = thr
        r[17], r[18], r[19] = a, b, row
        r[20] = len(p.instance_classes)
        cls[j, :len(p.instance_classes)] = p.instance_classes
        nblk = -(-(a + b) // 256)
        r[21], r[22] = blk, nblk
        row += a + b
        blk += nblk
    return rec, cls, blk


def mix_capacity(params: Sequence[MixParams], n1: Sequence[int], n2: Sequence[int]) -> int:
    """an upper bound of the rows a mix writes: cloud 1; LASER adds cloud 2; POLAR its sector rows and three copies of its
    instance rows"""
    cap = 0
    for p, a, b in zip(params, n1, n2):
        cap += int(a) + (int(b) if p.kind == LASER else (int(p.swap) + 3 * int(p.paste)) * int(b) if p.kind == POLAR else 0)
    return cap


def mix_points(pts1, lab1, pts2, lab2, params: MixParams):
    """One pair on the device: (points [m, F], labels [m] int64) of `params` applied to cloud 1 (pts1 [n1, F >= 3] float32,
    lab1 [n1]) with partner cloud 2.  Three launches and one host read (m)."""
    import torch
    from .. import backend as B
    if pts1.shape[1] != pts2.shape[1]:
        raise ValueError("both clouds must have the same columns")
    pts = torch.cat([pts1, pts2], 0).contiguous()
    lab = torch.cat([lab1.reshape(-1).long(), lab2.reshape(-1).long()], 0)
    out, out_lab, _, totals = B.stage_mix(pts, lab, [params], [pts1.shape[0]], [pts2.shape[0]])
    m = int(totals.tolist()[0])
    return out[:m], out_lab[:m]


def polarmix_points(pts1, lab1, pts2, lab2, params: MixParams):
    """PolarMix_semantickitti.py:61-96 / PolarMix_nuscenes.py:60-95 on the device: cloud 1 without its sector rows, cloud 2's
    sector rows (swap), cloud 2's instance rows grouped by class in `instance_classes` order and their two rotated copies
    (paste).  params: a POLAR record (alpha, beta, swap, paste, omega, instance_classes, tail_all)."""
    if params.kind != POLAR:
        raise ValueError("polarmix_points takes a POLAR record")
    return mix_points(pts1, lab1, pts2, lab2, params)


def lasermix_points(pts1, lab1, pts2, lab2, strategy, degrees: bool = False, dataset: str = "semantickitti"):
    """LaserMix_semantickitti.py on the device.  strategy: 0 .. 3 or its name.  degrees=False is `lasermix_aug` as both datasets
    call it (:11-114) - the identity, see the module docstring; degrees=True is `lasermix_aug_` (:116-219): inclination bands
    alternate between the clouds, concat(band 1 of cloud 1, band 2 of cloud 2, band 3 of cloud 1, ...).  dataset="nuscenes":
    `lasermix_aug_` of LaserMix_nuscenes.py (:116-201) with its own bands; inc6phi1 is a ValueError there."""
    if isinstance(strategy, str):
        strategy = STRATEGIES.index(strategy)
    return mix_points(pts1, lab1, pts2, lab2, MixParams(kind=LASER, strategy=int(strategy), degrees=bool(degrees), dataset=dataset))

