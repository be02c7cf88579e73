"""The range-view family's inputs on the device: `scan_rv`, `label_rv`, `mask_rv` and `scan_name` of a batch - what
SemkittiRangeViewDataset.__getitem__ (reference pcseg/data/dataset/semantickitti/semantickitti_rv.py:121-192) returns without
augmentation, through the default collate - from resident scans.

The reference projects every scan on the host (LaserScan.do_range_projection, laserscan.py:182-238: a norm, two inverse trigonometric
functions, an argsort by depth and four fancy assignments); here the whole batch is one call of ts_rv_project (csrc/range_view.hip).
Values in the reference's own float32 chain (include/taseg_hip.h states it); the one stated difference is the float32 arctan2 / arcsin,
which numpy does not round correctly and the device does.  Reproduced, not repaired: `mask = proj_idx > 0`, so a pixel won by a
scan's row 0 carries real values and mask 0.

The training form (`build_range_view_train_batch`) adds what the family's recipes switch on: the point augmentation of
LaserScan.open_scan (laserscan.py:104-143: drop, flip, scale, rotate, jitter), RangeShift, RangeMix (MixTeacherSemkitti), RangePaste
and RangeUnion.  The reference's random draws are made on the host, by `draw_range_view_params`, in its order and with its calls; all
per-point and per-pixel work is ts_rv_augment, ts_rv_project, ts_rv_label_counts and ts_rv_compose.  Reproduced, not repaired: the
scale touches x and y only; on the `< 0.5` branch the factor is the constant 1 / 1.05, not the reciprocal of the draw;
`'truck' 'other-vehicle'` in `instance_list` is one string and the list is unused.  Out of scope: the ScribbleKITTI and nuScenes
range datasets.
"""
import dataclasses
import re
from typing import Callable, Optional, Sequence, Tuple

import numpy as np
import torch

from taseg_amd import backend as B

__all__ = ["build_range_view_batch", "build_range_view_train_batch", "draw_range_view_params", "RangeViewAug", "mix_bounds",
           "MIX_STRATEGIES", "knn_weight", "ERR_BATCH", "ERR_PIXEL", "ERR_NONFINITE", "ERR_ORIGIN", "ERR_DROP"]

ERR_BATCH, ERR_PIXEL, ERR_NONFINITE, ERR_ORIGIN = 1, 2, 16, 32      # bits of the flag word (include/taseg_hip.h: TS_RV_ERR_*)
ERR_DROP = 64


def knn_weight(search: int, sigma: float) -> torch.Tensor:
    """`1 - get_gaussian_kernel(search, sigma, 1)` flattened [search * search] float32, with the reference's own torch expression on
    the CPU (range/utils.py:275-288, :320) - the kernel's weights are then the reference's bits"""
    import math
    x_coord = torch.arange(search)
    x_grid = x_coord.repeat(search).view(search, search)
    xy_grid = torch.stack([x_grid, x_grid.t()], dim=-1).float()
    mean, variance = (search - 1) / 2., sigma ** 2.
    g = (1. / (2. * math.pi * variance)) * torch.exp(-torch.sum((xy_grid - mean) ** 2., dim=-1) / (2 * variance))
    g = g / torch.sum(g)
    return (1 - g.view(search, search)).reshape(-1).float()


def build_range_view_batch(scans: Sequence[dict], hw: Tuple[int, int] = (64, 512), fov: Tuple[float, float] = (3.0, -25.0),
                           batch_dict=None):
    """The collated range-view batch of resident scans.  Every scan is a dict with `points` [n, >= 4] float32 on the device (x, y, z,
    remission), optionally `labels` [n] (mapped training labels) and `name`.  Returns a dict under the reference's keys

        scan_rv [B, 6, H, W] float32, label_rv [B, 1, H, W] int64 (when every scan has labels), mask_rv [B, 1, H, W] float32,
        scan_name (the names)

    and what the kNN step needs: proj_range [B, H, W], proj_x / proj_y [n] int32, unproj_range [n] float32, batch [n] int32,
    offset [B + 1] int64 (host: the scans' row ranges), proj_idx [B, H, W] int32, point_labels [n] int32 (with labels) and the flag
    word `range_view_err` [1] int32 (ERR_* bits).  With `batch_dict` the entries are stored there too.

    Launches, whatever the batch: 2 fills (the winner table to all ones, the flag word to 0), 1 copy each of the scans' first rows
    and batch indices to the device, 1 concatenation of the rows when there is more than one scan (and 1 of the labels), 2 kernels
    (points, pixels) - at most 8, and no host read; `mask_rv` is a view of `scan_rv`."""
    if len(scans) == 0:
        raise ValueError("build_range_view_batch: no scans")
    pts = [s["points"] for s in scans]
    dev = pts[0].device
    lens = [int(p.shape[0]) for p in pts]
    offset = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    feat = pts[0] if len(pts) == 1 else torch.cat([p[:, :4] for p in pts])
    if feat.dtype != torch.float32:
        feat = feat.float()
    with_labels = all(s.get("labels") is not None for s in scans)
    label = None
    if with_labels:
        labs = [torch.as_tensor(s["labels"]).to(dev).reshape(-1).int() for s in scans]
        label = labs[0] if len(labs) == 1 else torch.cat(labs)
    b = len(scans)
    first = torch.from_numpy(offset[:-1].astype(np.int32)).to(dev, non_blocking=True)
    batch = torch.from_numpy(np.repeat(np.arange(b, dtype=np.int32), lens)).to(dev, non_blocking=True)
    out = B.rv_project(feat, batch, first, b, int(hw[0]), int(hw[1]), float(fov[0]), float(fov[1]), label=label)
    res = {"scan_rv": out["scan_rv"], "mask_rv": out["scan_rv"][:, 5:6], "scan_name": [s.get("name") for s in scans],
           "proj_range": out["proj_range"], "proj_idx": out["proj_idx"], "proj_x": out["proj_x"], "proj_y": out["proj_y"],
           "unproj_range": out["unproj_range"], "batch": batch, "offset": torch.from_numpy(offset), "range_view_err": out["err"]}
    if with_labels:
        res["label_rv"], res["point_labels"] = out["label_rv"], label
    if batch_dict is not None:
        batch_dict.update(res)
    return res


# ------------------------------------------------------------------------------------------------------- training form
# MixTeacherSemkitti.forward (semantickitti_rv.py:383-392): the names np.random.choice draws from, in its order
MIX_STRATEGIES = {
    "mixture": ["col1row2", "col1row3", "col2row1", "col3row1", "col2row2", "col1row4", "col2row4"],
    "mixtureV2": ["col1row3", "col1row4", "col1row5", "col1row6", "col2row3", "col2row4", "col2row5", "col2row6", "col3row3",
                  "col3row4", "col3row5", "col3row6", "col4row3", "col4row4", "col4row5", "col4row6", "col6row4"],
}
# the methods the class defines (:481-1700); cutmix / cutout / mixup are dispatched (:466-473) but not defined
_MIX_DEFINED = {"col%drow%d" % (c, r) for c in (1, 2, 3, 4) for r in (1, 2, 3, 4, 5, 6)} - {"col1row1"} | {"col6row4"}


@dataclasses.dataclass
class RangeViewAug:
    """The nine switches of a range-view recipe (tools/cfgs/range/*.yaml: IF_DROP .. IF_JITTER booleans, IF_RANGE_MIX / SHIFT / PASTE /
    UNION probabilities) and the RangeMix strategy the dataset class fixes (semantickitti_rv.py:100)."""
    drop: bool = False
    flip: bool = False
    scale: bool = False
    rotate: bool = False
    jitter: bool = False
    range_mix: float = 0.0
    range_shift: float = 0.0
    range_paste: float = 0.0
    range_union: float = 0.0
    strategy: str = "mixtureV2"

    @classmethod
    def recipe(cls):
        """salsanext_res34.yaml"""
        return cls(True, True, True, True, True, 0.9, 0.9, 0.9, 0.0)


def _check_strategy(name):
    if name in MIX_STRATEGIES:
        return
    if name in ("cutmix", "cutout", "mixup"):
        raise ValueError("RangeMix strategy '%s' is dispatched but not defined in the reference" % name)
    if name not in _MIX_DEFINED:
        raise ValueError("unknown RangeMix strategy '%s'" % name)


def mix_bounds(strategy: str, h: int, w: int):
    """(row bounds, column bounds) of a colCrowR strategy, with the reference's own expressions per method: int(size / R) and its
    multiples; the middle bound of a 4-way split is int(size / 2) where the method writes it so (col1row4, col2row4; every col4*),
    2 * int(size / 4) elsewhere (col3row4, col4row4, col6row4); col6row4 takes int(W / 4) and its multiples up to 5 W / 4 - a bound
    at or beyond the size selects nothing."""
    _check_strategy(strategy)
    m = re.fullmatch(r"col(\d)row(\d)", strategy)
    if m is None:
        raise ValueError("mix_bounds: '%s' names a set of strategies, not one" % strategy)
    c, r = int(m.group(1)), int(m.group(2))
    if r == 4:
        h1 = int(h / 4)
        rows = [h1, int(h / 2) if c in (1, 2) else 2 * h1, 3 * h1]
    else:
        rows = [k * int(h / r) for k in range(1, r)]
    if c == 4:
        w1 = int(w / 4)
        cols = [w1, int(w / 2), 3 * w1]
    elif c == 6:
        cols = [k * int(w / 4) for k in range(1, 6)]
    else:
        cols = [k * int(w / c) for k in range(1, c)]
    return rows, cols


def _draw_scan(aug, n, rs):
    """the draws of one LaserScan.open_scan (laserscan.py:104-143) on a scan of n rows"""
    d = {"n": int(n), "drop": None, "flip": None, "scale": None, "rotate": None, "jitter": None}
    if aug.drop:
        max_num_drop = int(n * 0.1)
        if max_num_drop <= 0:
            raise ValueError("draw_range_view_params: drop needs a scan of at least 10 rows (got %d)" % n)
        num_drop = rs.randint(low=0, high=max_num_drop)
        d["drop"] = np.unique(rs.randint(low=0, high=n - 1, size=num_drop)).astype(np.int64)
    if aug.flip:
        d["flip"] = int(rs.choice(4, 1)[0])
    if aug.scale:
        scale = 1.05
        rand_scale = rs.uniform(1, scale)
        if rs.random_sample() < 0.5:
            rand_scale = 1 / scale
        d["scale"] = float(rand_scale)
    if aug.rotate:
        rotate_rad = np.deg2rad(rs.random_sample() * 360)
        d["rotate"] = (float(np.cos(rotate_rad)), float(np.sin(rotate_rad)))
    if aug.jitter:
        jitter = 0.1
        d["jitter"] = np.clip(rs.normal(0, jitter, 3), -3 * jitter, 3 * jitter)
    return d


def draw_range_view_params(aug: RangeViewAug, index: int, n_scans: int, n_points_of: Callable[[int], int], rs, pyr,
                           hw: Tuple[int, int] = (64, 512)) -> dict:
    """The random draws of ONE SemkittiRangeViewDataset.__getitem__(index) in training (semantickitti_rv.py:121-183), in the
    reference's order and with its calls, from rs (a numpy.random.RandomState: the reference's np.random) and pyr (a random.Random:
    its `random`, used for the split points only) - RandomState(s) / Random(s) reproduce np.random.seed(s) / random.seed(s).
    n_points_of(i): the row count of scan i (the partner's drop draw depends on it).  Returns

        index, partner (None without mix / paste / union), scan / partner_scan: {n, drop (np.unique of the draws: sorted indices, or
        None), flip (0 .. 3), scale (float), rotate ((cos, sin)), jitter (float64 [3])} - None where the switch is off -
        shift / partner_shift (0: none), strategy (the name, None without mix), mixture (0, 1, 2), paste, union (bools)

    A draw whose switch is off is not made where the reference does not make it (the point augmentation) and made and discarded where
    it does (shift, and mix / paste / union once any of the three is above 0).  ValueError before any draw: W < 200 with shift on,
    an undefined strategy name; a scan of fewer than 10 rows with drop on raises at its draw, as the reference's randint does."""
    w = int(hw[1])
    if aug.range_shift > 0 and w < 200:
        raise ValueError("draw_range_view_params: RangeShift draws its split from [100, W - 100]: W >= 200 (got %d)" % w)
    if aug.range_mix > 0:
        _check_strategy(aug.strategy)
    out = {"index": int(index), "partner": None, "partner_scan": None, "shift": 0, "partner_shift": 0, "strategy": None, "mixture": 0,
           "paste": False, "union": False}
    out["scan"] = _draw_scan(aug, n_points_of(index), rs)
    if rs.random_sample() >= (1 - aug.range_shift):
        out["shift"] = pyr.randint(100, w - 100)
    if aug.range_mix > 0 or aug.range_paste > 0 or aug.range_union > 0:
        idx = int(rs.randint(0, n_scans))
        out["partner"] = idx
        out["partner_scan"] = _draw_scan(aug, n_points_of(idx), rs)
        if rs.random_sample() >= (1 - aug.range_shift):
            out["partner_shift"] = pyr.randint(100, w - 100)
        if rs.random_sample() >= (1 - aug.range_mix):
            if aug.strategy in MIX_STRATEGIES:
                out["strategy"] = str(rs.choice(MIX_STRATEGIES[aug.strategy], size=1)[0])
            else:
                out["strategy"] = aug.strategy
            out["mixture"] = 1 if rs.random_sample() >= 0.5 else 2
        out["paste"] = bool(rs.random_sample() >= (1 - aug.range_paste))
        out["union"] = bool(rs.random_sample() >= (1 - aug.range_union))
    return out


def aug_record(d: Optional[dict]) -> np.ndarray:
    """one TS_RV_AUG_RECORD of doubles { c, s, scale, tx, ty, tz, bits, flip } from a scan's draws"""
    rec = np.zeros(B.RV_AUG_RECORD, dtype=np.float64)
    if d is None:
        return rec
    bits = 0
    if d.get("rotate") is not None:
        rec[0], rec[1] = d["rotate"]
        bits |= 1
    if d.get("scale") is not None:
        rec[2] = d["scale"]
        bits |= 2
    if d.get("flip") is not None:
        rec[7] = d["flip"]
        bits |= 4
    if d.get("jitter") is not None:
        rec[3:6] = d["jitter"]
        bits |= 8
    rec[6] = bits
    return rec


def compose_record(p: dict, h: int, w: int) -> np.ndarray:
    """one TS_RV_COMPOSE_RECORD of int32 { shift_a, shift_b, n_row_bounds, n_col_bounds, row_bounds[5], col_bounds[5], mixture,
    flags } from a sample's draws"""
    rec = np.zeros(B.RV_COMPOSE_RECORD, dtype=np.int32)
    for k, key in enumerate(("shift", "partner_shift")):
        s = int(p.get(key) or 0)
        if s < 0 or s >= w:
            raise ValueError("range view: a shift lies in [0, W) (got %d)" % s)
        rec[k] = s
    mixture = int(p.get("mixture") or 0)
    if mixture not in (0, 1, 2):
        raise ValueError("range view: mixture is 0, 1 or 2 (got %d)" % mixture)
    if mixture:
        rows, cols = mix_bounds(p["strategy"], h, w)
        rec[2], rec[3] = len(rows), len(cols)
        rec[4:4 + len(rows)] = rows
        rec[9:9 + len(cols)] = cols
    rec[14] = mixture
    rec[15] = (1 if p.get("paste") else 0) | (2 if p.get("union") else 0)
    return rec


def build_range_view_train_batch(scans: Sequence[dict], partners: Optional[Sequence[dict]], params: Sequence[dict],
                                 hw: Tuple[int, int] = (64, 512), fov: Tuple[float, float] = (3.0, -25.0)):
    """The collated TRAINING batch of the range-view family from resident scans: what SemkittiRangeViewDataset.__getitem__ returns
    with its augmentation on, through the default collate.  scans: the B primaries, dicts with `points` [n, >= 4] float32 on the
    device, `labels` [n] (mapped training labels) and `name`; partners: the B scans the draws chose (params[i]["partner"]), or None
    when mix, paste and union are all at 0 - then B clouds are projected and only the point augmentation and the shift apply;
    params: one `draw_range_view_params` result per sample.  Returns

        scan_rv [B, 6, H, W] float32, label_rv [B, 1, H, W] int64, mask_rv [B, 1, H, W] float32 (a view of scan_rv's channel 5),
        scan_name (the primaries' names), range_view_err [1] int32 (ERR_* bits; ERR_DROP: a drop index outside its cloud)

    The 2B clouds (B primaries, then B partners) go through ONE ts_rv_augment and ONE ts_rv_project call with 2B as the batch size;
    the stable compaction behind the drop takes at most 64 clouds, so B <= 32 with partners (the recipe's 30 per GPU gives 60) and
    B <= 64 without: more raises ValueError before any launch.  The resident scans are never written.

    Launches, whatever the batch, with partners and every switch on: 2 concatenations (rows, labels; int32 labels are not cast),
    6 copies to the device (batch indices, the input clouds' first rows, the augmentation records, the drop lists behind their
    offsets, the survivors' first rows, the compose records), 4 fills (flag word, keep bytes, winner table, class counts) and 8
    kernels (drop, count, scan, scatter; points, pixels; label counts; compose) - 20.  Without drop 2 fewer (lists, keep bytes) and
    no drop kernel; without any point augmentation ts_rv_augment is not called; without partners no class counts, and no compose
    unless a sample is shifted.  No host read: the survivors' first rows come from the lengths of the unique drop lists, which the
    host drew."""
    h, w = int(hw[0]), int(hw[1])
    nb = len(scans)
    if nb == 0:
        raise ValueError("build_range_view_train_batch: no scans")
    if len(params) != nb or (partners is not None and len(partners) != nb):
        raise ValueError("build_range_view_train_batch: one parameter set (and one partner) per scan")
    clouds = list(scans) + (list(partners) if partners is not None else [])
    nc = len(clouds)
    if nc > B.RV_MAX_CLOUDS:
        raise ValueError("build_range_view_train_batch: at most %d clouds in one call (got %d)" % (B.RV_MAX_CLOUDS, nc))
    draws = [p.get("scan") for p in params] + ([p.get("partner_scan") for p in params] if partners is not None else [])
    for p in params:
        if partners is None and (p.get("mixture") or p.get("paste") or p.get("union")):
            raise ValueError("build_range_view_train_batch: mix, paste and union need the partners")
    records = np.stack([compose_record(p, h, w) for p in params])
    pts = [s["points"] for s in clouds]
    B.L.require_device(*pts)
    if any(s.get("labels") is None for s in clouds):
        raise ValueError("build_range_view_train_batch: every scan needs its labels")
    dev = pts[0].device
    lens = np.array([int(p.shape[0]) for p in pts], dtype=np.int64)
    for d, n in zip(draws, lens):
        if d is not None and d.get("drop") is not None and len(d["drop"]) and (d["drop"][0] < 0 or d["drop"][-1] >= n):
            raise ValueError("build_range_view_train_batch: a drop index outside its scan of %d rows" % n)
    drops = [np.asarray(d["drop"], dtype=np.int64) if d is not None and d.get("drop") is not None else None for d in draws]
    with_drop = any(d is not None for d in drops)
    aug = np.stack([aug_record(d) for d in draws])
    with_aug = with_drop or bool(aug[:, 6].any())
    feat = pts[0] if nc == 1 else torch.cat([p[:, :4] for p in pts])
    if feat.dtype != torch.float32:
        feat = feat.float()
    labs = [torch.as_tensor(s["labels"]).to(dev).reshape(-1).int() for s in clouds]
    label = labs[0] if nc == 1 else torch.cat(labs)
    first_in = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    batch = torch.from_numpy(np.repeat(np.arange(nc, dtype=np.int32), lens)).to(dev, non_blocking=True)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    first = first_in
    if with_aug:
        kept = lens - np.array([0 if d is None else len(d) for d in drops], dtype=np.int64)
        first = np.concatenate([[0], np.cumsum(kept)[:-1]]).astype(np.int32)
        drop_t = off_t = None
        if with_drop:
            off = np.concatenate([[0], np.cumsum([0 if d is None else len(d) for d in drops])]).astype(np.int32)
            lists = np.concatenate([off] + [d.astype(np.int32) for d in drops if d is not None])
            both = torch.from_numpy(lists).to(dev, non_blocking=True)                    # one copy: the offsets, then the lists
            off_t, drop_t = both[:nc + 1], both[nc + 1:]
        feat, label, batch, _, _ = B.rv_augment(feat, batch, torch.from_numpy(first_in).to(dev, non_blocking=True), nc,
                                                torch.from_numpy(aug).to(dev, non_blocking=True), label=label, drop=drop_t,
                                                drop_off=off_t, err=err)
        n_kept = int(kept.sum())
        feat, label, batch = feat[:n_kept], label[:n_kept], batch[:n_kept]
    out = B.rv_project(feat, batch, torch.from_numpy(first).to(dev, non_blocking=True), nc, h, w, float(fov[0]), float(fov[1]),
                       label=label, err=err)
    scan_rv, label_rv = out["scan_rv"], out["label_rv"]
    if partners is not None or records[:, :2].any():
        rec_t = torch.from_numpy(records).to(dev, non_blocking=True)
        if partners is not None:
            counts = B.rv_label_counts(label_rv[nb:])
            scan_rv, label_rv = B.rv_compose(scan_rv[:nb], label_rv[:nb], rec_t, scan_rv[nb:], label_rv[nb:], counts)
        else:
            scan_rv, label_rv = B.rv_compose(scan_rv, label_rv, rec_t)
    return {"scan_rv": scan_rv, "label_rv": label_rv, "mask_rv": scan_rv[:, 5:6], "scan_name": [s.get("name") for s in scans],
            "range_view_err": err}
