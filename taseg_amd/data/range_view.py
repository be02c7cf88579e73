"""The range-view family's inputs on the device: `scan_rv`, `label_rv`, `mask_rv` and `scan_name` of a batch - what
SemkittiRangeViewDataset.__getitem__ (reference pcseg/data/dataset/semantickitti/semantickitti_rv.py:121-192) returns without
augmentation, through the default collate - from resident scans.

The reference projects every scan on the host (LaserScan.do_range_projection, laserscan.py:182-238: a norm, two inverse trigonometric
functions, an argsort by depth and four fancy assignments); here the whole batch is one call of ts_rv_project (csrc/range_view.hip).
Values in the reference's own float32 chain (include/taseg_hip.h states it); the one stated difference is the float32 arctan2 / arcsin,
which numpy does not round correctly and the device does.  Reproduced, not repaired: `mask = proj_idx > 0`, so a pixel won by a
scan's row 0 carries real values and mask 0.  Out of scope: the point augmentation of LaserScan.open_scan (drop, flip, scale, rotate,
jitter), RangeShift / RangeMix / RangePaste / RangeUnion, the ScribbleKITTI and nuScenes range datasets.
"""
from typing import Sequence, Tuple

import numpy as np
import torch

from taseg_amd import backend as B

__all__ = ["build_range_view_batch", "knn_weight", "ERR_BATCH", "ERR_PIXEL", "ERR_NONFINITE", "ERR_ORIGIN"]

ERR_BATCH, ERR_PIXEL, ERR_NONFINITE, ERR_ORIGIN = 1, 2, 16, 32      # bits of the flag word (include/taseg_hip.h: TS_RV_ERR_*)


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
