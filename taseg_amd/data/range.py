"""RPVNet's inputs on the device: `range_image` and `range_pxpy` of a batch (reference SemkittiFusionDataset.get_range_image and
collate_batch, pcseg/data/dataset/semantickitti/semantickitti_fusion.py:64-114, 198-220), from the batch's point rows.

The reference builds them per sample in numpy on the host; here the whole batch is one call of ts_range_inputs (csrc/range_stage.hip)
on rows that are on the device anyway.  Values in the reference's own precisions (include/taseg_hip.h states them); the one stated
difference is the float32 arctan2, which numpy does not round correctly and the device does.  `cv2.resize` of a 64 x 2048 image to
64 x 2048 is taken to be the identity.  Out of scope: the nuScenes and Waymo fusion dataset files, and scan mixing ahead of this stage.
"""
from typing import Sequence, Tuple

import numpy as np
import torch

from taseg_amd import backend as B

__all__ = ["draw_range_cut", "build_range_inputs", "ERR_BATCH", "ERR_RING", "ERR_NONFINITE"]

ERR_BATCH, ERR_RING, ERR_NONFINITE = 1, 8, 16      # bits of the flag word, beside ts_range_plan's 1 / 2 / 4 (include/taseg_hip.h)


def draw_range_cut(rng: np.random.RandomState) -> float:
    """the random cut of one sample, `(np.random.rand() - 0.5) * 2 * np.pi` (semantickitti_fusion.py:78): ONE rand(), drawn after the
    sample's `draw_train_params` on the same generator - the reference augments the points before it builds the image"""
    return (rng.rand() - 0.5) * 2 * np.pi


def build_range_inputs(lidar, cuts: Sequence[float], hw: Tuple[int, int] = (64, 2048), batch_dict=None):
    """(range_image [B, 5, H, W] float32, range_pxpy [n, 3] float32, err [1] int32) for a collated batch's `lidar` (a SparseTensor
    on the device: F [n, >= 5] float32 = x, y, z, reflectivity, ring; C[:, -1] the sample) and one cut per sample.  With `batch_dict`
    the two are also stored under the reference's keys, the flag word under 'range_input_err'.

    Launches, whatever the batch: 2 fills (the winner table to -1, the flag word to 0), 1 copy of the cuts to the device, 1 strided
    copy of the batch column, 2 kernels (points, pixels) - 6, and no host read.  A row the stage leaves out (ERR_* bits) has
    px = py = NaN, which the model's range plan flags and drops again."""
    feats, coords = lidar.F, lidar.C
    b = len(cuts)
    cut = torch.as_tensor(np.asarray(cuts, dtype=np.float64).astype(np.float32)).to(feats.device, non_blocking=True)
    image, pxpy, err = B.range_inputs(feats.float() if feats.dtype != torch.float32 else feats, coords[:, -1].int().contiguous(), cut,
                                      b, int(hw[0]), int(hw[1]))
    if batch_dict is not None:
        batch_dict["range_image"], batch_dict["range_pxpy"], batch_dict["range_input_err"] = image, pxpy, err
    return image, pxpy, err
