"""Point <-> voxel glue of SPVCNN (reference pcseg/model/segmentor/fusion/spvcnn/utils.py): the three functions of that file.

`initial_voxelize` and `voxel_to_point` are the MinkUNet family's (the reference keeps one copy per model).  `point_to_voxel` differs
from minkunet/utils.py::point_to_voxel - the reference chain, kept there as it is - in two ways that change no result:

  index   column 0 of the trilinear map IS the point's own cell (csrc/coords.hip: corner k = 0 is (bx, by, bz); the reference:
          `get_kernel_offsets(2)` starts at (0, 0, 0) and `point_to_voxel` hashes the same floor(z.C / s) * s), so where
          `voxel_to_point` has cached the map of a stride, idx_query is that column and counts are the run lengths of its grouping:
          no hash, no table, no query;
  sum     `spvoxelize_mean` (ts_voxelize_mean_forward: fixed summation order) in place of `spvoxelize`'s float atomics.
"""
import torch

from taseg_amd import backend as B
from taseg_amd.torchsparse import PointTensor, SparseTensor
from taseg_amd.torchsparse.nn import functional as F
from ...voxel.minkunet.utils import initial_voxelize, voxel_to_point

__all__ = ["initial_voxelize", "point_to_voxel", "voxel_to_point", "point_to_voxel_index"]


def point_to_voxel_index(x: SparseTensor, z: PointTensor):
    """(idx_query int32 [N], counts int32 [M], groups) of `z`'s points over `x`'s voxels, cached in `z` per stride like the reference's
    idx_query / counts (utils.py:42-57); groups = backend.point_groups(idx_query, M), what `spvoxelize_mean` walks."""
    cache = z.additional_features
    groups = cache.setdefault("groups", {})
    if cache["idx_query"].get(x.s) is None or groups.get(x.s) is None:
        tri = z.idx_query.get(x.s) if z.idx_query is not None else None
        if tri is not None:
            idx_query = tri[:, 0].int().contiguous()
        else:
            s = x.s[0]
            cell = torch.cat([torch.floor(z.C[:, :3] / s).int() * s, z.C[:, -1].int().view(-1, 1)], 1)
            idx_query = F.sphashquery(F.sphash(cell), F.sphash(x.C)).int()
        offsets, entries = B.point_groups(idx_query, x.C.shape[0])
        cache["idx_query"][x.s] = idx_query
        cache["counts"][x.s] = offsets[1:] - offsets[:-1]
        groups[x.s] = (offsets, entries)
    return cache["idx_query"][x.s], cache["counts"][x.s], groups[x.s]


def point_to_voxel(x: SparseTensor, z: PointTensor) -> SparseTensor:
    """utils.py:41-65: the mean of `z`'s point features per voxel of `x`, on `x`'s coordinates and maps."""
    idx_query, _, groups = point_to_voxel_index(x, z)
    return x._like(F.spvoxelize_mean(z.F, idx_query, x.C.shape[0], groups))
