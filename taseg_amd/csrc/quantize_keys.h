// The 64-bit voxel key of the dataset-side voxelisation and the head flags of its sorted order (library-internal): written once,
// used by ts_sparse_quantize (csrc/quantize.hip) and ts_cylinder_voxels (csrc/cylinder_stage.hip).
//   key = batch (10 bits) | x + 2^17 (18 bits) | y + 2^17 (18 bits) | z + 2^17 (18 bits)
// so ascending keys are ascending (b, x, y, z) - torchsparse's sparse_quantize order inside every sample - and a STABLE sort keeps
// the rows of a voxel in input order: the head of a run is the voxel's first point (np.unique's first occurrence).
#pragma once
#include "common.h"

#define TQ_CBIAS (1 << 17)
#define TQ_CMASK ((1u << 18) - 1)
#define TQ_BATCH_SHIFT 54

static __global__ __launch_bounds__(256) void sq_pack_kernel(const int4 *__restrict__ c, int64_t n, uint64_t *__restrict__ keys,
                                                             int *__restrict__ vals, int *__restrict__ err) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    int4 v = c[i];
    bool ok = (unsigned)(v.x + TQ_CBIAS) <= TQ_CMASK && (unsigned)(v.y + TQ_CBIAS) <= TQ_CMASK &&
              (unsigned)(v.z + TQ_CBIAS) <= TQ_CMASK && (unsigned)v.w < 1024u;
    if (!ok) *err = 1;
    keys[i] = ((uint64_t)(unsigned)v.w << TQ_BATCH_SHIFT) | ((uint64_t)(unsigned)(v.x + TQ_CBIAS) << 36) |
              ((uint64_t)(unsigned)(v.y + TQ_CBIAS) << 18) | (uint64_t)(unsigned)(v.z + TQ_CBIAS);
    vals[i] = (int)i;
  }
}

static __global__ __launch_bounds__(256) void sq_flag_kernel(const uint64_t *__restrict__ keys, int64_t n,
                                                             unsigned *__restrict__ flags) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) flags[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}
