// The point-branch tail shared by csrc/spvcnn.hip (ts_point_tail_forward) and csrc/rpvnet.hip (ts_range_point_tail_forward): one
// kernel template, the range operand compiled in or out.  Row kernels of this family use 16-byte accesses per lane and one group of
// c / V lanes per row; both files are compiled with -ffp-contract=off, so every product and sum below keeps its own rounding.
#pragma once
#include <hip/hip_fp16.h>

#include "common.h"

namespace {

template <typename T, int V>
using ts_vec = T __attribute__((ext_vector_type(V)));

template <typename T> struct Lanes;                     // elements of one 16-byte access
template <> struct Lanes<float> { static constexpr int V = 4; };
template <> struct Lanes<_Float16> { static constexpr int V = 8; };

// out[i, :] = sum_k w[i, k] vox[idx[i, k], :] + relu((y[i, :] - mean) invstd gamma + beta): the trilinear sum over k = 0 .. 7 in k
// order with float32 accumulation, a missing corner (idx < 0, or w == 0) adding nothing - the arithmetic of devoxelize_fwd_kernel
// (csrc/pointops.hip) - and the BatchNorm term in the operation order of bn_act_fwd_kernel (csrc/bn.hip).  mask (optional) takes one
// sign bit of the BatchNorm term per element, a byte per 16-byte chunk of a row as ts_bn_act_forward lays it out: what
// ts_bn_act_train_backward needs to send the gradient of `out` through the ReLU.  A lane keeps mean, invstd, gamma and beta of its
// V channels in registers and walks the rows grid-stride.
//
// RANGE: one more gathered operand, sum_{j<4} bw[i, j] pix[bidx[i, j], :] over the mp rows of a channels-last map (bidx / bw [n, 8],
// columns 0 .. 3 read: the four bilinear corners in the order nw, ne, sw, se).  That sum runs in corner order from its own zero;
// out = (trilinear + bilinear) + BatchNorm term, the reference's left-to-right `z.F + r_z + z_point` (rpvnet.py:651).
template <typename T, bool RANGE>
__global__ __launch_bounds__(256) void point_tail_fwd_kernel(const T *__restrict__ y, const T *__restrict__ vox,
                                                             const int *__restrict__ idx, const float *__restrict__ w,
                                                             const T *__restrict__ pix, const int *__restrict__ bidx,
                                                             const float *__restrict__ bw, int64_t mp,
                                                             const float *__restrict__ mean, const float *__restrict__ invstd,
                                                             const float *__restrict__ gamma, const float *__restrict__ beta,
                                                             int64_t n, int c, int64_t m, T *__restrict__ out,
                                                             unsigned char *__restrict__ mask) {
  constexpr int V = Lanes<T>::V;
  typedef ts_vec<T, V> vec;
  const int cq = c / V, groups = 256 / cq;
  const int grp = threadIdx.x / cq, lane = threadIdx.x - grp * cq;
  if (grp >= groups) return;
  float mu[V], is[V], ga[V], be[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    mu[j] = mean[V * lane + j];
    is[j] = invstd[V * lane + j];
    ga[j] = gamma[V * lane + j];
    be[j] = beta[V * lane + j];
  }
  const int64_t step = (int64_t)gridDim.x * groups;
  for (int64_t i = (int64_t)blockIdx.x * groups + grp; i < n; i += step) {
    const int4 ia = *(const int4 *)(idx + i * 8), ib = *(const int4 *)(idx + i * 8 + 4);
    const float4 wa = *(const float4 *)(w + i * 8), wb = *(const float4 *)(w + i * 8 + 4);
    const int id[8] = {ia.x, ia.y, ia.z, ia.w, ib.x, ib.y, ib.z, ib.w};
    const float wk[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
    const vec yv = *(const vec *)(y + i * c + V * lane);
    vec f[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
#pragma unroll
      for (int j = 0; j < V; ++j) f[k][j] = (T)0;
      if (id[k] >= 0 && id[k] < m && wk[k] != 0.f) f[k] = *(const vec *)(vox + (int64_t)id[k] * c + V * lane);
    }
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] += wk[k] * (float)f[k][j];
    }
    if constexpr (RANGE) {
      const int4 ba = *(const int4 *)(bidx + i * 8);
      const float4 bwa = *(const float4 *)(bw + i * 8);
      const int bd[4] = {ba.x, ba.y, ba.z, ba.w};
      const float bk[4] = {bwa.x, bwa.y, bwa.z, bwa.w};
      vec g[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int j = 0; j < V; ++j) g[k][j] = (T)0;
        if (bd[k] >= 0 && bd[k] < mp && bk[k] != 0.f) g[k] = *(const vec *)(pix + (int64_t)bd[k] * c + V * lane);
      }
      float racc[V];
#pragma unroll
      for (int j = 0; j < V; ++j) racc[j] = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int j = 0; j < V; ++j) racc[j] += bk[k] * (float)g[k][j];
      }
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] += racc[j];
    }
    vec o;
    unsigned mk = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float t = ((float)yv[j] - mu[j]) * is[j] * ga[j] + be[j];
      t = fmaxf(t, 0.f);
      mk |= (t > 0.f ? 1u : 0u) << j;
      o[j] = (T)(acc[j] + t);
    }
    if (mask) mask[i * cq + lane] = (unsigned char)mk;
    *(vec *)(out + i * c + V * lane) = o;
  }
}

inline int rows_check(const char *who, int64_t n, int32_t c, int64_t m, int32_t half) {
  TS_REQUIRE(n >= 0 && m >= 0 && c > 0 && n < (1LL << 30) && m < (1LL << 31) - 1, TS_ERR_INVALID_ARGUMENT, "%s: bad sizes", who);
  TS_REQUIRE(c % (half ? 8 : 4) == 0 && c <= 1024, TS_ERR_UNSUPPORTED,
             "%s: C must be a multiple of %d (16-byte pieces of a row), <= 1024", who, half ? 8 : 4);
  return TS_OK;
}

inline bool aligned16(const void *a, const void *b = nullptr, const void *c = nullptr, const void *d = nullptr) {
  return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) == 0;
}

}  // namespace
