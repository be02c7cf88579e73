// The point-branch tail shared by csrc/spvcnn.hip (ts_point_tail_forward) and csrc/rpvnet.hip (ts_range_point_tail_forward): one
// kernel template, the range operand compiled in or out, and one launcher with the checks of both entry points.  A row kernel of
// csrc/rows.h's family; both files are compiled with -ffp-contract=off, so every product and sum below keeps its own rounding.
#pragma once
#include <algorithm>

#include "rows.h"

namespace {

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

// The checks, the grid rule and the launch of both entry points; `who` is the entry point that was called.  Without RANGE pix, bidx,
// bw and mp are not looked at (the callers pass null and 0).
template <bool RANGE>
int launch_point_tail(const char *who, const void *y, const void *vox, const int32_t *idx, const float *weight, const void *pix,
                      const int32_t *bidx, const float *bweight, int64_t mp, const float *mean, const float *invstd,
                      const float *gamma, const float *beta, int64_t n, int32_t c, int64_t m, int32_t half, void *out, uint8_t *mask,
                      hipStream_t stream) {
  const int rc = rows_check(who, n, c, m, half);
  if (rc != TS_OK) return rc;
  if (RANGE) TS_REQUIRE(mp >= 0 && mp < (1LL << 31) - 1, TS_ERR_INVALID_ARGUMENT, "%s: bad sizes", who);
  if (n == 0) return TS_OK;
  TS_REQUIRE(y && idx && weight && mean && invstd && gamma && beta && out && (vox || m == 0) &&
                 (!RANGE || (bidx && bweight && (pix || mp == 0))),
             TS_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
  TS_REQUIRE(aligned16(y, vox, out) && aligned16(idx, weight) && (!RANGE || aligned16(pix, bidx, bweight)), TS_ERR_INVALID_ARGUMENT,
             "%s: rows and maps must be 16-byte aligned", who);
  const unsigned grid = (unsigned)std::min<int64_t>(ts_cdiv(n, (int64_t)row_groups(c, half)), 8192);
  by_half(half, [&](auto t) {
    using T = decltype(t);
    point_tail_fwd_kernel<T, RANGE><<<grid, 256, 0, stream>>>((const T *)y, (const T *)vox, idx, weight, (const T *)pix, bidx, bweight,
                                                              mp, mean, invstd, gamma, beta, n, c, m, (T *)out, mask);
  });
  TS_CHECK_LAUNCH(who);
  return TS_OK;
}

}  // namespace
