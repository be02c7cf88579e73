// BatchNorm over [N, C] voxel features, training mode.
//
// The reference runs nn.BatchNorm1d / nn.SyncBatchNorm on the feature matrix of every sparse conv
// (R/pcseg/model/segmentor/voxel/minkunet/minkunet.py:23-29, TS/torchsparse/nn/utils/apply.py:10-16), followed by
// the residual add and the ReLU as separate passes.  This file holds
//   * ONE kernel set on <T, VE> for fp32 rows (<float, 4>) and IEEE half rows (<_Float16, 8>): sliced partial sums
//     (bn_partial_kernel), BN apply (+ residual) (+ ReLU) forward (bn_act_fwd_kernel) and its backward from two float
//     coefficients per channel (bn_act_bwd_coef_kernel); a thread owns one 16-byte chunk of a row, BnVec<T, VE>;
//   * the precision-free pieces: the finish kernels that add the slices' partials in double, statistics finalisation
//     (ts_bn_finalize), the fp32 backward from double sums (bn_act_bwd_kernel, ts_bn_act_backward);
//   * one host driver per operation on <T, VE> (bn_train_forward, bn_train_backward, bn_sync_stats,
//     bn_sync_backward_reduce, bn_apply_forward, bn_apply_backward_coef); the extern "C" entry points pick an instantiation;
//   * BatchNorm -> (+ residual) -> LeakyReLU of the range-view trunks (ts_bn_leaky_act_train_*): the same kernels with ACT = 1;
//   * LeakyReLU -> BatchNorm2d of the dense 2-D branch (lbn_*), which shares the slice rule, the LDS fold and the finishes.
// Accumulation: float per lane over one slice (<= ~350 rows), double across slices.
#include <stdlib.h>

#include "common.h"

// mean / invstd from the double sums + running-statistics update (nn.BatchNorm1d semantics: biased variance
// for normalisation, unbiased for running_var, momentum update), one tiny launch instead of ~8 tensor ops.
__global__ void bn_finalize_kernel(const double *__restrict__ sums, const double *__restrict__ total_dev,
                                   double total_host, int c, float eps, float momentum,
                                   float *__restrict__ running_mean, float *__restrict__ running_var,
                                   float *__restrict__ mean, float *__restrict__ invstd) {
  int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= c) return;
  const double total = total_dev ? *total_dev : total_host;
  const double m = sums[ch] / total;
  double var = sums[c + ch] / total - m * m;
  if (var < 0.0) var = 0.0;
  mean[ch] = (float)m;
  invstd[ch] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) running_mean[ch] = (1.f - momentum) * running_mean[ch] + momentum * (float)m;
  if (running_var) {
    const double unbiased = total > 1.0 ? var * total / (total - 1.0) : var;
    running_var[ch] = (1.f - momentum) * running_var[ch] + momentum * (float)unbiased;
  }
}

extern "C" int ts_bn_finalize(const double *sums, const double *total_dev, double total_host, int32_t c, float eps,
                              float momentum, float *running_mean, float *running_var, float *mean, float *invstd,
                              ts_stream_t stream) {
  TS_REQUIRE(sums && mean && invstd && c > 0, TS_ERR_INVALID_ARGUMENT, "ts_bn_finalize: bad arguments");
  TS_REQUIRE(total_dev || total_host > 0.0, TS_ERR_INVALID_ARGUMENT, "ts_bn_finalize: empty batch");
  bn_finalize_kernel<<<(unsigned)ts_cdiv(c, 256), 256, 0, (hipStream_t)stream>>>(
      sums, total_dev, total_host, c, eps, momentum, running_mean, running_var, mean, invstd);
  TS_CHECK_LAUNCH("ts_bn_finalize");
  return TS_OK;
}

// One 16-byte chunk of a row: 4 floats or 8 halves.
template <typename T, int VE>
struct alignas(VE * sizeof(T)) BnVec {
  T x[VE];
};

// A thread's VE channels of a per-channel fp32 vector.  The fp32 kernels take them as one 16-byte load (their entry points demand
// the alignment); the half kernels read 8 scalars and demand none.
template <int VE>
__device__ __forceinline__ BnVec<float, VE> bn_load_ch(const float *__restrict__ p) {
  if constexpr (VE == 4) {
    return *(const BnVec<float, 4> *)p;
  } else {
    BnVec<float, VE> v;
#pragma unroll
    for (int i = 0; i < VE; ++i) v.x[i] = p[i];
    return v;
  }
}

// ------------------------------------------------------------------------------------------------------
// Fused BatchNorm-apply (+ residual add) (+ ReLU) and its backward: one pass each instead of
// batch_norm_elemt -> add -> relu (forward) and relu-backward -> reduce -> batch_norm_backward_elemt (backward).
//   forward   out = act((x - mean) * invstd * w + b [+ res])
//   backward  g = gout * (out > 0)          (act = relu; the forward stores one sign bit per element, a byte per chunk of 8
//                                            halves, the low 4 bits of a byte per chunk of 4 floats)
//             sums[0] = sum g, sums[1] = sum g (x - mean)                            (ts_bn_act_backward_reduce)
//             gx = (g - sums[0]/N - (x - mean) invstd^2 sums[1]/N) invstd w ,  gres = g   (ts_bn_act_backward)
// Activations, residual and gradients are T in HBM; every reduction / normalisation runs in fp32 (statistics, affine parameters
// and parameter gradients stay fp32, as under torch.autocast).
// ACT 0: ReLU when `relu` is set (the sparse blocks).  ACT 1: LeakyReLU(slope) behind the sum (the range-view trunks' BasicBlock,
// ts_bn_leaky_act_train_*, which pass relu = 1 for the mask): the mask bit is still the sign of the stored value, and an element that is stored as 0
// has taken the slope branch, as leaky_relu_backward decides it.
template <typename T, int VE, int ACT = 0>
__global__ __launch_bounds__(256) void bn_act_fwd_kernel(const BnVec<T, VE> *__restrict__ X, const BnVec<T, VE> *__restrict__ RES,
                                                         const float *__restrict__ mean, const float *__restrict__ invstd,
                                                         const float *__restrict__ w, const float *__restrict__ b, int64_t total,
                                                         int cq, int relu, BnVec<T, VE> *__restrict__ OUT,
                                                         unsigned char *__restrict__ MASK, float slope) {
  using V = BnVec<T, VE>;
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (; e < total; e += step) {
    const int q = (int)(e % cq) * VE;
    const V x = X[e];
    const BnVec<float, VE> m = bn_load_ch<VE>(mean + q), s = bn_load_ch<VE>(invstd + q);
    const BnVec<float, VE> ww = bn_load_ch<VE>(w + q), bb = bn_load_ch<VE>(b + q);
    V r;
    if (RES) r = RES[e];
    V y;
    unsigned mk = 0;
#pragma unroll
    for (int i = 0; i < VE; ++i) {
      float v = ((float)x.x[i] - m.x[i]) * s.x[i] * ww.x[i] + bb.x[i];
      if (RES) v += (float)r.x[i];
      if (ACT == 1) v = v > 0.f ? v : v * slope;
      else if (relu) v = fmaxf(v, 0.f);
      const T h = (T)v;
      // the mask bit is the sign of the STORED value (what torch's ReLU backward looks at): a positive fp32 value below half's
      // smallest subnormal rounds to zero and passes no gradient
      if (relu) mk |= (h > (T)0 ? 1u : 0u) << i;
      y.x[i] = h;
    }
    if (relu && MASK) MASK[e] = (unsigned char)mk;
    OUT[e] = y;
  }
}

__global__ __launch_bounds__(256) void bn_act_bwd_kernel(const float4 *__restrict__ GOUT,
                                                         const unsigned char *__restrict__ MASK,
                                                         const float4 *__restrict__ X, const float *__restrict__ mean,
                                                         const float *__restrict__ invstd,
                                                         const float *__restrict__ w, const double *__restrict__ sums,
                                                         const double *__restrict__ total_dev, double total_host,
                                                         int64_t total4, int c, float4 *__restrict__ GX,
                                                         float4 *__restrict__ GRES) {
  const int cq = c >> 2;
  const double total = total_dev ? *total_dev : total_host;
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (; e < total4; e += step) {
    const int q = (int)(e % cq) * 4;
    float4 g = GOUT[e];
    if (MASK) {
      const unsigned mk = MASK[e];
      g.x = (mk & 1) ? g.x : 0.f; g.y = (mk & 2) ? g.y : 0.f;
      g.z = (mk & 4) ? g.z : 0.f; g.w = (mk & 8) ? g.w : 0.f;
    }
    if (GRES) GRES[e] = g;
    const float4 x = X[e];
    const float4 m = *(const float4 *)(mean + q), s = *(const float4 *)(invstd + q), ww = *(const float4 *)(w + q);
    float gx[4];
    const float gv[4] = {g.x, g.y, g.z, g.w}, xv[4] = {x.x, x.y, x.z, x.w}, mv[4] = {m.x, m.y, m.z, m.w},
                sv[4] = {s.x, s.y, s.z, s.w}, wv[4] = {ww.x, ww.y, ww.z, ww.w};
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const float mdy = (float)(sums[q + l] / total);
      const float k2 = (float)(sums[c + q + l] / total) * sv[l] * sv[l];
      gx[l] = (gv[l] - mdy - (xv[l] - mv[l]) * k2) * sv[l] * wv[l];
    }
    GX[e] = make_float4(gx[0], gx[1], gx[2], gx[3]);
  }
}

static bool bn_aligned(const void *p) { return (((uintptr_t)p) & 15) == 0; }
// the per-channel vectors that bn_load_ch<4> reads 16 bytes at a time
template <int VE>
static bool bn_ch_aligned(const float *p) { return VE != 4 || bn_aligned(p); }

// grid of an elementwise kernel over `total` chunks (grid-stride past 2^16 workgroups)
static unsigned bn_grid(int64_t total) { return (unsigned)std::min<int64_t>(ts_cdiv(total, 256), 1 << 16); }

// ------------------------------------------------------------------------------------------------------
// Single-process training BatchNorm (+ residual) (+ ReLU), one host call per direction.
//
// Every launch is cut into <= 512 slices of at least 32 rows, each slice writes its float partial sums to scratch (no
// memset, no atomics, and the result does not depend on the order workgroups finish in), and a small second kernel adds
// the partials in double and finishes the per-channel math: mean / invstd / running statistics in the forward pass;
// grad_weight, grad_bias and the two coefficients of the input gradient in the backward pass (which the elementwise
// kernel then reads as floats instead of dividing doubles per element).
//   forward   bn_train_forward  = bn_partial<0> -> bn_fwd_finish -> bn_act_fwd
//   backward  bn_train_backward = bn_partial<1|2> -> bn_bwd_finish -> bn_act_bwd_coef
#define BN_MAX_SLICES 512

// rows per slice: whole passes of a workgroup, whose 256 threads cover 256 / (C / VE) rows at a time
template <int VE>
static inline int bn_rows_per_slice(int64_t n, int c) {
  const int rpp = 256 / (c / VE);
  const int64_t rows = std::max<int64_t>(ts_cdiv(n, BN_MAX_SLICES), 32);
  return (int)(ts_cdiv(rows, rpp) * rpp);
}

// Tail of a partial-sums kernel: every lane's VE sums to LDS, the rpp lanes of a channel added in float in ascending order, two
// floats per channel to the slice's partials [2][C].
template <int VE>
__device__ __forceinline__ void bn_fold_slice(const BnVec<float, VE> &s0, const BnVec<float, VE> &s1, float (&red)[2][256 * VE],
                                              int c, int cq, int rpp, float *__restrict__ part) {
  const int tid = threadIdx.x;
  *(BnVec<float, VE> *)&red[0][tid * VE] = s0;
  *(BnVec<float, VE> *)&red[1][tid * VE] = s1;
  __syncthreads();
  float *out = part + (int64_t)blockIdx.x * 2 * c;
  for (int ch = tid; ch < c; ch += 256) {
    const int q = (unsigned)ch / VE, l = (unsigned)ch % VE;
    float a = 0.f, b = 0.f;
    for (int y = 0; y < rpp; ++y) {
      a += red[0][(y * cq + q) * VE + l];
      b += red[1][(y * cq + q) * VE + l];
    }
    out[ch] = a;
    out[c + ch] = b;
  }
}

// row-loop unroll depth of bn_partial_kernel: 64 bytes of a column in flight per thread and stream
template <typename T>
constexpr int bn_row_unroll = sizeof(T) == 4 ? 4 : 2;
// waves per SIMD the compiler plans bn_partial_kernel for.  Half rows under the mask: 5 (94 VGPRs) - planning for 7 it fits 71
// VGPRs by waiting for each row's loads before it issues the next one's, 0.0285 against 0.0259 ms at 178k x 32
template <typename T, int MODE>
constexpr int bn_partial_waves = sizeof(T) == 2 && MODE >= 2 ? 5 : 8;

// MODE 0: (x, x^2)   1: (dy, dy (x - mean))   2: same with the ReLU mask applied to dy   3: same with the LeakyReLU mask (a cleared
// bit scales dy by `slope` instead of dropping it)
// The second sum takes every product by a fused multiply-add, written out so that the rounding does not hang on what the compiler
// contracts (left to it, the half form once kept two channels of eight on a multiply and an add).
template <typename T, int VE, int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, bn_partial_waves<T, MODE>)))
void bn_partial_kernel(const T *__restrict__ X, const T *__restrict__ DY, const unsigned char *__restrict__ MASK,
                       const float *__restrict__ mean, int64_t n, int c, int rows_per_wg, float *__restrict__ part, float slope) {
  using V = BnVec<T, VE>;
  __shared__ float red[2][256 * VE];
  const int cq = c / VE, rpp = 256 / cq;
  const int tid = threadIdx.x, ty = tid / cq, tx = tid - ty * cq;
  const bool active = ty < rpp;
  BnVec<float, VE> s0 = {}, s1 = {}, mu = {};
  if (MODE != 0 && active) mu = bn_load_ch<VE>(mean + VE * tx);
  const int64_t r_beg = (int64_t)blockIdx.x * rows_per_wg, r_end = min(n, r_beg + rows_per_wg);
  if (active) {
#pragma unroll bn_row_unroll<T>
    for (int64_t r = r_beg + ty; r < r_end; r += rpp) {
      // the row is read in place: with a local copy of the chunk in this loop the compiler no longer counts its trips and unrolls it
      // with an exit test between the rows instead of a remainder loop (4 to 10 VGPRs more, an occupancy step in MODE 1 and 2)
      const V &x = *(const V *)(X + r * c + VE * tx);
      if (MODE == 0) {
#pragma unroll
        for (int i = 0; i < VE; ++i) {
          const float v = (float)x.x[i];
          s0.x[i] += v;
          s1.x[i] = __builtin_fmaf(v, v, s1.x[i]);
        }
      } else {
        const V &d = *(const V *)(DY + r * c + VE * tx);
        const unsigned mk = MODE >= 2 ? MASK[r * cq + tx] : 0xFFu;
#pragma unroll
        for (int i = 0; i < VE; ++i) {
          const float dy = (float)d.x[i];                       // read before the test: every lane loads its whole chunk
          const float dv = ((mk >> i) & 1) ? dy : (MODE == 3 ? dy * slope : 0.f);
          s0.x[i] += dv;
          s1.x[i] = __builtin_fmaf(dv, (float)x.x[i] - mu.x[i], s1.x[i]);
        }
      }
    }
  }
  bn_fold_slice<VE>(s0, s1, red, c, cq, rpp, part);
}

// 8 channels per workgroup, 32 lanes per channel over the slices (<= 16 partials per lane, all loads issued
// before the first add); double accumulation in a fixed order.
#define BN_FIN_CH 8
#define BN_FIN_LANES 32
__device__ __forceinline__ void bn_sum_slices(const float *__restrict__ part, int slices, int c, int ch, int sl,
                                              double (&red)[2][BN_FIN_CH][BN_FIN_LANES + 1], double &s0, double &s1) {
  constexpr int PER = BN_MAX_SLICES / BN_FIN_LANES;
  // unconditional loads from clamped addresses, masked afterwards: a predicated load compiles to a branch plus
  // a full wait per element (32 serialised round trips, 10 us for this tiny kernel)
  float va[PER], vb[PER];
  const int chc = min(ch, c - 1);
#pragma unroll
  for (int t = 0; t < PER; ++t) {
    const int g = min(sl + t * BN_FIN_LANES, slices - 1);
    va[t] = part[(int64_t)g * 2 * c + chc];
    vb[t] = part[(int64_t)g * 2 * c + c + chc];
  }
  double a = 0.0, b = 0.0;
#pragma unroll
  for (int t = 0; t < PER; ++t) {
    const bool ok = sl + t * BN_FIN_LANES < slices;
    a += ok ? (double)va[t] : 0.0;
    b += ok ? (double)vb[t] : 0.0;
  }
  const int cl = threadIdx.x % BN_FIN_CH;
  red[0][cl][sl] = a;
  red[1][cl][sl] = b;
  __syncthreads();
  s0 = s1 = 0.0;
  if (sl == 0) {
    for (int i = 0; i < BN_FIN_LANES; ++i) {
      s0 += red[0][cl][i];
      s1 += red[1][cl][i];
    }
  }
}

__global__ __launch_bounds__(256) void bn_fwd_finish_kernel(const float *__restrict__ part, int slices, double total,
                                                            int c, float eps, float momentum,
                                                            float *__restrict__ running_mean,
                                                            float *__restrict__ running_var, float *__restrict__ mean,
                                                            float *__restrict__ invstd,
                                                            int64_t *__restrict__ num_batches_tracked) {
  __shared__ double red[2][BN_FIN_CH][BN_FIN_LANES + 1];
  const int ch = blockIdx.x * BN_FIN_CH + (threadIdx.x % BN_FIN_CH), sl = threadIdx.x / BN_FIN_CH;
  if (num_batches_tracked && blockIdx.x == 0 && threadIdx.x == 0) *num_batches_tracked += 1;
  double s0, s1;
  bn_sum_slices(part, slices, c, ch, sl, red, s0, s1);
  if (sl != 0 || ch >= c) return;
  const double m = s0 / total;
  double var = s1 / total - m * m;
  if (var < 0.0) var = 0.0;
  mean[ch] = (float)m;
  invstd[ch] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) running_mean[ch] = (1.f - momentum) * running_mean[ch] + momentum * (float)m;
  if (running_var) {
    const double unbiased = total > 1.0 ? var * total / (total - 1.0) : var;
    running_var[ch] = (1.f - momentum) * running_var[ch] + momentum * (float)unbiased;
  }
}

__global__ __launch_bounds__(256) void bn_bwd_finish_kernel(const float *__restrict__ part, int slices, double total,
                                                            int c, const float *__restrict__ invstd,
                                                            float *__restrict__ coef, float *__restrict__ grad_weight,
                                                            float *__restrict__ grad_bias) {
  __shared__ double red[2][BN_FIN_CH][BN_FIN_LANES + 1];
  const int ch = blockIdx.x * BN_FIN_CH + (threadIdx.x % BN_FIN_CH), sl = threadIdx.x / BN_FIN_CH;
  double s0, s1;
  bn_sum_slices(part, slices, c, ch, sl, red, s0, s1);
  if (sl != 0 || ch >= c) return;
  const float is = invstd[ch];
  coef[ch] = (float)(s0 / total);                  // mean of dy
  coef[c + ch] = (float)(s1 / total) * is * is;    // mean of dy (x - mean), times invstd^2
  if (grad_bias) grad_bias[ch] = (float)s0;
  if (grad_weight) grad_weight[ch] = (float)s1 * is;
}

template <typename T, int VE, int ACT = 0>
__global__ __launch_bounds__(256) void bn_act_bwd_coef_kernel(const BnVec<T, VE> *__restrict__ GOUT,
                                                              const unsigned char *__restrict__ MASK,
                                                              const BnVec<T, VE> *__restrict__ X, const float *__restrict__ mean,
                                                              const float *__restrict__ invstd, const float *__restrict__ w,
                                                              const float *__restrict__ coef, int64_t total, int c,
                                                              BnVec<T, VE> *__restrict__ GX, BnVec<T, VE> *__restrict__ GRES,
                                                              float slope) {
  using V = BnVec<T, VE>;
  const int cq = c / VE;
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (; e < total; e += step) {
    const int q = (int)(e % cq) * VE;
    const V gin = GOUT[e], x = X[e];
    const unsigned mk = MASK ? MASK[e] : 0xFFu;
    const BnVec<float, VE> m = bn_load_ch<VE>(mean + q), s = bn_load_ch<VE>(invstd + q), ww = bn_load_ch<VE>(w + q);
    const BnVec<float, VE> c0 = bn_load_ch<VE>(coef + q), c1 = bn_load_ch<VE>(coef + c + q);
    V g, gx;
#pragma unroll
    for (int i = 0; i < VE; ++i) {
      const float gv = ((mk >> i) & 1) ? (float)gin.x[i] : (ACT == 1 ? (float)gin.x[i] * slope : 0.f);
      g.x[i] = (T)gv;
      gx.x[i] = (T)((gv - c0.x[i] - ((float)x.x[i] - m.x[i]) * c1.x[i]) * s.x[i] * ww.x[i]);
    }
    if (GRES) GRES[e] = g;
    GX[e] = gx;
  }
}

// ------------------------------------------------------------------------------------------------------
// SyncBatchNorm halves: the same sliced reductions, finished into DOUBLE sums that the host all-reduces
// (one collective of [2C + 1] doubles in the forward pass, [2C] in the backward pass - torch's SyncBatchNorm
// all-gathers per-rank mean / invstd / count instead).  The elementwise halves are ts_bn_finalize +
// ts_bn_act_forward and ts_bn_act_backward above.
__global__ __launch_bounds__(256) void bn_sums_finish_kernel(const float *__restrict__ part, int slices, int c,
                                                             double count, const float *__restrict__ invstd,
                                                             double *__restrict__ sums,
                                                             float *__restrict__ grad_weight,
                                                             float *__restrict__ grad_bias) {
  __shared__ double red[2][BN_FIN_CH][BN_FIN_LANES + 1];
  const int ch = blockIdx.x * BN_FIN_CH + (threadIdx.x % BN_FIN_CH), sl = threadIdx.x / BN_FIN_CH;
  double s0, s1;
  bn_sum_slices(part, slices, c, ch, sl, red, s0, s1);
  if (count >= 0.0 && blockIdx.x == 0 && threadIdx.x == 0) sums[2 * c] = count;   // forward pack: [sum, sumsq, n]
  if (sl != 0 || ch >= c) return;
  sums[ch] = s0;
  sums[c + ch] = s1;
  if (grad_bias) grad_bias[ch] = (float)s0;                       // local (per-rank) parameter gradients
  if (grad_weight) grad_weight[ch] = (float)s1 * invstd[ch];
}

// the two float coefficients of bn_act_bwd_coef_kernel from all-reduced double sums
__global__ void bn_coef_from_sums_kernel(const double *__restrict__ sums, const double *__restrict__ total_dev,
                                         double total_host, const float *__restrict__ invstd, int c,
                                         float *__restrict__ coef) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= c) return;
  const double total = total_dev ? *total_dev : total_host;
  const float is = invstd[ch];
  coef[ch] = (float)(sums[ch] / total);
  coef[c + ch] = (float)(sums[c + ch] / total) * is * is;
}

// ------------------------------------------------------------------------------------------------------
// Host side: one driver per operation on <T, VE>; `what` is the entry point's name in every message.
//   <float, 4>     C % 4, C <= 1024, the per-channel vectors a kernel reads 16-byte aligned
//   <_Float16, 8>  C % 8, C <= 2048, no alignment demand on the per-channel vectors

// TS_OPT_DEBUG_BN_ABLATE (diagnostic, fp32 path).  Bits 0 / 1 (WRONG results, timing only): skip the forward statistics pass
// (bn_partial<0>) / the forward elementwise pass of the blocks without a residual.  Garbage activations also change what the
// chip draws, so the CLEAN measurement is bits 2 / 3: run the same pass TWICE (same results) - the step's slow-down is what one such
// pass costs in the step, launch gap included: the most "statistics in the epilogue of the pass that produces y" / "normalise where
// the consumer gathers the row" could save.
static int bn_debug_ablate() { return (int)ts_get_option(TS_OPT_DEBUG_BN_ABLATE); }

extern "C" size_t ts_bn_train_workspace_bytes(int32_t c) {
  // float partials [BN_MAX_SLICES][2][C] + float coefficients [2][C]
  return ((size_t)BN_MAX_SLICES * 2 * c + 2 * (size_t)c) * sizeof(float);
}

template <int VE>
static int bn_check_size(const char *what, int64_t n, int32_t c) {
  TS_REQUIRE(n > 0 && c > 0 && c % VE == 0 && c <= 256 * VE, TS_ERR_UNSUPPORTED, "%s: need N > 0 and C a multiple of %d, <= %d", what,
             VE, 256 * VE);
  return TS_OK;
}

// the sliced sums of one matrix into part [slices][2][C]; MODE from the arguments: no dy = 0, dy = 1, dy and mask = 2 (ACT 0) or 3
// (ACT 1, whose callers always hold a mask)
template <typename T, int VE, int ACT = 0>
static int bn_launch_partial(const void *x, const void *dy, const uint8_t *mask, const float *mean, int64_t n, int c, float *part,
                             hipStream_t stream, float slope = 0.f) {
  const int rows = bn_rows_per_slice<VE>(n, c);
  const int slices = (int)ts_cdiv(n, rows);
  if (!dy)
    bn_partial_kernel<T, VE, 0><<<slices, 256, 0, stream>>>((const T *)x, nullptr, nullptr, nullptr, n, c, rows, part, 0.f);
  else if (mask)
    bn_partial_kernel<T, VE, ACT == 1 ? 3 : 2><<<slices, 256, 0, stream>>>((const T *)x, (const T *)dy, mask, mean, n, c, rows, part,
                                                                           slope);
  else
    bn_partial_kernel<T, VE, 1><<<slices, 256, 0, stream>>>((const T *)x, (const T *)dy, nullptr, mean, n, c, rows, part, 0.f);
  return slices;
}

template <typename T, int VE, int ACT = 0>
static void bn_launch_act_fwd(const void *x, const void *residual, const float *mean, const float *invstd, const float *weight,
                              const float *bias, int64_t n, int c, int relu, void *out, uint8_t *mask, hipStream_t stream,
                              float slope = 0.f) {
  using V = BnVec<T, VE>;
  const int64_t total = n * (c / VE);
  bn_act_fwd_kernel<T, VE, ACT><<<bn_grid(total), 256, 0, stream>>>((const V *)x, (const V *)residual, mean, invstd, weight, bias,
                                                                    total, c / VE, relu, (V *)out, mask, slope);
}

template <typename T, int VE, int ACT = 0>
static void bn_launch_act_bwd_coef(const void *grad_out, const uint8_t *mask, const void *x, const float *mean, const float *invstd,
                                   const float *weight, const float *coef, int64_t n, int c, void *grad_x, void *grad_residual,
                                   hipStream_t stream, float slope = 0.f) {
  using V = BnVec<T, VE>;
  const int64_t total = n * (c / VE);
  bn_act_bwd_coef_kernel<T, VE, ACT><<<bn_grid(total), 256, 0, stream>>>((const V *)grad_out, mask, (const V *)x, mean, invstd, weight,
                                                                         coef, total, c, (V *)grad_x, (V *)grad_residual, slope);
}

template <typename T, int VE, int ACT = 0>
static int bn_train_forward(const char *what, const void *x, const void *residual, const float *weight, const float *bias,
                            float *running_mean, float *running_var, int64_t *num_batches_tracked, int64_t n, int32_t c, float eps,
                            float momentum, int32_t relu, float *mean, float *invstd, void *out, uint8_t *mask, void *ws,
                            size_t ws_bytes, hipStream_t stream, float slope = 0.f) {
  const int rc = bn_check_size<VE>(what, n, c);
  if (rc != TS_OK) return rc;
  TS_REQUIRE(x && weight && bias && mean && invstd && out && ws, TS_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
  TS_REQUIRE(ws_bytes >= ts_bn_train_workspace_bytes(c), TS_ERR_INVALID_ARGUMENT, "%s: workspace too small", what);
  TS_REQUIRE(bn_aligned(x) && bn_aligned(out) && bn_ch_aligned<VE>(mean) && bn_ch_aligned<VE>(invstd) && bn_ch_aligned<VE>(weight) &&
                 bn_ch_aligned<VE>(bias) && (!residual || bn_aligned(residual)) && bn_aligned(ws),
             TS_ERR_INVALID_ARGUMENT, "%s: pointers must be 16-byte aligned", what);
  float *part = (float *)ws;
  const int ablate = sizeof(T) == 4 && ACT == 0 ? bn_debug_ablate() : 0;   // diagnostic (wrong results, timing only), see above
  int slices = (int)ts_cdiv(n, bn_rows_per_slice<VE>(n, c));
  if (!(ablate & 1)) slices = bn_launch_partial<T, VE>(x, nullptr, nullptr, nullptr, n, c, part, stream);
  if (ablate & 4) bn_launch_partial<T, VE>(x, nullptr, nullptr, nullptr, n, c, part, stream);   // the pass once more
  bn_fwd_finish_kernel<<<(unsigned)ts_cdiv(c, BN_FIN_CH), 256, 0, stream>>>(part, slices, (double)n, c, eps, momentum, running_mean,
                                                                           running_var, mean, invstd, num_batches_tracked);
  if (!((ablate & 2) && !residual && relu))
    bn_launch_act_fwd<T, VE, ACT>(x, residual, mean, invstd, weight, bias, n, c, relu, out, mask, stream, slope);
  if ((ablate & 8) && !residual && relu)          // the same pass once more (same results)
    bn_launch_act_fwd<T, VE>(x, residual, mean, invstd, weight, bias, n, c, relu, out, mask, stream);
  TS_CHECK_LAUNCH(what);
  return TS_OK;
}

template <typename T, int VE, int ACT = 0>
static int bn_train_backward(const char *what, const void *grad_out, const uint8_t *mask, const void *x, const float *mean,
                             const float *invstd, const float *weight, int64_t n, int32_t c, void *grad_x, void *grad_residual,
                             float *grad_weight, float *grad_bias, void *ws, size_t ws_bytes, hipStream_t stream, float slope = 0.f) {
  const int rc = bn_check_size<VE>(what, n, c);
  if (rc != TS_OK) return rc;
  TS_REQUIRE(grad_out && x && mean && invstd && weight && grad_x && ws, TS_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
  TS_REQUIRE(ws_bytes >= ts_bn_train_workspace_bytes(c), TS_ERR_INVALID_ARGUMENT, "%s: workspace too small", what);
  TS_REQUIRE(bn_aligned(grad_out) && bn_aligned(x) && bn_aligned(grad_x) && bn_ch_aligned<VE>(mean) && bn_ch_aligned<VE>(invstd) &&
                 bn_ch_aligned<VE>(weight) && (!grad_residual || bn_aligned(grad_residual)) && bn_aligned(ws),
             TS_ERR_INVALID_ARGUMENT, "%s: pointers must be 16-byte aligned", what);
  float *part = (float *)ws;
  float *coef = part + (size_t)BN_MAX_SLICES * 2 * c;
  const int slices = bn_launch_partial<T, VE, ACT>(x, grad_out, mask, mean, n, c, part, stream, slope);
  bn_bwd_finish_kernel<<<(unsigned)ts_cdiv(c, BN_FIN_CH), 256, 0, stream>>>(part, slices, (double)n, c, invstd, coef, grad_weight,
                                                                           grad_bias);
  bn_launch_act_bwd_coef<T, VE, ACT>(grad_out, mask, x, mean, invstd, weight, coef, n, c, grad_x, grad_residual, stream, slope);
  TS_CHECK_LAUNCH(what);
  return TS_OK;
}

template <typename T, int VE>
static int bn_sync_stats(const char *what, const void *x, int64_t n, int32_t c, double *pack, void *ws, size_t ws_bytes,
                         hipStream_t stream) {
  const int rc = bn_check_size<VE>(what, n, c);
  if (rc != TS_OK) return rc;
  TS_REQUIRE(x && pack && ws && bn_aligned(x) && bn_aligned(ws), TS_ERR_INVALID_ARGUMENT, "%s: bad pointer", what);
  TS_REQUIRE(ws_bytes >= ts_bn_train_workspace_bytes(c), TS_ERR_INVALID_ARGUMENT, "%s: workspace too small", what);
  float *part = (float *)ws;
  const int slices = bn_launch_partial<T, VE>(x, nullptr, nullptr, nullptr, n, c, part, stream);
  bn_sums_finish_kernel<<<(unsigned)ts_cdiv(c, BN_FIN_CH), 256, 0, stream>>>(part, slices, c, (double)n, nullptr, pack, nullptr,
                                                                            nullptr);
  TS_CHECK_LAUNCH(what);
  return TS_OK;
}

template <typename T, int VE>
static int bn_sync_backward_reduce(const char *what, const void *grad_out, const uint8_t *mask, const void *x, const float *mean,
                                   const float *invstd, int64_t n, int32_t c, double *sums, float *grad_weight, float *grad_bias,
                                   void *ws, size_t ws_bytes, hipStream_t stream) {
  const int rc = bn_check_size<VE>(what, n, c);
  if (rc != TS_OK) return rc;
  TS_REQUIRE(grad_out && x && mean && invstd && sums && ws, TS_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
  TS_REQUIRE(bn_aligned(grad_out) && bn_aligned(x) && bn_ch_aligned<VE>(mean) && bn_aligned(ws), TS_ERR_INVALID_ARGUMENT,
             "%s: pointers must be 16-byte aligned", what);
  TS_REQUIRE(ws_bytes >= ts_bn_train_workspace_bytes(c), TS_ERR_INVALID_ARGUMENT, "%s: workspace too small", what);
  float *part = (float *)ws;
  const int slices = bn_launch_partial<T, VE>(x, grad_out, mask, mean, n, c, part, stream);
  bn_sums_finish_kernel<<<(unsigned)ts_cdiv(c, BN_FIN_CH), 256, 0, stream>>>(part, slices, c, -1.0, invstd, sums, grad_weight,
                                                                            grad_bias);
  TS_CHECK_LAUNCH(what);
  return TS_OK;
}

// The size check is the caller's: ts_bn_act_forward takes an empty matrix and any C % 4, ts_bn_act_forward_f16 the training bounds.
template <typename T, int VE>
static int bn_apply_forward(const char *what, const void *x, const void *residual, const float *mean, const float *invstd,
                            const float *weight, const float *bias, int64_t n, int32_t c, int32_t relu, void *out, uint8_t *mask,
                            hipStream_t stream) {
  TS_REQUIRE(x && mean && invstd && weight && bias && out, TS_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
  TS_REQUIRE(bn_aligned(x) && bn_aligned(out) && bn_ch_aligned<VE>(mean) && bn_ch_aligned<VE>(invstd) && bn_ch_aligned<VE>(weight) &&
                 bn_ch_aligned<VE>(bias) && (!residual || bn_aligned(residual)),
             TS_ERR_INVALID_ARGUMENT, "%s: pointers must be 16-byte aligned", what);
  bn_launch_act_fwd<T, VE>(x, residual, mean, invstd, weight, bias, n, c, relu, out, mask, stream);
  TS_CHECK_LAUNCH(what);
  return TS_OK;
}

// Elementwise backward from all-reduced double sums, through two float coefficients per channel in ws (>= 2 C floats).  Only the half
// entry point takes this form: fp32 ts_bn_act_backward has no workspace argument and divides the doubles per element.
template <typename T, int VE>
static int bn_apply_backward_coef(const char *what, const void *grad_out, const uint8_t *mask, const void *x, const float *mean,
                                  const float *invstd, const float *weight, const double *sums, const double *total_dev,
                                  double total_host, int64_t n, int32_t c, void *grad_x, void *grad_residual, void *ws,
                                  size_t ws_bytes, hipStream_t stream) {
  const int rc = bn_check_size<VE>(what, n, c);
  if (rc != TS_OK) return rc;
  TS_REQUIRE(grad_out && x && mean && invstd && weight && sums && grad_x && ws, TS_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
  TS_REQUIRE(total_dev || total_host > 0.0, TS_ERR_INVALID_ARGUMENT, "%s: empty batch", what);
  TS_REQUIRE(ws_bytes >= 2 * (size_t)c * sizeof(float), TS_ERR_INVALID_ARGUMENT, "%s: workspace too small", what);
  TS_REQUIRE(bn_aligned(grad_out) && bn_aligned(x) && bn_aligned(grad_x) && bn_ch_aligned<VE>(mean) && bn_ch_aligned<VE>(invstd) &&
                 bn_ch_aligned<VE>(weight) && (!grad_residual || bn_aligned(grad_residual)) && bn_aligned(ws),
             TS_ERR_INVALID_ARGUMENT, "%s: pointers must be 16-byte aligned", what);
  float *coef = (float *)ws;
  bn_coef_from_sums_kernel<<<(unsigned)ts_cdiv(c, 256), 256, 0, stream>>>(sums, total_dev, total_host, invstd, c, coef);
  bn_launch_act_bwd_coef<T, VE>(grad_out, mask, x, mean, invstd, weight, coef, n, c, grad_x, grad_residual, stream);
  TS_CHECK_LAUNCH(what);
  return TS_OK;
}

// ---- the entry points (include/taseg_hip.h): fp32 rows, then half rows
extern "C" int ts_bn_act_forward(const float *x, const float *residual, const float *mean, const float *invstd,
                                 const float *weight, const float *bias, int64_t n, int32_t c, int32_t relu, float *out,
                                 uint8_t *mask, ts_stream_t stream) {
  TS_REQUIRE(n >= 0 && c > 0 && (c & 3) == 0, TS_ERR_UNSUPPORTED, "ts_bn_act_forward: C must be a multiple of 4");
  if (n == 0) return TS_OK;
  return bn_apply_forward<float, 4>("ts_bn_act_forward", x, residual, mean, invstd, weight, bias, n, c, relu, out, mask,
                                    (hipStream_t)stream);
}

extern "C" int ts_bn_act_backward(const float *grad_out, const uint8_t *mask, const float *x, const float *mean,
                                  const float *invstd, const float *weight, const double *sums, const double *total_dev,
                                  double total_host, int64_t n, int32_t c, float *grad_x, float *grad_residual,
                                  ts_stream_t stream) {
  TS_REQUIRE(n >= 0 && c > 0 && (c & 3) == 0, TS_ERR_UNSUPPORTED, "ts_bn_act_backward: C must be a multiple of 4");
  if (n == 0) return TS_OK;
  TS_REQUIRE(grad_out && x && mean && invstd && weight && sums && grad_x, TS_ERR_INVALID_ARGUMENT,
             "ts_bn_act_backward: null pointer");
  TS_REQUIRE(total_dev || total_host > 0.0, TS_ERR_INVALID_ARGUMENT, "ts_bn_act_backward: empty batch");
  TS_REQUIRE(bn_aligned(grad_out) && bn_aligned(x) && bn_aligned(grad_x) &&
                 (!grad_residual || bn_aligned(grad_residual)) && bn_aligned(mean) && bn_aligned(invstd) &&
                 bn_aligned(weight),
             TS_ERR_INVALID_ARGUMENT, "ts_bn_act_backward: pointers must be 16-byte aligned");
  const int64_t total4 = n * (c / 4);
  bn_act_bwd_kernel<<<bn_grid(total4), 256, 0, (hipStream_t)stream>>>((const float4 *)grad_out, mask, (const float4 *)x, mean,
                                                                      invstd, weight, sums, total_dev, total_host, total4, c,
                                                                      (float4 *)grad_x, (float4 *)grad_residual);
  TS_CHECK_LAUNCH("ts_bn_act_backward");
  return TS_OK;
}

extern "C" int ts_bn_act_train_forward(const float *x, const float *residual, const float *weight, const float *bias,
                                       float *running_mean, float *running_var, int64_t *num_batches_tracked,
                                       int64_t n, int32_t c, float eps, float momentum, int32_t relu, float *mean,
                                       float *invstd, float *out, uint8_t *mask, void *ws, size_t ws_bytes,
                                       ts_stream_t stream) {
  return bn_train_forward<float, 4>("ts_bn_act_train_forward", x, residual, weight, bias, running_mean, running_var,
                                    num_batches_tracked, n, c, eps, momentum, relu, mean, invstd, out, mask, ws, ws_bytes,
                                    (hipStream_t)stream);
}

extern "C" int ts_bn_act_train_backward(const float *grad_out, const uint8_t *mask, const float *x, const float *mean,
                                        const float *invstd, const float *weight, int64_t n, int32_t c, float *grad_x,
                                        float *grad_residual, float *grad_weight, float *grad_bias, void *ws,
                                        size_t ws_bytes, ts_stream_t stream) {
  return bn_train_backward<float, 4>("ts_bn_act_train_backward", grad_out, mask, x, mean, invstd, weight, n, c, grad_x,
                                     grad_residual, grad_weight, grad_bias, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int ts_bn_sync_stats(const float *x, int64_t n, int32_t c, double *pack, void *ws, size_t ws_bytes,
                                ts_stream_t stream) {
  return bn_sync_stats<float, 4>("ts_bn_sync_stats", x, n, c, pack, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int ts_bn_sync_backward_reduce(const float *grad_out, const uint8_t *mask, const float *x, const float *mean,
                                          const float *invstd, int64_t n, int32_t c, double *sums, float *grad_weight,
                                          float *grad_bias, void *ws, size_t ws_bytes, ts_stream_t stream) {
  return bn_sync_backward_reduce<float, 4>("ts_bn_sync_backward_reduce", grad_out, mask, x, mean, invstd, n, c, sums,
                                           grad_weight, grad_bias, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int ts_bn_act_train_forward_f16(const void *x, const void *residual, const float *weight, const float *bias,
                                           float *running_mean, float *running_var, int64_t *num_batches_tracked,
                                           int64_t n, int32_t c, float eps, float momentum, int32_t relu, float *mean,
                                           float *invstd, void *out, uint8_t *mask, void *ws, size_t ws_bytes,
                                           ts_stream_t stream) {
  return bn_train_forward<_Float16, 8>("ts_bn_act_train_forward_f16", x, residual, weight, bias, running_mean, running_var,
                                       num_batches_tracked, n, c, eps, momentum, relu, mean, invstd, out, mask, ws, ws_bytes,
                                       (hipStream_t)stream);
}

extern "C" int ts_bn_act_train_backward_f16(const void *grad_out, const uint8_t *mask, const void *x, const float *mean,
                                            const float *invstd, const float *weight, int64_t n, int32_t c,
                                            void *grad_x, void *grad_residual, float *grad_weight, float *grad_bias,
                                            void *ws, size_t ws_bytes, ts_stream_t stream) {
  return bn_train_backward<_Float16, 8>("ts_bn_act_train_backward_f16", grad_out, mask, x, mean, invstd, weight, n, c, grad_x,
                                        grad_residual, grad_weight, grad_bias, ws, ws_bytes, (hipStream_t)stream);
}

// SyncBatchNorm halves for half-storage activations (the reference's actual recipe is AMP + DDP + SyncBatchNorm,
// R/dist_train.sh:17-19): the same double sums cross the ranks, activations and gradients stay half in HBM.
extern "C" int ts_bn_sync_stats_f16(const void *x, int64_t n, int32_t c, double *pack, void *ws, size_t ws_bytes,
                                    ts_stream_t stream) {
  return bn_sync_stats<_Float16, 8>("ts_bn_sync_stats_f16", x, n, c, pack, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int ts_bn_act_forward_f16(const void *x, const void *residual, const float *mean, const float *invstd,
                                     const float *weight, const float *bias, int64_t n, int32_t c, int32_t relu,
                                     void *out, uint8_t *mask, ts_stream_t stream) {
  const int rc = bn_check_size<8>("ts_bn_act_forward_f16", n, c);
  if (rc != TS_OK) return rc;
  return bn_apply_forward<_Float16, 8>("ts_bn_act_forward_f16", x, residual, mean, invstd, weight, bias, n, c, relu, out, mask,
                                       (hipStream_t)stream);
}

extern "C" int ts_bn_sync_backward_reduce_f16(const void *grad_out, const uint8_t *mask, const void *x, const float *mean,
                                              const float *invstd, int64_t n, int32_t c, double *sums,
                                              float *grad_weight, float *grad_bias, void *ws, size_t ws_bytes,
                                              ts_stream_t stream) {
  return bn_sync_backward_reduce<_Float16, 8>("ts_bn_sync_backward_reduce_f16", grad_out, mask, x, mean, invstd, n, c, sums,
                                              grad_weight, grad_bias, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int ts_bn_act_backward_f16(const void *grad_out, const uint8_t *mask, const void *x, const float *mean,
                                      const float *invstd, const float *weight, const double *sums,
                                      const double *total_dev, double total_host, int64_t n, int32_t c, void *grad_x,
                                      void *grad_residual, void *ws, size_t ws_bytes, ts_stream_t stream) {
  return bn_apply_backward_coef<_Float16, 8>("ts_bn_act_backward_f16", grad_out, mask, x, mean, invstd, weight, sums, total_dev,
                                             total_host, n, c, grad_x, grad_residual, ws, ws_bytes, (hipStream_t)stream);
}

// BatchNorm (training) -> (+ residual) -> LeakyReLU(slope): the ts_bn_act_train_* chain on the ACT = 1 instantiations (the range-view
// trunks' conv -> BN -> LeakyReLU and conv -> BN -> += identity -> LeakyReLU, R/pcseg/model/segmentor/range/fidnet/model/semantic/
// fidnet.py:114-128).  The mask is required: the backward has nothing else to tell the two branches apart.
extern "C" int ts_bn_leaky_act_train_forward(const void *x, const void *residual, const float *weight, const float *bias,
                                             float *running_mean, float *running_var, int64_t *num_batches_tracked, int64_t n, int32_t c,
                                             float eps, float momentum, float slope, int32_t half, float *mean, float *invstd, void *out,
                                             uint8_t *mask, void *ws, size_t ws_bytes, ts_stream_t stream) {
  const char *what = "ts_bn_leaky_act_train_forward";
  const int rc = half ? bn_check_size<8>(what, n, c) : bn_check_size<4>(what, n, c);
  if (rc != TS_OK) return rc;
  TS_REQUIRE(c <= 1024, TS_ERR_UNSUPPORTED, "%s: C <= 1024", what);
  TS_REQUIRE(mask, TS_ERR_INVALID_ARGUMENT, "%s: null mask", what);
  return half ? bn_train_forward<_Float16, 8, 1>(what, x, residual, weight, bias, running_mean, running_var, num_batches_tracked, n, c,
                                                 eps, momentum, 1, mean, invstd, out, mask, ws, ws_bytes, (hipStream_t)stream, slope)
              : bn_train_forward<float, 4, 1>(what, x, residual, weight, bias, running_mean, running_var, num_batches_tracked, n, c, eps,
                                              momentum, 1, mean, invstd, out, mask, ws, ws_bytes, (hipStream_t)stream, slope);
}

extern "C" int ts_bn_leaky_act_train_backward(const void *grad_out, const uint8_t *mask, const void *x, const float *mean,
                                              const float *invstd, const float *weight, int64_t n, int32_t c, float slope, int32_t half,
                                              void *grad_x, void *grad_residual, float *grad_weight, float *grad_bias, void *ws,
                                              size_t ws_bytes, ts_stream_t stream) {
  const char *what = "ts_bn_leaky_act_train_backward";
  const int rc = half ? bn_check_size<8>(what, n, c) : bn_check_size<4>(what, n, c);
  if (rc != TS_OK) return rc;
  TS_REQUIRE(c <= 1024, TS_ERR_UNSUPPORTED, "%s: C <= 1024", what);
  TS_REQUIRE(mask, TS_ERR_INVALID_ARGUMENT, "%s: null mask", what);
  return half ? bn_train_backward<_Float16, 8, 1>(what, grad_out, mask, x, mean, invstd, weight, n, c, grad_x, grad_residual, grad_weight,
                                                  grad_bias, ws, ws_bytes, (hipStream_t)stream, slope)
              : bn_train_backward<float, 4, 1>(what, grad_out, mask, x, mean, invstd, weight, n, c, grad_x, grad_residual, grad_weight,
                                               grad_bias, ws, ws_bytes, (hipStream_t)stream, slope);
}

// ------------------------------------------------------------------------------------------------------
// LeakyReLU -> BatchNorm (training) in one chain of passes, for the dense 2-D branch of TIAF (R/pcseg/model/segmentor/voxel/
// minkunet/unet2d.py:24-30,71,108: every block computes `bn(act(conv(x)))` with `nn.LeakyReLU()`, slope 0.01).  A channels-last
// feature stack [T, H, W, C] IS a row matrix [T*H*W, C], so the sliced statistics / double finish of the sparse BatchNorm above
// serve it; what differs is the activation IN FRONT of the normalisation:
//   forward   a = leaky(x);  out = (a - mean(a)) * invstd(a) * w + b             (x = the convolution's output, kept for backward)
//   backward  gw = sum dy (a - mean) invstd,  gb = sum dy,  ga = (dy - mean(dy) - (a - mean) invstd^2 mean(dy (a - mean))) invstd w,
//             gx = ga * (x > 0 ? 1 : slope)
// Three launches per direction (partial sums -> finish -> elementwise), 2 reads + 1 write of N*C*s forward, 3 reads + 1 write
// backward, where the library path of this PyTorch-ROCm takes a LeakyReLU pass, a layout copy and three MIOpen BatchNorm kernels
// forward, and as many backward.  T = float (4 channels per thread) or _Float16 (8 per thread); statistics fp32 / double.
__device__ __forceinline__ float lbn_leaky(float v, float slope) { return v > 0.f ? v : v * slope; }

// MODE 0: (a, a^2)   1: (dy, dy (a - mean))
template <typename T, int VE, int MODE>
__global__ __launch_bounds__(256) void lbn_partial_kernel(const T *__restrict__ X, const T *__restrict__ DY, const float *__restrict__ mean,
                                                          float slope, int64_t n, int c, int rows_per_wg, float *__restrict__ part) {
  using V = BnVec<T, VE>;
  __shared__ float red[2][256 * VE];
  const int cq = c / VE, rpp = 256 / cq;
  const int tid = threadIdx.x, ty = tid / cq, tx = tid - ty * cq;
  const bool active = ty < rpp;
  BnVec<float, VE> s0 = {}, s1 = {};
  float mu[VE];
#pragma unroll
  for (int i = 0; i < VE; ++i) mu[i] = 0.f;
  if (MODE != 0 && active) {
#pragma unroll
    for (int i = 0; i < VE; ++i) mu[i] = mean[VE * tx + i];
  }
  const int64_t r_beg = (int64_t)blockIdx.x * rows_per_wg, r_end = min(n, r_beg + rows_per_wg);
  if (active) {
    auto add = [&](const V &x, const V &d) {
      if (MODE == 0) {
#pragma unroll
        for (int i = 0; i < VE; ++i) {
          const float a = lbn_leaky((float)x.x[i], slope);
          s0.x[i] += a;
          s1.x[i] += a * a;
        }
      } else {
#pragma unroll
        for (int i = 0; i < VE; ++i) {
          const float dv = (float)d.x[i];
          s0.x[i] += dv;
          s1.x[i] += dv * (lbn_leaky((float)x.x[i], slope) - mu[i]);
        }
      }
    };
    // 8 rows per trip, their loads issued together (the sums still in row order): a workgroup walks ~10 k rows of a full-resolution
    // map with one 16-byte load per thread and row - at one or two in flight per thread the 512 workgroups ran at 2.9 TB/s, the
    // latency of their loads
    constexpr int U = 8;
    int64_t r = r_beg + ty;
    for (; r + (int64_t)(U - 1) * rpp < r_end; r += (int64_t)U * rpp) {
      V x[U], d[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        x[u] = *(const V *)(X + (r + (int64_t)u * rpp) * c + VE * tx);
        if (MODE != 0) d[u] = *(const V *)(DY + (r + (int64_t)u * rpp) * c + VE * tx);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) add(x[u], d[u]);
    }
    for (; r < r_end; r += rpp) {
      const V x = *(const V *)(X + r * c + VE * tx);
      V d = x;
      if (MODE != 0) d = *(const V *)(DY + r * c + VE * tx);
      add(x, d);
    }
  }
  bn_fold_slice<VE>(s0, s1, red, c, cq, rpp, part);
}

template <typename T, int VE>
__global__ __launch_bounds__(256) void lbn_fwd_kernel(const BnVec<T, VE> *__restrict__ X, const float *__restrict__ mean,
                                                      const float *__restrict__ invstd, const float *__restrict__ w,
                                                      const float *__restrict__ b, float slope, int64_t total, int cq,
                                                      const BnVec<T, VE> *__restrict__ RES, BnVec<T, VE> *__restrict__ OUT) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (; e < total; e += step) {
    const int q = (int)(e % cq) * VE;
    const BnVec<T, VE> x = X[e];
    BnVec<T, VE> y;
#pragma unroll
    for (int i = 0; i < VE; ++i)
      y.x[i] = (T)((lbn_leaky((float)x.x[i], slope) - mean[q + i]) * invstd[q + i] * w[q + i] + b[q + i]);
    if (RES) {                                             // the block's residual sum: added to the ROUNDED result, as the module pair does
      const BnVec<T, VE> r = RES[e];
#pragma unroll
      for (int i = 0; i < VE; ++i) y.x[i] = (T)((float)y.x[i] + (float)r.x[i]);
    }
    OUT[e] = y;
  }
}

template <typename T, int VE>
__global__ __launch_bounds__(256) void lbn_bwd_kernel(const BnVec<T, VE> *__restrict__ GOUT, const BnVec<T, VE> *__restrict__ X,
                                                      const float *__restrict__ mean, const float *__restrict__ invstd,
                                                      const float *__restrict__ w, const float *__restrict__ coef, float slope,
                                                      int64_t total, int c, BnVec<T, VE> *__restrict__ GX) {
  const int cq = c / VE;
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (; e < total; e += step) {
    const int q = (int)(e % cq) * VE;
    const BnVec<T, VE> g = GOUT[e], x = X[e];
    BnVec<T, VE> gx;
#pragma unroll
    for (int i = 0; i < VE; ++i) {
      const float xv = (float)x.x[i];
      const float ga = ((float)g.x[i] - coef[q + i] - (lbn_leaky(xv, slope) - mean[q + i]) * coef[c + q + i]) * invstd[q + i] * w[q + i];
      gx.x[i] = (T)(xv > 0.f ? ga : ga * slope);
    }
    GX[e] = gx;
  }
}

static int lbn_check(const char *what, int64_t n, int32_t c, int32_t half, size_t ws_bytes) {
  const int ve = half ? 8 : 4;
  TS_REQUIRE(n > 0 && c > 0 && c % ve == 0 && c / ve <= 256 && c <= 1024, TS_ERR_UNSUPPORTED,
             "%s: need N > 0 and C a multiple of %d, <= 1024", what, ve);
  TS_REQUIRE(ws_bytes >= ts_bn_train_workspace_bytes(c), TS_ERR_WORKSPACE_TOO_SMALL, "%s: workspace too small", what);
  return TS_OK;
}

template <typename T, int VE>
static void lbn_forward_launch(const void *x, const float *weight, const float *bias, float *running_mean, float *running_var,
                               int64_t *nbt, int64_t n, int c, float eps, float momentum, float slope, float *mean, float *invstd,
                               const void *residual, void *out, float *part, hipStream_t stream) {
  const int rows = bn_rows_per_slice<VE>(n, c);
  const int slices = (int)ts_cdiv(n, rows);
  lbn_partial_kernel<T, VE, 0><<<slices, 256, 0, stream>>>((const T *)x, nullptr, nullptr, slope, n, c, rows, part);
  bn_fwd_finish_kernel<<<(unsigned)ts_cdiv(c, BN_FIN_CH), 256, 0, stream>>>(part, slices, (double)n, c, eps, momentum, running_mean,
                                                                           running_var, mean, invstd, nbt);
  const int64_t total = n * (c / VE);
  lbn_fwd_kernel<T, VE><<<bn_grid(total), 256, 0, stream>>>((const BnVec<T, VE> *)x, mean, invstd, weight, bias, slope, total, c / VE,
                                                  (const BnVec<T, VE> *)residual, (BnVec<T, VE> *)out);
}

template <typename T, int VE>
static void lbn_backward_launch(const void *grad_out, const void *x, const float *mean, const float *invstd, const float *weight,
                                int64_t n, int c, float slope, void *grad_x, float *grad_weight, float *grad_bias, float *part,
                                hipStream_t stream) {
  float *coef = part + (size_t)BN_MAX_SLICES * 2 * c;
  const int rows = bn_rows_per_slice<VE>(n, c);
  const int slices = (int)ts_cdiv(n, rows);
  lbn_partial_kernel<T, VE, 1><<<slices, 256, 0, stream>>>((const T *)x, (const T *)grad_out, mean, slope, n, c, rows, part);
  bn_bwd_finish_kernel<<<(unsigned)ts_cdiv(c, BN_FIN_CH), 256, 0, stream>>>(part, slices, (double)n, c, invstd, coef, grad_weight,
                                                                           grad_bias);
  const int64_t total = n * (c / VE);
  lbn_bwd_kernel<T, VE><<<bn_grid(total), 256, 0, stream>>>((const BnVec<T, VE> *)grad_out, (const BnVec<T, VE> *)x, mean, invstd, weight,
                                                  coef, slope, total, c, (BnVec<T, VE> *)grad_x);
}

// out [N, C] = BatchNorm_train(LeakyReLU_slope(x [N, C])) (+ residual [N, C], may be NULL: the block's `skip + y`, added to the rounded
// result); mean / invstd [C] (of the activated values) are kept for the backward; running statistics (may be NULL) and
// num_batches_tracked (may be NULL) updated as nn.BatchNorm2d does.  half != 0: IEEE half rows.
// ws >= ts_bn_train_workspace_bytes(c), every pointer 16-byte aligned.
extern "C" int ts_leaky_bn_train_forward(const void *x, const float *weight, const float *bias, float *running_mean, float *running_var,
                                         int64_t *num_batches_tracked, int64_t n, int32_t c, float eps, float momentum, float slope,
                                         int32_t half, float *mean, float *invstd, const void *residual, void *out, void *ws,
                                         size_t ws_bytes, ts_stream_t stream_) {
  const int rc = lbn_check("ts_leaky_bn_train_forward", n, c, half, ws_bytes);
  if (rc != TS_OK) return rc;
  TS_REQUIRE(x && weight && bias && mean && invstd && out && ws, TS_ERR_INVALID_ARGUMENT, "ts_leaky_bn_train_forward: null pointer");
  TS_REQUIRE(bn_aligned(x) && bn_aligned(out) && bn_aligned(ws) && bn_aligned(residual), TS_ERR_INVALID_ARGUMENT,
             "ts_leaky_bn_train_forward: pointers must be 16-byte aligned");
  if (half)
    lbn_forward_launch<_Float16, 8>(x, weight, bias, running_mean, running_var, num_batches_tracked, n, c, eps, momentum, slope, mean,
                                    invstd, residual, out, (float *)ws, (hipStream_t)stream_);
  else
    lbn_forward_launch<float, 4>(x, weight, bias, running_mean, running_var, num_batches_tracked, n, c, eps, momentum, slope, mean,
                                 invstd, residual, out, (float *)ws, (hipStream_t)stream_);
  TS_CHECK_LAUNCH("ts_leaky_bn_train_forward");
  return TS_OK;
}

// grad_x [N, C] (with respect to the LeakyReLU's input), grad_weight / grad_bias [C] (may be NULL) from grad_out [N, C]
extern "C" int ts_leaky_bn_train_backward(const void *grad_out, const void *x, const float *mean, const float *invstd,
                                          const float *weight, int64_t n, int32_t c, float slope, int32_t half, void *grad_x,
                                          float *grad_weight, float *grad_bias, void *ws, size_t ws_bytes, ts_stream_t stream_) {
  const int rc = lbn_check("ts_leaky_bn_train_backward", n, c, half, ws_bytes);
  if (rc != TS_OK) return rc;
  TS_REQUIRE(grad_out && x && mean && invstd && weight && grad_x && ws, TS_ERR_INVALID_ARGUMENT, "ts_leaky_bn_train_backward: null pointer");
  TS_REQUIRE(bn_aligned(grad_out) && bn_aligned(x) && bn_aligned(grad_x) && bn_aligned(ws), TS_ERR_INVALID_ARGUMENT,
             "ts_leaky_bn_train_backward: pointers must be 16-byte aligned");
  if (half)
    lbn_backward_launch<_Float16, 8>(grad_out, x, mean, invstd, weight, n, c, slope, grad_x, grad_weight, grad_bias, (float *)ws,
                                     (hipStream_t)stream_);
  else
    lbn_backward_launch<float, 4>(grad_out, x, mean, invstd, weight, n, c, slope, grad_x, grad_weight, grad_bias, (float *)ws,
                                  (hipStream_t)stream_);
  TS_CHECK_LAUNCH("ts_leaky_bn_train_backward");
  return TS_OK;
}
