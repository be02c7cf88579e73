// Flat-buffer AdamW step on the buckets of taseg_amd.optim.FlatAdamW (the range-view recipes: OPTIMIZER adamw,
// GRAD_NORM_CLIP 10, SCHEDULER onecycle).  Norm, skip decision, clip coefficient and loss scale are ts_sgd_grad_stats and
// ts_sgd_decide of optim.hip; this file reads their state[2] (clip coefficient x 1 / scale) and state[3] (skip) and adds
//   ts_adamw_prepare          per bucket, one thread per slot: the step counter of every live slot moves on by one and
//                             the scalars torch's _single_tensor_adam hands to ATen are written, in double from the
//                             group's doubles, rounded to float once each
//   ts_adamw_apply_segments   per bucket: p, m, v updated in place from p, g, m, v - ts_sgd_apply_segments' tiles with
//                             four streams, 28 bytes per element
// with no host read: the counters live on the device, so a skipped step (non-finite gradients) and a slot without a
// gradient do not advance them and the host never learns of either.
// Compiled with -ffp-contract=off: every operation of the element rule is rounded on its own, in ATen's order, and
// tests/adamw_ref.py restates it in numpy float32 to the bit.  sqrtf and the division are the correctly rounded forms
// (no fast-math, no approximate intrinsics).
#include "common.h"

__device__ __forceinline__ int64_t adamw_slot_end(const TsSgdSlot &r) { return r.offset + ((r.count + 15) & ~(int64_t)15); }

// sgd_slot_skipped's rule (optim.hip): no gradient here this step; with several ranks the all-reduced flag says whether
// SOME rank had one - then the averaged gradient is applied here too and the replicas stay identical
__device__ __forceinline__ bool adamw_slot_skipped(const TsSgdSlot &r, const float *__restrict__ flags) {
  return r.unused != 0 && (flags == nullptr || flags[r.flag_index] == 0.f);
}

__global__ __launch_bounds__(256) void adamw_prepare_kernel(const TsSgdSlot *__restrict__ slots, int n_slots,
                                                            const float *__restrict__ flags,
                                                            const float *__restrict__ state,
                                                            const TsAdamwGroup *__restrict__ groups, int n_groups,
                                                            int32_t *__restrict__ step, TsAdamwCoef *__restrict__ coef) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_slots || state[3] != 0.f) return;
  const TsSgdSlot r = slots[s];
  if (adamw_slot_skipped(r, flags)) return;
  const TsAdamwGroup h = groups[min(max(r.group, 0), n_groups - 1)];
  const int32_t t = step[s] + 1;
  step[s] = t;
  // torch: bias_correction1 = 1 - beta1 ** step; step_size = lr / bias_correction1; bias_correction2_sqrt =
  // (1 - beta2 ** step) ** 0.5 - Python floats, i.e. doubles; the betas are the group's CURRENT values
  const double bc1 = 1.0 - pow(h.beta1, (double)t);
  const double bc2 = 1.0 - pow(h.beta2, (double)t);
  TsAdamwCoef c;
  c.decay = (float)(1.0 - h.lr * h.weight_decay);
  c.w1 = (float)(1.0 - h.beta1);
  c.b2 = (float)h.beta2;
  c.w2 = (float)(1.0 - h.beta2);
  c.neg_step_size = (float)(-(h.lr / bc1));
  c.bc2_sqrt = (float)sqrt(bc2);
  c.eps = (float)h.eps;
  c.live = 1 | (h.weight_decay != 0.0 ? 2 : 0);      // bit 1: the decay product is made (torch skips the mul_ at 0)
  coef[s] = c;
}

// One element, ATen's order (mul_, lerp_, mul_ + addcmul_, sqrt / div / add_, addcdiv_):
//   g' = g gs;  p1 = p decay;  d = g' - m;  m' = w1 < 0.5 ? m + w1 d : g' - d (1 - w1);  v' = b2 v + (w2 g') g'
//   den = sqrtf(v') / bc2_sqrt + eps;  p' = p1 + (neg_step_size m') / den
// The padding between slots holds p = g = m = v = 0: m' = 0, v' = 0, den = 0 / bc2_sqrt + eps = eps > 0 (the host
// refuses eps <= 0) and p' = 0 + 0 / eps = 0 - it stays zero.
__device__ __forceinline__ void adamw_elem(float &p, float g, float &m, float &v, float gs, const TsAdamwCoef &c) {
  const float gg = g * gs;
  const float p1 = (c.live & 2) ? p * c.decay : p;
  const float d = gg - m;
  const float m1 = c.w1 < 0.5f ? m + c.w1 * d : gg - d * (1.f - c.w1);
  const float v1 = c.b2 * v + (c.w2 * gg) * gg;
  const float den = sqrtf(v1) / c.bc2_sqrt + c.eps;
  m = m1;
  v = v1;
  p = p1 + (c.neg_step_size * m1) / den;
}

__device__ __forceinline__ void adamw_vec(float4 &p, const float4 &g, float4 &m, float4 &v, float gs,
                                          const TsAdamwCoef &c) {
  adamw_elem(p.x, g.x, m.x, v.x, gs, c);
  adamw_elem(p.y, g.y, m.y, v.y, gs, c);
  adamw_elem(p.z, g.z, m.z, v.z, gs, c);
  adamw_elem(p.w, g.w, m.w, v.w, gs, c);
}

// sgd_apply_segments_kernel's walk (optim.hip) with one more stream: a tile of TS_SGD_TILE elements per iteration, 256
// lanes x 4 float4 per stream, all sixteen 16-byte loads of a lane issued before the first use; tile_first[t] names the
// slot of the tile's first element.  A tile inside one slot reads slot record and coefficients from wave-uniform
// addresses (scalar loads) and skips with a uniform `continue`; a tile with a slot boundary lets every lane walk the
// slot offsets forward to its own; the bucket's partial last tile goes one float4 at a time.
__global__ __launch_bounds__(256) void adamw_apply_segments_kernel(
    float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v, int64_t n,
    const float *__restrict__ state, const TsSgdSlot *__restrict__ slots, int n_slots,
    const int32_t *__restrict__ tile_first, int64_t n_tiles, const float *__restrict__ flags,
    const TsAdamwCoef *__restrict__ coef) {
  const float skip_step = state[3], gs = state[2];
  constexpr int U = TS_SGD_TILE / (256 * 4);   // float4 per lane, stream and tile
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int64_t base = t * TS_SGD_TILE;
    const int64_t i0 = base + (int64_t)threadIdx.x * 4;
    if (base + TS_SGD_TILE <= n) {             // a whole tile: the loads need nothing but `base`
      float4 pv[U], gv[U], mv[U], vv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        pv[u] = *(const float4 *)(p + i0 + u * 1024);
        gv[u] = *(const float4 *)(g + i0 + u * 1024);
        mv[u] = *(const float4 *)(m + i0 + u * 1024);
        vv[u] = *(const float4 *)(v + i0 + u * 1024);
      }
      if (skip_step != 0.f) return;
      const int s0 = min(max(tile_first[t], 0), n_slots - 1);
      const TsSgdSlot r0 = slots[s0];
      if (base + TS_SGD_TILE <= adamw_slot_end(r0)) {     // ... inside slot s0: everything about it is wave-uniform
        if (adamw_slot_skipped(r0, flags)) continue;
        const TsAdamwCoef c = coef[s0];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          adamw_vec(pv[u], gv[u], mv[u], vv[u], gs, c);
          *(float4 *)(m + i0 + u * 1024) = mv[u];
          *(float4 *)(v + i0 + u * 1024) = vv[u];
          *(float4 *)(p + i0 + u * 1024) = pv[u];
        }
      } else {                                 // ... with a slot boundary in it: i ascends with u, s only moves forward
        int s = s0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t i = i0 + u * 1024;
          while (s + 1 < n_slots && i >= slots[s + 1].offset) ++s;
          const TsSgdSlot r = slots[s];
          if (adamw_slot_skipped(r, flags)) continue;
          const TsAdamwCoef c = coef[s];
          adamw_vec(pv[u], gv[u], mv[u], vv[u], gs, c);
          *(float4 *)(m + i) = mv[u];
          *(float4 *)(v + i) = vv[u];
          *(float4 *)(p + i) = pv[u];
        }
      }
    } else {                                   // the last, partial tile: the same walk, one float4 at a time
      if (skip_step != 0.f) return;
      int s = min(max(tile_first[t], 0), n_slots - 1);
#pragma unroll 1
      for (int64_t i = i0; i < n; i += 1024) {
        while (s + 1 < n_slots && i >= slots[s + 1].offset) ++s;
        const TsSgdSlot r = slots[s];
        if (adamw_slot_skipped(r, flags)) continue;
        const TsAdamwCoef c = coef[s];
        float4 pw = *(const float4 *)(p + i);
        const float4 gw = *(const float4 *)(g + i);
        float4 mw = *(const float4 *)(m + i);
        float4 vw = *(const float4 *)(v + i);
        adamw_vec(pw, gw, mw, vw, gs, c);
        *(float4 *)(m + i) = mw;
        *(float4 *)(v + i) = vw;
        *(float4 *)(p + i) = pw;
      }
    }
  }
}

extern "C" int ts_adamw_prepare(const TsSgdSlot *slots, int32_t n_slots, const float *flags, const float *state,
                                const TsAdamwGroup *groups, int32_t n_groups, int32_t *step, TsAdamwCoef *coef,
                                ts_stream_t stream) {
  TS_REQUIRE(n_slots >= 0 && n_groups >= 1 && state, TS_ERR_INVALID_ARGUMENT, "ts_adamw_prepare: bad arguments");
  if (n_slots == 0) return TS_OK;
  TS_REQUIRE(slots && groups && step && coef, TS_ERR_INVALID_ARGUMENT, "ts_adamw_prepare: null pointer");
  TS_REQUIRE(((((uintptr_t)groups) | ((uintptr_t)slots)) & 7) == 0 && ((((uintptr_t)step) | ((uintptr_t)coef)) & 3) == 0,
             TS_ERR_INVALID_ARGUMENT, "ts_adamw_prepare: misaligned table");
  adamw_prepare_kernel<<<(unsigned)ts_cdiv(n_slots, 256), 256, 0, (hipStream_t)stream>>>(slots, n_slots, flags, state,
                                                                                        groups, n_groups, step, coef);
  TS_CHECK_LAUNCH("ts_adamw_prepare");
  return TS_OK;
}

extern "C" int ts_adamw_apply_segments(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                                       const float *state, const TsSgdSlot *slots, int32_t n_slots,
                                       const int32_t *tile_first, int64_t n_tiles, const float *flags,
                                       const TsAdamwCoef *coef, ts_stream_t stream) {
  TS_REQUIRE(n >= 0 && state && n_slots >= 0, TS_ERR_INVALID_ARGUMENT, "ts_adamw_apply_segments: bad arguments");
  if (n == 0 || n_slots == 0) return TS_OK;
  TS_REQUIRE(param && grad && exp_avg && exp_avg_sq && slots && tile_first && coef, TS_ERR_INVALID_ARGUMENT,
             "ts_adamw_apply_segments: null pointer");
  TS_REQUIRE(n % 4 == 0 &&
                 ((((uintptr_t)param) | ((uintptr_t)grad) | ((uintptr_t)exp_avg) | ((uintptr_t)exp_avg_sq)) & 15) == 0,
             TS_ERR_INVALID_ARGUMENT,
             "ts_adamw_apply_segments: buckets must be 16-byte aligned and a multiple of 4 elements long");
  TS_REQUIRE(n_tiles == ts_cdiv(n, TS_SGD_TILE), TS_ERR_INVALID_ARGUMENT,
             "ts_adamw_apply_segments: tile_first must hold one entry per TS_SGD_TILE elements");
  const unsigned grid = (unsigned)std::min<int64_t>(n_tiles, 2048);
  adamw_apply_segments_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(param, grad, exp_avg, exp_avg_sq, n, state, slots,
                                                                     n_slots, tile_first, n_tiles, flags, coef);
  TS_CHECK_LAUNCH("ts_adamw_apply_segments");
  return TS_OK;
}
