// Flat-buffer SGD step with gradient-norm clipping and AMP loss-scale handling, all decided on the device.
//
// The reference's step (R/train.py:399-417) is scaler.unscale_ -> clip_grad_norm_(10) -> scaler.step(SGD) ->
// scaler.update(): torch runs it as ~10 multi-tensor launches over 380 parameters plus one device->host read
// (GradScaler.step asks found_inf.item()), which drains the launch queue once per step.  Here parameters, gradients
// and momentum live in a few flat buckets (taseg_amd.optim.FlatSGD) and the step is
//   ts_sgd_grad_stats   per bucket: sum of squares + non-finite flag of the (scaled) gradients -> stats buffer
//   ts_sgd_decide       one thread: total norm of the UNSCALED gradients, clip coefficient, skip flag, new loss scale
//   ts_sgd_apply        per bucket: p, m updated in place unless the step is skipped
// with no host read anywhere.  Arithmetic = torch.optim.SGD (momentum, weight decay, dampening 0) +
// torch.nn.utils.clip_grad_norm_ + GradScaler.
//   ts_sgd_apply_segments   ts_sgd_apply per PARAMETER SLOT of the bucket, still one launch: every slot has its own
//                           hyper-parameter group (the reference's `sgd_fc`), a slot without a gradient this step is left
//                           alone (torch.optim.SGD skips a parameter whose .grad is None), Nesterov momentum.  Nesterov is
//                           there for loaded checkpoints (a saved param_groups may say `nesterov: True`, and
//                           SGD.load_state_dict adopts it); the reference's build_optimizer still ignores its own NESTEROV
//                           key (optim/__init__.py:15-21).  This is the entry FlatSGD.step() calls.
#include "common.h"

// state (float[8], device): 0 loss scale, 1 growth tracker, 2 clip coefficient x inv_scale (what multiplies the stored
// gradient), 3 skip flag, 4 total norm (unscaled), 5 first-step flag (momentum buffers empty)
#define SGD_STATE_FLOATS 8

__global__ __launch_bounds__(256) void sgd_grad_stats_kernel(const float *__restrict__ g, int64_t n,
                                                             double *__restrict__ sumsq, int *__restrict__ nonfinite) {
  __shared__ double red[256];
  double acc = 0.0;
  int bad = 0;
  int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const int64_t step = (int64_t)gridDim.x * blockDim.x * 4;
  for (; i + 3 * step + 3 < n; i += 4 * step) {       // four independent 16-byte loads in flight per thread
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *(const float4 *)(g + i + u * step);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc += (double)v[u].x * v[u].x + (double)v[u].y * v[u].y + (double)v[u].z * v[u].z + (double)v[u].w * v[u].w;
      bad |= !(isfinite(v[u].x) && isfinite(v[u].y) && isfinite(v[u].z) && isfinite(v[u].w));
    }
  }
  for (; i + 3 < n; i += step) {
    const float4 v = *(const float4 *)(g + i);
    acc += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
    bad |= !(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w));
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t t = n & ~(int64_t)3; t < n; ++t) {   // tail (n % 4 elements)
      acc += (double)g[t] * g[t];
      bad |= !isfinite(g[t]);
    }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(sumsq, red[0]);
  if (bad) atomicOr(nonfinite, 1);
}

__global__ void sgd_decide_kernel(double *__restrict__ sumsq, int *__restrict__ nonfinite, float *__restrict__ state,
                                  float max_norm, float growth, float backoff, int growth_interval, int amp) {
  const float scale = amp ? state[0] : 1.f;
  const float inv = 1.f / scale;
  const bool bad = *nonfinite != 0 || !isfinite(*sumsq);
  const float norm = (float)sqrt(*sumsq) * inv;                        // norm of the unscaled gradients
  float coef = max_norm > 0.f ? max_norm / (norm + 1e-6f) : 1.f;       // clip_grad_norm_: min(1, max / (norm + eps))
  coef = fminf(coef, 1.f);
  state[2] = coef * inv;
  state[3] = bad ? 1.f : 0.f;
  state[4] = norm;
  if (amp) {                                                           // GradScaler.update()
    if (bad) {
      state[0] = scale * backoff;
      state[1] = 0.f;
    } else {
      const float tracker = state[1] + 1.f;
      if ((int)tracker >= growth_interval) {
        const float grown = scale * growth;
        if (isfinite(grown)) state[0] = grown;                           // torch does not grow the scale past fp32 bounds to inf
        state[1] = 0.f;
      } else {
        state[1] = tracker;
      }
    }
  }
  *sumsq = 0.0;          // re-arm for the next step
  *nonfinite = 0;
}

__global__ __launch_bounds__(256) void sgd_apply_kernel(float *__restrict__ p, const float *__restrict__ g,
                                                        float *__restrict__ m, int64_t n,
                                                        const float *__restrict__ state, float lr, float momentum,
                                                        float weight_decay, int first) {
  if (state[3] != 0.f) return;                 // non-finite gradients: skip the step (GradScaler semantics)
  const float gs = state[2];
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    const float pv = p[i];
    const float d = g[i] * gs + weight_decay * pv;
    const float buf = first ? d : momentum * m[i] + d;
    m[i] = buf;
    p[i] = pv - lr * buf;
  }
}

// ---- ts_sgd_apply_segments ----------------------------------------------------------------------------------------
// One workgroup iteration = one tile of TS_SGD_TILE elements: 256 lanes x 4 float4 per stream (p, g, m read; p, m
// written), all twelve 16-byte loads of a lane issued before the first use.  tile_first[t] names the slot that holds
// the tile's first element (built once on the host: the layout never changes), so finding the slot is ONE scalar load
// per tile and no second pass over the bucket.  Slots start on 16-element boundaries and a float4 starts on a 4-element
// one, so a float4 never straddles two slots.
//   * tile inside one slot (all but ~one tile per slot of a large layer): slot record, skip decision and
//     hyper-parameters are scalar loads from wave-uniform addresses, the skip is a uniform `continue`;
//   * tile with a slot boundary in it: each lane walks the slot offsets forward from the tile's first slot to its own.
// The loads of a whole tile are issued first and the slot is looked up under them (a skipped tile has read for nothing:
// the unused heads are a small share of the bytes).
// The padding between slots is processed like ts_sgd_apply processes it: p = g = m = 0 there, and
// d = 0 * gs + wd * 0 = 0, m = momentum * 0 + 0 = 0, p = 0 - lr * 0 = 0 - it stays zero.
__device__ __forceinline__ int64_t sgd_slot_end(const TsSgdSlot &r) { return r.offset + ((r.count + 15) & ~(int64_t)15); }

__device__ __forceinline__ bool sgd_slot_skipped(const TsSgdSlot &r, const float *__restrict__ flags) {
  // no gradient here this step; with several ranks the all-reduced flag says whether SOME rank had one (then the
  // averaged gradient is applied here too - DDP's rule - and the replicas stay identical)
  return r.unused != 0 && (flags == nullptr || flags[r.flag_index] == 0.f);
}

// exactly sgd_apply_kernel's roundings per element, so one group without Nesterov gives ts_sgd_apply's bits
// (tests/test_gpu_flat_optim.py holds the two kernels against each other); Nesterov is torch's
// d_p.add(buf, alpha = momentum)
__device__ __forceinline__ void sgd_elem(float &p, float g, float &m, float gs, float lr, float momentum,
                                         float weight_decay, int nesterov, int first) {
  const float pv = p;
  float d;
  {
    // sgd_apply_kernel's d is compiled as two rounded products and an add (its two multiplies pair into one packed
    // multiply before any contraction is tried); the fma chain after it is contracted in both kernels
#pragma clang fp contract(off)
    d = g * gs + weight_decay * pv;
  }
  const float buf = first ? d : momentum * m + d;
  m = buf;
  if (nesterov) {
    const float step = d + momentum * buf;
    p = pv - lr * step;
  } else {
    p = pv - lr * buf;
  }
}

__device__ __forceinline__ void sgd_vec(float4 &p, const float4 &g, float4 &m, float gs, const TsSgdGroup &h, int first) {
  sgd_elem(p.x, g.x, m.x, gs, h.lr, h.momentum, h.weight_decay, h.nesterov, first);
  sgd_elem(p.y, g.y, m.y, gs, h.lr, h.momentum, h.weight_decay, h.nesterov, first);
  sgd_elem(p.z, g.z, m.z, gs, h.lr, h.momentum, h.weight_decay, h.nesterov, first);
  sgd_elem(p.w, g.w, m.w, gs, h.lr, h.momentum, h.weight_decay, h.nesterov, first);
}

__global__ __launch_bounds__(256) void sgd_apply_segments_kernel(
    float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, int64_t n, const float *__restrict__ state,
    const TsSgdSlot *__restrict__ slots, int n_slots, const int32_t *__restrict__ tile_first, int64_t n_tiles,
    const float *__restrict__ flags, const TsSgdGroup *__restrict__ groups, int n_groups, TsSgdGroup one, int first) {
  // state[3] != 0: non-finite gradients, the step is skipped (GradScaler semantics) - asked before the first write, AFTER the
  // tile's loads are on their way: the scalar chain (state, tile_first -> slot record -> flag / group) runs under them
  const float skip_step = state[3], gs = state[2];
  constexpr int U = TS_SGD_TILE / (256 * 4);   // float4 per lane, stream and tile
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int64_t base = t * TS_SGD_TILE;
    const int64_t i0 = base + (int64_t)threadIdx.x * 4;
    if (base + TS_SGD_TILE <= n) {             // a whole tile (all but the bucket's last): the loads need nothing but `base`
      float4 pv[U], gv[U], mv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        pv[u] = *(const float4 *)(p + i0 + u * 1024);
        gv[u] = *(const float4 *)(g + i0 + u * 1024);
        mv[u] = *(const float4 *)(m + i0 + u * 1024);
      }
      if (skip_step != 0.f) return;
      const int s0 = min(max(tile_first[t], 0), n_slots - 1);
      const TsSgdSlot r0 = slots[s0];
      if (base + TS_SGD_TILE <= sgd_slot_end(r0)) {       // ... inside slot s0: everything about it is wave-uniform
        if (sgd_slot_skipped(r0, flags)) continue;
        TsSgdGroup h = one;
        if (groups) h = groups[min(max(r0.group, 0), n_groups - 1)];    // (a branch, not a select of addresses: scalar loads)
#pragma unroll
        for (int u = 0; u < U; ++u) {
          sgd_vec(pv[u], gv[u], mv[u], gs, h, first);
          *(float4 *)(m + i0 + u * 1024) = mv[u];
          *(float4 *)(p + i0 + u * 1024) = pv[u];
        }
      } else {                                 // ... with a slot boundary in it (about one tile per slot): every lane walks
        int s = s0;                            // from the tile's first slot to its own; i ascends with u, s only moves forward
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t i = i0 + u * 1024;
          while (s + 1 < n_slots && i >= slots[s + 1].offset) ++s;
          const TsSgdSlot r = slots[s];
          if (sgd_slot_skipped(r, flags)) continue;
          TsSgdGroup h = one;
          if (groups) h = groups[min(max(r.group, 0), n_groups - 1)];
          sgd_vec(pv[u], gv[u], mv[u], gs, h, first);
          *(float4 *)(m + i) = mv[u];
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
        if (sgd_slot_skipped(r, flags)) continue;
        TsSgdGroup h = one;
        if (groups) h = groups[min(max(r.group, 0), n_groups - 1)];
        float4 pw = *(const float4 *)(p + i);
        const float4 gw = *(const float4 *)(g + i);
        float4 mw = *(const float4 *)(m + i);
        sgd_vec(pw, gw, mw, gs, h, first);
        *(float4 *)(m + i) = mw;
        *(float4 *)(p + i) = pw;
      }
    }
  }
}

extern "C" int ts_sgd_grad_stats(const float *grad, int64_t n, double *sumsq, int32_t *nonfinite, ts_stream_t stream) {
  TS_REQUIRE(n >= 0 && sumsq && nonfinite, TS_ERR_INVALID_ARGUMENT, "ts_sgd_grad_stats: bad arguments");
  if (n == 0) return TS_OK;
  TS_REQUIRE(grad && (((uintptr_t)grad) & 15) == 0, TS_ERR_INVALID_ARGUMENT, "ts_sgd_grad_stats: grad must be 16-byte aligned");
  // few workgroups with long loops: every workgroup ends in ONE double atomic on the same address, and ~2000 of
  // those took longer (18 us) than reading the bucket
  const unsigned grid = (unsigned)std::min<int64_t>(ts_cdiv(n, 16384), 512);
  sgd_grad_stats_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(grad, n, sumsq, nonfinite);
  TS_CHECK_LAUNCH("ts_sgd_grad_stats");
  return TS_OK;
}

extern "C" int ts_sgd_decide(double *sumsq, int32_t *nonfinite, float *state, float max_norm, float growth,
                             float backoff, int32_t growth_interval, int32_t amp, ts_stream_t stream) {
  TS_REQUIRE(sumsq && nonfinite && state, TS_ERR_INVALID_ARGUMENT, "ts_sgd_decide: null pointer");
  sgd_decide_kernel<<<1, 1, 0, (hipStream_t)stream>>>(sumsq, nonfinite, state, max_norm, growth, backoff,
                                                      growth_interval, amp);
  TS_CHECK_LAUNCH("ts_sgd_decide");
  return TS_OK;
}

extern "C" int ts_sgd_apply(float *param, const float *grad, float *momentum_buf, int64_t n, const float *state,
                            float lr, float momentum, float weight_decay, int32_t first_step, ts_stream_t stream) {
  TS_REQUIRE(n >= 0 && state, TS_ERR_INVALID_ARGUMENT, "ts_sgd_apply: bad arguments");
  if (n == 0) return TS_OK;
  TS_REQUIRE(param && grad && momentum_buf, TS_ERR_INVALID_ARGUMENT, "ts_sgd_apply: null pointer");
  const unsigned grid = (unsigned)std::min<int64_t>(ts_cdiv(n, 256), 8192);
  sgd_apply_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(param, grad, momentum_buf, n, state, lr, momentum,
                                                          weight_decay, first_step);
  TS_CHECK_LAUNCH("ts_sgd_apply");
  return TS_OK;
}

extern "C" int ts_sgd_apply_segments(float *param, const float *grad, float *momentum_buf, int64_t n, const float *state,
                                     const TsSgdSlot *slots, int32_t n_slots, const int32_t *tile_first, int64_t n_tiles,
                                     const float *flags, const TsSgdGroup *groups, int32_t n_groups, float lr,
                                     float momentum, float weight_decay, int32_t nesterov, int32_t first_step,
                                     ts_stream_t stream) {
  TS_REQUIRE(n >= 0 && state && n_slots >= 0 && n_groups >= 1, TS_ERR_INVALID_ARGUMENT, "ts_sgd_apply_segments: bad arguments");
  if (n == 0 || n_slots == 0) return TS_OK;
  TS_REQUIRE(param && grad && momentum_buf && slots && tile_first, TS_ERR_INVALID_ARGUMENT,
             "ts_sgd_apply_segments: null pointer");
  TS_REQUIRE(n % 4 == 0 && ((((uintptr_t)param) | ((uintptr_t)grad) | ((uintptr_t)momentum_buf)) & 15) == 0,
             TS_ERR_INVALID_ARGUMENT, "ts_sgd_apply_segments: buckets must be 16-byte aligned and a multiple of 4 elements long");
  TS_REQUIRE(n_tiles == ts_cdiv(n, TS_SGD_TILE), TS_ERR_INVALID_ARGUMENT,
             "ts_sgd_apply_segments: tile_first must hold one entry per TS_SGD_TILE elements");
  TS_REQUIRE(groups || n_groups == 1, TS_ERR_INVALID_ARGUMENT, "ts_sgd_apply_segments: several groups need the device array");
  const TsSgdGroup one = {lr, momentum, weight_decay, nesterov};
  const unsigned grid = (unsigned)std::min<int64_t>(n_tiles, 2048);
  sgd_apply_segments_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(param, grad, momentum_buf, n, state, slots, n_slots,
                                                                   tile_first, n_tiles, flags, groups, n_groups, one,
                                                                   first_step);
  TS_CHECK_LAUNCH("ts_sgd_apply_segments");
  return TS_OK;
}
