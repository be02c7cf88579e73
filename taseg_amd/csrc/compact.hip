// The clamp of the fused clouds as one stable compaction for a whole batch (taseg_amd/data/nuscenes.py, the mix path).
// Reference (numpy, one sample at a time): R/pcseg/data/dataset/nuscenes/nuscenes_voxel_ms.py:122-125 and
// semantickitti/semantickitti_voxel_ms.py:121-124 - `point_ms[(point_ms[:, :3] >= point[:, :3].min(0)).all(1)]`.
//
// After a mix the current scan is no prefix of the fused cloud, so EVERY fused row is compared with its sample's minimum.  Rows
// are handled in blocks of 256, in the idiom of csrc/mix.hip:
//   1  cc_count_kernel    one lane per row: the survivors per block (wave ballots) and per (block, sample)
//   2  cc_scan_kernel     one block: the survivors of every sample, exclusive scan of the block counts
//   3  cc_scatter_kernel  rank inside the block from wave ballots, destination = block offset + rank
// Order is decided by counts and ranks alone - no atomics - so the rows keep their input order and the bits are the same every run.
#include "common.h"

#define CC_ROWS 256
#define CC_WAVES (CC_ROWS / TS_WAVE)

namespace {

// numpy's `>=` on float32: false for NaN on either side
__device__ __forceinline__ bool cc_keeps(float x, float y, float z, const float *__restrict__ lo, int s, int n_samples) {
  if (s < 0 || s >= n_samples) return false;
  const float *q = lo + 3 * s;
  return x >= q[0] && y >= q[1] && z >= q[2];
}

__global__ __launch_bounds__(CC_ROWS) void cc_count_kernel(const float *__restrict__ pts, int64_t n, int f,
                                                           const int *__restrict__ sample, const float *__restrict__ lo,
                                                           int n_samples, int *__restrict__ blk_cnt,
                                                           int *__restrict__ blk_sample) {
  __shared__ int wcnt[CC_WAVES];
  __shared__ int scnt[CC_WAVES][TS_CLAMP_MAX_SAMPLES];
  const int64_t i = (int64_t)blockIdx.x * CC_ROWS + threadIdx.x;
  const int lane = threadIdx.x & (TS_WAVE - 1), w = threadIdx.x / TS_WAVE;
  scnt[w][lane] = 0;                    // (TS_CLAMP_MAX_SAMPLES == TS_WAVE: every wave clears its own row)
  __syncthreads();
  int s = -1;
  bool keep = false;
  if (i < n) {
    const float *p = pts + i * f;
    s = sample[i];
    keep = cc_keeps(p[0], p[1], p[2], lo, s, n_samples);
  }
  unsigned long long rem = __ballot(keep);
  if (lane == 0) wcnt[w] = __popcll(rem);
  // `sample` ascends: a wave holds one sample, or a few at a boundary - one round per distinct sample (rem is wave-uniform)
  while (rem) {
    const int s0 = __shfl(s, __ffsll((long long)rem) - 1);
    const unsigned long long m = __ballot(keep && s == s0);
    if (lane == 0) scnt[w][s0] += __popcll(m);
    rem &= ~m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
    for (int v = 0; v < CC_WAVES; ++v) c += wcnt[v];
    blk_cnt[blockIdx.x] = c;
  }
  if (threadIdx.x < n_samples) {
    int c = 0;
    for (int v = 0; v < CC_WAVES; ++v) c += scnt[v][threadIdx.x];
    blk_sample[(int64_t)blockIdx.x * n_samples + threadIdx.x] = c;
  }
}

__global__ __launch_bounds__(256) void cc_scan_kernel(int n_blocks, int n_samples, const int *__restrict__ blk_cnt,
                                                      const int *__restrict__ blk_sample, int *__restrict__ offs,
                                                      int64_t *__restrict__ counts) {
  const int lane = threadIdx.x & (TS_WAVE - 1), w = threadIdx.x / TS_WAVE;
  // the survivors of every sample: one wave per sample, the blocks lane-strided (integer sums: any order gives the same value)
  for (int s = w; s < n_samples; s += 256 / TS_WAVE) {
    int c = 0;                           // (n < 2^30 rows in all)
    for (int b = lane; b < n_blocks; b += TS_WAVE) c += blk_sample[(int64_t)b * n_samples + s];
    for (int d = TS_WAVE / 2; d > 0; d >>= 1) c += __shfl_xor(c, d);
    if (lane == 0) counts[s] = (int64_t)c;
  }
  if (w != 0) return;
  int running = 0;
  for (int c = 0; c < n_blocks; c += TS_WAVE) {
    const int i = c + lane;
    const int v = i < n_blocks ? blk_cnt[i] : 0;
    int incl = v;
    for (int d = 1; d < TS_WAVE; d <<= 1) {
      const int t = __shfl_up(incl, d);
      if (lane >= d) incl += t;
    }
    if (i < n_blocks) offs[i] = running + incl - v;
    running += __shfl(incl, TS_WAVE - 1);
  }
}

template <bool VEC4>
__global__ __launch_bounds__(CC_ROWS) void cc_scatter_kernel(const float *__restrict__ pts, int64_t n, int f,
                                                             const int64_t *__restrict__ lab, const int *__restrict__ sample,
                                                             const float *__restrict__ lo, int n_samples,
                                                             const int *__restrict__ offs, float *__restrict__ out,
                                                             int64_t *__restrict__ out_lab, int64_t *__restrict__ out_sample,
                                                             int *__restrict__ out_sample32) {
  __shared__ int wcnt[CC_WAVES];
  const int64_t i = (int64_t)blockIdx.x * CC_ROWS + threadIdx.x;
  const int lane = threadIdx.x & (TS_WAVE - 1), w = threadIdx.x / TS_WAVE;
  int s = -1;
  bool keep = false;
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < n) {
    s = sample[i];
    if (VEC4) {
      p = reinterpret_cast<const float4 *>(pts)[i];
    } else {
      const float *q = pts + i * f;
      p = make_float4(q[0], q[1], q[2], 0.f);
    }
    keep = cc_keeps(p.x, p.y, p.z, lo, s, n_samples);       // the comparison of pass 1 on the same bits
  }
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wcnt[w] = __popcll(m);
  __syncthreads();
  if (!keep) return;
  int64_t dst = (int64_t)offs[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (int v = 0; v < w; ++v) dst += wcnt[v];
  if (dst >= n) return;                                     // (cannot happen: survivors <= rows; bounds every store)
  if (VEC4) {
    reinterpret_cast<float4 *>(out)[dst] = p;
  } else {
    const float *q = pts + i * f;
    float *o = out + dst * f;
    o[0] = p.x;
    o[1] = p.y;
    o[2] = p.z;
    for (int k = 3; k < f; ++k) o[k] = q[k];
  }
  out_lab[dst] = lab[i];
  out_sample[dst] = s;
  out_sample32[dst] = s;
}

struct CcWorkspace {
  int *blk_cnt, *offs, *blk_sample;
  size_t bytes;
};

CcWorkspace cc_carve(void *ws, int64_t n_blocks, int64_t n_samples) {
  CcWorkspace c;
  size_t at = 0;
  char *base = (char *)ws;
  c.blk_cnt = (int *)(base + at);
  at += ts_align_up((size_t)n_blocks * sizeof(int), 256);
  c.offs = (int *)(base + at);
  at += ts_align_up((size_t)n_blocks * sizeof(int), 256);
  c.blk_sample = (int *)(base + at);
  at += ts_align_up((size_t)n_blocks * n_samples * sizeof(int), 256);
  c.bytes = std::max<size_t>(at, 256);
  return c;
}

}  // namespace

extern "C" size_t ts_stage_clamp_compact_workspace_bytes(int64_t n, int32_t n_samples) {
  return cc_carve(nullptr, ts_cdiv(std::max<int64_t>(n, 0), CC_ROWS), std::max(n_samples, 0)).bytes;
}

extern "C" int ts_stage_clamp_compact(const float *points, int64_t n, int32_t point_stride, const int64_t *labels,
                                      const int32_t *sample, const float *lo, int32_t n_samples, float *out, int64_t *out_labels,
                                      int64_t *out_sample, int32_t *out_sample32, int64_t *counts, void *ws, size_t ws_bytes,
                                      ts_stream_t stream) {
  static_assert(TS_CLAMP_MAX_SAMPLES == TS_WAVE, "cc_count_kernel clears one LDS row per wave");
  TS_REQUIRE(n >= 0 && n < (int64_t)1 << 30 && point_stride >= 3 && n_samples >= 1 && n_samples <= TS_CLAMP_MAX_SAMPLES,
             TS_ERR_INVALID_ARGUMENT, "ts_stage_clamp_compact: bad sizes");
  TS_REQUIRE(lo && counts && ws && ((uintptr_t)ws & 3) == 0, TS_ERR_INVALID_ARGUMENT, "ts_stage_clamp_compact: null pointer");
  TS_REQUIRE(n == 0 || (points && labels && sample && out && out_labels && out_sample && out_sample32), TS_ERR_INVALID_ARGUMENT,
             "ts_stage_clamp_compact: null pointer");
  const int64_t n_blocks = ts_cdiv(n, CC_ROWS);
  const CcWorkspace c = cc_carve(ws, n_blocks, n_samples);
  TS_REQUIRE(ws_bytes >= c.bytes, TS_ERR_INVALID_ARGUMENT, "ts_stage_clamp_compact: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  if (n_blocks > 0) {
    cc_count_kernel<<<(int)n_blocks, CC_ROWS, 0, st>>>(points, n, point_stride, sample, lo, n_samples, c.blk_cnt, c.blk_sample);
    TS_CHECK_LAUNCH("ts_stage_clamp_compact (count)");
  }
  cc_scan_kernel<<<1, 256, 0, st>>>((int)n_blocks, n_samples, c.blk_cnt, c.blk_sample, c.offs, counts);
  TS_CHECK_LAUNCH("ts_stage_clamp_compact (scan)");
  if (n_blocks > 0) {
    if (point_stride == 4 && ((((uintptr_t)points) | ((uintptr_t)out)) & 15) == 0) {
      cc_scatter_kernel<true><<<(int)n_blocks, CC_ROWS, 0, st>>>(points, n, point_stride, labels, sample, lo, n_samples, c.offs, out,
                                                                 out_labels, out_sample, out_sample32);
    } else {
      cc_scatter_kernel<false><<<(int)n_blocks, CC_ROWS, 0, st>>>(points, n, point_stride, labels, sample, lo, n_samples, c.offs,
                                                                  out, out_labels, out_sample, out_sample32);
    }
    TS_CHECK_LAUNCH("ts_stage_clamp_compact (scatter)");
  }
  return TS_OK;
}
