// The clamp of the fused clouds as one stable compaction for a whole batch (taseg_amd/data/nuscenes.py, the mix path), and the
// scan pass that every compaction of csrc/compact.h shares.
// Reference (numpy, one sample at a time): R/pcseg/data/dataset/nuscenes/nuscenes_voxel_ms.py:122-125 and
// semantickitti/semantickitti_voxel_ms.py:121-124 - `point_ms[(point_ms[:, :3] >= point[:, :3].min(0)).all(1)]`.
//
// After a mix the current scan is no prefix of the fused cloud, so EVERY fused row is compared with its sample's minimum: the
// one-cloud driver of csrc/compact.h (cp_compact) with the clamp of csrc/stage_rules.h as the row rule, one tally per sample.
#include "compact.h"
#include "stage_rules.h"

namespace {

// the strided store: (x, y, z) as pass 3 read them, the further columns from the input row (q and o never overlap: as parameters
// they can say so, as members of a struct passed by value they cannot, and every load of q[k] would wait for the store before it)
__device__ __forceinline__ void cc_copy_row(const float *__restrict__ q, float *__restrict__ o, const float4 &p, int f) {
  o[0] = p.x;
  o[1] = p.y;
  o[2] = p.z;
  for (int k = 3; k < f; ++k) o[k] = q[k];
}

// VEC4: rows of four floats, 16-byte aligned - one 16-byte load and one 16-byte store per row, in both passes
template <bool VEC4>
struct CcRule : CpRule {
  typedef float4 Row;
  const float *pts;
  const int64_t *lab;
  const int *sample;
  const float *lo;
  float *out;
  int64_t *out_lab;
  int f;

  __device__ __forceinline__ bool keeps(int64_t i, bool in, float4 &p, int *s) const {
    *s = -1;
    if (!in) return false;
    *s = sample[i];
    if (VEC4) {
      p = reinterpret_cast<const float4 *>(pts)[i];
    } else {
      const float *q = pts + i * f;
      p = make_float4(q[0], q[1], q[2], 0.f);
    }
    return *s >= 0 && *s < n_samples && sr_clamp_keeps(p.x, p.y, p.z, lo, *s);
  }

  __device__ __forceinline__ void store(int64_t dst, int64_t i, const float4 &p) const {
    if (VEC4) {
      reinterpret_cast<float4 *>(out)[dst] = p;
    } else {
      cc_copy_row(pts + i * f, out + dst * f, p, f);
    }
    out_lab[dst] = lab[i];
  }
};

// blocks 0 .. n_clouds - 1: offs [n_clouds][n_blocks] = exclusive scans of blk_cnt, one block per cloud - every thread sums a
// contiguous chunk, the 256 chunk sums are scanned in LDS, every thread writes its chunk's running sums (a single wave walking
// 40 000 block counts 64 at a time waits for one load after the other);  block n_clouds + g: wave w sums row j = 4 g + w of
// blk_tally [n_tallies][n_blocks] into counts[j], the blocks lane-strided
__global__ __launch_bounds__(256) void cp_scan_kernel(int n_blocks, int n_clouds, int n_tallies, const int *__restrict__ blk_cnt,
                                                      const int *__restrict__ blk_tally, int *__restrict__ offs,
                                                      int64_t *__restrict__ counts) {
  __shared__ int part[256];
  const int lane = threadIdx.x & (TS_WAVE - 1), w = threadIdx.x / TS_WAVE;
  if ((int)blockIdx.x >= n_clouds) {
    const int j = ((int)blockIdx.x - n_clouds) * (256 / TS_WAVE) + w;
    if (j >= n_tallies) return;
    const int *row = blk_tally + (int64_t)j * n_blocks;
    int c = 0;                           // (n < 2^30 rows in all; integer sums: any order gives the same value)
    for (int b = lane; b < n_blocks; b += TS_WAVE) c += row[b];
    for (int d = TS_WAVE / 2; d > 0; d >>= 1) c += __shfl_xor(c, d);
    if (lane == 0) counts[j] = (int64_t)c;
    return;
  }
  const int *cnt = blk_cnt + (int64_t)blockIdx.x * n_blocks;
  int *out = offs + (int64_t)blockIdx.x * n_blocks;
  const int chunk = (n_blocks + 255) / 256;
  const int first = min((int)threadIdx.x * chunk, n_blocks), last = min(first + chunk, n_blocks);
  int sum = 0;
  for (int i = first; i < last; ++i) sum += cnt[i];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int t = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += t;
    __syncthreads();
  }
  int running = part[threadIdx.x] - sum;      // the block counts before this thread's chunk
  for (int i = first; i < last; ++i) {
    out[i] = running;
    running += cnt[i];
  }
}

}  // namespace

void ts_compact_scan(const CpWorkspace &c, int n_blocks, int n_clouds, int n_tallies, int64_t *counts, hipStream_t stream) {
  cp_scan_kernel<<<n_clouds + (int)ts_cdiv(n_tallies, 256 / TS_WAVE), 256, 0, stream>>>(n_blocks, n_clouds, n_tallies, c.blk_cnt,
                                                                                        c.blk_tally, c.offs, counts);
}

extern "C" size_t ts_stage_clamp_compact_workspace_bytes(int64_t n, int32_t n_samples) { return cp_compact_bytes(n, n_samples); }

extern "C" int ts_stage_clamp_compact(const float *points, int64_t n, int32_t point_stride, const int64_t *labels,
                                      const int32_t *sample, const float *lo, int32_t n_samples, float *out, int64_t *out_labels,
                                      int64_t *out_sample, int32_t *out_sample32, int64_t *counts, void *ws, size_t ws_bytes,
                                      ts_stream_t stream) {
  static_assert(TS_CLAMP_MAX_SAMPLES == TS_WAVE, "cp_count_kernel keeps one LDS counter per (wave, sample)");
  TS_REQUIRE(n >= 0 && n < (int64_t)1 << 30 && point_stride >= 3 && n_samples >= 1 && n_samples <= TS_CLAMP_MAX_SAMPLES,
             TS_ERR_INVALID_ARGUMENT, "ts_stage_clamp_compact: bad sizes");
  TS_REQUIRE(lo && counts && ws && ((uintptr_t)ws & 3) == 0, TS_ERR_INVALID_ARGUMENT, "ts_stage_clamp_compact: null pointer");
  TS_REQUIRE(n == 0 || (points && labels && sample && out && out_labels && out_sample && out_sample32), TS_ERR_INVALID_ARGUMENT,
             "ts_stage_clamp_compact: null pointer");
  const CpRule base = {n, n, n_samples, out_sample, out_sample32};          // (survivors <= rows: the outputs hold n rows)
  if (point_stride == 4 && ((((uintptr_t)points) | ((uintptr_t)out)) & 15) == 0)
    return cp_compact(CcRule<true>{base, points, labels, sample, lo, out, out_labels, point_stride}, "ts_stage_clamp_compact", counts,
                      ws, ws_bytes, (hipStream_t)stream);
  return cp_compact(CcRule<false>{base, points, labels, sample, lo, out, out_labels, point_stride}, "ts_stage_clamp_compact", counts,
                    ws, ws_bytes, (hipStream_t)stream);
}
