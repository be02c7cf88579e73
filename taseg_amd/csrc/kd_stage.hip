// Both fused clouds of the mask-distillation recipe's batch from ONE pass over the pose-fused history (taseg_amd/data/kd.py).
// Reference (numpy, one sample at a time): R/pcseg/data/dataset/semantickitti/semantickitti_ms_kd.py:141-147 (the student's cloud
// `raw_data_ms`: history filtered by the pseudo labels under FLEXIBLE_STEPS; the teacher's `raw_data_ms_gt`: the SAME fused history
// filtered by the annotations under FLEXIBLE_STEPS_GT; :332-344 the two masks; :280-284 append_time_flag) and
// semantickitti_voxel_ms_kd.py:125-132 (both clouds clamped to the current scan's minimum; :88 `num_points_ms_gt` is taken BEFORE
// the clamp and never updated).
//
// Every history row is read once and written to up to two destinations: the three passes of csrc/compact.h over TWO clouds, with
// three tallies per sample (kept A / kept B / B's step rule before the clamp).  Its own:
//   lp_flags           the row rule: both class-step lookups and the clamp (csrc/stage_rules.h)
//   lp_scatter_kernel  history blocks: destination = current rows of the samples up to the row's own + block offset + rank;  current
//                      blocks: destination = index + kept history of the samples before the row's own (a running sum of the <= 64
//                      sample counts, in LDS), in both clouds
#include "compact.h"
#include "stage_rules.h"

#define LP_F 5                           // x, y, z, intensity, time flag

namespace {

struct LpRule {
  const unsigned char *table_a, *table_b;
  const int64_t *cls_a, *cls_b, *sample_of_scan;
  const int *scan;
  const float *lo;
  int n_scans, cols, neg_col, n_samples;
};

// bit 0: kept for A, bit 1: kept for B, bit 2: B's step rule alone (before the clamp); *sample = the row's sample or -1
__device__ __forceinline__ int lp_flags(const LpRule &r, int64_t i, float x, float y, float z, int *sample) {
  const int s = min(max(r.scan[i], 0), r.n_scans - 1);
  const int64_t b = r.sample_of_scan[s];
  *sample = -1;
  if (b < 0 || b >= r.n_samples) return 0;
  *sample = (int)b;
  const bool sa = sr_class_step(r.table_a, s, r.cls_a[i], r.cols, r.neg_col);
  const bool sb = sr_class_step(r.table_b, s, r.cls_b[i], r.cols, r.neg_col);
  const bool in = sr_clamp_keeps(x, y, z, r.lo, b);
  return (sa && in ? 1 : 0) | (sb && in ? 2 : 0) | (sb ? 4 : 0);
}

__global__ __launch_bounds__(CP_ROWS) void lp_count_kernel(const float *__restrict__ hist, int64_t n_hist, LpRule r,
                                                           int *__restrict__ blk_cnt, int *__restrict__ blk_tally) {
  __shared__ int wcnt[2][CP_WAVES];
  __shared__ int scnt[CP_WAVES][3 * TS_WAVE];
  const int64_t i = (int64_t)blockIdx.x * CP_ROWS + threadIdx.x;
  cp_tally_clear<3>(scnt);
  __syncthreads();
  int s = -1, fl = 0;
  if (i < n_hist) {
    const float *p = hist + i * 4;
    fl = lp_flags(r, i, p[0], p[1], p[2], &s);
  }
  const bool hit[3] = {(fl & 1) != 0, (fl & 2) != 0, (fl & 4) != 0};
  cp_ballot(hit[0], wcnt[0]);
  cp_ballot(hit[1], wcnt[1]);
  cp_tally_wave<3>(s, hit, scnt);
  __syncthreads();
  if (threadIdx.x < 2) blk_cnt[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = cp_block_sum(wcnt[threadIdx.x]);
  cp_tally_store<3>(scnt, 3 * r.n_samples, blk_tally);
}

struct LpOut {
  float *pts_a, *pts_b;
  int64_t *lab_a, *sample_a, *sample_b;
  int *sample32_a, *sample32_b;
  unsigned char *is_cur_a;
  int64_t capacity;
};

__device__ __forceinline__ void lp_store_row(float *__restrict__ pts, int64_t dst, float4 p, float flag) {
  float *o = pts + dst * LP_F;
  o[0] = p.x;
  o[1] = p.y;
  o[2] = p.z;
  o[3] = p.w;
  o[4] = flag;                           // append_time_flag (semantickitti_ms_kd.py:280-284)
}

template <bool VEC4>
__global__ __launch_bounds__(CP_ROWS) void lp_scatter_kernel(const float *__restrict__ cur, int64_t n_cur, int cur_stride,
                                                             const int64_t *__restrict__ cur_lab,
                                                             const int64_t *__restrict__ cur_start,
                                                             const float *__restrict__ hist, int64_t n_hist,
                                                             const int64_t *__restrict__ hist_lab, LpRule r, int n_hist_blocks,
                                                             const int *__restrict__ offs, const int64_t *__restrict__ counts,
                                                             LpOut o) {
  __shared__ int wcnt[2][CP_WAVES];
  __shared__ int64_t cs[TS_STAGE_PAIR_MAX_SAMPLES + 1];
  __shared__ int64_t kstart[2][TS_STAGE_PAIR_MAX_SAMPLES];   // kept history rows of the samples before s, cloud A and cloud B
  if (threadIdx.x <= r.n_samples) cs[threadIdx.x] = cur_start[threadIdx.x];
  if ((int)blockIdx.x < n_hist_blocks) {
    const int64_t i = (int64_t)blockIdx.x * CP_ROWS + threadIdx.x;
    int s = -1, fl = 0;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n_hist) {
      if (VEC4) {
        p = reinterpret_cast<const float4 *>(hist)[i];
      } else {
        const float *q = hist + i * 4;
        p = make_float4(q[0], q[1], q[2], q[3]);
      }
      fl = lp_flags(r, i, p.x, p.y, p.z, &s);               // the decisions of pass 1 on the same bits
    }
    const CpBallot ba = cp_ballot(fl & 1, wcnt[0]), bb = cp_ballot(fl & 2, wcnt[1]);
    __syncthreads();
    if (!(fl & 3)) return;
    const int64_t head = cs[s + 1];                         // the current rows of the samples up to the row's own
    if (fl & 1) {
      const int64_t dst = head + offs[blockIdx.x] + cp_rank(ba, wcnt[0]);
      if (dst >= 0 && dst < o.capacity) {                   // (cannot fail: kept rows <= rows; bounds every store)
        lp_store_row(o.pts_a, dst, p, 0.f);
        o.lab_a[dst] = hist_lab[i];
        o.sample_a[dst] = s;
        o.sample32_a[dst] = s;
        o.is_cur_a[dst] = 0;
      }
    }
    if (fl & 2) {
      const int64_t dst = head + offs[(int64_t)n_hist_blocks + blockIdx.x] + cp_rank(bb, wcnt[1]);
      if (dst >= 0 && dst < o.capacity) {
        lp_store_row(o.pts_b, dst, p, 0.f);
        o.sample_b[dst] = s;
        o.sample32_b[dst] = s;
      }
    }
    return;
  }
  if (threadIdx.x < 2) {
    int64_t run = 0;
    for (int s = 0; s < r.n_samples; ++s) {
      kstart[threadIdx.x][s] = run;
      run += counts[3 * s + threadIdx.x];
    }
  }
  __syncthreads();
  const int64_t i = (int64_t)(blockIdx.x - n_hist_blocks) * CP_ROWS + threadIdx.x;
  if (i >= n_cur) return;
  // the row's sample: the last s with cur_start[s] <= i (an empty sample shares its start with the next one)
  int lo = 0, hi = r.n_samples;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cs[mid] <= i) lo = mid; else hi = mid;
  }
  const int s = lo;
  const float *q = cur + i * cur_stride;
  const float4 p = make_float4(q[0], q[1], q[2], q[3]);
  const int64_t da = i + kstart[0][s], db = i + kstart[1][s];
  if (da >= 0 && da < o.capacity) {
    lp_store_row(o.pts_a, da, p, 1.f);
    o.lab_a[da] = cur_lab[i];
    o.sample_a[da] = s;
    o.sample32_a[da] = s;
    o.is_cur_a[da] = 1;
  }
  if (db >= 0 && db < o.capacity) {
    lp_store_row(o.pts_b, db, p, 1.f);
    o.sample_b[db] = s;
    o.sample32_b[db] = s;
  }
}

}  // namespace

extern "C" size_t ts_stage_layout_pair_workspace_bytes(int64_t n_hist, int32_t n_samples) {
  return cp_carve(nullptr, ts_cdiv(std::max<int64_t>(n_hist, 0), CP_ROWS), 2, 3 * (int64_t)std::max(n_samples, 0)).bytes;
}

extern "C" int ts_stage_layout_pair(const float *cur, int64_t n_cur, int32_t cur_stride, const int64_t *cur_labels,
                                    const int64_t *cur_start, const float *hist, int64_t n_hist, const int64_t *hist_labels,
                                    const int32_t *scan_idx, const int64_t *cls_a, const int64_t *cls_b, const uint8_t *table_a,
                                    const uint8_t *table_b, int32_t n_scans, int32_t table_cols, int32_t neg_col,
                                    const int64_t *sample_of_scan, const float *lo, int32_t n_samples, float *out_a,
                                    int64_t *out_labels_a, int64_t *out_sample_a, int32_t *out_sample32_a, uint8_t *out_is_cur_a,
                                    float *out_b, int64_t *out_sample_b, int32_t *out_sample32_b, int64_t capacity,
                                    int64_t *counts, void *ws, size_t ws_bytes, ts_stream_t stream) {
  static_assert(TS_STAGE_PAIR_MAX_SAMPLES == TS_WAVE, "lp_count_kernel keeps three LDS counters per (wave, sample)");
  static_assert(3 * TS_STAGE_PAIR_MAX_SAMPLES <= CP_ROWS, "lp_count_kernel writes one tally per lane");
  TS_REQUIRE(n_cur >= 0 && n_hist >= 0 && n_cur + n_hist < (int64_t)1 << 30 && cur_stride >= 4 && n_scans >= 1 &&
                 table_cols >= 1 && n_samples >= 1 && n_samples <= TS_STAGE_PAIR_MAX_SAMPLES && capacity >= n_cur + n_hist,
             TS_ERR_INVALID_ARGUMENT, "ts_stage_layout_pair: bad sizes");
  TS_REQUIRE(cur_start && lo && counts && ws, TS_ERR_INVALID_ARGUMENT, "ts_stage_layout_pair: null pointer");
  TS_REQUIRE(((uintptr_t)ws & 3) == 0, TS_ERR_INVALID_ARGUMENT, "ts_stage_layout_pair: the workspace must be 4-byte aligned");
  TS_REQUIRE(n_cur + n_hist == 0 ||
                 (out_a && out_labels_a && out_sample_a && out_sample32_a && out_is_cur_a && out_b && out_sample_b && out_sample32_b),
             TS_ERR_INVALID_ARGUMENT, "ts_stage_layout_pair: null pointer");
  TS_REQUIRE(n_cur == 0 || (cur && cur_labels), TS_ERR_INVALID_ARGUMENT, "ts_stage_layout_pair: null pointer");
  TS_REQUIRE(n_hist == 0 || (hist && hist_labels && scan_idx && cls_a && cls_b && table_a && table_b && sample_of_scan),
             TS_ERR_INVALID_ARGUMENT, "ts_stage_layout_pair: null pointer");
  const int64_t n_blocks = ts_cdiv(n_hist, CP_ROWS), n_cur_blocks = ts_cdiv(n_cur, CP_ROWS);
  const CpWorkspace c = cp_carve(ws, n_blocks, 2, 3 * n_samples);
  TS_REQUIRE(ws_bytes >= c.bytes, TS_ERR_INVALID_ARGUMENT, "ts_stage_layout_pair: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const LpRule r = {table_a, table_b, cls_a, cls_b, sample_of_scan, scan_idx, lo, n_scans, table_cols, neg_col, n_samples};
  if (n_blocks > 0) {
    lp_count_kernel<<<(int)n_blocks, CP_ROWS, 0, st>>>(hist, n_hist, r, c.blk_cnt, c.blk_tally);
    TS_CHECK_LAUNCH("ts_stage_layout_pair (count)");
  }
  ts_compact_scan(c, (int)n_blocks, 2, 3 * n_samples, counts, st);
  TS_CHECK_LAUNCH("ts_stage_layout_pair (scan)");
  if (n_blocks + n_cur_blocks > 0) {
    const LpOut o = {out_a, out_b, out_labels_a, out_sample_a, out_sample_b, out_sample32_a, out_sample32_b, out_is_cur_a, capacity};
    const int grid = (int)(n_blocks + n_cur_blocks);
    if ((((uintptr_t)hist) & 15) == 0) {
      lp_scatter_kernel<true><<<grid, CP_ROWS, 0, st>>>(cur, n_cur, cur_stride, cur_labels, cur_start, hist, n_hist, hist_labels, r,
                                                        (int)n_blocks, c.offs, counts, o);
    } else {
      lp_scatter_kernel<false><<<grid, CP_ROWS, 0, st>>>(cur, n_cur, cur_stride, cur_labels, cur_start, hist, n_hist, hist_labels,
                                                         r, (int)n_blocks, c.offs, counts, o);
    }
    TS_CHECK_LAUNCH("ts_stage_layout_pair (scatter)");
  }
  return TS_OK;
}
