// Moving-object augmentation of the SMSA recipe on the device (taseg_amd/data/moving.py draws, this file measures and moves rows).
// Reference (numpy in DataLoader workers, one sample at a time): R/pcseg/data/dataset/semantickitti/semantickitti_ms_ms.py:305-351
// `static2moving` and :353-384 `moving2static`, called at :152-163 for the sample and at :198-207 / :248-257 for its mix partner,
// on the current scan and the pose-fused, un-filtered history rows, BEFORE the class-step mask is applied (:165).
//
// Rows of a call: the current scans of all clouds (samples and partners), then their history rows; every row carries its FULL
// uint32 label (as int64), its cloud and - a history row - its frame offset.  An INSTANCE is a full label; the candidates of a
// cloud are the distinct full labels of its current rows with raw class 18, 20, 253 or 255, sorted, all clouds' tables one after
// the other (cand_start).
//   ts_stage_moving_stats
//     1  mov_init_kernel     counters and min / max cells of every candidate
//     2  mov_probe_kernel    one lane per row: the row's candidate (binary search in its cloud's table; a row of another raw
//                            class costs no probe), counts and float32 min / max with INTEGER atomics (exact, order-free), the
//                            matching rows per 256-row block (pass 1 of csrc/compact.h)
//     3  mov_scan_kernel     its own one-wave exclusive scan of those block counts: int64 offsets and the total, `matched`
//     4  mov_compact_kernel  the matching rows (candidate, x, y, kind) in ROW ORDER (pass 3 of csrc/compact.h)
//     5  mov_gather_kernel   one wave per candidate: its rows out of that list, in order: current x / y, history y, x / y at
//                            frame offset -1
//     6  mov_mean_kernel     one wave per (candidate, column): numpy's float32 mean - chunks of 8192, numpy's pairwise rule
//                            inside a chunk (eight running sums held by eight lanes), the chunk sums added in order, / (float)n
//   ts_stage_moving_apply    one lane per row: the row's record (binary search in the cloud's uploaded record table), centre
//                            shift, per-offset shift, raw-class rewrite, the mapped label through the 260-entry table
// No float atomics, order decided by counts and ranks alone: the same bits every run.
#include "compact.h"

#define MOV_NONE 0xFFFF
#define MOV_CHUNK 8192          // numpy's reduction buffer: a strided float32 column is summed in pieces of 8192
#define MOV_LEAF 128            // PW_BLOCKSIZE of numpy's pairwise sum
#define MOV_DEPTH 16

namespace {

// float32 <-> unsigned with the same order (finite values and infinities)
__device__ __forceinline__ unsigned mov_enc(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float mov_dec(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

__device__ __forceinline__ bool mov_class(int64_t l) {
  const int c = (int)(l & 0xFFFF);
  return c == 18 || c == 20 || c == 253 || c == 255;
}

// index of `key` in the sorted table[lo .. hi), or -1
__device__ __forceinline__ int mov_find(const int64_t *__restrict__ table, int lo, int hi, int64_t key) {
  const int end = hi;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (table[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return (lo < end && table[lo] == key) ? lo : -1;
}

__global__ __launch_bounds__(256) void mov_init_kernel(int cap, int *__restrict__ counts, unsigned *__restrict__ mm) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= cap) return;
  counts[3 * k] = counts[3 * k + 1] = counts[3 * k + 2] = 0;
  mm[4 * k] = mm[4 * k + 2] = 0xFFFFFFFFu;   // minima
  mm[4 * k + 1] = mm[4 * k + 3] = 0u;        // maxima
}

__global__ __launch_bounds__(CP_ROWS) void mov_probe_kernel(const float *__restrict__ pts, int64_t n_rows, int64_t n_cur, int f,
                                                             const int64_t *__restrict__ lab, const int *__restrict__ cloud,
                                                             const int *__restrict__ delta, const int64_t *__restrict__ cand,
                                                             const int *__restrict__ cand_start, int n_clouds, int cap,
                                                             unsigned short *__restrict__ slot, int *__restrict__ counts,
                                                             unsigned *__restrict__ mm, int *__restrict__ blk_cnt) {
  __shared__ int wcnt[CP_WAVES];
  const int64_t r = (int64_t)blockIdx.x * CP_ROWS + threadIdx.x;
  int s = -1;
  if (r < n_rows) {
    const int64_t l = lab[r];
    if (mov_class(l)) {
      const int c = cloud[r];
      if (c >= 0 && c < n_clouds) s = mov_find(cand, min(cand_start[c], cap), min(cand_start[c + 1], cap), l);
    }
    slot[r] = s < 0 ? (unsigned short)MOV_NONE : (unsigned short)s;
    if (s >= 0) {
      if (r < n_cur) {
        atomicAdd(&counts[3 * s], 1);
      } else {
        atomicAdd(&counts[3 * s + 1], 1);
        if (delta[r] == -1) atomicAdd(&counts[3 * s + 2], 1);
        const unsigned x = mov_enc(pts[r * f]), y = mov_enc(pts[r * f + 1]);
        atomicMin(&mm[4 * s], x);
        atomicMax(&mm[4 * s + 1], x);
        atomicMin(&mm[4 * s + 2], y);
        atomicMax(&mm[4 * s + 3], y);
      }
    }
  }
  cp_ballot(s >= 0, wcnt);
  __syncthreads();
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = cp_block_sum(wcnt);
}

// one wave: exclusive scan of blk_cnt into blk_off, the total into matched[0]
__global__ __launch_bounds__(TS_WAVE) void mov_scan_kernel(int64_t n_blocks, const int *__restrict__ blk_cnt,
                                                           int64_t *__restrict__ blk_off, int64_t *__restrict__ matched) {
  const int lane = threadIdx.x;
  int64_t running = 0;
  for (int64_t c = 0; c < n_blocks; c += TS_WAVE) {
    const int64_t i = c + lane;
    const int v = i < n_blocks ? blk_cnt[i] : 0;
    const int incl = cp_wave_inclusive(v, lane);
    if (i < n_blocks) blk_off[i] = running + incl - v;
    running += __shfl(incl, TS_WAVE - 1);
  }
  if (lane == 0) matched[0] = running;
}

__global__ __launch_bounds__(CP_ROWS) void mov_compact_kernel(const float *__restrict__ pts, int64_t n_rows, int64_t n_cur, int f,
                                                               const int *__restrict__ delta,
                                                               const unsigned short *__restrict__ slot,
                                                               const int64_t *__restrict__ blk_off, int64_t cap_rows,
                                                               unsigned short *__restrict__ l_slot,
                                                               unsigned char *__restrict__ l_kind, float *__restrict__ l_x,
                                                               float *__restrict__ l_y) {
  __shared__ int wcnt[CP_WAVES];
  const int64_t r = (int64_t)blockIdx.x * CP_ROWS + threadIdx.x;
  const unsigned short s = r < n_rows ? slot[r] : (unsigned short)MOV_NONE;
  const bool hit = s != MOV_NONE;
  const CpBallot b = cp_ballot(hit, wcnt);
  __syncthreads();
  if (!hit) return;
  const int64_t dst = blk_off[blockIdx.x] + cp_rank(b, wcnt);
  if (dst >= cap_rows) return;          // (the caller sees matched > cap_rows)
  l_slot[dst] = s;
  l_kind[dst] = r < n_cur ? 0 : (delta[r] == -1 ? 2 : 1);      // current | history | history at frame offset -1
  l_x[dst] = pts[r * f];
  l_y[dst] = pts[r * f + 1];
}

// one wave per candidate: its rows of the list, in order, into its own range [base, base + n_cur + n_hist) of v_x / v_y
// (current rows first) and the rows at frame offset -1 into p_x / p_y from `base`
__global__ __launch_bounds__(TS_WAVE) void mov_gather_kernel(const int *__restrict__ cand_start, int n_clouds, int cap,
                                                             const int *__restrict__ counts, const int64_t *__restrict__ matched,
                                                             int64_t cap_rows, const unsigned short *__restrict__ l_slot,
                                                             const unsigned char *__restrict__ l_kind,
                                                             const float *__restrict__ l_x, const float *__restrict__ l_y,
                                                             int64_t *__restrict__ c_base, float *__restrict__ v_x,
                                                             float *__restrict__ v_y, float *__restrict__ p_x,
                                                             float *__restrict__ p_y) {
  const int k = blockIdx.x, lane = threadIdx.x;
  const int n_cand = min(cand_start[n_clouds], cap);
  if (k >= n_cand) return;
  int64_t part = 0;
  for (int j = lane; j < k; j += TS_WAVE) part += counts[3 * j] + counts[3 * j + 1];
  for (int d = TS_WAVE / 2; d > 0; d >>= 1) part += __shfl_xor(part, d);
  const int64_t base = part, total = matched[0];
  const int64_t n_c = counts[3 * k], n_h = counts[3 * k + 1];
  if (total > cap_rows || base + n_c + n_h > cap_rows) {     // the list is cut short: no means (the caller raises)
    if (lane == 0) c_base[k] = -1;
    return;
  }
  if (lane == 0) c_base[k] = base;
  int64_t at_c = base, at_h = base + n_c, at_p = base;
  for (int64_t c = 0; c < total; c += TS_WAVE) {
    const int64_t i = c + lane;
    const bool mine = i < total && l_slot[i] == k;
    const int kind = mine ? l_kind[i] : -1;
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long mc = __ballot(kind == 0), mh = __ballot(kind >= 1), mp = __ballot(kind == 2);
    if (kind == 0) {
      const int64_t d = at_c + __popcll(mc & below);
      if (d < base + n_c) {
        v_x[d] = l_x[i];
        v_y[d] = l_y[i];
      }
    }
    if (kind >= 1) {
      const int64_t d = at_h + __popcll(mh & below);
      if (d < base + n_c + n_h) v_y[d] = l_y[i];
    }
    if (kind == 2) {
      const int64_t d = at_p + __popcll(mp & below);
      if (d < base + n_h) {
        p_x[d] = l_x[i];
        p_y[d] = l_y[i];
      }
    }
    at_c += __popcll(mc);
    at_h += __popcll(mh);
    at_p += __popcll(mp);
  }
}

// numpy's pairwise sum of a[0 .. n), n <= MOV_CHUNK, by one wave; lane j & 7 holds running sum j of a block of <= 128 terms.
// Every lane returns the sum.  (numpy/core/src/umath/loops_utils.h.src `pairwise_sum`: n < 8 sequential from 0; n <= 128 eight
// running sums, ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), the remainder sequentially; else split at n / 2 rounded down
// to a multiple of 8.)
__device__ float mov_pairwise(const float *__restrict__ a, int n, int lane8) {
#pragma clang fp contract(off)
  int off[MOV_DEPTH], len[MOV_DEPTH], state[MOV_DEPTH];
  float left[MOV_DEPTH];
  int sp = 0;
  off[0] = 0;
  len[0] = n;
  state[0] = 0;
  float ret = 0.f;
  while (sp >= 0) {
    const int o = off[sp], m = len[sp];
    if (m < 8) {
      float res = 0.f;
      for (int i = 0; i < m; ++i) res += a[o + i];
      ret = res;
      --sp;
    } else if (m <= MOV_LEAF || sp >= MOV_DEPTH - 1) {
      const int top = m - (m % 8);
      float r = a[o + lane8];
      for (int i = 8; i < top; i += 8) r += a[o + i + lane8];
      float t = r + __shfl_down(r, 1);
      t = t + __shfl_down(t, 2);
      t = t + __shfl_down(t, 4);
      float res = __shfl(t, 0);
      for (int i = top; i < m; ++i) res += a[o + i];
      ret = res;
      --sp;
    } else {
      int n2 = m / 2;
      n2 -= n2 % 8;
      if (state[sp] == 0) {
        state[sp] = 1;
        off[sp + 1] = o;
        len[sp + 1] = n2;
        state[sp + 1] = 0;
        ++sp;
      } else if (state[sp] == 1) {
        left[sp] = ret;
        state[sp] = 2;
        off[sp + 1] = o + n2;
        len[sp + 1] = m - n2;
        state[sp + 1] = 0;
        ++sp;
      } else {
        ret = left[sp] + ret;
        --sp;
      }
    }
  }
  return ret;
}

// column.mean() of a strided float32 column as numpy evaluates it: 0 + chunk sums in order, / (float)n  (0.f / 0.f = NaN for n = 0)
__device__ float mov_mean(const float *__restrict__ a, int64_t n, int lane8) {
#pragma clang fp contract(off)
  float total = 0.f;
  for (int64_t c = 0; c < n; c += MOV_CHUNK) total += mov_pairwise(a + c, (int)min((int64_t)MOV_CHUNK, n - c), lane8);
  return total / (float)n;
}

// grid (cap, 5): stats[k] = { min x, max x, min y, max y of the history rows, mean history y, mean x / y at frame offset -1,
// mean current x / y }
__global__ __launch_bounds__(TS_WAVE) void mov_mean_kernel(const int *__restrict__ cand_start, int n_clouds, int cap,
                                                           const int *__restrict__ counts, const unsigned *__restrict__ mm,
                                                           const int64_t *__restrict__ c_base, const float *__restrict__ v_x,
                                                           const float *__restrict__ v_y, const float *__restrict__ p_x,
                                                           const float *__restrict__ p_y, float *__restrict__ stats) {
  const int k = blockIdx.x, col = blockIdx.y, lane = threadIdx.x;
  if (k >= min(cand_start[n_clouds], cap)) return;
  const int64_t base = c_base[k], n_c = counts[3 * k], n_h = counts[3 * k + 1], n_p = counts[3 * k + 2];
  float *out = stats + (int64_t)k * TS_MOVING_STATS;
  if (col == 0 && lane < 4) {
    const float inf = __uint_as_float(0x7F800000u);
    out[lane] = n_h > 0 ? mov_dec(mm[4 * k + lane]) : ((lane & 1) ? -inf : inf);
  }
  float mean = __uint_as_float(0x7FC00000u);
  if (base >= 0) {
    const float *a = col == 0 ? v_y + base + n_c : col == 1 ? p_x + base : col == 2 ? p_y + base : col == 3 ? v_x + base : v_y + base;
    const int64_t n = col == 0 ? n_h : col <= 2 ? n_p : n_c;
    mean = mov_mean(a, n, lane & 7);
  }
  if (lane == 0) out[4 + col] = mean;
}

__global__ __launch_bounds__(256) void mov_apply_kernel(float *__restrict__ pts, int64_t n_rows, int64_t n_cur, int f,
                                                             const int64_t *__restrict__ lab, const int *__restrict__ cloud,
                                                             const int *__restrict__ delta, const int64_t *__restrict__ rec_lab,
                                                             const int *__restrict__ rec_start, int n_clouds,
                                                             const double *__restrict__ rec, const int64_t *__restrict__ lut,
                                                             int64_t *__restrict__ out_lab) {
#pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return;
  const int64_t l = lab[r];
  int raw = (int)(l & 0xFFFF);
  if (mov_class(l)) {
    const int c = cloud[r];
    const int s = (c >= 0 && c < n_clouds) ? mov_find(rec_lab, rec_start[c], rec_start[c + 1], l) : -1;
    if (s >= 0) {
      const double *q = rec + (int64_t)s * TS_MOVING_RECORD;
      const int kind = (int)q[0];
      float *p = pts + r * f;
      // semantickitti_ms_ms.py:322-329: `y -= center_shift` / `y += center_shift` on the instance's history AND current rows
      // (a float32 array and a Python float: the scalar is rounded to float32; field 1 holds it with its sign)
      if (kind == 1 && q[1] != 0.0) p[1] = p[1] + (float)q[1];
      if (r >= n_cur) {
        const int d = delta[r];
        // :331-344: += (delta_idx / step * shift), a Python float product rounded to float32, then float32 addition
        if (kind == 1) p[0] = p[0] + (float)((double)d * q[2]);
        if (kind == 2) p[1] = p[1] + (float)((double)d * q[2]);
        // :369-377: the shift is an np.float32, `delta_idx / step * shift` a float32 product
        if (kind == 3) {
          p[0] = p[0] + (float)d * (float)q[3];
          p[1] = p[1] + (float)d * (float)q[4];
        }
      }
      if (kind != 0) raw = (int)q[5];      // :346-349, :379-382
    }
  }
  out_lab[r] = raw < 260 ? lut[raw] : 0;
}

struct MovWorkspace {
  unsigned *mm;
  int *blk_cnt;
  int64_t *blk_off, *c_base;
  unsigned short *slot, *l_slot;
  unsigned char *l_kind;
  float *l_x, *l_y, *v_x, *v_y, *p_x, *p_y;
  size_t bytes;
};

MovWorkspace mov_carve(void *ws, int64_t n_rows, int64_t cap, int64_t cap_rows) {
  MovWorkspace m;
  size_t at = 0;
  char *base = (char *)ws;
  const int64_t n_blocks = ts_cdiv(n_rows, CP_ROWS);
  auto take = [&](size_t bytes) {
    char *p = base + at;
    at += ts_align_up(bytes, 256);
    return p;
  };
  m.blk_off = (int64_t *)take((size_t)n_blocks * sizeof(int64_t));
  m.c_base = (int64_t *)take((size_t)cap * sizeof(int64_t));
  m.mm = (unsigned *)take((size_t)cap * 4 * sizeof(unsigned));
  m.blk_cnt = (int *)take((size_t)n_blocks * sizeof(int));
  float **fl[] = {&m.l_x, &m.l_y, &m.v_x, &m.v_y, &m.p_x, &m.p_y};
  for (float **p : fl) *p = (float *)take((size_t)cap_rows * sizeof(float));
  m.slot = (unsigned short *)take((size_t)n_rows * sizeof(unsigned short));
  m.l_slot = (unsigned short *)take((size_t)cap_rows * sizeof(unsigned short));
  m.l_kind = (unsigned char *)take((size_t)cap_rows);
  m.bytes = at;
  return m;
}

}  // namespace

extern "C" size_t ts_stage_moving_workspace_bytes(int64_t n_rows, int32_t cap, int64_t cap_rows) {
  return mov_carve(nullptr, std::max<int64_t>(n_rows, 0), std::max(cap, 0), std::max<int64_t>(cap_rows, 0)).bytes;
}

extern "C" int ts_stage_moving_stats(const float *points, int64_t n_rows, int64_t n_cur, int32_t point_stride,
                                     const int64_t *labels, const int32_t *cloud, const int32_t *delta, const int64_t *cand,
                                     const int32_t *cand_start, int32_t n_clouds, int32_t cap, int64_t cap_rows, int32_t *counts,
                                     float *stats, int64_t *matched, void *ws, size_t ws_bytes, ts_stream_t stream) {
  TS_REQUIRE(n_rows >= 0 && n_rows < (int64_t)1 << 31 && n_cur >= 0 && n_cur <= n_rows && point_stride >= 2 && n_clouds > 0 &&
                 n_clouds <= 1024 && cap > 0 && cap <= TS_MOVING_MAX_CANDIDATES && cap_rows >= 0 && cap_rows < (int64_t)1 << 31,
             TS_ERR_INVALID_ARGUMENT, "ts_stage_moving_stats: bad sizes");
  TS_REQUIRE(cand && cand_start && counts && stats && matched && ws && ((uintptr_t)ws & 7) == 0, TS_ERR_INVALID_ARGUMENT,
             "ts_stage_moving_stats: null pointer");
  TS_REQUIRE(n_rows == 0 || (points && labels && cloud && delta), TS_ERR_INVALID_ARGUMENT, "ts_stage_moving_stats: null pointer");
  const MovWorkspace m = mov_carve(ws, n_rows, cap, cap_rows);
  TS_REQUIRE(ws_bytes >= m.bytes, TS_ERR_INVALID_ARGUMENT, "ts_stage_moving_stats: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_blocks = ts_cdiv(n_rows, CP_ROWS);
  mov_init_kernel<<<(int)ts_cdiv(cap, 256), 256, 0, st>>>(cap, counts, m.mm);
  TS_CHECK_LAUNCH("ts_stage_moving_stats (init)");
  if (n_blocks > 0) {
    mov_probe_kernel<<<(int)n_blocks, CP_ROWS, 0, st>>>(points, n_rows, n_cur, point_stride, labels, cloud, delta, cand, cand_start,
                                                         n_clouds, cap, m.slot, counts, m.mm, m.blk_cnt);
    TS_CHECK_LAUNCH("ts_stage_moving_stats (probe)");
  }
  mov_scan_kernel<<<1, TS_WAVE, 0, st>>>(n_blocks, m.blk_cnt, m.blk_off, matched);
  TS_CHECK_LAUNCH("ts_stage_moving_stats (scan)");
  if (n_blocks > 0) {
    mov_compact_kernel<<<(int)n_blocks, CP_ROWS, 0, st>>>(points, n_rows, n_cur, point_stride, delta, m.slot, m.blk_off, cap_rows,
                                                           m.l_slot, m.l_kind, m.l_x, m.l_y);
    TS_CHECK_LAUNCH("ts_stage_moving_stats (compact)");
  }
  mov_gather_kernel<<<cap, TS_WAVE, 0, st>>>(cand_start, n_clouds, cap, counts, matched, cap_rows, m.l_slot, m.l_kind, m.l_x, m.l_y,
                                             m.c_base, m.v_x, m.v_y, m.p_x, m.p_y);
  TS_CHECK_LAUNCH("ts_stage_moving_stats (gather)");
  mov_mean_kernel<<<dim3(cap, 5), TS_WAVE, 0, st>>>(cand_start, n_clouds, cap, counts, m.mm, m.c_base, m.v_x, m.v_y, m.p_x, m.p_y,
                                                    stats);
  TS_CHECK_LAUNCH("ts_stage_moving_stats (mean)");
  return TS_OK;
}

extern "C" int ts_stage_moving_apply(float *points, int64_t n_rows, int64_t n_cur, int32_t point_stride, const int64_t *labels,
                                     const int32_t *cloud, const int32_t *delta, const int64_t *rec_labels,
                                     const int32_t *rec_start, int32_t n_clouds, const double *records, const int64_t *lut,
                                     int64_t *out_labels, ts_stream_t stream) {
  TS_REQUIRE(n_rows >= 0 && n_rows < (int64_t)1 << 31 && n_cur >= 0 && n_cur <= n_rows && point_stride >= 2 && n_clouds > 0 &&
                 n_clouds <= 1024,
             TS_ERR_INVALID_ARGUMENT, "ts_stage_moving_apply: bad sizes");
  TS_REQUIRE(rec_start && lut, TS_ERR_INVALID_ARGUMENT, "ts_stage_moving_apply: null pointer");
  if (n_rows == 0) return TS_OK;
  TS_REQUIRE(points && labels && cloud && delta && out_labels, TS_ERR_INVALID_ARGUMENT, "ts_stage_moving_apply: null pointer");
  mov_apply_kernel<<<(int)ts_cdiv(n_rows, 256), 256, 0, (hipStream_t)stream>>>(
      points, n_rows, n_cur, point_stride, labels, cloud, delta, rec_labels, rec_start, n_clouds, records, lut, out_labels);
  TS_CHECK_LAUNCH("ts_stage_moving_apply");
  return TS_OK;
}
