// Scan mixing of the training recipe on the device: PolarMix and LaserMix (taseg_amd/data/mix.py draws, this file moves rows).
// Reference (numpy in DataLoader workers, one sample at a time): R/pcseg/data/dataset/semantickitti/semantickitti_ms.py:151-237
// calling PolarMix_semantickitti.py:10-96 (swap: np.where / np.delete / np.concatenate; rotate_copy: np.where per class, np.dot)
// and LaserMix_semantickitti.py:11-219 (boolean masks per inclination band, np.concatenate); nuscenes/nuscenes_ms.py:132-214 with
// PolarMix_nuscenes.py / LaserMix_nuscenes.py.
//
// A mix is a stable multi-segment partition of the rows of two clouds plus two rotated copies of one block of segments.  JOBS (one
// per sample, any number per call) are concatenated job-major, cloud 1 before cloud 2; every job owns whole 256-row blocks.
// The three passes of csrc/compact.h, counted and ranked per SEGMENT (its ballot, rank and scan-step helpers; the scan kernel is
// this file's own: per job, over 18 segments):
//   1  mix_key_kernel      one lane per row: segment ids (A, B) of the row (B: the instance class of a cloud-2 row, which may ALSO
//                          be a sector row), and the rows per (block, segment)
//   2  mix_scan_kernel     one block per job: exclusive scan of those counts over the job's blocks, segment bases, the job's rows
//   3  mix_scatter_kernel  destination = job base + segment base + block offset + rank inside the block
// No atomics: the result is the reference's order and the same bits every run.
#include "compact.h"
#include "stage_rules.h"

#define MIX_NSEG (2 + TS_MIX_MAX_CLASSES)   // POLAR: 0 cloud 1 kept, 1 cloud 2's sector, 2 + k instance class k ; LASER: band j
#define MIX_DROP 0xFF
#define MIX_META (MIX_NSEG + 1)             // per job: segment bases, instance rows

namespace {

// the job that owns block b (record fields 21 / 22: first block, blocks); uniform over the block
__device__ __forceinline__ int mix_job_of_block(const double *__restrict__ rec, int n_jobs, int b) {
  int j = 0;
  for (int t = 0; t < n_jobs; ++t) {
    const int first = (int)rec[(int64_t)t * TS_MIX_RECORD + 21], nb = (int)rec[(int64_t)t * TS_MIX_RECORD + 22];
    if (b >= first && b < first + nb) j = t;
  }
  return j;
}

__global__ __launch_bounds__(CP_ROWS) void mix_key_kernel(const float *__restrict__ pts, int64_t n_rows, int f,
                                                           const int64_t *__restrict__ lab,
                                                           const unsigned char *__restrict__ keep,
                                                           const double *__restrict__ rec, const int *__restrict__ classes,
                                                           int n_jobs, uchar2 *__restrict__ keys, int *__restrict__ counts) {
#pragma clang fp contract(off)
  __shared__ int wcnt[MIX_NSEG][CP_WAVES];
  const int b = blockIdx.x, j = mix_job_of_block(rec, n_jobs, b);
  const double *q = rec + (int64_t)j * TS_MIX_RECORD;
  const int kind = (int)q[0];
  const int64_t n1 = (int64_t)q[17], n2 = (int64_t)q[18], row0 = (int64_t)q[19];
  const int64_t r = (int64_t)(b - (int)q[21]) * CP_ROWS + threadIdx.x;
  const int64_t row = row0 + r;
  unsigned char A = MIX_DROP, B = MIX_DROP;
  if (r < n1 + n2 && row < n_rows) {
    const bool second = r >= n1;
    const float *p = pts + row * f;
    const double X = p[0], Y = p[1], Z = p[2];
    if (kind == 2) {
      // PolarMix_semantickitti.py:12-17: yaw = -arctan2(y, x) on float32 columns; a row is in the sector iff alpha < yaw < beta
      const float yaw = (float)(-atan2(Y, X));
      const bool in = q[3] != 0.0 && yaw > (float)q[1] && yaw < (float)q[2];
      if (!second) {
        A = in ? MIX_DROP : 0;
      } else {
        A = in ? 1 : MIX_DROP;
        if (q[4] != 0.0) {
          // :37-40: instance rows grouped by class, in the list's order
          const int64_t l = lab[row];
          const int nk = (int)q[20];
          for (int k = 0; k < TS_MIX_MAX_CLASSES; ++k)
            if (k < nk && B == MIX_DROP && (int64_t)classes[j * TS_MIX_MAX_CLASSES + k] == l) B = (unsigned char)(2 + k);
        }
      }
    } else if (kind == 1) {
      // LaserMix_semantickitti.py:17-24 (:122-129 with `/ np.pi * 180`), float64: the cloud is concatenated with its int labels
      const double rho = sqrt(X * X + Y * Y);
      double inc = atan2(Z, rho);
      if (q[10] != 0.0) inc = inc / 3.141592653589793 * 180;
      int band = 0;
      const int nt = (int)q[11];
      for (int t = 0; t < 5; ++t)
        if (t < nt && inc <= q[12 + t]) ++band;
      // :43 concat(sup_p1, unsup_p2, sup_p3, ...): even bands (from 0) come from cloud 1, odd ones from cloud 2
      A = (inc == inc && ((band & 1) != 0) == second) ? (unsigned char)band : MIX_DROP;
    } else {
      A = second ? MIX_DROP : 0;
    }
    if (keep && keep[row] == 0) A = B = MIX_DROP;
    keys[row] = make_uchar2(A, B);
  }
  for (int s = 0; s < MIX_NSEG; ++s) cp_ballot(A == s || B == s, wcnt[s]);
  __syncthreads();
  if (threadIdx.x < MIX_NSEG) counts[(int64_t)b * MIX_NSEG + threadIdx.x] = cp_block_sum(wcnt[threadIdx.x]);
}

__global__ __launch_bounds__(256) void mix_scan_kernel(const double *__restrict__ rec, int n_blocks,
                                                       const int *__restrict__ counts, int *__restrict__ offs,
                                                       int64_t *__restrict__ meta, int64_t *__restrict__ totals) {
  __shared__ int seg_total[MIX_NSEG];
  const int j = blockIdx.x;
  const double *q = rec + (int64_t)j * TS_MIX_RECORD;
  const int first = (int)q[21];
  const int nb = min((int)q[22], n_blocks - first);
  const int lane = threadIdx.x & (TS_WAVE - 1), w = threadIdx.x / TS_WAVE;
  for (int s = w; s < MIX_NSEG; s += 256 / TS_WAVE) {
    int running = 0;
    for (int c = 0; c < nb; c += TS_WAVE) {
      const int i = c + lane;
      const int v = i < nb ? counts[(int64_t)(first + i) * MIX_NSEG + s] : 0;
      const int incl = cp_wave_inclusive(v, lane);
      if (i < nb) offs[(int64_t)(first + i) * MIX_NSEG + s] = running + incl - v;
      running += __shfl(incl, TS_WAVE - 1);
    }
    if (lane == 0) seg_total[s] = running;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t base = 0, inst = 0;
    for (int s = 0; s < MIX_NSEG; ++s) {
      meta[(int64_t)j * MIX_META + s] = base;
      base += seg_total[s];
      if (s >= 2) inst += seg_total[s];
    }
    if ((int)q[0] != 2) inst = 0;          // only PolarMix pastes rotated copies
    meta[(int64_t)j * MIX_META + MIX_NSEG] = inst;
    totals[j] = base + 2 * inst;
  }
}

// np.dot(xyz_f32, [[c, s, 0], [-s, c, 0], [0, 0, 1]]) stored into a float32 array (PolarMix_semantickitti.py:48-53): the rotation
// of csrc/stage_rules.h, one rounding to float32
__device__ __forceinline__ float4 mix_rotate(float4 p, double c, double s) {
  const double3 r = sr_rotate_z(p.x, p.y, p.z, c, s);
  return make_float4((float)r.x, (float)r.y, (float)r.z, p.w);
}

// one output row: xyz (and column 3 under VEC4) from `head`, the other columns from the source row - all of them (tail_all) or
// only column 3 with zeros behind it (PolarMix_nuscenes.py:51-53: np.zeros_like, then columns 0 .. 3)
template <bool VEC4>
__device__ __forceinline__ void mix_store(float *__restrict__ out, int64_t *__restrict__ out_lab, int *__restrict__ out_job,
                                          int64_t dst, int64_t cap, int f, float4 head, const float *__restrict__ src, bool tail_all,
                                          int64_t l, int j) {
  if (dst < 0 || dst >= cap) return;
  if (VEC4) {
    reinterpret_cast<float4 *>(out)[dst] = head;
  } else {
    float *w = out + dst * f;
    w[0] = head.x;
    w[1] = head.y;
    w[2] = head.z;
    for (int k = 3; k < f; ++k) w[k] = (tail_all || k == 3) ? src[k] : 0.f;
  }
  out_lab[dst] = l;
  out_job[dst] = j;
}

template <bool VEC4>
__global__ __launch_bounds__(CP_ROWS) void mix_scatter_kernel(const float *__restrict__ pts, int64_t n_rows, int f,
                                                               const int64_t *__restrict__ lab, const uchar2 *__restrict__ keys,
                                                               const double *__restrict__ rec, int n_jobs,
                                                               const int *__restrict__ offs, const int64_t *__restrict__ meta,
                                                               const int64_t *__restrict__ totals, float *__restrict__ out,
                                                               int64_t *__restrict__ out_lab, int *__restrict__ out_job,
                                                               int64_t cap) {
  __shared__ int wcnt[MIX_NSEG][CP_WAVES];
  __shared__ int64_t sbase[MIX_NSEG];
  __shared__ int64_t job_base;
  const int b = blockIdx.x, j = mix_job_of_block(rec, n_jobs, b);
  const double *q = rec + (int64_t)j * TS_MIX_RECORD;
  const int64_t n1 = (int64_t)q[17], n2 = (int64_t)q[18], row0 = (int64_t)q[19];
  const int64_t r = (int64_t)(b - (int)q[21]) * CP_ROWS + threadIdx.x;
  const int64_t row = row0 + r;
  const bool valid = r < n1 + n2 && row < n_rows;
  if (threadIdx.x < MIX_NSEG) sbase[threadIdx.x] = meta[(int64_t)j * MIX_META + threadIdx.x] + offs[(int64_t)b * MIX_NSEG + threadIdx.x];
  if (threadIdx.x == 0) {
    int64_t s = 0;
    for (int t = 0; t < j; ++t) s += totals[t];      // rows of the jobs before this one
    job_base = s;
  }
  unsigned char A = MIX_DROP, B = MIX_DROP;
  if (valid) {
    const uchar2 k = keys[row];
    A = k.x;
    B = k.y;
  }
  CpBallot ba = {}, bb = {};
  for (int s = 0; s < MIX_NSEG; ++s) {
    const CpBallot m = cp_ballot(A == s || B == s, wcnt[s]);
    if (A == s) ba = m;
    if (B == s) bb = m;
  }
  __syncthreads();
  if (!valid || (A == MIX_DROP && B == MIX_DROP)) return;
  float4 p;
  const float *src = pts + row * f;
  if (VEC4) {
    p = reinterpret_cast<const float4 *>(pts)[row];
  } else {
    p = make_float4(src[0], src[1], src[2], 0.f);
  }
  const int64_t l = lab[row];
  if (A < MIX_NSEG) {
    const int64_t dst = job_base + sbase[A] + cp_rank(ba, wcnt[A]);
    mix_store<VEC4>(out, out_lab, out_job, dst, cap, f, p, src, true, l, j);
  }
  if (B < MIX_NSEG) {
    const int64_t dst = job_base + sbase[B] + cp_rank(bb, wcnt[B]);
    const int64_t inst = meta[(int64_t)j * MIX_META + MIX_NSEG];
    const bool tail_all = q[9] != 0.0;
    mix_store<VEC4>(out, out_lab, out_job, dst, cap, f, p, src, true, l, j);
    mix_store<VEC4>(out, out_lab, out_job, dst + inst, cap, f, mix_rotate(p, q[5], q[6]), src, tail_all, l, j);
    mix_store<VEC4>(out, out_lab, out_job, dst + 2 * inst, cap, f, mix_rotate(p, q[7], q[8]), src, tail_all, l, j);
  }
}

struct MixWorkspace {
  uchar2 *keys;
  int *counts, *offs;
  int64_t *meta;
  size_t bytes;
};

MixWorkspace mix_carve(void *ws, int64_t n_rows, int64_t n_blocks, int64_t n_jobs) {
  MixWorkspace m;
  size_t at = 0;
  char *base = (char *)ws;
  m.meta = (int64_t *)(base + at);
  at += ts_align_up((size_t)n_jobs * MIX_META * sizeof(int64_t), 256);
  m.counts = (int *)(base + at);
  at += ts_align_up((size_t)n_blocks * MIX_NSEG * sizeof(int), 256);
  m.offs = (int *)(base + at);
  at += ts_align_up((size_t)n_blocks * MIX_NSEG * sizeof(int), 256);
  m.keys = (uchar2 *)(base + at);
  at += ts_align_up((size_t)n_rows * sizeof(uchar2), 256);
  m.bytes = at;
  return m;
}

}  // namespace

extern "C" size_t ts_stage_mix_workspace_bytes(int64_t n_rows, int64_t n_blocks, int32_t n_jobs) {
  return mix_carve(nullptr, std::max<int64_t>(n_rows, 0), std::max<int64_t>(n_blocks, 0), std::max(n_jobs, 0)).bytes;
}

extern "C" int ts_stage_mix(const float *points, int64_t n_rows, int32_t point_stride, const int64_t *labels, const uint8_t *keep,
                            const double *records, const int32_t *classes, int32_t n_jobs, int64_t n_blocks, float *out,
                            int64_t *out_labels, int32_t *out_job, int64_t capacity, int64_t *totals, void *ws, size_t ws_bytes,
                            ts_stream_t stream) {
  TS_REQUIRE(n_rows >= 0 && n_rows < (int64_t)1 << 30 && point_stride >= 3 && n_jobs > 0 && n_jobs <= 1024 && n_blocks >= 0 &&
                 n_blocks <= n_rows / CP_ROWS + n_jobs && capacity >= 0,
             TS_ERR_INVALID_ARGUMENT, "ts_stage_mix: bad sizes");
  TS_REQUIRE(records && classes && totals && ws && ((uintptr_t)ws & 7) == 0, TS_ERR_INVALID_ARGUMENT, "ts_stage_mix: null pointer");
  TS_REQUIRE(n_rows == 0 || (points && labels), TS_ERR_INVALID_ARGUMENT, "ts_stage_mix: null pointer");
  TS_REQUIRE(capacity == 0 || (out && out_labels && out_job), TS_ERR_INVALID_ARGUMENT, "ts_stage_mix: null pointer");
  const MixWorkspace m = mix_carve(ws, n_rows, n_blocks, n_jobs);
  TS_REQUIRE(ws_bytes >= m.bytes, TS_ERR_INVALID_ARGUMENT, "ts_stage_mix: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  if (n_blocks > 0) {
    mix_key_kernel<<<(int)n_blocks, CP_ROWS, 0, st>>>(points, n_rows, point_stride, labels, keep, records, classes, n_jobs, m.keys,
                                                       m.counts);
    TS_CHECK_LAUNCH("ts_stage_mix (keys)");
  }
  mix_scan_kernel<<<n_jobs, 256, 0, st>>>(records, (int)n_blocks, m.counts, m.offs, m.meta, totals);
  TS_CHECK_LAUNCH("ts_stage_mix (scan)");
  if (n_blocks > 0) {
    if (point_stride == 4 && ((((uintptr_t)points) | ((uintptr_t)out)) & 15) == 0) {
      mix_scatter_kernel<true><<<(int)n_blocks, CP_ROWS, 0, st>>>(points, n_rows, point_stride, labels, m.keys, records, n_jobs,
                                                                   m.offs, m.meta, totals, out, out_labels, out_job, capacity);
    } else {
      mix_scatter_kernel<false><<<(int)n_blocks, CP_ROWS, 0, st>>>(points, n_rows, point_stride, labels, m.keys, records, n_jobs,
                                                                    m.offs, m.meta, totals, out, out_labels, out_job, capacity);
    }
    TS_CHECK_LAUNCH("ts_stage_mix (scatter)");
  }
  return TS_OK;
}
