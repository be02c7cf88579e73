// The evaluation tail of the segmentors for a whole batch (R/pcseg/model/segmentor/voxel/minkunet/minkunet.py:435-455,
// minkunet_ms.py:433-458: per scene `out[scene mask][inverse_map of the scene]`, arg-max, trimmed to the scan's own points).
// The reference loops over the scenes with boolean masks (~12 launches and 6 host reads per scene); the tensor form of round 3 did
// the batch at once with three stable sorts by scene and ~45 small tensor ops - 1 ms of host time per pass, which made the
// evaluation loop under autocast host-bound.  Here:
//   ts_scene_counts  rows per scene of the voxel / point / label index arrays (+ are they grouped by scene in ascending order, as
//                    sparse_collate builds them?  + any index outside the batch?) - one launch, counters through LDS
//   ts_unvoxelise    mapped[p, :] = logits[start_v[scene_p] + inverse_map[p], :] and arg-max (first maximum), a wave per 64 / C
//                    points: rows of C <= 64 values move as whole rows - one launch
// For arrays grouped by scene (every collated batch) the scene-major order IS the array order: no sort.  Anything else is
// flagged, and the caller falls back to the sorted form (taseg_amd/pcseg/model/.../minkunet.py::unvoxelise_predictions).
// Second half of the file: evaluation that stays on the device (ts_eval_rows, ts_eval_confusion, ts_eval_votes and their _rows forms).
#include "common.h"
#include "compact.h"

#define ET_MAX_SCENES 64

__global__ __launch_bounds__(256) void scene_counts_kernel(const int *__restrict__ b0, int64_t s0, int64_t n0,
                                                           const int *__restrict__ b1, int64_t s1, int64_t n1,
                                                           const int *__restrict__ b2, int64_t s2, int64_t n2, int n_scenes,
                                                           unsigned long long *__restrict__ counts, int *__restrict__ flags) {
  __shared__ unsigned cnt[3][ET_MAX_SCENES];
  for (int i = threadIdx.x; i < 3 * ET_MAX_SCENES; i += 256) (&cnt[0][0])[i] = 0;
  __syncthreads();
  int bad = 0;
  const int64_t step = (int64_t)gridDim.x * 256;
  auto walk = [&](const int *b, int64_t stride, int64_t n, int which) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
      const int v = b[i * stride];
      if (v < 0 || v >= n_scenes) {
        bad |= 1;
      } else {
        atomicAdd(&cnt[which][v], 1u);
      }
      if (i > 0 && b[(i - 1) * stride] > v) bad |= 2;
    }
  };
  walk(b0, s0, n0, 0);
  walk(b1, s1, n1, 1);
  walk(b2, s2, n2, 2);
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * n_scenes; i += 256) {
    const unsigned c = cnt[i / n_scenes][i % n_scenes];
    if (c) atomicAdd(&counts[i], (unsigned long long)c);
  }
  if (bad) atomicOr(flags, bad);
}

extern "C" int ts_scene_counts(const int32_t *b_vox, int64_t stride_vox, int64_t n_vox, const int32_t *b_pts, int64_t stride_pts,
                               int64_t n_pts, const int32_t *b_lab, int64_t stride_lab, int64_t n_lab, int32_t n_scenes, int64_t *counts,
                               int32_t *flags, ts_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  TS_REQUIRE(n_scenes > 0 && n_scenes <= ET_MAX_SCENES && n_vox >= 0 && n_pts >= 0 && n_lab >= 0 && counts && flags &&
                 stride_vox > 0 && stride_pts > 0 && stride_lab > 0,
             TS_ERR_INVALID_ARGUMENT, "ts_scene_counts: bad arguments (at most %d scenes)", ET_MAX_SCENES);
  TS_REQUIRE((n_vox == 0 || b_vox) && (n_pts == 0 || b_pts) && (n_lab == 0 || b_lab), TS_ERR_INVALID_ARGUMENT, "ts_scene_counts: null pointer");
  TS_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)3 * n_scenes * 8, stream), "ts_scene_counts: memset");
  TS_CHECK_HIP(hipMemsetAsync(flags, 0, 4, stream), "ts_scene_counts: memset");
  const int64_t n = std::max(n_vox, std::max(n_pts, n_lab));
  if (n == 0) return TS_OK;
  const unsigned grid = (unsigned)std::min<int64_t>(ts_cdiv(n, 256 * 8), 1024);
  scene_counts_kernel<<<grid, 256, 0, stream>>>(b_vox, stride_vox, n_vox, b_pts, stride_pts, n_pts, b_lab, stride_lab, n_lab, n_scenes,
                                                (unsigned long long *)counts, flags);
  TS_CHECK_LAUNCH("ts_scene_counts");
  return TS_OK;
}

// one thread per (point, 4-column piece): a row of C values leaves as C / 4 16-byte stores (C % 4 == 0) or element-wise
template <typename T>
__global__ __launch_bounds__(256) void unvoxelise_kernel(const T *__restrict__ logits, int C, const long long *__restrict__ counts,
                                                         int n_scenes, const int *__restrict__ b_pts, int64_t stride_pts,
                                                         const long long *__restrict__ inv, int64_t n_pts, T *__restrict__ mapped,
                                                         long long *__restrict__ pred, int *__restrict__ flags) {
  __shared__ long long start[ET_MAX_SCENES + 1];
  if (threadIdx.x == 0) {
    long long acc = 0;
    for (int s = 0; s < n_scenes; ++s) {
      start[s] = acc;
      acc += counts[s];
    }
    start[n_scenes] = acc;
  }
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n_pts) return;
  const int scene = b_pts[p * stride_pts];
  const long long local = inv[p];
  long long row = -1;
  if (scene >= 0 && scene < n_scenes) {
    if (local >= 0 && local < start[scene + 1] - start[scene]) row = start[scene] + local;
  }
  if (row < 0) {
    atomicOr(flags, 4);                 // the reference's indexing would raise
    if (pred) pred[p] = 0;
    if (mapped)
      for (int c = 0; c < C; ++c) mapped[p * C + c] = (T)0.f;
    return;
  }
  const T *src = logits + row * C;
  float best = -INFINITY;
  int arg = 0;
  for (int c = 0; c < C; ++c) {
    const T v = src[c];
    if (mapped) mapped[p * C + c] = v;
    const float f = (float)v;
    if (f > best || (f != f && best == best)) {      // first maximum; a NaN wins like torch.argmax
      best = f;
      arg = c;
    }
  }
  if (pred) pred[p] = arg;
}

extern "C" int ts_unvoxelise(const void *logits, int32_t half, int32_t C, const int64_t *counts, int32_t n_scenes, const int32_t *b_pts,
                             int64_t stride_pts, const int64_t *inv, int64_t n_pts, void *mapped, int64_t *pred, int32_t *flags,
                             ts_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  TS_REQUIRE(C > 0 && C <= 4096 && n_scenes > 0 && n_scenes <= ET_MAX_SCENES && n_pts >= 0 && stride_pts > 0 && counts && flags,
             TS_ERR_INVALID_ARGUMENT, "ts_unvoxelise: bad arguments");
  if (n_pts == 0) return TS_OK;
  TS_REQUIRE(logits && b_pts && inv && (mapped || pred), TS_ERR_INVALID_ARGUMENT, "ts_unvoxelise: null pointer");
  const unsigned grid = (unsigned)ts_cdiv(n_pts, 256);
  if (half)
    unvoxelise_kernel<_Float16><<<grid, 256, 0, stream>>>((const _Float16 *)logits, C, (const long long *)counts, n_scenes, b_pts, stride_pts,
                                                          (const long long *)inv, n_pts, (_Float16 *)mapped, (long long *)pred, flags);
  else
    unvoxelise_kernel<float><<<grid, 256, 0, stream>>>((const float *)logits, C, (const long long *)counts, n_scenes, b_pts, stride_pts,
                                                       (const long long *)inv, n_pts, (float *)mapped, (long long *)pred, flags);
  TS_CHECK_LAUNCH("ts_unvoxelise");
  return TS_OK;
}

// ---------------------------------------------------------------------------------------------------- evaluation on the device
// What the trainer does with the eval dictionary (R/train.py:35-52, 465-540) without the dictionary: the logits of a batch become
// additions to a resident confusion matrix (validation) or the summed votes of one scan, their arg-max and the label payload (TTA).
//   ts_eval_rows       point_mask given (Ms models): the stable compaction of the kept points through cp_compact - per kept point
//                      its voxel index inside its scene, per scene the kept count K_s; three launches, no atomics for order
//   ts_eval_confusion  one launch: a lane per kept point j < m_s of scene s, arg-max of its logits row, tally through LDS
//   ts_eval_votes      one launch: a lane per point of the scan walks the votes in order (float32 sum in vote order: the bits of
//                      numpy's `total += logits[v]`), arg-max, payload store, optional sums / three largest sums
// Without a mask the kept points are a per-scene prefix of the point array: the reduce kernels index `inv` themselves.
//   ts_eval_confusion_rows / ts_eval_votes_rows  the same two launches for a model whose logits rows are NOT grouped by scene
//                      (Cylinder_TS: ascending hash over the batch): a point names its logits row itself (`grows`, the batch-wide
//                      hash lookup), labels are aligned with the points.  Same kernels, a second row rule in et_row.
// Every index is range-checked before it addresses a load: inverse map entries against the scene's voxel count AND the logits'
// row count, global rows against the logits' row count, point / label / table positions against the lengths of their arrays.

namespace {

struct EtRule : CpRule {
  typedef int Row;
  const unsigned char *mask;
  const int *b_pts;
  int64_t stride;
  const long long *inv;
  int *rows;

  __device__ __forceinline__ bool keeps(int64_t i, bool in, int &local, int *s) const {
    *s = -1;
    local = -1;
    if (!in || mask[i] == 0) return false;
    const int sc = b_pts[i * stride];
    if (sc < 0 || sc >= n_samples) return false;      // (ts_scene_counts has raised flag bit 0)
    *s = sc;
    const long long v = inv[i];
    local = (v < 0 || v > 0x7fffffffLL) ? -1 : (int)v;      // the reduce kernel checks it against the scene's voxel count
    return true;
  }

  __device__ __forceinline__ void store(int64_t dst, int64_t, const int &local) const { rows[dst] = local; }
};

struct EtScenes {                      // per-scene layout of a batch in LDS
  long long start_v[ET_MAX_SCENES], start_p[ET_MAX_SCENES], start_l[ET_MAX_SCENES], start_k[ET_MAX_SCENES];
  long long cnt_v[ET_MAX_SCENES], cnt_l[ET_MAX_SCENES];      // cnt_l: min(labels of the scene, num_points)
  long long m[ET_MAX_SCENES], start_m[ET_MAX_SCENES + 1];
  int flags;
};

struct EtBatch {
  const long long *counts;             // ts_scene_counts: [3][n_scenes]
  const int *scene_flags;              // ... and its flags
  int n_scenes;
  const long long *inv;                // no mask: [n_pts]
  const int *rows;                     // mask: ts_eval_rows' table [n_pts] ...
  const long long *kept;               // ... and counts [n_scenes]
  const long long *grows;              // the _rows calls: [n_pts] GLOBAL logits row of every point (-1: none); labels follow the points
  long long n_vox, n_pts, n_lab;
  const long long *num_points, *num_points_ms;
};

// every thread of the block calls it (n_scenes <= ET_MAX_SCENES <= blockDim.x); ends with a barrier
__device__ __forceinline__ void et_layout(const EtBatch &b, EtScenes &L) {
  const int t = threadIdx.x;
  if (t < b.n_scenes) {
    const long long cv = b.counts[t], cp = b.counts[b.n_scenes + t], cl = b.grows ? cp : b.counts[2 * b.n_scenes + t];
    const long long np0 = b.num_points[t], np = np0 > 0 ? np0 : 0;
    const long long k = b.kept ? b.kept[t] : cp;
    L.cnt_v[t] = cv;
    L.start_p[t] = cp;                 // (counts first, summed below)
    L.start_l[t] = cl;
    L.start_k[t] = k;
    L.cnt_l[t] = cl < np ? cl : np;
    L.m[t] = k < np ? k : np;
  }
  if (t == 0) L.flags = *b.scene_flags;
  __syncthreads();
  if (t < b.n_scenes && b.num_points_ms && b.num_points_ms[t] != L.start_p[t]) atomicOr(&L.flags, 32);
  __syncthreads();
  if (t == 0) {
    long long av = 0, ap = 0, al = 0, ak = 0, am = 0;
    for (int s = 0; s < b.n_scenes; ++s) {
      const long long cv = L.cnt_v[s], cp = L.start_p[s], cl = L.start_l[s], ck = L.start_k[s];
      L.start_v[s] = av;
      L.start_p[s] = ap;
      L.start_l[s] = al;
      L.start_k[s] = ak;
      L.start_m[s] = am;
      av += cv;
      ap += cp;
      al += cl;
      ak += ck;
      am += L.m[s];
    }
    L.start_m[b.n_scenes] = am;
  }
  __syncthreads();
}

// logits row of kept point j < m_s of scene s, -1 where the inverse map / the global row (or, cannot happen, a position) is out
// of range
__device__ __forceinline__ long long et_row(const EtBatch &b, const EtScenes &L, int s, long long j) {
  if (b.grows) {
    const long long at = L.start_p[s] + j;
    const long long r = (at >= 0 && at < b.n_pts) ? b.grows[at] : -1;
    return (r >= 0 && r < b.n_vox) ? r : -1;
  }
  long long local = -1;
  if (b.kept) {
    const long long at = L.start_k[s] + j;
    if (at >= 0 && at < b.n_pts) local = b.rows[at];
  } else {
    const long long at = L.start_p[s] + j;
    if (at >= 0 && at < b.n_pts) local = b.inv[at];
  }
  if (local < 0 || local >= L.cnt_v[s]) return -1;
  const long long r = L.start_v[s] + local;
  return r < b.n_vox ? r : -1;
}

__device__ __forceinline__ void et_argmax(float f, int c, float &best, int &arg) {
  if (f > best || (f != f && best == best)) {      // first maximum; a NaN wins (unvoxelise_kernel, torch.argmax, np.argmax)
    best = f;
    arg = c;
  }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void eval_confusion_kernel(const T *__restrict__ logits, int C, EtBatch b, const void *__restrict__ labels,
                                                             int label_bytes, unsigned long long *__restrict__ hist,
                                                             int *__restrict__ pred, long long pred_cap, long long *__restrict__ m_out,
                                                             int *__restrict__ flags) {
  __shared__ EtScenes L;
  __shared__ unsigned tab[32 * 32];
  const bool lds = C <= 32;
  if (lds)
    for (int i = threadIdx.x; i < C * C; i += 256) tab[i] = 0;
  et_layout(b, L);
  int bad = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) bad = L.flags;
  if (m_out && blockIdx.x == 0 && (int)threadIdx.x < b.n_scenes) m_out[threadIdx.x] = L.m[threadIdx.x];
  const int no_row = b.grows ? 64 : 4;
  const long long total = L.start_m[b.n_scenes], step = (long long)gridDim.x * 256;
  int s = 0;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += step) {
    while (s < b.n_scenes - 1 && q >= L.start_m[s + 1]) ++s;
    const long long j = q - L.start_m[s];
    const long long r = et_row(b, L, s, j);
    if (r < 0) {
      bad |= no_row;
      if (pred && q < pred_cap) pred[q] = 0;
      continue;
    }
    float best = -INFINITY;
    int arg = 0;
    if constexpr (VEC) {
      const float4 *src = reinterpret_cast<const float4 *>(logits + r * C);
      for (int c = 0; c < C; c += 4) {
        const float4 v = src[c >> 2];
        et_argmax(v.x, c, best, arg);
        et_argmax(v.y, c + 1, best, arg);
        et_argmax(v.z, c + 2, best, arg);
        et_argmax(v.w, c + 3, best, arg);
      }
    } else {
      const T *src = logits + r * C;
      for (int c = 0; c < C; ++c) et_argmax((float)src[c], c, best, arg);
    }
    if (pred && q < pred_cap) pred[q] = arg;
    if (L.cnt_l[s] != L.m[s]) continue;      // numpy would fail on the shapes: the scan contributes nothing (bit 3, below)
    const long long at = L.start_l[s] + j;
    if (at < 0 || at >= b.n_lab) continue;
    long long lab;
    if (label_bytes == 1)
      lab = ((const unsigned char *)labels)[at];
    else if (label_bytes == 4)
      lab = ((const int *)labels)[at];
    else
      lab = ((const long long *)labels)[at];
    if (lab < 0 || lab >= C) continue;       // fast_hist's k mask
    if (lds)
      atomicAdd(&tab[(int)lab * C + arg], 1u);
    else
      atomicAdd(&hist[lab * C + arg], 1ull);
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < b.n_scenes && L.cnt_l[threadIdx.x] != L.m[threadIdx.x]) bad |= 8;
  __syncthreads();
  if (lds)
    for (int i = threadIdx.x; i < C * C; i += 256) {
      const unsigned c = tab[i];
      if (c) atomicAdd(&hist[i], (unsigned long long)c);
    }
  if (bad) atomicOr(flags, bad);
}

#define ET_COLS 32       // the columns a lane sums in registers at once (a wider row takes ceil(C / 32) walks over the votes)

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void eval_votes_kernel(const T *__restrict__ logits, int C, EtBatch b, void *__restrict__ label,
                                                         int label_bytes, float *__restrict__ sums, float *__restrict__ top3,
                                                         long long cap, long long *__restrict__ n_out, int *__restrict__ flags) {
  __shared__ EtScenes L;
  et_layout(b, L);
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  int bad = first ? L.flags : 0;
  const long long n = L.m[0];
  bool equal = n <= cap;                 // (n <= n_pts / n_scenes <= cap follows from the counts; it bounds every store)
  for (int s = 1; s < b.n_scenes; ++s) equal = equal && L.m[s] == n;
  if (!equal) {                          // block-uniform: nothing is written
    if (first) atomicOr(flags, bad | 16);
    return;
  }
  if (first) *n_out = n;
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j < n) {
    float best = -INFINITY, t0 = -INFINITY, t1 = -INFINITY, t2 = -INFINITY;
    int arg = 0;
    for (int c0 = 0; c0 < C; c0 += ET_COLS) {
      float acc[ET_COLS];
#pragma unroll
      for (int k = 0; k < ET_COLS; ++k) acc[k] = 0.f;
      bool any = false;
      for (int v = 0; v < b.n_scenes; ++v) {
        const long long r = et_row(b, L, v, j);
        if (r < 0) {
          bad |= b.grows ? 64 : 4;
          continue;
        }
        const T *src = logits + r * C + c0;
        if constexpr (VEC) {
#pragma unroll
          for (int k = 0; k < ET_COLS; k += 4) {
            if (c0 + k < C) {
              const float4 x = *reinterpret_cast<const float4 *>(src + k);
              if (any) {
                acc[k] += x.x;
                acc[k + 1] += x.y;
                acc[k + 2] += x.z;
                acc[k + 3] += x.w;
              } else {
                acc[k] = x.x;
                acc[k + 1] = x.y;
                acc[k + 2] = x.z;
                acc[k + 3] = x.w;
              }
            }
          }
        } else {
#pragma unroll
          for (int k = 0; k < ET_COLS; ++k) {
            if (c0 + k < C) {
              const float x = (float)src[k];
              acc[k] = any ? acc[k] + x : x;
            }
          }
        }
        any = true;
      }
#pragma unroll
      for (int k = 0; k < ET_COLS; ++k) {
        if (c0 + k < C) {
          const float f = acc[k];
          et_argmax(f, c0 + k, best, arg);
          if (f > t0) {
            t2 = t1;
            t1 = t0;
            t0 = f;
          } else if (f > t1) {
            t2 = t1;
            t1 = f;
          } else if (f > t2) {
            t2 = f;
          }
          if (sums && !VEC) sums[j * C + c0 + k] = f;
        }
      }
      if (sums && VEC) {
#pragma unroll
        for (int k = 0; k < ET_COLS; k += 4)
          if (c0 + k < C) *reinterpret_cast<float4 *>(sums + j * C + c0 + k) = make_float4(acc[k], acc[k + 1], acc[k + 2], acc[k + 3]);
      }
    }
    if (label_bytes == 1)
      ((unsigned char *)label)[j] = (unsigned char)arg;
    else
      ((unsigned *)label)[j] = (unsigned)arg;
    if (top3) {
      top3[j * 3] = t0;
      top3[j * 3 + 1] = t1;
      top3[j * 3 + 2] = t2;
    }
  }
  if (bad) atomicOr(flags, bad);
}

int et_check_batch(const char *name, const void *logits, int32_t C, int64_t n_vox, const int64_t *counts, const int32_t *scene_flags,
                   int32_t n_scenes, const int64_t *inv, const int32_t *rows, const int64_t *kept, const int64_t *grows, int64_t n_pts,
                   const int64_t *num_points, int32_t *flags) {
  TS_REQUIRE(C > 0 && C <= 4096 && n_scenes > 0 && n_scenes <= ET_MAX_SCENES && n_vox >= 0 && n_pts >= 0 && n_vox < (int64_t)1 << 40 &&
                 n_pts < (int64_t)1 << 40,
             TS_ERR_INVALID_ARGUMENT, "%s: bad sizes (at most %d scenes)", name, ET_MAX_SCENES);
  TS_REQUIRE(counts && scene_flags && num_points && flags, TS_ERR_INVALID_ARGUMENT, "%s: null pointer", name);
  TS_REQUIRE(!(kept && inv) && !(rows && !kept) && !(grows && (inv || rows || kept)), TS_ERR_INVALID_ARGUMENT,
             "%s: either the inverse map or the table and counts of ts_eval_rows (the _rows calls: the global rows alone)", name);
  TS_REQUIRE(n_pts == 0 || ((grows || (kept ? rows != nullptr : inv != nullptr)) && (n_vox == 0 || logits)), TS_ERR_INVALID_ARGUMENT,
             "%s: null pointer", name);
  return TS_OK;
}

// the launches both forms of a call share: half rows element-wise, float rows as float4 where C and the pointers allow
int et_launch_confusion(const char *name, const void *logits, int32_t half, int32_t C, const EtBatch &b, const void *labels,
                        int32_t label_bytes, int64_t *hist, int32_t *pred, int64_t pred_cap, int64_t *m_out, int32_t *flags,
                        hipStream_t stream) {
  // (without points one block still runs: it carries ts_scene_counts' flags and the per-scene checks over)
  const unsigned grid = (unsigned)std::min<int64_t>(std::max<int64_t>(ts_cdiv(b.n_pts, 256), 1), 1024);
  unsigned long long *h = (unsigned long long *)hist;
  long long *m = (long long *)m_out;
  if (half)
    eval_confusion_kernel<_Float16, false><<<grid, 256, 0, stream>>>((const _Float16 *)logits, C, b, labels, label_bytes, h, pred, pred_cap, m,
                                                                     flags);
  else if (C % 4 == 0 && ((uintptr_t)logits & 15) == 0)
    eval_confusion_kernel<float, true><<<grid, 256, 0, stream>>>((const float *)logits, C, b, labels, label_bytes, h, pred, pred_cap, m, flags);
  else
    eval_confusion_kernel<float, false><<<grid, 256, 0, stream>>>((const float *)logits, C, b, labels, label_bytes, h, pred, pred_cap, m, flags);
  TS_CHECK_LAUNCH(name);
  return TS_OK;
}

int et_launch_votes(const char *name, const void *logits, int32_t half, int32_t C, const EtBatch &b, void *label, int32_t label_bytes,
                    float *sums, float *top3, int64_t cap, int64_t *n_out, int32_t *flags, hipStream_t stream) {
  TS_REQUIRE(cap >= 0 && n_out && (cap == 0 || label) && (label_bytes == 1 || label_bytes == 4) && (!top3 || C >= 3), TS_ERR_INVALID_ARGUMENT,
             "%s: bad arguments (labels of 1 or 4 bytes; the three largest sums need 3 classes)", name);
  TS_REQUIRE(label_bytes == 1 || ((uintptr_t)label & 3) == 0, TS_ERR_INVALID_ARGUMENT, "%s: unaligned label buffer", name);
  TS_REQUIRE(ts_cdiv(cap, 256) < (int64_t)1 << 31, TS_ERR_INVALID_ARGUMENT, "%s: too many rows", name);
  const unsigned grid = (unsigned)std::max<int64_t>(ts_cdiv(cap, 256), 1);
  if (half)
    eval_votes_kernel<_Float16, false><<<grid, 256, 0, stream>>>((const _Float16 *)logits, C, b, label, label_bytes, sums, top3, cap,
                                                                 (long long *)n_out, flags);
  else if (C % 4 == 0 && ((uintptr_t)logits & 15) == 0 && (!sums || ((uintptr_t)sums & 15) == 0))
    eval_votes_kernel<float, true><<<grid, 256, 0, stream>>>((const float *)logits, C, b, label, label_bytes, sums, top3, cap, (long long *)n_out,
                                                             flags);
  else
    eval_votes_kernel<float, false><<<grid, 256, 0, stream>>>((const float *)logits, C, b, label, label_bytes, sums, top3, cap,
                                                              (long long *)n_out, flags);
  TS_CHECK_LAUNCH(name);
  return TS_OK;
}

}  // namespace

extern "C" size_t ts_eval_rows_workspace_bytes(int64_t n_pts, int32_t n_scenes) {
  const int64_t n = std::max<int64_t>(n_pts, 0);
  return cp_compact_bytes(n, n_scenes) + ts_align_up((size_t)n * 8, 256) + ts_align_up((size_t)n * 4, 256);
}

extern "C" int ts_eval_rows(const uint8_t *point_mask, const int32_t *b_pts, int64_t stride_pts, const int64_t *inv, int64_t n_pts,
                            int32_t n_scenes, int32_t *rows, int64_t *kept, void *ws, size_t ws_bytes, ts_stream_t stream) {
  TS_REQUIRE(n_pts >= 0 && n_pts < (int64_t)1 << 30 && n_scenes >= 1 && n_scenes <= ET_MAX_SCENES && stride_pts > 0,
             TS_ERR_INVALID_ARGUMENT, "ts_eval_rows: bad sizes (at most %d scenes)", ET_MAX_SCENES);
  TS_REQUIRE(kept && ws && ((uintptr_t)ws & 7) == 0, TS_ERR_INVALID_ARGUMENT, "ts_eval_rows: null or unaligned pointer");
  TS_REQUIRE(n_pts == 0 || (point_mask && b_pts && inv && rows), TS_ERR_INVALID_ARGUMENT, "ts_eval_rows: null pointer");
  TS_REQUIRE(ws_bytes >= ts_eval_rows_workspace_bytes(n_pts, n_scenes), TS_ERR_WORKSPACE_TOO_SMALL, "ts_eval_rows: workspace too small");
  const size_t cp_bytes = cp_compact_bytes(n_pts, n_scenes);
  int64_t *sample64 = (int64_t *)((char *)ws + cp_bytes);      // the driver's per-survivor samples: not read here
  int32_t *sample32 = (int32_t *)((char *)sample64 + ts_align_up((size_t)n_pts * 8, 256));
  EtRule r;
  r.n_rows = n_pts;
  r.capacity = n_pts;
  r.n_samples = n_scenes;
  r.out_sample = sample64;
  r.out_sample32 = sample32;
  r.mask = point_mask;
  r.b_pts = b_pts;
  r.stride = stride_pts;
  r.inv = (const long long *)inv;
  r.rows = rows;
  return cp_compact(r, "ts_eval_rows", kept, ws, cp_bytes, (hipStream_t)stream);
}

extern "C" int ts_eval_confusion(const void *logits, int32_t half, int32_t C, int64_t n_vox, const int64_t *counts,
                                 const int32_t *scene_flags, int32_t n_scenes, const int64_t *inv, const int32_t *rows,
                                 const int64_t *kept, int64_t n_pts, const void *labels, int32_t label_bytes, int64_t n_lab,
                                 const int64_t *num_points, const int64_t *num_points_ms, int64_t *hist, int32_t *pred,
                                 int64_t pred_cap, int32_t *flags, ts_stream_t stream) {
  const int rc = et_check_batch("ts_eval_confusion", logits, C, n_vox, counts, scene_flags, n_scenes, inv, rows, kept, nullptr, n_pts,
                                num_points, flags);
  if (rc != TS_OK) return rc;
  TS_REQUIRE(hist && n_lab >= 0 && (n_lab == 0 || labels) && (label_bytes == 1 || label_bytes == 4 || label_bytes == 8) && pred_cap >= 0,
             TS_ERR_INVALID_ARGUMENT, "ts_eval_confusion: bad arguments (labels of 1, 4 or 8 bytes)");
  const EtBatch b = {(const long long *)counts, scene_flags, n_scenes, (const long long *)inv, rows, (const long long *)kept, nullptr,
                     n_vox, n_pts, n_lab, (const long long *)num_points, (const long long *)num_points_ms};
  return et_launch_confusion("ts_eval_confusion", logits, half, C, b, labels, label_bytes, hist, pred, pred_cap, nullptr, flags,
                             (hipStream_t)stream);
}

extern "C" int ts_eval_votes(const void *logits, int32_t half, int32_t C, int64_t n_vox, const int64_t *counts, const int32_t *scene_flags,
                             int32_t n_scenes, const int64_t *inv, const int32_t *rows, const int64_t *kept, int64_t n_pts,
                             const int64_t *num_points, const int64_t *num_points_ms, void *label, int32_t label_bytes, float *sums,
                             float *top3, int64_t cap, int64_t *n_out, int32_t *flags, ts_stream_t stream) {
  const int rc = et_check_batch("ts_eval_votes", logits, C, n_vox, counts, scene_flags, n_scenes, inv, rows, kept, nullptr, n_pts, num_points,
                                flags);
  if (rc != TS_OK) return rc;
  const EtBatch b = {(const long long *)counts, scene_flags, n_scenes, (const long long *)inv, rows, (const long long *)kept, nullptr,
                     n_vox, n_pts, 0, (const long long *)num_points, (const long long *)num_points_ms};
  return et_launch_votes("ts_eval_votes", logits, half, C, b, label, label_bytes, sums, top3, cap, n_out, flags, (hipStream_t)stream);
}

// The _rows forms: the point's logits row comes with the point (grows), the labels are aligned with the points (n_lab = n_pts,
// cnt_l = cnt_p in et_layout, so bit 3 cannot rise), no mask and no multi-scan counts.
extern "C" int ts_eval_confusion_rows(const void *logits, int32_t half, int32_t C, int64_t n_vox, const int64_t *counts,
                                      const int32_t *scene_flags, int32_t n_scenes, const int64_t *grows, int64_t n_pts,
                                      const void *labels, int32_t label_bytes, const int64_t *num_points, int64_t *hist, int32_t *pred,
                                      int64_t pred_cap, int64_t *m_out, int32_t *flags, ts_stream_t stream) {
  const int rc = et_check_batch("ts_eval_confusion_rows", logits, C, n_vox, counts, scene_flags, n_scenes, nullptr, nullptr, nullptr, grows,
                                n_pts, num_points, flags);
  if (rc != TS_OK) return rc;
  TS_REQUIRE(hist && (n_pts == 0 || (labels && grows)) && (label_bytes == 1 || label_bytes == 4 || label_bytes == 8) && pred_cap >= 0,
             TS_ERR_INVALID_ARGUMENT, "ts_eval_confusion_rows: bad arguments (labels of 1, 4 or 8 bytes)");
  const EtBatch b = {(const long long *)counts, scene_flags, n_scenes, nullptr, nullptr, nullptr, (const long long *)grows,
                     n_vox, n_pts, n_pts, (const long long *)num_points, nullptr};
  return et_launch_confusion("ts_eval_confusion_rows", logits, half, C, b, labels, label_bytes, hist, pred, pred_cap, m_out, flags,
                             (hipStream_t)stream);
}

extern "C" int ts_eval_votes_rows(const void *logits, int32_t half, int32_t C, int64_t n_vox, const int64_t *counts,
                                  const int32_t *scene_flags, int32_t n_scenes, const int64_t *grows, int64_t n_pts,
                                  const int64_t *num_points, void *label, int32_t label_bytes, float *sums, float *top3, int64_t cap,
                                  int64_t *n_out, int32_t *flags, ts_stream_t stream) {
  const int rc = et_check_batch("ts_eval_votes_rows", logits, C, n_vox, counts, scene_flags, n_scenes, nullptr, nullptr, nullptr, grows,
                                n_pts, num_points, flags);
  if (rc != TS_OK) return rc;
  TS_REQUIRE(n_pts == 0 || grows, TS_ERR_INVALID_ARGUMENT, "ts_eval_votes_rows: null pointer");
  const EtBatch b = {(const long long *)counts, scene_flags, n_scenes, nullptr, nullptr, nullptr, (const long long *)grows,
                     n_vox, n_pts, 0, (const long long *)num_points, nullptr};
  return et_launch_votes("ts_eval_votes_rows", logits, half, C, b, label, label_bytes, sums, top3, cap, n_out, flags, (hipStream_t)stream);
}
