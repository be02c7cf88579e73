// The cylinder data stage on the device (taseg_amd/data/cylinder.py).
// Reference (host numpy in a DataLoader worker, one sample at a time):
//   pcseg/data/dataset/semantickitti/semantickitti_cylinder.py:19-22    cart2polar
//   :144-160  polar coordinates in degrees, clip, cell, voxel centres, the feature row
//   :32-45    voxelize_with_label: sparse_quantize + a Python loop over every point + argmax
//   :176-219  collate_batch (inverse_map concatenated WITHOUT an offset: local to its sample)
// Two memory-bound passes around the stable radix sort of csrc/quantize_keys.h: ts_cylinder_cells (one lane per row, no reuse,
// no LDS) and the chain of ts_cylinder_voxels (head flags, scan, per-sample starts, scatter, vote).  This file is compiled with
// -ffp-contract=off (csrc/build.py): every operation below keeps its own rounding, as numpy's.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "common.h"
#include "quantize_keys.h"

namespace {

struct CylSpace {
  double lo[3], hi[3], step[3];
};

// 16-byte pieces of a feature row: rows of 5 + F floats start on a 4-byte boundary only
typedef float cyl_f4 __attribute__((ext_vector_type(4), aligned(4)));

// floor((clip(v, lo, hi) - lo) / step) in float64 (:153; numpy promotes the float32 polar array to float64 against the bounds).
// The comparisons are numpy's minimum(maximum(v, lo), hi); v is finite here.
__device__ __forceinline__ int cyl_cell(float v, double lo, double hi, double step) {
  double c = (double)v;
  c = c < lo ? lo : c;
  c = c > hi ? hi : c;
  return (int)floor((c - lo) / step);
}

// (float32(cell) + 0.5) * step + lo (:156, :158): the sum in float32 (exact), product and sum in float64, one rounding to float32
__device__ __forceinline__ float cyl_centre(int cell, double lo, double step) {
  const double h = (double)((float)cell + 0.5f);
  const double prod = h * step;
  return (float)(prod + lo);
}

template <int F>       // F = 4, 5: the row length known (F = 4 rows 16-byte aligned: one 16-byte load); 0: any F >= 4
__global__ __launch_bounds__(256) void cyl_cells_kernel(const float *__restrict__ pts, int64_t n, int pstride,
                                                        const int *__restrict__ sample, const CylSpace sp,
                                                        int4 *__restrict__ cells, longlong4 *__restrict__ coord,
                                                        float *__restrict__ feat, int *__restrict__ flag) {
  const int f = F ? F : pstride;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    float x, y, z, w;
    if (F == 4) {
      const float4 p = reinterpret_cast<const float4 *>(pts)[i];
      x = p.x, y = p.y, z = p.z, w = p.w;
    } else {
      const float *r = pts + i * f;
      x = r[0], y = r[1], z = r[2], w = r[3];
    }
    const int b = sample ? sample[i] : 0;
    // :20-21, :145: rho and the degrees in float32; phi is the float64 arc tangent rounded once (include/taseg_hip.h)
    const float rho = (float)sqrt((double)__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)));   // (correctly rounded: 53 >= 2 * 24 + 2)
    const float phi = (float)atan2((double)y, (double)x);
    const float deg = __fmul_rn(__fdiv_rn(phi, 3.14159274f), 180.f);
    int cx = 0, cy = 0, cz = 0;
    if (isfinite(x) && isfinite(y) && isfinite(z)) {
      cx = cyl_cell(rho, sp.lo[0], sp.hi[0], sp.step[0]);
      cy = cyl_cell(deg, sp.lo[1], sp.hi[1], sp.step[1]);
      cz = cyl_cell(z, sp.lo[2], sp.hi[2], sp.step[2]);
    } else {
      *flag = TS_CYL_FLAG_NONFINITE;          // (every writer stores the same word)
    }
    cells[i] = make_int4(cx, cy, cz, b);
    longlong4 c64;
    c64.x = cx, c64.y = cy, c64.z = cz, c64.w = b;
    coord[i] = c64;
    float *o = feat + i * (int64_t)(f + 5);
    cyl_f4 a, q;
    a[0] = cyl_centre(cx, sp.lo[0], sp.step[0]);
    a[1] = cyl_centre(cy, sp.lo[1], sp.step[1]);
    a[2] = cyl_centre(cz, sp.lo[2], sp.step[2]);
    a[3] = rho;
    q[0] = deg;
    q[1] = z;
    q[2] = x;
    q[3] = y;
    *reinterpret_cast<cyl_f4 *>(o) = a;
    *reinterpret_cast<cyl_f4 *>(o + 4) = q;
    o[8] = w;
    if (F != 4)
      for (int k = 4; k < f; ++k) o[5 + k] = pts[i * f + k];
  }
}

// start[b] = rank of the first voxel of a sample >= b (b = 0 .. n_samples; start[n_samples] = m), counts[b] = voxels of sample b,
// counts[n_samples] = m.  One workgroup; the sorted keys carry the sample in their top bits.
__global__ __launch_bounds__(256) void cyl_starts_kernel(const uint64_t *__restrict__ keys, const unsigned *__restrict__ ranks,
                                                         int64_t n, int n_samples, int *__restrict__ start,
                                                         int *__restrict__ counts) {
  for (int b = threadIdx.x; b <= n_samples; b += blockDim.x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int)(keys[mid] >> TQ_BATCH_SHIFT) < b) lo = mid + 1; else hi = mid;
    }
    // the first row of a sample heads a run: its inclusive rank - 1 is the voxel's rank
    start[b] = lo < n ? (int)ranks[lo] - 1 : (int)ranks[n - 1];
  }
  __syncthreads();
  for (int b = threadIdx.x; b <= n_samples; b += blockDim.x)
    counts[b] = b < n_samples ? start[b + 1] - start[b] : start[n_samples];
}

// Sorted position i: v = ranks[i] - 1 its voxel.  The head of a run names the voxel's representative (its first row in input order)
// and where the run begins; every row learns its voxel's rank inside its own sample.
__global__ __launch_bounds__(256) void cyl_scatter_kernel(const uint64_t *__restrict__ keys, const int *__restrict__ vals,
                                                          const unsigned *__restrict__ ranks, int64_t n, int n_samples,
                                                          const int *__restrict__ start, const int *__restrict__ err,
                                                          int *__restrict__ out_index, int64_t *__restrict__ out_inverse,
                                                          int *__restrict__ run, int *__restrict__ flag) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  if (i == 0 && *err) *flag = TS_CYL_FLAG_RANGE;
  for (; i < n; i += step) {
    const int v = (int)ranks[i] - 1;
    const uint64_t key = keys[i];
    const int src = vals[i];
    if (i == 0 || key != keys[i - 1]) {
      out_index[v] = src;
      run[v] = (int)i;
    }
    if (i == n - 1) run[v + 1] = (int)n;
    const int b = min((int)(key >> TQ_BATCH_SHIFT), n_samples - 1);
    out_inverse[src] = (int64_t)(v - start[b]);
  }
}

// The majority vote (:38-43).  32 lanes per voxel, lane c counts class c in an integer register: the lanes load 32 labels of the run
// at once, then every lane sees each of them through a shuffle; a run longer than 32 rows loops.  An ignored label matches no lane.
// arg-max over the 32 lanes: more votes win, equal votes go to the lower class (np.argmax's first maximum), no vote at all leaves
// class 0.  No table in memory, no atomics, integer arithmetic only: the same bits every run.
__global__ __launch_bounds__(256) void cyl_vote_kernel(const int *__restrict__ vals, const int *__restrict__ run,
                                                       const int64_t *__restrict__ labels, const int *__restrict__ counts,
                                                       int n_samples, int num_classes, int64_t ignore_label,
                                                       int64_t *__restrict__ voxel_label, int *__restrict__ flag) {
  const int m = counts[n_samples];
  const int lane = threadIdx.x & 31;
  const int64_t groups = (int64_t)gridDim.x * (blockDim.x >> 5);
  // (the 32 lanes of a group take every branch below together: the width-32 shuffles always find their whole group active)
  for (int64_t v = (int64_t)blockIdx.x * (blockDim.x >> 5) + (threadIdx.x >> 5); v < m; v += groups) {
    const int beg = run[v], end = run[v + 1];
    int cnt = 0;
    bool bad = false;
    for (int at = beg; at < end; at += 32) {
      const int e = at + lane;
      int lab = -1;
      if (e < end) {
        const int64_t l = labels[vals[e]];
        if (l == ignore_label) lab = -1;                       // (:41, before the class is looked at)
        else if (l >= 0 && l < num_classes) lab = (int)l;
        else bad = true;
      }
      const int have = min(end - at, 32);
      for (int k = 0; k < have; ++k) cnt += (__shfl(lab, k, 32) == lane) ? 1 : 0;
    }
    if (bad) *flag = TS_CYL_FLAG_LABEL;
    int best = cnt, cls = lane;
#pragma unroll
    for (int d = 16; d > 0; d >>= 1) {
      const int oc = __shfl_xor(best, d, 32), ol = __shfl_xor(cls, d, 32);
      const bool take = oc > best || (oc == best && ol < cls);
      best = take ? oc : best;
      cls = take ? ol : cls;
    }
    if (lane == 0) voxel_label[v] = cls;
  }
}

}  // namespace

extern "C" int ts_cylinder_cells(const float *points, int64_t n, int32_t point_stride, const int32_t *sample_idx,
                                 const double *space, int32_t *cells, int64_t *point_coord, float *point_feature,
                                 int32_t *flag, ts_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  TS_REQUIRE(n >= 0 && n < (1LL << 30), TS_ERR_INVALID_ARGUMENT, "ts_cylinder_cells: bad n");
  TS_REQUIRE(point_stride >= 4 && point_stride <= 64, TS_ERR_UNSUPPORTED,
             "ts_cylinder_cells: rows of 4 .. 64 floats (x, y, z, intensity, ...), got %d", point_stride);
  TS_REQUIRE(space, TS_ERR_INVALID_ARGUMENT, "ts_cylinder_cells: null space");
  CylSpace sp;
  for (int d = 0; d < 3; ++d) {
    sp.lo[d] = space[d];
    sp.hi[d] = space[3 + d];
    sp.step[d] = space[6 + d];
    TS_REQUIRE(sp.hi[d] > sp.lo[d] && sp.step[d] > 0.0 && (sp.hi[d] - sp.lo[d]) / sp.step[d] < (double)TQ_CBIAS,
               TS_ERR_INVALID_ARGUMENT, "ts_cylinder_cells: need min < max, interval > 0 and fewer than 2^17 cells on axis %d", d);
  }
  if (n == 0) return TS_OK;
  TS_REQUIRE(points && cells && point_coord && point_feature && flag, TS_ERR_INVALID_ARGUMENT, "ts_cylinder_cells: null pointer");
  TS_REQUIRE(((uintptr_t)cells & 15) == 0 && ((uintptr_t)point_coord & 31) == 0 && ((uintptr_t)point_feature & 3) == 0,
             TS_ERR_INVALID_ARGUMENT, "ts_cylinder_cells: cells must be 16-byte, point_coord 32-byte aligned");
  const int grid = (int)std::min<int64_t>(ts_cdiv(n, 256), 4096);
  int4 *c4 = (int4 *)cells;
  longlong4 *c8 = (longlong4 *)point_coord;
  if (point_stride == 4 && ((uintptr_t)points & 15) == 0)
    cyl_cells_kernel<4><<<grid, 256, 0, stream>>>(points, n, point_stride, sample_idx, sp, c4, c8, point_feature, flag);
  else if (point_stride == 5)
    cyl_cells_kernel<5><<<grid, 256, 0, stream>>>(points, n, point_stride, sample_idx, sp, c4, c8, point_feature, flag);
  else
    cyl_cells_kernel<0><<<grid, 256, 0, stream>>>(points, n, point_stride, sample_idx, sp, c4, c8, point_feature, flag);
  TS_CHECK_LAUNCH("ts_cylinder_cells");
  return TS_OK;
}

static size_t cyl_sort_scratch_bytes(size_t nn) { return ts_align_up(nn * 24 + (4u << 20), 256); }

extern "C" size_t ts_cylinder_voxels_workspace_bytes(int64_t n, int32_t n_samples) {
  const size_t nn = (size_t)(n < 1 ? 1 : n), nb = (size_t)(n_samples < 1 ? 1 : n_samples);
  // keys x 2, values x 2, head flags, ranks, run starts [n + 1], sample starts [B + 1], the key-range word, sort / scan scratch
  return 2 * ts_align_up(nn * 8, 256) + 4 * ts_align_up(nn * 4, 256) + ts_align_up((nn + 1) * 4, 256) +
         ts_align_up((nb + 1) * 4, 256) + 256 + cyl_sort_scratch_bytes(nn);
}

extern "C" int ts_cylinder_voxels(const int32_t *cells, const int64_t *labels, int64_t n, int32_t n_samples, int32_t num_classes,
                                  int64_t ignore_label, int32_t *out_index, int64_t *out_inverse, int64_t *voxel_label,
                                  int32_t *counts, int32_t *flags, void *ws, size_t ws_bytes, ts_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  TS_REQUIRE(n >= 0 && n < (1LL << 30), TS_ERR_INVALID_ARGUMENT, "ts_cylinder_voxels: bad n");
  TS_REQUIRE(n_samples >= 1 && n_samples <= 1024, TS_ERR_INVALID_ARGUMENT, "ts_cylinder_voxels: 1 .. 1024 samples, got %d", n_samples);
  TS_REQUIRE(num_classes >= 1 && num_classes <= 32, TS_ERR_UNSUPPORTED,
             "ts_cylinder_voxels: 1 .. 32 classes (one lane of the vote per class), got %d", num_classes);
  TS_REQUIRE(counts && flags, TS_ERR_INVALID_ARGUMENT, "ts_cylinder_voxels: null counts / flags");
  if (n == 0) {
    TS_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)(n_samples + 1) * 4, stream), "cylinder_voxels memset");
    return TS_OK;
  }
  TS_REQUIRE(cells && labels && out_index && out_inverse && voxel_label, TS_ERR_INVALID_ARGUMENT, "ts_cylinder_voxels: null pointer");
  TS_REQUIRE(((uintptr_t)cells & 15) == 0, TS_ERR_INVALID_ARGUMENT, "ts_cylinder_voxels: cells must be 16-byte aligned");
  TS_REQUIRE(ws && ws_bytes >= ts_cylinder_voxels_workspace_bytes(n, n_samples), TS_ERR_WORKSPACE_TOO_SMALL,
             "ts_cylinder_voxels: workspace %zu < %zu", ws_bytes, ts_cylinder_voxels_workspace_bytes(n, n_samples));
  TS_REQUIRE(((uintptr_t)ws & 255) == 0, TS_ERR_INVALID_ARGUMENT, "workspace must be 256-byte aligned");
  const size_t nn = (size_t)n;
  const size_t kb = ts_align_up(nn * 8, 256), vb = ts_align_up(nn * 4, 256);
  char *p = (char *)ws;
  uint64_t *ka = (uint64_t *)p;
  p += kb;
  uint64_t *kbuf = (uint64_t *)p;
  p += kb;
  int *va = (int *)p;
  p += vb;
  int *vbuf = (int *)p;
  p += vb;
  unsigned *heads = (unsigned *)p;
  p += vb;
  unsigned *ranks = (unsigned *)p;
  p += vb;
  int *run = (int *)p;
  p += ts_align_up((nn + 1) * 4, 256);
  int *start = (int *)p;
  p += ts_align_up((size_t)(n_samples + 1) * 4, 256);
  int *err = (int *)p;
  p += 256;
  void *tmp = p;
  const size_t tmp_bytes = ws_bytes - (size_t)(p - (char *)ws);

  TS_CHECK_HIP(hipMemsetAsync(err, 0, 256, stream), "cylinder_voxels memset");
  const int grid = (int)std::min<int64_t>(ts_cdiv(n, 256), 4096);
  sq_pack_kernel<<<grid, 256, 0, stream>>>((const int4 *)cells, n, ka, va, err);
  TS_CHECK_LAUNCH("ts_cylinder_voxels/pack");
  size_t need = 0;
  TS_CHECK_HIP(rocprim::radix_sort_pairs(nullptr, need, ka, kbuf, va, vbuf, nn, 0u, 64u, stream), "sort size query");
  TS_REQUIRE(need <= tmp_bytes, TS_ERR_WORKSPACE_TOO_SMALL, "ts_cylinder_voxels: sort scratch %zu > %zu", need, tmp_bytes);
  size_t tb = tmp_bytes;
  TS_CHECK_HIP(rocprim::radix_sort_pairs(tmp, tb, ka, kbuf, va, vbuf, nn, 0u, 64u, stream), "radix_sort_pairs");
  sq_flag_kernel<<<grid, 256, 0, stream>>>(kbuf, n, heads);
  TS_CHECK_LAUNCH("ts_cylinder_voxels/flag");
  need = 0;
  TS_CHECK_HIP(rocprim::inclusive_scan(nullptr, need, heads, ranks, nn, rocprim::plus<unsigned>(), stream), "scan size query");
  TS_REQUIRE(need <= tmp_bytes, TS_ERR_WORKSPACE_TOO_SMALL, "ts_cylinder_voxels: scan scratch too small");
  tb = tmp_bytes;
  TS_CHECK_HIP(rocprim::inclusive_scan(tmp, tb, heads, ranks, nn, rocprim::plus<unsigned>(), stream), "inclusive_scan");
  cyl_starts_kernel<<<1, 256, 0, stream>>>(kbuf, ranks, n, n_samples, start, counts);
  TS_CHECK_LAUNCH("ts_cylinder_voxels/starts");
  cyl_scatter_kernel<<<grid, 256, 0, stream>>>(kbuf, vbuf, ranks, n, n_samples, start, err, out_index, out_inverse, run,
                                               flags + 2);
  TS_CHECK_LAUNCH("ts_cylinder_voxels/scatter");
  // 8 voxels per workgroup; the grid covers the n voxels there can be at most, a group past the m there are stops at once
  const int vgrid = (int)std::min<int64_t>(ts_cdiv(n, 8), 8192);
  cyl_vote_kernel<<<vgrid, 256, 0, stream>>>(vbuf, run, labels, counts, n_samples, num_classes, ignore_label, voxel_label,
                                             flags + 1);
  TS_CHECK_LAUNCH("ts_cylinder_voxels/vote");
  return TS_OK;
}
