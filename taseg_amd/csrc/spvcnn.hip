// Kernels of the SPVCNN segmentor (reference pcseg/model/segmentor/fusion/spvcnn/spvcnn.py) that the rest of the library does not
// already serve in a form fit for a training loop:
//   * the mean-voxelisation of point rows with a FIXED summation order (spvcnn/utils.py:41-65 `point_to_voxel`, three times per
//     pass at strides 1, 16 and 4; the float atomics of ts_voxelize_forward land 120 000 x 256 adds on 1 379 x 256 addresses at
//     stride 16 and change their order from run to run);
//   * the tail of the point branch, z.F = devoxelize(x.F) + ReLU(BN(Linear(z.F))) (spvcnn.py:417-444), in one pass over the rows.
// Both are bandwidth kernels of the csrc/rows.h family: 16-byte accesses per lane, one group of c / V lanes per row, voxel or
// piece, every output element written exactly once, no atomics, no fill.  Compiled with -ffp-contract=off (csrc/build.py): every
// product and sum below keeps its own rounding, so tests/spvcnn_ref.py restates the mean bit for bit.
#include "point_tail.h"

namespace {

int g_piece_rows = 32;                                  // P: rows per piece (16, 32 or 64; profiles/spvcnn_step.txt has the comparison)

__device__ __forceinline__ int clamp_row(int r, int64_t n) { return min(max(r, 0), (int)(n - 1)); }

// acc += feat[ent[e], lane's channels] / cnt for e = beg .. end - 1 in ascending order; the rows are loaded four at a time
// (independent loads) and added one after the other.  The division is a float32 division of the widened element, as in the
// reference's kernel (voxelize_cuda.cu: `feat / count`).
template <typename T>
__device__ __forceinline__ void add_rows(const T *__restrict__ feat, const int *__restrict__ ent, int beg, int end, int64_t n, int c,
                                         int lane, float cnt, float (&acc)[Lanes<T>::V]) {
  constexpr int V = Lanes<T>::V;
  typedef ts_vec<T, V> vec;
  int e = beg;
  for (; e + 4 <= end; e += 4) {
    int r[4];
    vec f[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) r[u] = clamp_row(ent[e + u], n);
#pragma unroll
    for (int u = 0; u < 4; ++u) f[u] = *(const vec *)(feat + (int64_t)r[u] * c + V * lane);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] += (float)f[u][j] / cnt;
    }
  }
  for (; e < end; ++e) {
    const int r = clamp_row(ent[e], n);
    const vec f = *(const vec *)(feat + (int64_t)r * c + V * lane);
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] += (float)f[j] / cnt;
  }
}

// ------------------------------------------------------------------------------------------------------ mean-voxelisation
// The rows are grouped by voxel (ts_point_groups: stable, ascending row index inside a voxel).  A voxel's run of cnt rows is cut into
// pieces of P consecutive rows counted from its first row; each piece is summed in ascending order, the piece sums are then added in
// ascending piece order; a voxel of at most P rows is one sequential sum.
//
// Stage 1, the FULL pieces of the voxels of more than P rows: a run of P positions holds exactly one multiple of P, so the work item
// q = 0 .. ceil(n / P) - 1 looks at position t = q P of the grouped list, finds the voxel of the row that sits there (idx[ent[t]]) and
// the piece around t; if that piece is a full one of a voxel of more than P rows, the item sums it into part[q, :] (float32).  The
// grid is sized from n alone - no host read - and every piece is owned by one item.
template <typename T>
__global__ __launch_bounds__(256) void voxel_mean_pieces_kernel(const T *__restrict__ feat, const int *__restrict__ idx,
                                                                const int *__restrict__ off, const int *__restrict__ ent, int64_t n,
                                                                int c, int64_t m, int P, int64_t n_items, float *__restrict__ part) {
  constexpr int V = Lanes<T>::V;
  const int cq = c / V, groups = 256 / cq;
  const int grp = threadIdx.x / cq, lane = threadIdx.x - grp * cq;
  if (grp >= groups) return;
  const int64_t q = (int64_t)blockIdx.x * groups + grp;
  if (q >= n_items) return;
  const int64_t t = q * P;
  if (t >= min((int64_t)off[m], n)) return;             // behind the grouped rows
  const int r = ent[t];
  if (r < 0 || r >= n) return;
  const int v = idx[r];
  if (v < 0 || v >= m) return;
  const int beg = off[v], end = off[v + 1], cnt = end - beg;
  if (cnt <= P || t < beg || t >= end) return;          // a short voxel is summed in stage 2
  const int s = beg + (int)((t - beg) / P) * P;
  if (s + P > end) return;                              // the voxel's last, partial piece: stage 2
  float acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
  add_rows<T>(feat, ent, s, s + P, n, c, lane, (float)cnt, acc);
  float4 *dst = (float4 *)(part + q * c + V * lane);
#pragma unroll
  for (int j = 0; j < V; j += 4) dst[j / 4] = make_float4(acc[j], acc[j + 1], acc[j + 2], acc[j + 3]);
}

// Stage 2, one group of lanes per voxel: at most P rows - the sequential sum; more - the full pieces' sums from `part` in ascending
// piece order (four loads at a time, added in order), then the sum of the last, partial piece.  A voxel without rows stores zeros; a
// half result is rounded once, here.
template <typename T>
__global__ __launch_bounds__(256) void voxel_mean_finish_kernel(const T *__restrict__ feat, const int *__restrict__ off,
                                                                const int *__restrict__ ent, int64_t n, int c, int64_t m, int P,
                                                                const float *__restrict__ part, T *__restrict__ out) {
  constexpr int V = Lanes<T>::V;
  typedef ts_vec<T, V> vec;
  const int cq = c / V, groups = 256 / cq;
  const int grp = threadIdx.x / cq, lane = threadIdx.x - grp * cq;
  if (grp >= groups) return;
  const int64_t v = (int64_t)blockIdx.x * groups + grp;
  if (v >= m) return;
  const int beg = min(max(off[v], 0), (int)n), end = min(max(off[v + 1], beg), (int)n), cnt = end - beg;
  float acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
  if (cnt <= P) {
    add_rows<T>(feat, ent, beg, end, n, c, lane, (float)cnt, acc);
  } else {
    const int n_full = cnt / P;
    int p = 0;
    for (; p + 4 <= n_full; p += 4) {
      float4 s[4][V / 4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t q = ((int64_t)beg + (int64_t)(p + u) * P + P - 1) / P;       // the multiple of P inside the piece
        const float4 *src = (const float4 *)(part + q * c + V * lane);
#pragma unroll
        for (int j = 0; j < V / 4; ++j) s[u][j] = src[j];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int j = 0; j < V / 4; ++j) {
          acc[4 * j] += s[u][j].x; acc[4 * j + 1] += s[u][j].y; acc[4 * j + 2] += s[u][j].z; acc[4 * j + 3] += s[u][j].w;
        }
      }
    }
    for (; p < n_full; ++p) {
      const int64_t q = ((int64_t)beg + (int64_t)p * P + P - 1) / P;
      const float4 *src = (const float4 *)(part + q * c + V * lane);
#pragma unroll
      for (int j = 0; j < V / 4; ++j) {
        const float4 s = src[j];
        acc[4 * j] += s.x; acc[4 * j + 1] += s.y; acc[4 * j + 2] += s.z; acc[4 * j + 3] += s.w;
      }
    }
    if (beg + n_full * P < end) {
      float last[V];
#pragma unroll
      for (int j = 0; j < V; ++j) last[j] = 0.f;
      add_rows<T>(feat, ent, beg + n_full * P, end, n, c, lane, (float)cnt, last);
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] += last[j];
    }
  }
  vec o;
#pragma unroll
  for (int j = 0; j < V; ++j) o[j] = (T)acc[j];
  *(vec *)(out + v * c + V * lane) = o;
}

// The adjoint is a gather: grad_feat[i] = grad_out[idx[i]] / cnt of that voxel, zeros for a row that took no part.
template <typename T>
__global__ __launch_bounds__(256) void voxel_mean_bwd_kernel(const T *__restrict__ gout, const int *__restrict__ idx,
                                                             const int *__restrict__ off, int64_t n, int c, int64_t m,
                                                             T *__restrict__ gfeat) {
  constexpr int V = Lanes<T>::V;
  typedef ts_vec<T, V> vec;
  const int cq = c / V, groups = 256 / cq;
  const int grp = threadIdx.x / cq, lane = threadIdx.x - grp * cq;
  if (grp >= groups) return;
  const int64_t i = (int64_t)blockIdx.x * groups + grp;
  if (i >= n) return;
  const int v = idx[i];
  vec g;
#pragma unroll
  for (int j = 0; j < V; ++j) g[j] = (T)0;
  if (v >= 0 && v < m) {
    const int cnt = off[v + 1] - off[v];
    if (cnt > 0) {
      const vec go = *(const vec *)(gout + (int64_t)v * c + V * lane);
      const float cf = (float)cnt;
#pragma unroll
      for (int j = 0; j < V; ++j) g[j] = (T)((float)go[j] / cf);
    }
  }
  *(vec *)(gfeat + i * c + V * lane) = g;
}

// The point tail (ts_point_tail_forward) is launch_point_tail<false> of point_tail.h, which csrc/rpvnet.hip shares.

}  // namespace

extern "C" int32_t ts_voxelize_mean_piece_rows(void) { return g_piece_rows; }

// for tools/time_spvcnn_step.py's comparison of the three piece lengths only: the length is part of the summation rule
extern "C" int ts_voxelize_mean_set_piece_rows(int32_t rows) {
  TS_REQUIRE(rows == 16 || rows == 32 || rows == 64, TS_ERR_INVALID_ARGUMENT, "ts_voxelize_mean_set_piece_rows: 16, 32 or 64");
  g_piece_rows = rows;
  return TS_OK;
}

extern "C" size_t ts_point_groups_workspace_bytes(int64_t n) { return ts_group_slots_workspace_bytes(n < 0 ? 0 : n); }

extern "C" int ts_point_groups(const int32_t *idx, int64_t n, int64_t m, int32_t *offsets, int32_t *entries, void *ws,
                               size_t ws_bytes, ts_stream_t stream_) {
  return ts_group_slots(idx, nullptr, n, m, offsets, entries, ws, ws_bytes, (hipStream_t)stream_, "ts_point_groups");
}

extern "C" size_t ts_voxelize_mean_workspace_bytes(int64_t n, int32_t c) {
  const size_t pieces = (size_t)ts_cdiv(n < 0 ? 0 : n, (int64_t)g_piece_rows), cs = (size_t)(c < 0 ? 0 : c);
  return ts_align_up((pieces + 1) * cs * sizeof(float), 256);
}

extern "C" int ts_voxelize_mean_forward(const void *feat, const int32_t *idx, const int32_t *offsets, const int32_t *entries,
                                        int64_t n, int32_t c, int64_t m, int32_t half, void *out, void *ws, size_t ws_bytes,
                                        ts_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = rows_check("ts_voxelize_mean_forward", n, c, m, half);
  if (rc != TS_OK) return rc;
  if (m == 0) return TS_OK;
  TS_REQUIRE(out && offsets && (n == 0 || (feat && idx && entries && ws)), TS_ERR_INVALID_ARGUMENT,
             "ts_voxelize_mean_forward: null pointer");
  TS_REQUIRE(aligned16(feat, out, ws), TS_ERR_INVALID_ARGUMENT, "ts_voxelize_mean_forward: rows must be 16-byte aligned");
  TS_REQUIRE(n == 0 || ws_bytes >= ts_voxelize_mean_workspace_bytes(n, c), TS_ERR_INVALID_ARGUMENT,
             "ts_voxelize_mean_forward: workspace too small");
  const int P = g_piece_rows;
  const int groups = row_groups(c, half);
  const int64_t n_items = ts_cdiv(n, (int64_t)P);
  float *part = (float *)ws;
  if (n_items > 0) {
    const unsigned grid = (unsigned)ts_cdiv(n_items, (int64_t)groups);
    by_half(half, [&](auto t) {
      using T = decltype(t);
      voxel_mean_pieces_kernel<T><<<grid, 256, 0, stream>>>((const T *)feat, idx, offsets, entries, n, c, m, P, n_items, part);
    });
    TS_CHECK_LAUNCH("ts_voxelize_mean_forward/pieces");
  }
  const unsigned grid = (unsigned)ts_cdiv(m, (int64_t)groups);
  by_half(half, [&](auto t) {
    using T = decltype(t);
    voxel_mean_finish_kernel<T><<<grid, 256, 0, stream>>>((const T *)feat, offsets, entries, n, c, m, P, part, (T *)out);
  });
  TS_CHECK_LAUNCH("ts_voxelize_mean_forward/finish");
  return TS_OK;
}

extern "C" int ts_voxelize_mean_backward(const void *grad_out, const int32_t *idx, const int32_t *offsets, int64_t n, int32_t c,
                                         int64_t m, int32_t half, void *grad_feat, ts_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = rows_check("ts_voxelize_mean_backward", n, c, m, half);
  if (rc != TS_OK) return rc;
  if (n == 0) return TS_OK;
  TS_REQUIRE(grad_feat && idx && (m == 0 || (grad_out && offsets)), TS_ERR_INVALID_ARGUMENT,
             "ts_voxelize_mean_backward: null pointer");
  TS_REQUIRE(aligned16(grad_out, grad_feat), TS_ERR_INVALID_ARGUMENT, "ts_voxelize_mean_backward: rows must be 16-byte aligned");
  const unsigned grid = (unsigned)ts_cdiv(n, (int64_t)row_groups(c, half));
  by_half(half, [&](auto t) {
    using T = decltype(t);
    voxel_mean_bwd_kernel<T><<<grid, 256, 0, stream>>>((const T *)grad_out, idx, offsets, n, c, m, (T *)grad_feat);
  });
  TS_CHECK_LAUNCH("ts_voxelize_mean_backward");
  return TS_OK;
}

extern "C" int ts_point_tail_forward(const void *y, const void *vox, const int32_t *idx, const float *weight, const float *mean,
                                     const float *invstd, const float *gamma, const float *beta, int64_t n, int32_t c, int64_t m,
                                     int32_t half, void *out, uint8_t *mask, ts_stream_t stream_) {
  return launch_point_tail<false>("ts_point_tail_forward", y, vox, idx, weight, nullptr, nullptr, nullptr, 0, mean, invstd, gamma,
                                  beta, n, c, m, half, out, mask, (hipStream_t)stream_);
}
