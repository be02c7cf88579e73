// Kernels of the Cylinder_TS segmentor (reference pcseg/model/segmentor/voxel/cylinder3d/cylinder_ts.py) that the rest of the
// library does not already serve: the max-voxelisation of point features (tools/utils/common/seg_utils.py:385-401,
// `torch_scatter.scatter_max(z.F, idx_query, dim=0)[0]`) and the sigmoid gate of ReconBlock (cylinder_ts.py:368-384).  Both are
// bandwidth kernels of the csrc/rows.h family: 16-byte accesses per lane, every output element written exactly once, no atomics, no
// fill.
#include "rows.h"

namespace {

// ------------------------------------------------------------------------------------------------------ max-voxelisation
// The rows are grouped by voxel first (ts_group_slots: stable, ascending row index inside a voxel).  One group of c / V lanes
// per voxel - a whole wave at c = 256 floats, whose lanes then read one 1 KB row per step - walks the voxel's rows in ascending
// order.  The maximum starts from the voxel's FIRST row (never from zero: all-negative columns) and only a strictly greater
// value replaces it, so `arg` is the smallest row index that attains the maximum; a NaN never compares greater and is kept only
// where it sits in the voxel's first row.  Rows are taken four at a time (independent loads), compared in order.
template <typename T>
__global__ __launch_bounds__(256) void voxel_max_fwd_kernel(const T *__restrict__ feat, const int *__restrict__ off,
                                                            const int *__restrict__ ent, int64_t m, int c, T *__restrict__ out,
                                                            int *__restrict__ arg) {
  constexpr int V = Lanes<T>::V;
  typedef ts_vec<T, V> vec;
  const int cq = c / V, groups = 256 / cq;
  const int grp = threadIdx.x / cq, lane = threadIdx.x - grp * cq;
  if (grp >= groups) return;
  const int64_t v = (int64_t)blockIdx.x * groups + grp;
  if (v >= m) return;
  const int beg = off[v], end = off[v + 1];
  vec best;
  int at[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    best[j] = (T)0;
    at[j] = -1;
  }
  int e = beg;
  if (e < end) {
    const int r = ent[e++];
    best = *(const vec *)(feat + (int64_t)r * c + V * lane);
#pragma unroll
    for (int j = 0; j < V; ++j) at[j] = r;
  }
  for (; e + 4 <= end; e += 4) {
    int r[4];
    vec f[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) r[u] = ent[e + u];
#pragma unroll
    for (int u = 0; u < 4; ++u) f[u] = *(const vec *)(feat + (int64_t)r[u] * c + V * lane);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const bool gt = f[u][j] > best[j];
        best[j] = gt ? f[u][j] : best[j];
        at[j] = gt ? r[u] : at[j];
      }
    }
  }
  for (; e < end; ++e) {
    const int r = ent[e];
    const vec f = *(const vec *)(feat + (int64_t)r * c + V * lane);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const bool gt = f[j] > best[j];
      best[j] = gt ? f[j] : best[j];
      at[j] = gt ? r : at[j];
    }
  }
  *(vec *)(out + v * c + V * lane) = best;
  int4 *ap = (int4 *)(arg + v * c + V * lane);
#pragma unroll
  for (int j = 0; j < V; j += 4) ap[j / 4] = make_int4(at[j], at[j + 1], at[j + 2], at[j + 3]);
}

// The adjoint is a gather: row i takes the gradient of its voxel in the channels where it is the recorded arg-max, zero elsewhere
// (and everywhere for a skipped row).  One group of c / V lanes per row; every element of grad_feat written once.
template <typename T>
__global__ __launch_bounds__(256) void voxel_max_bwd_kernel(const T *__restrict__ gout, const int *__restrict__ idx,
                                                            const int *__restrict__ arg, int64_t n, int c, int64_t m,
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
    const vec go = *(const vec *)(gout + (int64_t)v * c + V * lane);
    const int4 *ap = (const int4 *)(arg + (int64_t)v * c + V * lane);
#pragma unroll
    for (int j = 0; j < V; j += 4) {
      const int4 a = ap[j / 4];
      g[j] = a.x == (int)i ? go[j] : (T)0;
      g[j + 1] = a.y == (int)i ? go[j + 1] : (T)0;
      g[j + 2] = a.z == (int)i ? go[j + 2] : (T)0;
      g[j + 3] = a.w == (int)i ? go[j + 3] : (T)0;
    }
  }
  *(vec *)(gfeat + i * c + V * lane) = g;
}

// ------------------------------------------------------------------------------------------------------------ sigmoid gate
__device__ __forceinline__ float sigmoidf(float a) { return 1.f / (1.f + expf(-a)); }

template <typename T>
__global__ __launch_bounds__(256) void sigmoid3_gate_fwd_kernel(const T *__restrict__ x, const T *__restrict__ u,
                                                                const T *__restrict__ v, const T *__restrict__ w, int64_t nv,
                                                                T *__restrict__ out) {
  constexpr int V = Lanes<T>::V;
  typedef ts_vec<T, V> vec;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nv) return;
  const vec xv = ((const vec *)x)[i], uv = ((const vec *)u)[i], vv = ((const vec *)v)[i], wv = ((const vec *)w)[i];
  vec o;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const float s = sigmoidf((float)uv[j]) + sigmoidf((float)vv[j]) + sigmoidf((float)wv[j]);
    o[j] = (T)(s * (float)xv[j]);
  }
  ((vec *)out)[i] = o;
}

template <typename T>
__global__ __launch_bounds__(256) void sigmoid3_gate_bwd_kernel(const T *__restrict__ go, const T *__restrict__ x,
                                                                const T *__restrict__ u, const T *__restrict__ v,
                                                                const T *__restrict__ w, int64_t nv, T *__restrict__ gx,
                                                                T *__restrict__ gu, T *__restrict__ gv, T *__restrict__ gw) {
  constexpr int V = Lanes<T>::V;
  typedef ts_vec<T, V> vec;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nv) return;
  const vec gov = ((const vec *)go)[i], xv = ((const vec *)x)[i], uv = ((const vec *)u)[i], vv = ((const vec *)v)[i],
            wv = ((const vec *)w)[i];
  vec ox, ou, ov, ow;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const float g = (float)gov[j], su = sigmoidf((float)uv[j]), sv = sigmoidf((float)vv[j]), sw = sigmoidf((float)wv[j]);
    const float gxs = g * (float)xv[j];              // gradient that reaches each of the three sigmoids
    ox[j] = (T)(g * (su + sv + sw));
    ou[j] = (T)(gxs * ((1.f - su) * su));
    ov[j] = (T)(gxs * ((1.f - sv) * sv));
    ow[j] = (T)(gxs * ((1.f - sw) * sw));
  }
  ((vec *)gx)[i] = ox;
  ((vec *)gu)[i] = ou;
  ((vec *)gv)[i] = ov;
  ((vec *)gw)[i] = ow;
}

int gate_check(const char *who, int64_t n, int32_t c, int32_t half, int64_t *nv) {
  TS_REQUIRE(n >= 0 && c > 0 && n < (1LL << 31) && c <= (1 << 20), TS_ERR_INVALID_ARGUMENT, "%s: bad sizes", who);
  TS_REQUIRE(c % (half ? 8 : 4) == 0, TS_ERR_UNSUPPORTED, "%s: C must be a multiple of %d", who, half ? 8 : 4);
  *nv = n * c / (half ? 8 : 4);
  TS_REQUIRE(ts_cdiv(*nv, 256) < (1LL << 31), TS_ERR_UNSUPPORTED, "%s: too many elements for one launch", who);
  return TS_OK;
}

}  // namespace

extern "C" size_t ts_voxelize_max_workspace_bytes(int64_t n, int64_t m) {
  const size_t ns = (size_t)(n < 0 ? 0 : n), ms = (size_t)(m < 0 ? 0 : m);
  return ts_align_up((ms + 1) * 4, 256) + ts_align_up((ns + 1) * 4, 256) + ts_group_slots_workspace_bytes(n);
}

extern "C" int ts_voxelize_max_forward(const void *feat, const int32_t *idx, int64_t n, int32_t c, int64_t m, int32_t half,
                                       void *out, int32_t *arg, void *ws, size_t ws_bytes, ts_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = rows_check("ts_voxelize_max_forward", n, c, m, half);
  if (rc != TS_OK) return rc;
  if (m == 0) return TS_OK;
  TS_REQUIRE(out && arg && ws && (n == 0 || (feat && idx)), TS_ERR_INVALID_ARGUMENT, "ts_voxelize_max_forward: null pointer");
  TS_REQUIRE(aligned16(feat, out, arg), TS_ERR_INVALID_ARGUMENT, "ts_voxelize_max_forward: rows must be 16-byte aligned");
  TS_REQUIRE(ws_bytes >= ts_voxelize_max_workspace_bytes(n, m), TS_ERR_INVALID_ARGUMENT,
             "ts_voxelize_max_forward: workspace too small");
  char *p = (char *)ws;
  int *off = (int *)p;
  p += ts_align_up((size_t)(m + 1) * 4, 256);
  int *ent = (int *)p;
  p += ts_align_up((size_t)(n + 1) * 4, 256);
  const int grc = ts_group_slots(idx, nullptr, n, m, off, ent, p, ws_bytes - (size_t)(p - (char *)ws), stream,
                                 "ts_voxelize_max_forward");
  if (grc != TS_OK) return grc;
  const unsigned grid = (unsigned)ts_cdiv(m, row_groups(c, half));
  by_half(half, [&](auto t) {
    using T = decltype(t);
    voxel_max_fwd_kernel<T><<<grid, 256, 0, stream>>>((const T *)feat, off, ent, m, c, (T *)out, arg);
  });
  TS_CHECK_LAUNCH("ts_voxelize_max_forward");
  return TS_OK;
}

extern "C" int ts_voxelize_max_backward(const void *grad_out, const int32_t *idx, const int32_t *arg, int64_t n, int32_t c,
                                        int64_t m, int32_t half, void *grad_feat, ts_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = rows_check("ts_voxelize_max_backward", n, c, m, half);
  if (rc != TS_OK) return rc;
  if (n == 0) return TS_OK;
  TS_REQUIRE(grad_feat && idx && (m == 0 || (grad_out && arg)), TS_ERR_INVALID_ARGUMENT, "ts_voxelize_max_backward: null pointer");
  TS_REQUIRE(aligned16(grad_out, grad_feat, arg), TS_ERR_INVALID_ARGUMENT, "ts_voxelize_max_backward: rows must be 16-byte aligned");
  const unsigned grid = (unsigned)ts_cdiv(n, row_groups(c, half));
  by_half(half, [&](auto t) {
    using T = decltype(t);
    voxel_max_bwd_kernel<T><<<grid, 256, 0, stream>>>((const T *)grad_out, idx, arg, n, c, m, (T *)grad_feat);
  });
  TS_CHECK_LAUNCH("ts_voxelize_max_backward");
  return TS_OK;
}

extern "C" int ts_sigmoid3_gate_forward(const void *x, const void *u, const void *v, const void *w, int64_t n, int32_t c,
                                        int32_t half, void *out, ts_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int64_t nv = 0;
  const int rc = gate_check("ts_sigmoid3_gate_forward", n, c, half, &nv);
  if (rc != TS_OK) return rc;
  if (nv == 0) return TS_OK;
  TS_REQUIRE(x && u && v && w && out, TS_ERR_INVALID_ARGUMENT, "ts_sigmoid3_gate_forward: null pointer");
  TS_REQUIRE(aligned16(x, u, v, w) && aligned16(out), TS_ERR_INVALID_ARGUMENT,
             "ts_sigmoid3_gate_forward: pointers must be 16-byte aligned");
  const unsigned grid = (unsigned)ts_cdiv(nv, 256);
  by_half(half, [&](auto t) {
    using T = decltype(t);
    sigmoid3_gate_fwd_kernel<T><<<grid, 256, 0, stream>>>((const T *)x, (const T *)u, (const T *)v, (const T *)w, nv, (T *)out);
  });
  TS_CHECK_LAUNCH("ts_sigmoid3_gate_forward");
  return TS_OK;
}

extern "C" int ts_sigmoid3_gate_backward(const void *grad_out, const void *x, const void *u, const void *v, const void *w,
                                         int64_t n, int32_t c, int32_t half, void *grad_x, void *grad_u, void *grad_v,
                                         void *grad_w, ts_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  int64_t nv = 0;
  const int rc = gate_check("ts_sigmoid3_gate_backward", n, c, half, &nv);
  if (rc != TS_OK) return rc;
  if (nv == 0) return TS_OK;
  TS_REQUIRE(grad_out && x && u && v && w && grad_x && grad_u && grad_v && grad_w, TS_ERR_INVALID_ARGUMENT,
             "ts_sigmoid3_gate_backward: null pointer");
  TS_REQUIRE(aligned16(x, u, v, w) && aligned16(grad_out, grad_x, grad_u, grad_v) && aligned16(grad_w), TS_ERR_INVALID_ARGUMENT,
             "ts_sigmoid3_gate_backward: pointers must be 16-byte aligned");
  const unsigned grid = (unsigned)ts_cdiv(nv, 256);
  by_half(half, [&](auto t) {
    using T = decltype(t);
    sigmoid3_gate_bwd_kernel<T><<<grid, 256, 0, stream>>>((const T *)grad_out, (const T *)x, (const T *)u, (const T *)v, (const T *)w,
                                                          nv, (T *)grad_x, (T *)grad_u, (T *)grad_v, (T *)grad_w);
  });
  TS_CHECK_LAUNCH("ts_sigmoid3_gate_backward");
  return TS_OK;
}
