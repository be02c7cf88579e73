// The "fully interpolation decoding" step of FIDNet and CENet (R/pcseg/model/segmentor/range/fidnet/model/semantic/fidnet.py:300-311,
// R/pcseg/model/segmentor/range/cenet/model/semantic/cenet.py:233-243):
//   res_k = F.interpolate(x_k, size = (H, W), mode = 'bilinear', align_corners = True)        k = 2, 3, 4 (the 1/2, 1/4, 1/8 maps)
//   cat   = torch.cat([x, x_1, res_2, res_3, res_4], dim = 1)
// on channels-last rows, in ONE pass over the result: cat [T, H, W, Ca + Cb + 3 Cl] from x [T, H, W, Ca], x1 [T, H, W, Cb] and three
// coarse maps xk [T, hk, wk, Cl] (1 <= hk <= H, 1 <= wk <= W), every operand read in place.  ATen runs it as three interpolation writes
// and a concatenation that reads and rewrites every channel; its gradient (upsample_bilinear2d_backward) adds with float atomics.
//
// THE INTERPOLATION RULE (the contract; it is ATen's device kernel for align_corners = True - ATen/native/cuda/UpSample.cuh:
// area_pixel_compute_scale, area_pixel_compute_source_index, and the body of upsample_bilinear2d_out_frame), all in float32:
//   scale_h = out_h > 1 ? (float)(in_h - 1) / (out_h - 1) : 0                          (one division, on the host, as ATen's host code)
//   h1r = scale_h * (float)y;  h1 = (int)h1r (truncation);  h1p = h1 < in_h - 1 ? 1 : 0;  h1lambda = h1r - (float)h1;  h0lambda = 1 - h1lambda
//   the same along the width: w1, w1p, w1lambda, w0lambda
//   val = h0lambda * (w0lambda * v[h1][w1]       + w1lambda * v[h1][w1 + w1p])
//       + h1lambda * (w0lambda * v[h1 + h1p][w1] + w1lambda * v[h1 + h1p][w1 + w1p])
// - four products and one sum per bracket, two products, one sum: every operation rounded on its own (this file is compiled with
// -ffp-contract=off), a half value widened first, ONE rounding at a half store.  The level maps res_k [T, H, W, Cl] (three pointers,
// may be NULL: CENet's auxiliary heads read them) receive the same stored values as their slices of cat.
//
// THE TABLES.  ts_fid_upcat_tables writes, per level and axis, i0[out] = h1 (int32), lam[out] = h1lambda (float) and
// first[in + 1] = the lower bound of i0: first[r] = the smallest y with i0[y] >= r (first[in] = out).  The forward reads i0 / lam; the
// backward reads the same i0 / lam and takes its ranges from `first`, so the two passes cannot disagree about a corner.
//
// THE ADJOINT, a gather without atomics or fill.  Coarse pixel (r, c) of level k collects from the fine rows y in
// [first_h[max(r - 1, 0)], first_h[r + 1]) and columns x in [first_w[max(c - 1, 0)], first_w[c + 1]): the pixels whose corner set
// {h1, h1 + h1p} x {w1, w1 + w1p} can hold it.  With g = (float)grad_cat[t, y, x, slice k] (+ (float)grad_res_k[t, y, x] when given, one
// float sum) a fine pixel contributes, corner row cy = 0, 1 then corner column cx = 0, 1, each corner that IS (r, c):
//   term = (ly[cy] * lx[cx]) * g            ly = {h0lambda, h1lambda}, lx = {w0lambda, w1lambda}
// (a clamped neighbour - h1p = 0 - names the same coarse pixel twice and contributes two terms).  THE ORDER OF THE ADDITIONS: the fine rows
// of the range are dealt to S partial sums, row y to partial (y - y_lo) % S with y_lo the range's first row; a partial adds its rows in
// ascending y, a row's columns in ascending x, a pixel's corners as above, from 0; the result is partial 0 + partial 1 + .. in that
// order.  S = max(1, min(8, (H / hk) / 2, 256 / (Cl / V))) (integer divisions, V = 4 floats or 8 halves of a 16-byte piece): 1, 2 and 4
// at the 1/2, 1/4 and 1/8 levels of a 128-channel map, so that a coarse pixel of the 1/8 level, with its ~16 x 16 contributors, is
// served by four lanes per piece.  grad_x / grad_x1 are 16-byte copies of their slices.  Every output element is written once; two calls
// give the same bits.
#include "rows.h"

namespace {

struct FidLevel {
  int h, w;               // the coarse map's size
  int i0h, lamh, firsth;  // offsets (in 4-byte words) into the tables
  int i0w, lamw, firstw;
  float sh, sw;           // the two scales
};

struct FidPlan {
  FidLevel lv[3];
  int words;
};

inline float fid_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (out - 1) : 0.f; }

inline FidPlan fid_plan(int H, int W, const int32_t *hk, const int32_t *wk) {
  FidPlan p;
  int at = 0;
  for (int k = 0; k < 3; ++k) {
    FidLevel &l = p.lv[k];
    l.h = hk[k], l.w = wk[k];
    l.i0h = at, at += H;
    l.lamh = at, at += H;
    l.firsth = at, at += l.h + 1;
    l.i0w = at, at += W;
    l.lamw = at, at += W;
    l.firstw = at, at += l.w + 1;
    l.sh = fid_scale(l.h, H), l.sw = fid_scale(l.w, W);
  }
  p.words = at;
  return p;
}

// one block per (level, axis): the out entries of i0 / lam, then the in + 1 lower bounds of i0
__global__ __launch_bounds__(256) void fid_tables_kernel(FidPlan p, int H, int W, int32_t *__restrict__ tab) {
  const FidLevel &l = p.lv[blockIdx.x >> 1];
  const bool wide = blockIdx.x & 1;
  const int out = wide ? W : H, in = wide ? l.w : l.h;
  const float scale = wide ? l.sw : l.sh;
  int32_t *i0 = tab + (wide ? l.i0w : l.i0h), *first = tab + (wide ? l.firstw : l.firsth);
  float *lam = (float *)tab + (wide ? l.lamw : l.lamh);
  for (int y = threadIdx.x; y < out; y += 256) {
    const float r = scale * (float)y;
    // (the product can round up to in - 1 + ulp but not to in: the index stays inside; the clamp costs nothing and keeps it so)
    const int i = min((int)r, in - 1);
    i0[y] = i;
    lam[y] = r - (float)i;
  }
  __syncthreads();
  for (int r = threadIdx.x; r <= in; r += 256) {
    int lo = 0, hi = out;                       // smallest y with i0[y] >= r
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (i0[mid] >= r) hi = mid;
      else lo = mid + 1;
    }
    first[r] = lo;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void fid_upcat_fwd_kernel(const T *__restrict__ x, const T *__restrict__ x1, const T *__restrict__ xk0,
                                                            const T *__restrict__ xk1, const T *__restrict__ xk2, FidPlan p,
                                                            const int32_t *__restrict__ tab, int H, int W, int Ca, int Cb, int Cl,
                                                            unsigned n_items, T *__restrict__ cat, T *__restrict__ r0,
                                                            T *__restrict__ r1, T *__restrict__ r2) {
  constexpr int V = Lanes<T>::V;
  using vec = ts_vec<T, V>;
  const unsigned item = blockIdx.x * 256u + threadIdx.x;
  if (item >= n_items) return;
  const int Cc = Ca + Cb + 3 * Cl;
  const unsigned P = (unsigned)Cc / V, j = item % P, pix = item / P;
  const int ch = (int)j * V;
  T *dst = cat + (size_t)pix * Cc + ch;
  if (ch < Ca) {
    *(vec *)dst = *(const vec *)(x + (size_t)pix * Ca + ch);
    return;
  }
  if (ch < Ca + Cb) {
    *(vec *)dst = *(const vec *)(x1 + (size_t)pix * Cb + (ch - Ca));
    return;
  }
  const int k = (ch - Ca - Cb) / Cl, cl = (ch - Ca - Cb) - k * Cl;
  const FidLevel &l = p.lv[k];
  const T *src = k == 0 ? xk0 : k == 1 ? xk1 : xk2;
  T *res = k == 0 ? r0 : k == 1 ? r1 : r2;
  const unsigned X = pix % (unsigned)W, rest = pix / (unsigned)W, Y = rest % (unsigned)H, t = rest / (unsigned)H;
  const int h1 = tab[l.i0h + Y], w1 = tab[l.i0w + X];
  const float h1l = ((const float *)tab)[l.lamh + Y], w1l = ((const float *)tab)[l.lamw + X];
  const float h0l = 1.f - h1l, w0l = 1.f - w1l;
  const int h1p = h1 < l.h - 1 ? 1 : 0, w1p = w1 < l.w - 1 ? 1 : 0;
  const T *base = src + (((size_t)t * l.h + h1) * l.w + w1) * Cl + cl;
  const vec v00 = *(const vec *)base, v01 = *(const vec *)(base + (size_t)w1p * Cl);
  const vec v10 = *(const vec *)(base + (size_t)h1p * l.w * Cl), v11 = *(const vec *)(base + ((size_t)h1p * l.w + w1p) * Cl);
  vec o;
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const float top = w0l * (float)v00[i] + w1l * (float)v01[i];
    const float bot = w0l * (float)v10[i] + w1l * (float)v11[i];
    o[i] = (T)(h0l * top + h1l * bot);
  }
  *(vec *)dst = o;
  if (res) *(vec *)(res + (size_t)pix * Cl + cl) = o;
}

// grad_x / grad_x1: 16-byte copies of their slices of grad_cat
template <typename T>
__global__ __launch_bounds__(256) void fid_split_bwd_kernel(const T *__restrict__ gcat, int Ca, int Cb, int Cc, unsigned n_items,
                                                            T *__restrict__ gx, T *__restrict__ gx1) {
  constexpr int V = Lanes<T>::V;
  using vec = ts_vec<T, V>;
  const unsigned item = blockIdx.x * 256u + threadIdx.x;
  if (item >= n_items) return;
  const unsigned P = (unsigned)(Ca + Cb) / V, j = item % P, pix = item / P;
  const int ch = (int)j * V;
  const vec v = *(const vec *)(gcat + (size_t)pix * Cc + ch);
  if (ch < Ca) *(vec *)(gx + (size_t)pix * Ca + ch) = v;
  else *(vec *)(gx1 + (size_t)pix * Cb + (ch - Ca)) = v;
}

// one level's gradient: a block holds G coarse pixels x S partial sums x Pl pieces (threads beyond G * S * Pl idle), thread =
// (g * S + s) * Pl + jl; the S partials of a piece meet in LDS and lane s = 0 adds them in order
template <typename T>
__global__ __launch_bounds__(256) void fid_up_bwd_kernel(const T *__restrict__ gcat, const T *__restrict__ gres, FidLevel l,
                                                         const int32_t *__restrict__ tab, int H, int W, int Cc, int c_off, int Cl, int S,
                                                         int G, unsigned n_pix, T *__restrict__ gxk) {
  constexpr int V = Lanes<T>::V;
  using vec = ts_vec<T, V>;
  __shared__ float part[256 * V];
  const int Pl = Cl / V, tid = threadIdx.x;
  const int jl = tid % Pl, gs = tid / Pl, s = gs % S, g = gs / S;
  const unsigned pix = blockIdx.x * (unsigned)G + g;
  const bool live = g < G && pix < n_pix;
  float acc[V];
#pragma unroll
  for (int i = 0; i < V; ++i) acc[i] = 0.f;
  if (live) {
    const int c = pix % (unsigned)l.w, rest = pix / (unsigned)l.w, r = rest % (unsigned)l.h, t = rest / (unsigned)l.h;
    const int32_t *i0h = tab + l.i0h, *i0w = tab + l.i0w, *fh = tab + l.firsth, *fw = tab + l.firstw;
    const float *lamh = (const float *)tab + l.lamh, *lamw = (const float *)tab + l.lamw;
    const int y_lo = fh[max(r - 1, 0)], y_hi = fh[r + 1], x_lo = fw[max(c - 1, 0)], x_hi = fw[c + 1];
    for (int y = y_lo + s; y < y_hi; y += S) {
      const int h1 = i0h[y], h1p = h1 < l.h - 1 ? 1 : 0;
      const float h1l = lamh[y];
      const float ly[2] = {1.f - h1l, h1l};
      const bool hit_y[2] = {h1 == r, h1 + h1p == r};
      const T *grow = gcat + (((size_t)t * H + y) * W) * Cc + c_off + jl * V;
      const T *rrow = gres ? gres + (((size_t)t * H + y) * W) * Cl + jl * V : nullptr;
      for (int x = x_lo; x < x_hi; ++x) {
        const int w1 = i0w[x], w1p = w1 < l.w - 1 ? 1 : 0;
        const float w1l = lamw[x];
        const float lx[2] = {1.f - w1l, w1l};
        const bool hit_x[2] = {w1 == c, w1 + w1p == c};
        const vec gv = *(const vec *)(grow + (size_t)x * Cc);
        float gf[V];
#pragma unroll
        for (int i = 0; i < V; ++i) gf[i] = (float)gv[i];
        if (rrow) {
          const vec rv = *(const vec *)(rrow + (size_t)x * Cl);
#pragma unroll
          for (int i = 0; i < V; ++i) gf[i] = gf[i] + (float)rv[i];
        }
#pragma unroll
        for (int cy = 0; cy < 2; ++cy) {
#pragma unroll
          for (int cx = 0; cx < 2; ++cx) {
            if (hit_y[cy] && hit_x[cx]) {
              const float wgt = ly[cy] * lx[cx];
#pragma unroll
              for (int i = 0; i < V; ++i) acc[i] = acc[i] + wgt * gf[i];
            }
          }
        }
      }
    }
  }
  if (S > 1) {
#pragma unroll
    for (int i = 0; i < V; ++i) part[tid * V + i] = acc[i];
    __syncthreads();
    if (live && s == 0) {
      for (int q = 1; q < S; ++q) {
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] = acc[i] + part[(tid + q * Pl) * V + i];
      }
    }
  }
  if (live && s == 0) {
    vec o;
#pragma unroll
    for (int i = 0; i < V; ++i) o[i] = (T)acc[i];
    *(vec *)(gxk + (size_t)pix * Cl + jl * V) = o;
  }
}

inline int fid_row_split(int H, int hk, int Cl, int V) { return std::max(1, std::min(std::min(8, (H / hk) / 2), 256 / (Cl / V))); }

int fid_check(const char *who, int32_t T, int32_t H, int32_t W, const int32_t *hk, const int32_t *wk, int32_t Ca, int32_t Cb, int32_t Cl,
              int32_t half) {
  TS_REQUIRE(T >= 0 && H > 0 && W > 0 && hk && wk && Ca > 0 && Cb > 0 && Cl > 0, TS_ERR_INVALID_ARGUMENT, "%s: bad sizes", who);
  for (int k = 0; k < 3; ++k)
    TS_REQUIRE(hk[k] >= 1 && hk[k] <= H && wk[k] >= 1 && wk[k] <= W, TS_ERR_INVALID_ARGUMENT,
               "%s: a coarse map must be 1 .. H by 1 .. W", who);
  const int v = half ? 8 : 4;
  TS_REQUIRE(Ca % v == 0 && Cb % v == 0 && Cl % v == 0 && Ca <= 1024 && Cb <= 1024 && Cl <= 1024, TS_ERR_UNSUPPORTED,
             "%s: every operand's channels must be a multiple of %d (16-byte pieces of a row), <= 1024", who, v);
  TS_REQUIRE((int64_t)T * H * W * ((Ca + Cb + 3 * Cl) / v) < (1LL << 32) - 256, TS_ERR_UNSUPPORTED,
             "%s: stack too large for 32-bit item indices", who);
  return TS_OK;
}

}  // namespace

extern "C" size_t ts_fid_upcat_tables_bytes(int32_t H, int32_t W) {
  // per level: i0 and lam of both axes, and at most H + 1 / W + 1 lower bounds
  return (size_t)3 * (3 * ((size_t)H + W) + 2) * sizeof(int32_t);
}

extern "C" int ts_fid_upcat_tables(int32_t H, int32_t W, const int32_t *hk, const int32_t *wk, void *tables, size_t tables_bytes,
                                   ts_stream_t stream_) {
  TS_REQUIRE(H > 0 && W > 0 && hk && wk && tables, TS_ERR_INVALID_ARGUMENT, "ts_fid_upcat_tables: bad arguments");
  for (int k = 0; k < 3; ++k)
    TS_REQUIRE(hk[k] >= 1 && hk[k] <= H && wk[k] >= 1 && wk[k] <= W, TS_ERR_INVALID_ARGUMENT,
               "ts_fid_upcat_tables: a coarse map must be 1 .. H by 1 .. W");
  TS_REQUIRE(tables_bytes >= ts_fid_upcat_tables_bytes(H, W), TS_ERR_WORKSPACE_TOO_SMALL, "ts_fid_upcat_tables: buffer too small");
  const FidPlan p = fid_plan(H, W, hk, wk);
  fid_tables_kernel<<<6, 256, 0, (hipStream_t)stream_>>>(p, H, W, (int32_t *)tables);
  TS_CHECK_LAUNCH("ts_fid_upcat_tables");
  return TS_OK;
}

extern "C" int ts_fid_upcat_rows_forward(const void *x, const void *x1, const void *xk0, const void *xk1, const void *xk2, const void *tables,
                                         int32_t T, int32_t H, int32_t W, const int32_t *hk, const int32_t *wk, int32_t Ca, int32_t Cb,
                                         int32_t Cl, int32_t half, void *cat, void *res0, void *res1, void *res2, ts_stream_t stream_) {
  const char *who = "ts_fid_upcat_rows_forward";
  const int rc = fid_check(who, T, H, W, hk, wk, Ca, Cb, Cl, half);
  if (rc != TS_OK) return rc;
  if (T == 0) return TS_OK;
  TS_REQUIRE(x && x1 && xk0 && xk1 && xk2 && tables && cat, TS_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
  TS_REQUIRE(aligned16(x, x1, xk0, xk1) && aligned16(xk2, cat, res0, res1) && aligned16(res2, tables), TS_ERR_INVALID_ARGUMENT,
             "%s: pointers must be 16-byte aligned", who);
  const FidPlan p = fid_plan(H, W, hk, wk);
  const int64_t n_items = (int64_t)T * H * W * ((Ca + Cb + 3 * Cl) / (half ? 8 : 4));
  by_half(half, [&](auto t) {
    using E = decltype(t);
    fid_upcat_fwd_kernel<E><<<(unsigned)ts_cdiv(n_items, 256), 256, 0, (hipStream_t)stream_>>>(
        (const E *)x, (const E *)x1, (const E *)xk0, (const E *)xk1, (const E *)xk2, p, (const int32_t *)tables, H, W, Ca, Cb, Cl,
        (unsigned)n_items, (E *)cat, (E *)res0, (E *)res1, (E *)res2);
  });
  TS_CHECK_LAUNCH(who);
  return TS_OK;
}

extern "C" int ts_fid_upcat_rows_backward(const void *grad_cat, const void *grad_res0, const void *grad_res1, const void *grad_res2,
                                          const void *tables, int32_t T, int32_t H, int32_t W, const int32_t *hk, const int32_t *wk,
                                          int32_t Ca, int32_t Cb, int32_t Cl, int32_t half, void *grad_x, void *grad_x1, void *grad_xk0,
                                          void *grad_xk1, void *grad_xk2, ts_stream_t stream_) {
  const char *who = "ts_fid_upcat_rows_backward";
  const int rc = fid_check(who, T, H, W, hk, wk, Ca, Cb, Cl, half);
  if (rc != TS_OK) return rc;
  if (T == 0) return TS_OK;
  TS_REQUIRE(grad_cat && tables && grad_x && grad_x1 && grad_xk0 && grad_xk1 && grad_xk2, TS_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
  TS_REQUIRE(aligned16(grad_cat, grad_res0, grad_res1, grad_res2) && aligned16(tables, grad_x, grad_x1, grad_xk0) &&
                 aligned16(grad_xk1, grad_xk2),
             TS_ERR_INVALID_ARGUMENT, "%s: pointers must be 16-byte aligned", who);
  const FidPlan p = fid_plan(H, W, hk, wk);
  const int v = half ? 8 : 4, Cc = Ca + Cb + 3 * Cl;
  const int64_t n_split = (int64_t)T * H * W * ((Ca + Cb) / v);
  const void *gres[3] = {grad_res0, grad_res1, grad_res2};
  void *gxk[3] = {grad_xk0, grad_xk1, grad_xk2};
  hipStream_t stream = (hipStream_t)stream_;
  by_half(half, [&](auto t) {
    using E = decltype(t);
    fid_split_bwd_kernel<E><<<(unsigned)ts_cdiv(n_split, 256), 256, 0, stream>>>((const E *)grad_cat, Ca, Cb, Cc, (unsigned)n_split,
                                                                                 (E *)grad_x, (E *)grad_x1);
    for (int k = 0; k < 3; ++k) {
      const FidLevel &l = p.lv[k];
      const int S = fid_row_split(H, l.h, Cl, v), G = 256 / (S * (Cl / v));
      const int64_t n_pix = (int64_t)T * l.h * l.w;
      fid_up_bwd_kernel<E><<<(unsigned)ts_cdiv(n_pix, G), 256, 0, stream>>>((const E *)grad_cat, (const E *)gres[k], l,
                                                                            (const int32_t *)tables, H, W, Cc, Ca + Cb + k * Cl, Cl, S, G,
                                                                            (unsigned)n_pix, (E *)gxk[k]);
    }
  });
  TS_CHECK_LAUNCH(who);
  return TS_OK;
}
