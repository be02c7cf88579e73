// The range-view family's data stage and post-processing on the device, for a whole batch:
//   ts_rv_project   LaserScan.do_range_projection (reference pcseg/data/dataset/semantickitti/laserscan.py:182-238) and
//                   SemkittiRangeViewDataset.prepare_input_label_semantic_with_mask (semantickitti_rv.py:284-301): per scan on the host
//                   a norm, two inverse trigonometric functions, an argsort by depth and four fancy assignments - here two kernels.
//   ts_rv_knn       KNN.forward (pcseg/model/segmentor/range/utils.py:300-341): per scan two [1, S S, n] unfold gathers, a topk, two
//                   gathers and a scatter_add_ into a one-hot - here one lane per point, selection and vote in registers.
//   ts_rv_augment   LaserScan.open_scan's point augmentation (laserscan.py:104-143: np.delete of the dropped rows, flip, scale, rotate,
//                   jitter) of a whole batch into a NEW cloud: a kernel that clears a keep byte per dropped row, then the stable
//                   compaction of compact.h with the augmentation in its rule.
//   ts_rv_label_counts / ts_rv_compose   RangeShift, RangeMix, RangePaste, RangeUnion (semantickitti_rv.py:137-183, :197-320,
//                   MixTeacherSemkitti) of a batch of projected images: class counts of the partner images, then one thread per
//                   output pixel that decides between the primary and the partner and copies once.
// Every value in the reference's own float32 chain, operation by operation (numpy 2: Python scalars are weak, so the chain stays
// float32); compiled with -ffp-contract=off.  The one stated difference: numpy's float32 arctan2 / arcsin are not correctly rounded,
// here they are the (float) of the double functions - as ts_cylinder_cells and ts_range_inputs.
#include "common.h"
#include "compact.h"

namespace {

constexpr float kPi = 3.14159265358979323846f;         // (float)np.pi
constexpr unsigned long long kEmpty = 0xFFFFFFFFFFFFFFFFULL;

// One thread per point row i = feat[i, 0 .. 3] = x, y, z, remission; batch[i] = its scan; first[b] = the scan's first row.
//   depth  sqrtf((x x + y y) + z z)                        np.linalg.norm(points, 2, axis=1) on float32 rows
//   yaw    -(float)atan2((double)y, (double)x), pitch (float)asin((double)(z / depth))
//   proj_x 0.5f (yaw / (float)pi + 1.0f) W, proj_y (1.0f - (pitch + (float)|fov_down|) / (float)fov) H, floor, clamp
// and ONE 64-bit atomicMin of (bits of depth) << 32 | (i - first[b]) on the pixel's slot of `table` (pre-filled with all ones): the
// pixel's winner is the row of smallest depth, the lowest index among equal depths - what the reference's descending stable sort
// followed by "last assignment wins" leaves - whatever the order the threads arrive in.  A row with a non-finite coordinate (16),
// depth == 0 (32) or a batch index outside [0, B) / a row in front of its scan's first (1) takes no part: proj_x = proj_y = -1,
// unproj_range = -1, and its bit in *err.
__global__ __launch_bounds__(256) void rv_points_kernel(const float *__restrict__ feat, int64_t ld, const int *__restrict__ batch,
                                                        const int *__restrict__ first, int64_t n, int B, int H, int W, float fd_abs,
                                                        float fov, int *__restrict__ proj_x, int *__restrict__ proj_y,
                                                        float *__restrict__ unproj_range, unsigned long long *__restrict__ table,
                                                        int *__restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float *p = feat + i * ld;
  const float x = p[0], y = p[1], z = p[2];
  const int b = batch[i];
  int flag = 0;
  int64_t local = -1;
  if (b < 0 || b >= B) {
    flag |= 1;
  } else {
    local = i - (int64_t)first[b];
    if (local < 0) flag |= 1;
  }
  float depth = -1.f;
  if (!isfinite(x) || !isfinite(y) || !isfinite(z)) {
    flag |= 16;
  } else {
    depth = sqrtf((x * x + y * y) + z * z);
    if (depth == 0.f) flag |= 32;
  }
  int col = -1, row = -1;
  if (flag == 0) {
    const float yaw = -(float)atan2((double)y, (double)x);
    const float pitch = (float)asin((double)(z / depth));
    float fx = 0.5f * (yaw / kPi + 1.0f);
    float fy = 1.0f - (pitch + fd_abs) / fov;
    fx = fx * (float)W;
    fy = fy * (float)H;
    fx = fmaxf(0.f, fminf((float)(W - 1), floorf(fx)));
    fy = fmaxf(0.f, fminf((float)(H - 1), floorf(fy)));
    col = (int)fx;
    row = (int)fy;
    const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned long long)(uint32_t)local;
    atomicMin(table + ((int64_t)b * H + row) * W + col, key);
  } else {
    atomicOr(err, flag);
    depth = -1.f;
  }
  proj_x[i] = col;
  proj_y[i] = row;
  unproj_range[i] = depth;
}

// One thread per pixel: the winner's x / 50, y / 50, z / 3, remission, depth / 80 (float32 divisions), mask = (local index > 0) -
// the reference's `proj_idx > 0`, reproduced: a pixel won by a scan's row 0 carries real values and mask 0 - the range, the local
// index and the label; or the background -1 / 50, -1 / 50, -1 / 3, -1, -1 / 80, 0, range -1, index -1, label 0.
__global__ __launch_bounds__(256) void rv_pixels_kernel(const float *__restrict__ feat, int64_t ld, const int *__restrict__ first,
                                                        const int *__restrict__ label, const unsigned long long *__restrict__ table,
                                                        int64_t n, int B, int64_t hw, float *__restrict__ scan_rv,
                                                        float *__restrict__ proj_range, int *__restrict__ proj_idx,
                                                        int64_t *__restrict__ label_rv) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= (int64_t)B * hw) return;
  const int64_t b = q / hw, r = q - b * hw;
  const unsigned long long key = table[q];
  float vx = -1.f, vy = -1.f, vz = -1.f, rem = -1.f, range = -1.f, mask = 0.f;
  int idx = -1;
  int64_t lab = 0;
  if (key != kEmpty) {
    const int64_t local = (int64_t)(uint32_t)key;
    const int64_t row = (int64_t)first[b] + local;
    if (row >= 0 && row < n) {
      const float *p = feat + row * ld;
      vx = p[0]; vy = p[1]; vz = p[2]; rem = p[3];
      range = __uint_as_float((uint32_t)(key >> 32));
      idx = (int)local;
      mask = local > 0 ? 1.f : 0.f;
      if (label) lab = (int64_t)label[row];
    }
  }
  float *dst = scan_rv + b * 6 * hw + r;
  dst[0] = vx / 50.0f;
  dst[hw] = vy / 50.0f;
  dst[2 * hw] = vz / 3.0f;
  dst[3 * hw] = rem;
  dst[4 * hw] = range / 80.0f;
  dst[5 * hw] = mask;
  proj_range[q] = range;
  proj_idx[q] = idx;
  if (label_rv) label_rv[q] = lab;
}

// One lane per point: the S x S window of its pixel, K rounds of a minimum over the S S distances by ascending (distance, slot), the
// vote of the K selected classes.  The distances stay in registers (every index below is a compile-time constant after unrolling),
// the taken slots in one 64-bit mask, the counts of classes 1 .. 31 in four 64-bit words of eight 8-bit fields (a count is at most
// S S = 49): no scratch, no [S S, n] temporaries.  The class of a selected slot is read when it is selected - K loads that hit the
// lines the range window just touched - so the window's classes need no registers of their own.
template <int S>
__global__ __launch_bounds__(256) void rv_knn_kernel(const float *__restrict__ proj_range, const int *__restrict__ proj_class,
                                                     const float *__restrict__ unproj_range, const int *__restrict__ px,
                                                     const int *__restrict__ py, const int *__restrict__ batch,
                                                     const float *__restrict__ weight, int64_t n, int B, int H, int W, int K,
                                                     float cutoff, int nclasses, int *__restrict__ label, int *__restrict__ err) {
  constexpr int SS = S * S, P = (S - 1) / 2, CENTRE = (SS - 1) / 2;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int b = batch[i], x = px[i], y = py[i];
  int flag = 0;
  if (b < 0 || b >= B) flag |= 1;
  if (x < 0 || x >= W || y < 0 || y >= H) flag |= 2;
  if (flag) {
    atomicOr(err, flag);
    label[i] = 0;
    return;
  }
  const float rp = unproj_range[i];
  const float *img = proj_range + (int64_t)b * H * W;
  const int *cls = proj_class + (int64_t)b * H * W;
  float d[SS];
#pragma unroll
  for (int dy = 0; dy < S; ++dy) {
#pragma unroll
    for (int dx = 0; dx < S; ++dx) {
      const int s = dy * S + dx;
      const int yy = y + dy - P, xx = x + dx - P;
      const bool inside = yy >= 0 && yy < H && xx >= 0 && xx < W;
      float r = inside ? img[(int64_t)yy * W + xx] : 0.f;              // F.unfold's zero padding: no wrap in azimuth
      if (r < 0.f) r = __builtin_inff();
      if (s == CENTRE) r = rp;
      float v = fabsf(r - rp) * weight[s];
      if (!(v == v)) v = __builtin_inff();                             // a NaN distance counts as +inf: the order stays total
      d[s] = v;
    }
  }
  unsigned long long taken = 0, c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  for (int k = 0; k < K; ++k) {
    float best = 0.f;
    int bs = -1;
#pragma unroll
    for (int s = 0; s < SS; ++s) {
      const bool is_free = ((taken >> s) & 1ULL) == 0;
      if (is_free && (bs < 0 || d[s] < best)) {
        best = d[s];
        bs = s;
      }
    }
    taken |= 1ULL << bs;
    const int dy = bs / S, dx = bs - dy * S;
    const int yy = y + dy - P, xx = x + dx - P;
    int c = 0;
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) c = cls[(int64_t)yy * W + xx];
    if (cutoff > 0.f && best > cutoff) c = nclasses;
    const bool votes = c >= 1 && c < nclasses;
    const unsigned long long inc = 1ULL << ((c & 7) * 8);
    const int word = c >> 3;
    c0 += (votes && word == 0) ? inc : 0ULL;
    c1 += (votes && word == 1) ? inc : 0ULL;
    c2 += (votes && word == 2) ? inc : 0ULL;
    c3 += (votes && word == 3) ? inc : 0ULL;
  }
  int best_c = 1, best_n = -1;
#pragma unroll
  for (int c = 1; c < 32; ++c) {
    const unsigned long long word = (c >> 3) == 0 ? c0 : (c >> 3) == 1 ? c1 : (c >> 3) == 2 ? c2 : c3;
    const int cnt = (int)((word >> ((c & 7) * 8)) & 0xFFULL);
    if (c < nclasses && cnt > best_n) {                               // the first maximum: argmax(dim=1) of [:, 1:-1], + 1
      best_n = cnt;
      best_c = c;
    }
  }
  label[i] = best_c;
}

// ------------------------------------------------------------------------------------------------ training augmentation
// LaserScan.open_scan's point augmentation (laserscan.py:113-143) of one row by one record of TS_RV_AUG_RECORD doubles
//   { c, s, scale, tx, ty, tz, bits, flip }   bits: 1 rotate, 2 scale, 4 flip, 8 jitter ; flip: 0 .. 3
// in the reference's order - flip, scale, rotate, jitter - and with ITS roundings: it assigns back into the float32 array after
// every step, so every step rounds to float32 (not sr_augment's single rounding at the end).  Scale: x and y only, a float32
// product with (float)scale (a Python float is a weak scalar).  Rotation: np.dot(float32 [n, 2], float64 2 x 2) is dgemm's
// fused-multiply-add chain in k order, rounded once.  Jitter: float32 += float64 adds in float64.  A step that is off is skipped.
__device__ __forceinline__ void rv_augment_row(const double *__restrict__ a, float &x, float &y, float &z) {
#pragma clang fp contract(off)
  const int bits = (int)a[6];
  if (bits & 4) {
    const int flip = (int)a[7];
    if (flip & 1) x = -x;
    if (flip & 2) y = -y;
  }
  if (bits & 2) {
    const float f = (float)a[2];
    x = __fmul_rn(x, f);
    y = __fmul_rn(y, f);
  }
  if (bits & 1) {
    const double X = x, Y = y, c = a[0], s = a[1];
    x = (float)fma(Y, -s, X * c);
    y = (float)fma(Y, c, X * s);
  }
  if (bits & 8) {
    x = (float)((double)x + a[3]);
    y = (float)((double)y + a[4]);
    z = (float)((double)z + a[5]);
  }
}

// One thread per entry of the concatenated drop lists: entry j belongs to the last cloud b with drop_off[b] <= j and names the
// row first[b] + drop[j] of the input.  An index outside its cloud sets TS_RV_ERR_DROP and clears nothing.
__global__ __launch_bounds__(256) void rv_drop_kernel(const int *__restrict__ drop, const int *__restrict__ drop_off, int64_t n_drop,
                                                      const int *__restrict__ first, int64_t n, int B,
                                                      unsigned char *__restrict__ keep, int *__restrict__ err) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_drop) return;
  int b = 0;
  for (int k = 1; k < B; ++k)
    if ((int64_t)drop_off[k] <= j) b = k;
  const int64_t lo = first[b], hi = b + 1 < B ? (int64_t)first[b + 1] : n, d = drop[j];
  if (lo < 0 || hi > n || d < 0 || lo + d >= hi) {
    atomicOr(err, TS_RV_ERR_DROP);
    return;
  }
  keep[lo + d] = 0;
}

// ts_rv_augment's rule for cp_compact: a row survives when its keep byte is set (no table: every row) and its cloud is in [0, B);
// the survivor is the augmented row, its label goes with it.
struct RaRule : CpRule {
  typedef float4 Row;
  const float *feat;
  int64_t ld;
  const int *batch, *label;
  const unsigned char *keep;
  const double *params;      // [n_samples, TS_RV_AUG_RECORD]
  float4 *out;               // [capacity]
  int *out_label, *err;

  __device__ __forceinline__ bool keeps(int64_t i, bool in, Row &o, int *s) const {
    *s = -1;
    if (!in) return false;
    const int b = batch[i];
    if (b < 0 || b >= n_samples) {
      atomicOr(err, TS_RV_ERR_BATCH);
      return false;
    }
    if (keep && keep[i] == 0) return false;
    *s = b;
    const float *p = feat + i * ld;
    o = make_float4(p[0], p[1], p[2], p[3]);
    rv_augment_row(params + (int64_t)TS_RV_AUG_RECORD * b, o.x, o.y, o.z);
    return true;
  }

  __device__ __forceinline__ void store(int64_t dst, int64_t i, const Row &o) const {
    out[dst] = o;
    if (out_label) out_label[dst] = label[i];
  }
};

// The pixels of every class in every image: LDS counters per block, then one integer atomicAdd per class that occurred.
__global__ __launch_bounds__(256) void rv_counts_kernel(const int64_t *__restrict__ label, int64_t hw, int *__restrict__ counts) {
  __shared__ int h[TS_RV_CLASSES];
  if (threadIdx.x < TS_RV_CLASSES) h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t b = blockIdx.y;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < hw; r += (int64_t)gridDim.x * 256) {
    const int64_t l = label[b * hw + r];
    if (l >= 0 && l < TS_RV_CLASSES) atomicAdd(&h[(int)l], 1);
  }
  __syncthreads();
  if (threadIdx.x < TS_RV_CLASSES && h[threadIdx.x] != 0) atomicAdd(counts + b * TS_RV_CLASSES + threadIdx.x, h[threadIdx.x]);
}

// RangePaste's classes (semantickitti_rv.py:215-279): 2 .. 8, 12, 16, 18, 19
constexpr unsigned kPasteSet = 0x1FCu | (1u << 12) | (1u << 16) | (1u << 18) | (1u << 19);

// One thread per output pixel (b, y, x): RangeShift, RangeMix, RangePaste, RangeUnion of semantickitti_rv.py:137-183 as ONE choice
// between the primary's pixel (y, (x + shift_a) mod W) and the partner's (y, (x + shift_b) mod W), then one copy of six values and
// the label.  rec = records + TS_RV_COMPOSE_RECORD b (layout: include/taseg_hip.h).
__global__ __launch_bounds__(256) void rv_compose_kernel(const float *__restrict__ scan_a, const int64_t *__restrict__ label_a,
                                                         const float *__restrict__ scan_b, const int64_t *__restrict__ label_b,
                                                         const int *__restrict__ counts, const int *__restrict__ records, int B, int H,
                                                         int W, float *__restrict__ out_scan, int64_t *__restrict__ out_label) {
  const int64_t hw = (int64_t)H * W;
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= (int64_t)B * hw) return;
  const int64_t b = q / hw, r = q - b * hw;
  const int y = (int)(r / W), x = (int)(r - (int64_t)y * W);
  const int *rec = records + (int64_t)TS_RV_COMPOSE_RECORD * b;
  const int sa = ((rec[0] % W) + W) % W, sb = ((rec[1] % W) + W) % W;
  int xa = x + sa, xb = x + sb;
  if (xa >= W) xa -= W;
  if (xb >= W) xb -= W;
  const int64_t ra = (int64_t)y * W + xa, rb = (int64_t)y * W + xb;
  bool take_b = false;
  if (scan_b) {
    const int mixture = rec[14], flags = rec[15];
    if (mixture == 1 || mixture == 2) {
      const int nr = min(max(rec[2], 0), 5), nc = min(max(rec[3], 0), 5);
      int cell = 0;
      for (int k = 0; k < nr; ++k) cell += rec[4 + k] <= y;
      for (int k = 0; k < nc; ++k) cell += rec[9 + k] <= x;
      const bool even = (cell & 1) == 0;
      take_b = mixture == 1 ? !even : even;
    }
    if ((flags & 1) && !take_b) {
      const int64_t lb = label_b[b * hw + rb];
      if (lb >= 0 && lb < TS_RV_CLASSES && ((kPasteSet >> (int)lb) & 1u) && counts[b * TS_RV_CLASSES + lb] > 20) take_b = true;
    }
    if ((flags & 2) && !take_b && scan_a[(b * 6 + 5) * hw + ra] == 0.f) take_b = true;
  }
  const float *src = take_b ? scan_b + b * 6 * hw + rb : scan_a + b * 6 * hw + ra;
  float *dst = out_scan + b * 6 * hw + r;
#pragma unroll
  for (int c = 0; c < 6; ++c) dst[c * hw] = src[c * hw];
  out_label[q] = take_b ? label_b[b * hw + rb] : label_a[b * hw + ra];
}

}  // namespace

extern "C" int ts_rv_project(const float *feat, int64_t ld, const int32_t *batch, const int32_t *first, const int32_t *label, int64_t n,
                             int32_t B, int32_t H, int32_t W, double fov_up, double fov_down, int32_t *proj_x, int32_t *proj_y,
                             float *unproj_range, uint64_t *table, float *scan_rv, float *proj_range, int32_t *proj_idx,
                             int64_t *label_rv, int32_t *err, ts_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  TS_REQUIRE(n >= 0 && n < (1LL << 31) - 1 && ld >= 4 && B > 0 && H > 0 && W > 0 && (int64_t)B * H * W < (1LL << 31) - 1,
             TS_ERR_INVALID_ARGUMENT, "ts_rv_project: bad sizes");
  TS_REQUIRE(table && scan_rv && proj_range && proj_idx && err && first && (n == 0 || (feat && batch && proj_x && proj_y && unproj_range)),
             TS_ERR_INVALID_ARGUMENT, "ts_rv_project: null pointer");
  TS_REQUIRE((label == nullptr || label_rv != nullptr) && (label_rv == nullptr || label != nullptr || n == 0), TS_ERR_INVALID_ARGUMENT,
             "ts_rv_project: label and label_rv go together");
  // laserscan.py:182-184 in double, as Python evaluates it; the arrays meet the results as weak scalars, so as float32
  const double up = fov_up / 180.0 * 3.141592653589793, down = fov_down / 180.0 * 3.141592653589793;
  const double fov = (down < 0 ? -down : down) + (up < 0 ? -up : up);
  TS_REQUIRE(fov > 0 && fov == fov, TS_ERR_INVALID_ARGUMENT, "ts_rv_project: empty field of view");
  if (n > 0) {
    rv_points_kernel<<<(unsigned)ts_cdiv(n, (int64_t)256), 256, 0, stream>>>(
        feat, ld, batch, first, n, B, H, W, (float)(down < 0 ? -down : down), (float)fov, proj_x, proj_y, unproj_range,
        (unsigned long long *)table, err);
    TS_CHECK_LAUNCH("ts_rv_project/points");
  }
  const int64_t hw = (int64_t)H * W;
  rv_pixels_kernel<<<(unsigned)ts_cdiv((int64_t)B * hw, (int64_t)256), 256, 0, stream>>>(
      feat, ld, first, label, (const unsigned long long *)table, n, B, hw, scan_rv, proj_range, proj_idx, (int64_t *)label_rv);
  TS_CHECK_LAUNCH("ts_rv_project/pixels");
  return TS_OK;
}

extern "C" int ts_rv_knn(const float *proj_range, const int32_t *proj_class, const float *unproj_range, const int32_t *px,
                         const int32_t *py, const int32_t *batch, const float *weight, int64_t n, int32_t B, int32_t H, int32_t W,
                         int32_t K, int32_t S, float cutoff, int32_t nclasses, int32_t *label, int32_t *err, ts_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  TS_REQUIRE(n >= 0 && n < (1LL << 31) - 1 && B > 0 && H > 0 && W > 0 && (int64_t)B * H * W < (1LL << 31) - 1,
             TS_ERR_INVALID_ARGUMENT, "ts_rv_knn: bad sizes");
  TS_REQUIRE((S == 3 || S == 5 || S == 7) && K >= 1 && K <= S * S && nclasses >= 2 && nclasses <= 32, TS_ERR_UNSUPPORTED,
             "ts_rv_knn: S in {3, 5, 7}, 1 <= K <= S S and 2 <= nclasses <= 32 (got S %d, K %d, nclasses %d)", S, K, nclasses);
  TS_REQUIRE(proj_range && proj_class && weight && err && (n == 0 || (unproj_range && px && py && batch && label)),
             TS_ERR_INVALID_ARGUMENT, "ts_rv_knn: null pointer");
  if (n == 0) return TS_OK;
  const unsigned blocks = (unsigned)ts_cdiv(n, (int64_t)256);
#define TS_RV_KNN(S_)                                                                                                        \
  rv_knn_kernel<S_><<<blocks, 256, 0, stream>>>(proj_range, proj_class, unproj_range, px, py, batch, weight, n, B, H, W, K, \
                                                cutoff, nclasses, label, err)
  if (S == 3) TS_RV_KNN(3);
  else if (S == 5) TS_RV_KNN(5);
  else TS_RV_KNN(7);
#undef TS_RV_KNN
  TS_CHECK_LAUNCH("ts_rv_knn");
  return TS_OK;
}

extern "C" size_t ts_rv_augment_workspace_bytes(int64_t n, int32_t B) { return cp_compact_bytes(n, B); }

extern "C" int ts_rv_augment(const float *feat, int64_t ld, const int32_t *batch, const int32_t *label, const int32_t *first, int64_t n,
                             int32_t B, const double *params, const int32_t *drop, const int32_t *drop_off, int64_t n_drop,
                             uint8_t *keep, float *out, int32_t *out_label, int64_t *out_sample, int32_t *out_sample32,
                             int64_t capacity, int64_t *counts, void *ws, size_t ws_bytes, int32_t *err, ts_stream_t stream_) {
  static_assert(TS_RV_MAX_CLOUDS == TS_WAVE, "cp_count_kernel keeps one LDS counter per (wave, sample)");
  hipStream_t stream = (hipStream_t)stream_;
  TS_REQUIRE(n >= 0 && n < (int64_t)1 << 30 && ld >= 4 && B >= 1 && B <= TS_RV_MAX_CLOUDS && capacity >= n && n_drop >= 0 &&
                 n_drop < (int64_t)1 << 30,
             TS_ERR_INVALID_ARGUMENT, "ts_rv_augment: bad sizes (at most %d clouds)", TS_RV_MAX_CLOUDS);
  TS_REQUIRE(params && counts && err && ws && ((uintptr_t)ws & 3) == 0 && ((uintptr_t)params & 7) == 0, TS_ERR_INVALID_ARGUMENT,
             "ts_rv_augment: null or misaligned pointer");
  TS_REQUIRE(n == 0 || (feat && batch && out && out_sample && out_sample32), TS_ERR_INVALID_ARGUMENT, "ts_rv_augment: null pointer");
  TS_REQUIRE(((uintptr_t)out & 15) == 0, TS_ERR_INVALID_ARGUMENT, "ts_rv_augment: out must be 16-byte aligned");
  TS_REQUIRE((label == nullptr) == (out_label == nullptr) || n == 0, TS_ERR_INVALID_ARGUMENT,
             "ts_rv_augment: label and out_label go together");
  TS_REQUIRE(drop == nullptr || (drop_off && first && (keep || n == 0)), TS_ERR_INVALID_ARGUMENT,
             "ts_rv_augment: drop lists need their offsets, the clouds' first rows and the keep bytes");
  if (drop && n_drop > 0 && n > 0) {
    rv_drop_kernel<<<(unsigned)ts_cdiv(n_drop, (int64_t)256), 256, 0, stream>>>(drop, drop_off, n_drop, first, n, B, keep, err);
    TS_CHECK_LAUNCH("ts_rv_augment/drop");
  }
  const RaRule r = {{n, capacity, B, out_sample, out_sample32}, feat, ld, batch, label, drop ? keep : nullptr, params, (float4 *)out,
                    out_label, err};
  return cp_compact(r, "ts_rv_augment", counts, ws, ws_bytes, stream);
}

extern "C" int ts_rv_label_counts(const int64_t *label, int32_t B, int32_t H, int32_t W, int32_t *counts, ts_stream_t stream_) {
  TS_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)B * H * W < (1LL << 31) - 1, TS_ERR_INVALID_ARGUMENT,
             "ts_rv_label_counts: bad sizes");
  TS_REQUIRE(label && counts, TS_ERR_INVALID_ARGUMENT, "ts_rv_label_counts: null pointer");
  const int64_t hw = (int64_t)H * W;
  const dim3 grid((unsigned)ts_cdiv(hw, (int64_t)1024), (unsigned)B);
  rv_counts_kernel<<<grid, 256, 0, (hipStream_t)stream_>>>(label, hw, counts);
  TS_CHECK_LAUNCH("ts_rv_label_counts");
  return TS_OK;
}

extern "C" int ts_rv_compose(const float *scan_a, const int64_t *label_a, const float *scan_b, const int64_t *label_b,
                             const int32_t *counts, const int32_t *records, int32_t B, int32_t H, int32_t W, float *out_scan,
                             int64_t *out_label, ts_stream_t stream_) {
  TS_REQUIRE(B > 0 && H > 0 && W > 0 && (int64_t)B * H * W * 6 < (1LL << 31) - 1, TS_ERR_INVALID_ARGUMENT, "ts_rv_compose: bad sizes");
  TS_REQUIRE(scan_a && label_a && records && out_scan && out_label, TS_ERR_INVALID_ARGUMENT, "ts_rv_compose: null pointer");
  TS_REQUIRE(scan_b == nullptr || (label_b && counts), TS_ERR_INVALID_ARGUMENT,
             "ts_rv_compose: the partner images come with their labels and class counts");
  TS_REQUIRE(out_scan != scan_a && out_scan != scan_b, TS_ERR_INVALID_ARGUMENT, "ts_rv_compose: not in place");
  rv_compose_kernel<<<(unsigned)ts_cdiv((int64_t)B * H * W, (int64_t)256), 256, 0, (hipStream_t)stream_>>>(
      scan_a, label_a, scan_b, label_b, counts, records, B, H, W, out_scan, out_label);
  TS_CHECK_LAUNCH("ts_rv_compose");
  return TS_OK;
}
