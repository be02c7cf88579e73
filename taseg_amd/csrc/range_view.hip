// The range-view family's data stage and post-processing on the device, for a whole batch:
//   ts_rv_project   LaserScan.do_range_projection (reference pcseg/data/dataset/semantickitti/laserscan.py:182-238) and
//                   SemkittiRangeViewDataset.prepare_input_label_semantic_with_mask (semantickitti_rv.py:284-301): per scan on the host
//                   a norm, two inverse trigonometric functions, an argsort by depth and four fancy assignments - here two kernels.
//   ts_rv_knn       KNN.forward (pcseg/model/segmentor/range/utils.py:300-341): per scan two [1, S S, n] unfold gathers, a topk, two
//                   gathers and a scatter_add_ into a one-hot - here one lane per point, selection and vote in registers.
// Every value in the reference's own float32 chain, operation by operation (numpy 2: Python scalars are weak, so the chain stays
// float32); compiled with -ffp-contract=off.  The one stated difference: numpy's float32 arctan2 / arcsin are not correctly rounded,
// here they are the (float) of the double functions - as ts_cylinder_cells and ts_range_inputs.
#include "common.h"

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
