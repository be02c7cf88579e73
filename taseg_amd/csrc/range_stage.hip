// RPVNet's inputs on the device: range_image [B, 5, H, W] and range_pxpy [n, 3] from a batch's point rows - what
// SemkittiFusionDataset.get_range_image (reference semantickitti_fusion.py:64-114) computes per sample in numpy on the host, for
// the whole batch in two kernels.  Every value in the reference's own precision, operation by operation (numpy 2 keeps the yaw
// chain in float32; px / py and the image values are float64 expressions cast once); compiled with -ffp-contract=off.  The one
// stated difference: numpy's float32 arctan2 is not correctly rounded, here it is (float)atan2 of the doubles - as ts_cylinder_cells.
#include "common.h"

namespace {

constexpr float kPi = 3.14159265358979323846f;         // (float)np.pi
constexpr float kTwoPi = 6.28318530717958647692f;      // (float)(2 * np.pi)

// np.remainder for float32: fmod, then the divisor's sign
__device__ __forceinline__ float np_mod(float a, float b) {
  float m = fmodf(a, b);
  if (m != 0.f) {
    if ((b < 0.f) != (m < 0.f)) m += b;
  } else {
    m = copysignf(0.f, b);
  }
  return m;
}

// One thread per point row i = feat[i, 0 .. 4] = x, y, z, reflectivity, ring; batch[i] = its sample.
//   yaw     (float)atan2((double)y, -(double)x) + cut[b]; yaw % 2 pi - pi; proj_x = 0.5 (yaw / pi + 1) (W - 1), all float32
//   column  (int32)rint(proj_x), row (int32)rint(ring)                     (np.round: half to even)
//   px, py  2 (column / (W - 1) - 0.5), 2 (row / (H - 1) - 0.5) in float64, rounded to float32 once (collate's .float())
// and an integer atomicMax of i on the pixel's entry of `table` (pre-filled with -1): "last row wins", as numpy's fancy assignment
// does, whatever the order the threads arrive in.  A row with a ring above H - 1 (the reference's assert) or below 0, a batch index
// outside [0, B) or a non-finite coordinate takes no part: pxpy = (b, NaN, NaN) - ts_range_plan flags and drops it again - and a bit
// in *err: 8 ring, 16 non-finite, 1 batch.
__global__ __launch_bounds__(256) void range_points_kernel(const float *__restrict__ feat, int64_t ld, const int *__restrict__ batch,
                                                           const float *__restrict__ cut, int64_t n, int B, int H, int W,
                                                           float *__restrict__ pxpy, int *__restrict__ table, int *__restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float *p = feat + i * ld;
  const float x = p[0], y = p[1], z = p[2], ring = p[4];
  const int b = batch[i];
  int flag = 0;
  if (b < 0 || b >= B) flag |= 1;
  if (!isfinite(x) || !isfinite(y) || !isfinite(z) || !isfinite(ring)) flag |= 16;
  else if (!(ring <= (float)(H - 1) && rintf(ring) >= 0.f)) flag |= 8;
  float fpx = __builtin_nanf(""), fpy = __builtin_nanf("");
  if (flag == 0) {
    float yaw = (float)atan2((double)y, -(double)x) + cut[b];
    yaw = np_mod(yaw, kTwoPi) - kPi;
    float proj_x = 0.5f * (yaw / kPi + 1.0f);
    proj_x = proj_x * (float)(W - 1);
    const int col = (int)rintf(proj_x), row = (int)rintf(ring);
    if (col < 0 || col >= W) {
      flag |= 16;
    } else {
      fpx = (float)(2.0 * ((double)col / (double)(W - 1) - 0.5));
      fpy = (float)(2.0 * ((double)row / (double)(H - 1) - 0.5));
      atomicMax(table + ((int64_t)b * H + row) * W + col, (int)i);
    }
  }
  if (flag) atomicOr(err, flag);
  pxpy[3 * i] = (float)b;
  pxpy[3 * i + 1] = fpx;
  pxpy[3 * i + 2] = fpy;
}

// One thread per pixel: the winner's five values - 25 (1 / depth - 0.4) and 20 (reflectivity - 0.5) in float64 on the float32
// quotient and value, cast once; x, y, z - or the background -10, -10, 0, 0, 0 (the reference's zeros through the same expressions).
// depth = sqrt((x x + y y) + z z) in float32 (np.linalg.norm on float32 rows).
__global__ __launch_bounds__(256) void range_image_kernel(const float *__restrict__ feat, int64_t ld, const int *__restrict__ table,
                                                          int64_t n, int B, int64_t hw, float *__restrict__ image) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= (int64_t)B * hw) return;
  const int64_t b = q / hw, r = q - b * hw;
  const int i = table[q];
  float v[5] = {-10.f, -10.f, 0.f, 0.f, 0.f};
  if (i >= 0 && i < n) {
    const float *p = feat + (int64_t)i * ld;
    const float x = p[0], y = p[1], z = p[2], refl = p[3];
    const float depth = sqrtf((x * x + y * y) + z * z);
    const float inv = 1.0f / depth;
    v[0] = (float)(25.0 * ((double)inv - 0.4));
    v[1] = (float)(20.0 * ((double)refl - 0.5));
    v[2] = x; v[3] = y; v[4] = z;
  }
  float *dst = image + b * 5 * hw + r;
#pragma unroll
  for (int k = 0; k < 5; ++k) dst[k * hw] = v[k];
}

}  // namespace

extern "C" int ts_range_inputs(const float *feat, int64_t ld, const int32_t *batch, const float *cut, int64_t n, int32_t B, int32_t H,
                               int32_t W, float *pxpy, int32_t *table, float *image, int32_t *err, ts_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  TS_REQUIRE(n >= 0 && n < (1LL << 31) - 1 && ld >= 5 && B > 0 && H > 1 && W > 1 && (int64_t)B * H * W < (1LL << 31) - 1,
             TS_ERR_INVALID_ARGUMENT, "ts_range_inputs: bad sizes");
  TS_REQUIRE(table && image && err && cut && (n == 0 || (feat && batch && pxpy)), TS_ERR_INVALID_ARGUMENT,
             "ts_range_inputs: null pointer");
  if (n > 0) {
    range_points_kernel<<<(unsigned)ts_cdiv(n, (int64_t)256), 256, 0, stream>>>(feat, ld, batch, cut, n, B, H, W, pxpy, table, err);
    TS_CHECK_LAUNCH("ts_range_inputs/points");
  }
  const int64_t hw = (int64_t)H * W;
  range_image_kernel<<<(unsigned)ts_cdiv((int64_t)B * hw, (int64_t)256), 256, 0, stream>>>(feat, ld, table, n, B, hw, image);
  TS_CHECK_LAUNCH("ts_range_inputs/image");
  return TS_OK;
}
