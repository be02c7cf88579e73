// The row rules of the data stage whose bits are pinned to numpy (library-internal): written once, used by every kernel that
// decides on or moves a row.
#pragma once
#include "common.h"

// (x, y, z) >= lo[sample] (semantickitti_voxel_ms.py:121-124): numpy's `>=` on float32, false for NaN on either side.  The caller
// checks the range of `sample`.
__device__ __forceinline__ bool sr_clamp_keeps(float x, float y, float z, const float *__restrict__ lo, int64_t sample) {
  const float *q = lo + 3 * sample;
  return x >= q[0] && y >= q[1] && z >= q[2];
}

// table[scan][class], the class-step rule (semantickitti_ms.py:303-308): a negative class reads column neg_col (KITTI: a pseudo
// label that is no class's canonical raw id: never kept)
__device__ __forceinline__ bool sr_class_step(const unsigned char *__restrict__ table, int scan, int64_t c, int cols, int neg_col) {
  if (c < 0) c = neg_col;
  return c >= 0 && c < cols && table[(int64_t)scan * cols + c] != 0;
}

// np.dot(xyz, [[c, s, 0], [-s, c, 0], [0, 0, 1]]) in float64: dgemm's fused-multiply-add chain in k order.  The order matters
// where x*c and y*s cancel (a point at 45 degrees of azimuth under the TTA rotation pi/4): what is left is the rounding error of
// the first product, and it decides the float32 result.
__device__ __forceinline__ double3 sr_rotate_z(double X, double Y, double Z, double c, double s) {
#pragma clang fp contract(off)          // only the explicit fma() fuse, whatever the including file is compiled with
  const double rx = fma(Z, 0.0, fma(Y, -s, X * c));
  const double ry = fma(Z, 0.0, fma(Y, c, X * s));
  const double rz = fma(Z, 1.0, fma(Y, 0.0, X * 0.0));
  return make_double3(rx, ry, rz);
}

// o = M v for a row-major 3 x 3: dgemm's fused-multiply-add chain in k order, one row of M per output.  (Ptr, here and below: a
// pointer to const double in whichever address space the caller's table lies.)
template <typename Ptr>
__device__ __forceinline__ void sr_mat3(Ptr M, const double (&v)[3], double (&o)[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 3; ++j) o[j] = __builtin_fma(M[3 * j + 2], v[2], __builtin_fma(M[3 * j + 1], v[1], M[3 * j] * v[0]));
}

// The multi-scan pose fuse of ts_fuse_scan (semantickitti_ms.py fuse_multi_scan) in place on (x, y, z): P = the scan's pose, Q = the
// current frame's, both [16] row-major, float32 throughout - numpy multiplies, then adds, in k order:
//   new_j = ((h0 P[j][0] + h1 P[j][1]) + h2 P[j][2]) + h3 P[j][3] - Q[j][3]      h = (x, y, z, 1)
//   out_j = (new0 Q[0][j] + new1 Q[1][j]) + new2 Q[2][j]
// __fmul_rn / __fadd_rn are inline functions of the HIP headers: no `#pragma clang fp contract(off)` here or in the caller reaches
// them, so every operation keeps its own rounding ONLY in a file that csrc/build.py compiles with -ffp-contract=off (EXTRA).
template <typename PtrP, typename PtrQ>
__device__ __forceinline__ void sr_fuse_pose(PtrP P, PtrQ Q, float &x, float &y, float &z) {
  const float h[4] = {x, y, z, 1.0f};
  float nw[3], o[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    float s = __fmul_rn(h[0], P[j * 4 + 0]);
    s = __fadd_rn(s, __fmul_rn(h[1], P[j * 4 + 1]));
    s = __fadd_rn(s, __fmul_rn(h[2], P[j * 4 + 2]));
    s = __fadd_rn(s, __fmul_rn(h[3], P[j * 4 + 3]));
    nw[j] = __fsub_rn(s, Q[j * 4 + 3]);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    float s = __fmul_rn(nw[0], Q[0 * 4 + j]);
    s = __fadd_rn(s, __fmul_rn(nw[1], Q[1 * 4 + j]));
    s = __fadd_rn(s, __fmul_rn(nw[2], Q[2 * 4 + j]));
    o[j] = s;
  }
  x = o[0];
  y = o[1];
  z = o[2];
}

// The KITTI camera projection, frustum test and pixel of ts_project_fov (semantickitti_ms_mm.py:419-434): P = P2 Tr [12] row-major,
// sum_k P[j][k] (x, y, z, 1)[k] as dgemm's chain in k order, the two divisions, astype(int).  row / col are 0 where the frustum
// test fails.  The flip and the crop test are the caller's.  (The image size by reference: a caller that holds it in a record reads
// it where the test uses it, after the divisions - by value the loads move up and tf_row holds 6 VGPRs more.)
template <typename Ptr>
__device__ __forceinline__ bool sr_project_fov(Ptr P, float x, float y, float z, const int &img_w, const int &img_h, int &row,
                                               int &col) {
#pragma clang fp contract(off)
  const double X = x, Y = y, Z = z;
  double uvz[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
    uvz[j] = __builtin_fma(P[4 * j + 3], 1.0, __builtin_fma(P[4 * j + 2], Z, __builtin_fma(P[4 * j + 1], Y, P[4 * j] * X)));
  const double u = uvz[0] / uvz[2], v = uvz[1] / uvz[2];
  row = 0;
  col = 0;
  if (!(x > 0.f && u > 0.0 && v > 0.0 && u < (double)img_w && v < (double)img_h)) return false;
  row = (int)v;                      // astype(int): truncation
  col = (int)u;
  return true;
}

// The camera chain, frustum test, half-resolution pixel and top-row cut of ts_project_cam (nuscenes_ms_mm.py:349-398; the layout of
// the 57 doubles: include/taseg_hip.h).  row / col are 0 where the frustum test fails; a pixel above the cut rows fails with its
// row - crop_top < 0 left in `row`.
template <typename Ptr>
__device__ __forceinline__ bool sr_project_cam(Ptr C, float x, float y, float z, int img_w, int img_h,
                                               int crop_top, int &row, int &col) {
#pragma clang fp contract(off)
  double a[3] = {(double)x, (double)y, (double)z}, b[3];
  sr_mat3(C, a, b);
#pragma unroll
  for (int j = 0; j < 3; ++j) b[j] = b[j] + C[9 + j];
  sr_mat3(C + 12, b, a);
#pragma unroll
  for (int j = 0; j < 3; ++j) a[j] = (a[j] + C[21 + j]) - C[24 + j];
  sr_mat3(C + 27, a, b);
#pragma unroll
  for (int j = 0; j < 3; ++j) b[j] = b[j] - C[36 + j];
  sr_mat3(C + 39, b, a);
  const double depth = a[2];
  // viewpad @ (x, y, z, 1): the 4th column of the padded intrinsic is zero, fma(0, 1, acc) = acc + 0
  double q[3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
    q[j] = __builtin_fma(0.0, 1.0, __builtin_fma(C[48 + 3 * j + 2], a[2], __builtin_fma(C[48 + 3 * j + 1], a[1], C[48 + 3 * j] * a[0])));
  const float u = (float)(q[0] / q[2]), v = (float)(q[1] / q[2]);
  bool ok = depth > 0.0 && u > 0.f && u < (float)img_w && v > 0.f && v < (float)img_h;
  row = 0;
  col = 0;
  if (ok) {
    row = ((int)v) >> 1;           // astype(int), then floor(0.5 * .) written back into the integer array
    col = ((int)u) >> 1;
    ok = row >= crop_top;
    row -= crop_top;
  }
  return ok;
}

// p @ B + b of ts_fuse_sweeps (flagB; transform_point, nuscenes_ms.py:348-373): Bb = B[9] row-major, b[3]; out_j = sum_k p_k B[k][j]
// as dgemm's chain, the translation added in float64, ONE rounding to float32
template <typename Ptr>
__device__ __forceinline__ void sr_move(Ptr Bb, float (&q)[3]) {
#pragma clang fp contract(off)
  const double d0 = q[0], d1 = q[1], d2 = q[2];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double acc = __builtin_fma(d2, Bb[6 + j], __builtin_fma(d1, Bb[3 + j], d0 * Bb[j]));
    q[j] = (float)(acc + Bb[9 + j]);
  }
}

// Point augmentation (R/tools/utils/common/seg_utils.py:102-166 aug_points_ms, :43-100 aug_points) of one row by one record of
// TS_AUG_RECORD doubles:
//   { c, s, scale, tx, ty, tz, bits, flip }   bits: 1 rotate, 2 scale, 4 flip, 8 translate, 16 scale in float32 ; flip: 0 .. 3
// The reference multiplies the float32 cloud with a float64 matrix (np.dot), so everything after the rotation is float64 and the
// store into its float32 array (semantickitti_voxel_ms.py:90) is the ONE rounding; a step that is switched off is skipped, not run
// with identity values (-0.0 + 0.0 = +0.0), so a record without bits returns the input's bits.  Bit 16: without the rotation the
// cloud is still float32 when it is scaled and numpy multiplies a float32 array by a Python float IN float32 - host-side choice
// (taseg_amd/data/augment.py), the kernels only honour it.
__device__ __forceinline__ void sr_augment(const double *__restrict__ a, float &x, float &y, float &z) {
#pragma clang fp contract(off)
  const int bits = (int)a[6];
  if (!(bits & 15)) return;
  double X = x, Y = y, Z = z;
  if (bits & 1) {
    const double3 r = sr_rotate_z(X, Y, Z, a[0], a[1]);
    X = r.x;
    Y = r.y;
    Z = r.z;
  }
  if (bits & 2) {
    if (bits & 16) {
      const float sc = (float)a[2];
      X = (double)__fmul_rn((float)X, sc);
      Y = (double)__fmul_rn((float)Y, sc);
      Z = (double)__fmul_rn((float)Z, sc);
    } else {
      X *= a[2];
      Y *= a[2];
      Z *= a[2];
    }
  }
  if (bits & 4) {
    const int flip = (int)a[7];
    if (flip & 1) X = -X;
    if (flip & 2) Y = -Y;
  }
  if (bits & 8) {
    X += a[3];
    Y += a[4];
    Z += a[5];
  }
  x = (float)X;
  y = (float)Y;
  z = (float)Z;
}
