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
