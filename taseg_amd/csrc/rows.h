// What the row kernels of csrc/cylinder.hip, csrc/spvcnn.hip, csrc/rpvnet.hip, csrc/point_tail.h and csrc/conv_pass2.hip share: 16-byte accesses per lane,
// one group of c / V lanes per row, voxel or piece, blocks of 256 threads.  Templates and inline functions only - every file that
// includes this keeps its own -ffp-contract setting (csrc/build.py).
#pragma once
#include <hip/hip_fp16.h>

#include "common.h"

namespace {

template <typename T, int V>
using ts_vec = T __attribute__((ext_vector_type(V)));

template <typename T> struct Lanes;                     // elements of one 16-byte access
template <> struct Lanes<float> { static constexpr int V = 4; };
template <> struct Lanes<_Float16> { static constexpr int V = 8; };

// the sizes every row entry point takes: n rows, m source rows, c channels in 16-byte pieces
inline int rows_check(const char *who, int64_t n, int32_t c, int64_t m, int32_t half) {
  TS_REQUIRE(n >= 0 && m >= 0 && c > 0 && n < (1LL << 30) && m < (1LL << 31) - 1, TS_ERR_INVALID_ARGUMENT, "%s: bad sizes", who);
  TS_REQUIRE(c % (half ? 8 : 4) == 0 && c <= 1024, TS_ERR_UNSUPPORTED,
             "%s: C must be a multiple of %d (16-byte pieces of a row), <= 1024", who, half ? 8 : 4);
  return TS_OK;
}

inline bool aligned16(const void *a, const void *b = nullptr, const void *c = nullptr, const void *d = nullptr) {
  return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) == 0;
}

// lane groups (rows, voxels or pieces) one block of 256 threads serves at row width c
inline int row_groups(int32_t c, int32_t half) { return 256 / (c / (half ? 8 : 4)); }

// f(T()) with T = _Float16 or float by the `half` flag of the C ABI: the one place a launch picks its element type.
//   by_half(half, [&](auto t) { using T = decltype(t); kernel<T><<<grid, 256, 0, stream>>>((const T *)x, ..., (T *)out); });
template <typename F>
inline void by_half(int32_t half, F &&f) {
  if (half) f(_Float16());
  else f(float());
}

}  // namespace
