// Pass 2 of the two-pass sparse convolution and of every class plan: out[j, :] = sum_k Z[pos[k, j], :] - a streaming reduction, for a
// fixed k the rows Z[pos[k, j]] of consecutive j are consecutive in memory.  Deterministic (fp32 additions from +0, k ascending), no
// atomics, every output row written once.  One kernel family for fp32 rows and half rows (fp32 sums, one rounding at the store):
// the bodies are written once on ts_vec<T, Lanes<T>::V> - the 16 bytes of a row a lane owns - and a ts_vec<float, V> accumulator
// (csrc/rows.h); the __global__ kernels below are wrappers that keep the names the recorded traffic tables and profiles are keyed by.
//
//   pass2_list_body<T, R>    the default: the live positions of a row compacted in LDS first, then R independent loads per round
//   pass2_regs_body<T, KT>   K position registers per lane (TASEG_GATHER_POSITIONS=1, ts_set_conv_impl(1), or outside the list range)
//   gather_sum_kernel<1, 0>  fp32 only: one element per lane, for c % 4 != 0 or operands off a 16-byte boundary
//
// Every form has the side job in front (the ordered sum of the weight-gradient partials of the launch before, common.h) and the
// addend behind the sum; the list form also takes the evaluation block's elementwise tail (TsGatherEpilogue) into its store.
// A position counts where 0 <= p < n_pairs, in both element types: a table that points outside Z skips that product instead of
// reading out of bounds (the half kernels used to test p >= 0 alone; for every valid table the bits are unchanged).
#include "rows.h"

namespace {

constexpr int PASS2_BLOCK = 256;   // threads of every workgroup of pass 2 (rows.h, row_groups: lane groups of a block of 256)

template <typename T, int V>
__device__ __forceinline__ void pass2_add(ts_vec<float, V> &acc, const ts_vec<T, V> &v) {
#pragma unroll
  for (int q = 0; q < V; ++q) acc[q] += (float)v[q];
}

template <typename T, int V>
__device__ __forceinline__ void pass2_store(T *p, const ts_vec<float, V> &acc) {
  ts_vec<T, V> o;
#pragma unroll
  for (int q = 0; q < V; ++q) o[q] = (T)acc[q];
  *(ts_vec<T, V> *)p = o;
}

// V per-channel values of the tail.  fp32 rows: one 16-byte read (the tail's eligibility demands the alignment, pass2_tail_aligned);
// half rows: eight elements of four fp32 vectors are two 16-byte reads each, read per element - no alignment demanded
template <int V>
__device__ __forceinline__ ts_vec<float, V> pass2_channels(const float *__restrict__ p) {
  if constexpr (V == 4) {
    return *(const ts_vec<float, 4> *)p;
  } else {
    ts_vec<float, V> v;
#pragma unroll
    for (int q = 0; q < V; ++q) v[q] = p[q];
    return v;
  }
}

// KT > 0: kernel volume known at compile time (27, 8): all K position loads are issued first, then all row
// loads - up to K independent 16-byte loads in flight per lane.  KT == 0: generic loop.
// every Z row is read exactly once: non-temporal loads keep it out of the way of the position table and of the next
// kernel's operands in L2 (step 19.33 -> 19.10 ms)
template <typename T, int KT>
__device__ __forceinline__ void pass2_regs_body(const T *__restrict__ Z, int C, const int *__restrict__ pos, int K, int64_t n,
                                                int64_t n_pairs, T *__restrict__ out, const TsWgradReduce &side,
                                                const T *__restrict__ addend) {
  constexpr int V = Lanes<T>::V;
  using VT = ts_vec<T, V>;
  const int cv = C / V;
  const int64_t total = n * cv;
  int64_t e = (int64_t)blockIdx.x * PASS2_BLOCK + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * PASS2_BLOCK;
  // side job (common.h): the ordered sum of the weight-gradient partials of the launch before this one
  for (int64_t i = e; i < (int64_t)side.K * side.cacb4; i += step) ts_wgrad_reduce_one(side, i);
  for (; e < total; e += step) {
    const int64_t j = e / cv;
    const int c = (int)(e - j * cv) * V;
    ts_vec<float, V> acc = {};
    if constexpr (KT > 0) {
      int p[KT];
#pragma unroll
      for (int k = 0; k < KT; ++k) p[k] = pos[(int64_t)k * n + j];
      VT f[KT];
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        f[k] = VT{};
        if (p[k] >= 0 && p[k] < n_pairs) f[k] = __builtin_nontemporal_load((const VT *)(Z + (int64_t)p[k] * C + c));
      }
#pragma unroll
      for (int k = 0; k < KT; ++k) pass2_add<T, V>(acc, f[k]);   // k ascending: fixed summation order
    } else {
#pragma unroll 4
      for (int k = 0; k < K; ++k) {
        const int p = pos[(int64_t)k * n + j];
        if (p >= 0 && p < n_pairs) pass2_add<T, V>(acc, *(const VT *)(Z + (int64_t)p * C + c));
      }
    }
    // one add per element after the sum over the offsets: the same bits as a separate a + b
    if (addend) pass2_add<T, V>(acc, *(const VT *)(addend + j * C + c));
    pass2_store<T, V>(out + j * C + c, acc);
  }
}

// Pass 2 with the live positions of a row compacted in LDS first: a workgroup owns rpw = 256 / (C / V) whole rows; half-waves
// load the K positions of a row (lane = offset), ballot the live ones and leave them - ascending offset, the fixed
// summation order - as a list in LDS; then a lane walks its row's list with R independent 16-byte loads per round.
// Against pass2_regs_body<T, K>: one position load per lane instead of K, only live rows requested, R + a few instead
// of 5 K registers (8 instead of 3 waves per SIMD).  Same additions in the same order: bit-identical sums.  K <= 32.
template <typename T, int R>
__device__ __forceinline__ void pass2_list_body(const T *__restrict__ Z, int C, const int *__restrict__ pos, int K, int64_t n,
                                                int64_t n_pairs, T *__restrict__ out, const TsWgradReduce &side,
                                                const T *__restrict__ addend, int rpw, const TsGatherEpilogue &epi) {
  constexpr int V = Lanes<T>::V;
  using VT = ts_vec<T, V>;
  __shared__ int lst[64][33];
  __shared__ int cnt[64];
  const int tid = threadIdx.x;
  {
    const int64_t e = (int64_t)blockIdx.x * PASS2_BLOCK + tid, step = (int64_t)gridDim.x * PASS2_BLOCK;
    for (int64_t i = e; i < (int64_t)side.K * side.cacb4; i += step) ts_wgrad_reduce_one(side, i);
  }
  const int64_t j0 = (int64_t)blockIdx.x * rpw;
  const int hw = tid >> 5, l = tid & 31;
  for (int base = 0; base < rpw; base += 8) {          // uniform trip count: the ballot below needs every lane
    const int r = base + hw;
    const int64_t j = j0 + r;
    int p = -1;
    if (r < rpw && j < n && l < K) p = pos[(int64_t)l * n + j];
    const bool live = p >= 0 && p < n_pairs;
    const unsigned long long m64 = __builtin_amdgcn_ballot_w64(live);
    const unsigned m = (tid & 32) ? (unsigned)(m64 >> 32) : (unsigned)m64;
    if (live) lst[r][__builtin_popcount(m & ((1u << l) - 1u))] = p;
    if (l == 0 && r < rpw) cnt[r] = __builtin_popcount(m);
  }
  __syncthreads();
  const int cv = C / V;
  const int r = tid / cv;
  const int64_t j = j0 + r;
  if (r >= rpw || j >= n) return;
  const int c = (tid - r * cv) * V;
  const int m = cnt[r];
  ts_vec<float, V> acc = {};
  for (int b = 0; b < m; b += R) {
    VT f[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      f[i] = VT{};
      if (b + i < m) f[i] = __builtin_nontemporal_load((const VT *)(Z + (int64_t)lst[r][b + i] * C + c));
    }
#pragma unroll
    for (int i = 0; i < R; ++i) pass2_add<T, V>(acc, f[i]);
  }
  if (addend) pass2_add<T, V>(acc, *(const VT *)(addend + j * C + c));
  if (epi.mean) {                        // evaluation block: bn_act_fwd_kernel's arithmetic on the fp32 sum
    const ts_vec<float, V> mu = pass2_channels<V>(epi.mean + c), s = pass2_channels<V>(epi.invstd + c);
    const ts_vec<float, V> ww = pass2_channels<V>(epi.w + c), bb = pass2_channels<V>(epi.b + c);
    VT res = {};
    if (epi.residual) res = *(const VT *)((const T *)epi.residual + j * C + c);
#pragma unroll
    for (int q = 0; q < V; ++q) {
      float v = (acc[q] - mu[q]) * s[q] * ww[q] + bb[q];
      if (epi.residual) v += (float)res[q];
      if (epi.relu) v = fmaxf(v, 0.f);
      acc[q] = v;
    }
  }
  pass2_store<T, V>(out + j * C + c, acc);
}

}  // namespace

template <int R>
__global__ __launch_bounds__(PASS2_BLOCK) void gather_list_kernel(const float *__restrict__ Z, int C, const int *__restrict__ pos, int K,
                                                          int64_t n, int64_t n_pairs, float *__restrict__ out, TsWgradReduce side,
                                                          const float *__restrict__ addend, int rpw, TsGatherEpilogue epi) {
  pass2_list_body<float, R>(Z, C, pos, K, n, n_pairs, out, side, addend, rpw, epi);
}

template <int R>
__global__ __launch_bounds__(PASS2_BLOCK) void gather_list_h_kernel(const _Float16 *__restrict__ Z, int C, const int *__restrict__ pos, int K,
                                                            int64_t n, int64_t n_pairs, _Float16 *__restrict__ out, TsWgradReduce side,
                                                            const _Float16 *__restrict__ addend, int rpw, TsGatherEpilogue epi) {
  pass2_list_body<_Float16, R>(Z, C, pos, K, n, n_pairs, out, side, addend, rpw, epi);
}

template <int KT>
__global__ __launch_bounds__(PASS2_BLOCK) void gather_sum_h_kernel(const _Float16 *__restrict__ Z, int C, const int *__restrict__ pos, int K,
                                                           int64_t n, int64_t n_pairs, _Float16 *__restrict__ out, TsWgradReduce side,
                                                           const _Float16 *__restrict__ addend) {
  pass2_regs_body<_Float16, KT>(Z, C, pos, K, n, n_pairs, out, side, addend);
}

// VEC == 4: the register form on fp32 rows.  VEC == 1 (KT == 0): one element per lane, any c and any alignment; fp32 only
template <int VEC, int KT>
__global__ __launch_bounds__(PASS2_BLOCK) void gather_sum_kernel(const float *__restrict__ Z, int C, const int *__restrict__ pos, int K,
                                                         int64_t n, int64_t n_pairs, float *__restrict__ out, TsWgradReduce side,
                                                         const float *__restrict__ addend) {
  if constexpr (VEC == 4) {
    pass2_regs_body<float, KT>(Z, C, pos, K, n, n_pairs, out, side, addend);
  } else {
    const int64_t total = n * C;
    int64_t e = (int64_t)blockIdx.x * PASS2_BLOCK + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * PASS2_BLOCK;
    for (int64_t i = e; i < (int64_t)side.K * side.cacb4; i += step) ts_wgrad_reduce_one(side, i);
    for (; e < total; e += step) {
      const int64_t j = e / C;
      const int c = (int)(e - j * C);
      float acc = 0.f;
#pragma unroll 4
      for (int k = 0; k < K; ++k) {
        const int p = pos[(int64_t)k * n + j];
        if (p >= 0 && p < n_pairs) acc += Z[(int64_t)p * C + c];
      }
      if (addend) acc += addend[j * C + c];
      out[j * C + c] = acc;
    }
  }
}

namespace {

// ---- which form runs: the one statement of the rules (backend.gather_sum_kernel_name mirrors it for the profiles)
template <typename T> struct Pass2;
template <> struct Pass2<float> {
  static constexpr int list_c_min = 16, list_c_max = 1024;
  template <int R> static auto list() { return gather_list_kernel<R>; }
  template <int KT> static auto regs() { return gather_sum_kernel<4, KT>; }
  // the tail reads its four per-channel vectors and the residual in 16-byte pieces
  static bool tail_aligned(const TsGatherEpilogue &e) { return aligned16(e.mean, e.invstd, e.w, e.b) && aligned16(e.residual); }
};
template <> struct Pass2<_Float16> {
  static constexpr int list_c_min = 64, list_c_max = 2048;   // 32 channels: 64 rows per workgroup, the list build costs more than it saves
  template <int R> static auto list() { return gather_list_h_kernel<R>; }
  template <int KT> static auto regs() { return gather_sum_h_kernel<KT>; }
  static bool tail_aligned(const TsGatherEpilogue &e) { return aligned16(e.residual); }   // the vectors are read per element
};

// rows in 16-byte pieces: both vector forms need it (half rows: the entry point demands it; fp32 rows: else the scalar form)
template <typename T>
bool pass2_vector(int c, const void *z, const void *out) { return c % Lanes<T>::V == 0 && aligned16(z, out); }

// the list form is the default: live positions compacted in LDS first; TASEG_GATHER_POSITIONS=1 in the environment
// keeps the K-register form (A/B runs), ts_set_conv_impl(1) too
template <typename T>
bool pass2_list_applies(int c, int K, const void *z, const void *out) {
  return pass2_vector<T>(c, z, out) && K <= 32 && c >= Pass2<T>::list_c_min && c <= Pass2<T>::list_c_max &&
         ts_get_option(TS_OPT_GATHER_POSITIONS) == 0 && g_ts_conv_impl != 1;
}

template <typename T>
int pass2_launch(const T *z, int c, const int *pos, int K, int64_t n_rows, int64_t n_pairs, T *out, const TsWgradReduce &side,
                 const T *addend, const TsGatherEpilogue *epi, hipStream_t stream) {
  constexpr int V = Lanes<T>::V;
  constexpr bool half = V == 8;
  // the tail rides on the list form alone; everything else is reported as "run the two launches"
  const bool list = pass2_list_applies<T>(c, K, z, out);
  if (epi && !(list && Pass2<T>::tail_aligned(*epi))) return TS_ERR_UNSUPPORTED;
  if (list) {
    const int rpw = row_groups(c, half);
    // R = 4 / 8 / 12 / 16 measured within 3 % of each other on every layer (profiles/r02_v9_gather_forms_probe.txt)
    Pass2<T>::template list<8>()<<<(unsigned)ts_cdiv(n_rows, rpw), PASS2_BLOCK, 0, stream>>>(z, c, pos, K, n_rows, n_pairs, out, side, addend, rpw,
                                                                                    epi ? *epi : TsGatherEpilogue{});
    TS_CHECK_LAUNCH(half ? "ts_conv_gather_sum_f16 (list)" : "conv_gather_sum (list)");
    return TS_OK;
  }
  if (pass2_vector<T>(c, z, out)) {
    const int grid = (int)std::min<int64_t>(ts_cdiv(n_rows * (c / V), PASS2_BLOCK), 1 << 20);
    auto kernel = K == 27 ? Pass2<T>::template regs<27>() : K == 8 ? Pass2<T>::template regs<8>() : Pass2<T>::template regs<0>();
    kernel<<<grid, PASS2_BLOCK, 0, stream>>>(z, c, pos, K, n_rows, n_pairs, out, side, addend);
  } else if constexpr (!half) {
    const int grid = (int)std::min<int64_t>(ts_cdiv(n_rows * c, PASS2_BLOCK), 1 << 20);
    gather_sum_kernel<1, 0><<<grid, PASS2_BLOCK, 0, stream>>>(z, c, pos, K, n_rows, n_pairs, out, side, addend);
  }
  TS_CHECK_LAUNCH(half ? "ts_conv_gather_sum_f16" : "conv_gather_sum");
  return TS_OK;
}

}  // namespace

int ts_conv_pass2(int32_t half, const void *z, int32_t c, const int32_t *pos, int32_t K, int64_t n_rows, int64_t n_pairs, void *out,
                  const TsWgradReduce *side_job, const void *addend, const TsGatherEpilogue *epi, ts_stream_t stream) {
  const char *who = half ? "ts_conv_gather_sum_f16" : "ts_conv_gather_sum";
  TsWgradReduce side = {};
  if (epi) {                               // no error text on this path: the caller falls back to the call without the tail
    if (!(K > 0 && n_rows > 0 && z && pos && out && !side_job && !addend && epi->mean && epi->invstd && epi->w && epi->b))
      return TS_ERR_UNSUPPORTED;
  } else {
    if (side_job) side = *side_job;
    TS_REQUIRE(!side_job || (n_rows > 0 && side.part && side.dW && side.nboffs && side.chunk > 0 && aligned16(side.part, side.dW)),
               TS_ERR_INVALID_ARGUMENT, "%s: bad side job", who);
    TS_REQUIRE(c > 0 && (!half || (c & 7) == 0) && K > 0 && n_rows >= 0 && n_pairs >= 0, TS_ERR_INVALID_ARGUMENT, "%s: bad sizes%s", who,
               half ? " (C must be a multiple of 8)" : "");
    if (n_rows == 0) return TS_OK;
    TS_REQUIRE(pos && out && (z || n_pairs == 0), TS_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    // fp32 rows off a 16-byte boundary take the scalar form; half rows have none
    TS_REQUIRE(!half || aligned16(z, out), TS_ERR_INVALID_ARGUMENT, "%s: pointers must be 16-byte aligned", who);
  }
  int rc = TS_OK;
  by_half(half, [&](auto t) {
    using T = decltype(t);
    rc = pass2_launch<T>((const T *)z, c, pos, K, n_rows, n_pairs, (T *)out, side, (const T *)addend, epi, (hipStream_t)stream);
  });
  return rc;
}

extern "C" int ts_conv_gather_sum(const float *z, int32_t c, const int32_t *pos, int32_t K, int64_t n_rows, int64_t n_pairs,
                                  float *out, ts_stream_t stream) {
  return ts_conv_pass2(0, z, c, pos, K, n_rows, n_pairs, out, nullptr, nullptr, nullptr, stream);
}

extern "C" int ts_conv_gather_sum_f16(const void *z, int32_t c, const int32_t *pos, int32_t K, int64_t n_rows, int64_t n_pairs,
                                      void *out, ts_stream_t stream) {
  return ts_conv_pass2(1, z, c, pos, K, n_rows, n_pairs, out, nullptr, nullptr, nullptr, stream);
}
