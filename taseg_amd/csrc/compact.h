// Stable compaction of rows in blocks of 256 (library-internal): the pieces every kernel family of the data stage builds its
// three passes from.
//   1  count    one lane per row: the kept rows per block (cp_ballot, cp_block_sum) and, where the caller reports per-sample
//               counts, the kept rows per (tally, block) (cp_tally_*)
//   2  scan     ts_compact_scan (csrc/compact.hip): exclusive scan of every cloud's block counts, every tally summed over the blocks
//   3  scatter  the decision of pass 1 recomputed on the same bits, destination = block offset + rank inside the block (cp_rank)
// Order is decided by counts and ranks alone - no atomics - so the rows keep their input order and the bits are the same every run.
// A family with one cloud and one tally per sample does not write the passes out: it gives a rule to cp_compact (below).
#pragma once
#include "common.h"

#define CP_ROWS 256
#define CP_WAVES (CP_ROWS / TS_WAVE)

struct CpBallot {
  unsigned long long mask;               // the wave's lanes that keep their row
  int lane, wave;
};

// Every thread of the block calls it; lane 0 of every wave stores the wave's count into the caller's wcnt[CP_WAVES].
__device__ __forceinline__ CpBallot cp_ballot(bool keep, int *wcnt) {
  CpBallot b;
  b.lane = threadIdx.x & (TS_WAVE - 1);
  b.wave = threadIdx.x / TS_WAVE;
  b.mask = __ballot(keep);
  if (b.lane == 0) wcnt[b.wave] = __popcll(b.mask);
  return b;
}

// After the caller's __syncthreads(): the rank of a kept lane among the kept rows of the block.
__device__ __forceinline__ int cp_rank(const CpBallot &b, const int *wcnt) {
  int r = __popcll(b.mask & ((1ull << b.lane) - 1ull));
  for (int v = 0; v < b.wave; ++v) r += wcnt[v];
  return r;
}

// After the caller's __syncthreads(): the kept rows of the block.
__device__ __forceinline__ int cp_block_sum(const int *wcnt) {
  int c = 0;
  for (int v = 0; v < CP_WAVES; ++v) c += wcnt[v];
  return c;
}

// Per-sample tallies of a block, K counters per sample, in the caller's scnt[CP_WAVES][K * TS_WAVE] (at most TS_WAVE samples;
// tally j = K * sample + counter).  cp_tally_clear, __syncthreads(), cp_tally_wave, __syncthreads(), cp_tally_store.
template <int K>
__device__ __forceinline__ void cp_tally_clear(int (*scnt)[K * TS_WAVE]) {
  for (int k = 0; k < K; ++k) scnt[threadIdx.x / TS_WAVE][K * (threadIdx.x & (TS_WAVE - 1)) + k] = 0;   // every wave its own row
}

// hit[k]: this lane's row counts for counter k; a lane with a hit carries its sample s in [0, TS_WAVE).  The samples ascend: a
// wave holds one sample, or a few at a boundary - one round per distinct sample (rem is wave-uniform).
template <int K>
__device__ __forceinline__ void cp_tally_wave(int s, const bool (&hit)[K], int (*scnt)[K * TS_WAVE]) {
  const int lane = threadIdx.x & (TS_WAVE - 1), w = threadIdx.x / TS_WAVE;
  bool any = false;
  for (int k = 0; k < K; ++k) any = any || hit[k];
  unsigned long long rem = __ballot(any);
  while (rem) {
    const int s0 = __shfl(s, __ffsll((long long)rem) - 1);
    const bool mine = any && s == s0;
    for (int k = 0; k < K; ++k) {
      const int c = __popcll(__ballot(mine && hit[k]));
      if (lane == 0) scnt[w][K * s0 + k] += c;
    }
    rem &= ~__ballot(mine);
  }
}

// blk_tally [n_tallies][gridDim.x]: count-major, the scan's waves read along a row
template <int K>
__device__ __forceinline__ void cp_tally_store(const int (*scnt)[K * TS_WAVE], int n_tallies, int *__restrict__ blk_tally) {
  if ((int)threadIdx.x >= n_tallies) return;
  int c = 0;
  for (int v = 0; v < CP_WAVES; ++v) c += scnt[v][threadIdx.x];
  blk_tally[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = c;
}

// One step of a scan that a single wave walks TS_WAVE values at a time: the inclusive sums of v over the lanes up to this one.
__device__ __forceinline__ int cp_wave_inclusive(int v, int lane) {
  for (int d = 1; d < TS_WAVE; d <<= 1) {
    const int t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  return v;
}

// blk_cnt, offs [n_clouds][n_blocks]; blk_tally [n_tallies][n_blocks]
struct CpWorkspace {
  int *blk_cnt, *offs, *blk_tally;
  size_t bytes;
};

static inline CpWorkspace cp_carve(void *ws, int64_t n_blocks, int64_t n_clouds, int64_t n_tallies) {
  CpWorkspace c;
  size_t at = 0;
  char *base = (char *)ws;
  c.blk_cnt = (int *)(base + at);
  at += ts_align_up((size_t)n_clouds * n_blocks * sizeof(int), 256);
  c.offs = (int *)(base + at);
  at += ts_align_up((size_t)n_clouds * n_blocks * sizeof(int), 256);
  c.blk_tally = (int *)(base + at);
  at += ts_align_up((size_t)n_tallies * n_blocks * sizeof(int), 256);
  c.bytes = std::max<size_t>(at, 256);
  return c;
}

// Pass 2, one launch (also for n_blocks == 0): c.offs = the exclusive scans of c.blk_cnt, counts[j] = tally j summed over the blocks
// (n < 2^30 rows in all).  The caller checks the launch.
void ts_compact_scan(const CpWorkspace &c, int n_blocks, int n_clouds, int n_tallies, int64_t *counts, hipStream_t stream);

// ---------------------------------------------------------------------------------------------------- one cloud, one tally per sample
// The three passes as something to call: a rule struct (in the caller's anonymous namespace, so that every file gets kernels of
// its own) derives from CpRule, travels to both kernels by value and gives
//   Row                              what pass 3 needs of a kept row
//   keeps(i, in, Row &, int *sample) does row i survive?  EVERY lane of the block calls it (a rule may vote across the wave); `in`:
//                                    the lane has a row.  *sample = the row's sample in [0, n_samples), -1 without a row.  Both
//                                    passes call it, so pass 3 decides on the bits pass 1 counted.
//   store(dst, i, row)               writes survivor i as output row dst, 0 <= dst < capacity
struct CpRule {
  int64_t n_rows, capacity;        // capacity >= n_rows: the rows every output holds
  int n_samples;                   // <= TS_WAVE
  int64_t *out_sample;             // [capacity] the survivors' samples, twice: int64 for indexing ...
  int *out_sample32;               // ... int32 for the next kernel
};

template <typename Rule>
__global__ __launch_bounds__(CP_ROWS) void cp_count_kernel(Rule r, int *__restrict__ blk_cnt, int *__restrict__ blk_tally) {
  __shared__ int wcnt[CP_WAVES];
  __shared__ int scnt[CP_WAVES][TS_WAVE];
  const int64_t i = (int64_t)blockIdx.x * CP_ROWS + threadIdx.x;
  cp_tally_clear<1>(scnt);
  __syncthreads();
  int s;
  typename Rule::Row row;
  bool keep[1];
  keep[0] = r.keeps(i, i < r.n_rows, row, &s);
  cp_ballot(keep[0], wcnt);
  cp_tally_wave<1>(s, keep, scnt);
  __syncthreads();
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = cp_block_sum(wcnt);
  cp_tally_store<1>(scnt, r.n_samples, blk_tally);
}

template <typename Rule>
__global__ __launch_bounds__(CP_ROWS) void cp_scatter_kernel(Rule r, const int *__restrict__ offs) {
  __shared__ int wcnt[CP_WAVES];
  const int64_t i = (int64_t)blockIdx.x * CP_ROWS + threadIdx.x;
  int s;
  typename Rule::Row row;
  const bool keep = r.keeps(i, i < r.n_rows, row, &s);
  const CpBallot b = cp_ballot(keep, wcnt);
  __syncthreads();
  if (!keep) return;
  const int64_t dst = offs[blockIdx.x] + cp_rank(b, wcnt);
  if (dst < 0 || dst >= r.capacity) return;       // (cannot happen: survivors <= rows <= capacity; bounds every store)
  r.store(dst, i, row);
  r.out_sample[dst] = s;
  r.out_sample32[dst] = s;
}

static inline size_t cp_compact_bytes(int64_t n_rows, int n_samples) {
  return cp_carve(nullptr, ts_cdiv(std::max<int64_t>(n_rows, 0), CP_ROWS), 1, std::max(n_samples, 0)).bytes;
}

static inline int cp_launched(const char *name, const char *pass) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return TS_OK;
  ts_set_error("%s (%s): launch failed: %s", name, pass, hipGetErrorString(e));
  return TS_ERR_LAUNCH_FAILED;
}

// The caller has checked its arguments (0 <= n_rows < 2^30, capacity >= n_rows, 1 <= n_samples <= TS_WAVE, ws 4-byte aligned);
// the workspace size is the last check before the first launch.  Without rows the scan still runs: it writes the counts.
template <typename Rule>
static int cp_compact(const Rule &r, const char *name, int64_t *counts, void *ws, size_t ws_bytes, hipStream_t st) {
  const int64_t n_blocks = ts_cdiv(r.n_rows, CP_ROWS);
  const CpWorkspace c = cp_carve(ws, n_blocks, 1, r.n_samples);
  TS_REQUIRE(ws_bytes >= c.bytes, TS_ERR_INVALID_ARGUMENT, "%s: workspace too small", name);
  int rc = TS_OK;
  if (n_blocks > 0) {
    cp_count_kernel<Rule><<<(int)n_blocks, CP_ROWS, 0, st>>>(r, c.blk_cnt, c.blk_tally);
    if ((rc = cp_launched(name, "count")) != TS_OK) return rc;
  }
  ts_compact_scan(c, (int)n_blocks, 1, r.n_samples, counts, st);
  if ((rc = cp_launched(name, "scan")) != TS_OK) return rc;
  if (n_blocks > 0) {
    cp_scatter_kernel<Rule><<<(int)n_blocks, CP_ROWS, 0, st>>>(r, c.offs);
    rc = cp_launched(name, "scatter");
  }
  return rc;
}
