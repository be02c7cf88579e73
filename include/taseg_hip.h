/*
 * taseg_hip.h — C ABI of libtaseg_hip.so, the MI355X (gfx950) backend for the
 * TASeg / OpenPCSeg sparse-convolution hot path.
 *
 * Every entry point below replaces one function of the reference's native
 * backend (the pybind module `torchsparse.backend`, mit-han-lab/torchsparse
 * v1.4.0 vendored at /root/reference/package/torchsparse.zip; paths below are
 * relative to the zip member `torchsparse/`) or one tensor-op sequence of its
 * Python rulebook construction.  The reference interface each one replaces is
 * cited as file:line.
 *
 * Conventions
 *   - plain C: device pointers + sizes, no torch / ATen types;
 *   - all pointers are DEVICE pointers unless the name ends in `_host`;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *     nothing here synchronises the host, allocates or frees device memory:
 *     scratch comes in through (`ws`, `ws_bytes`), sized by the matching
 *     `*_workspace_bytes()` query;
 *   - return value: TS_OK (0) or a negative TS_ERR_* code; ts_last_error()
 *     returns a thread-local message for the last failure (the reference
 *     throws std::invalid_argument, e.g. convolution_cuda.cu:57-59);
 *   - coordinates are int32 [N,4] rows (x, y, z, batch)  (utils/collate.py:26-31);
 *   - features are row-major float32 [N, C].
 */
#ifndef TASEG_HIP_H_
#define TASEG_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TS_OK 0
#define TS_ERR_INVALID_ARGUMENT (-1)
#define TS_ERR_WORKSPACE_TOO_SMALL (-2)
#define TS_ERR_LAUNCH_FAILED (-3)
#define TS_ERR_UNSUPPORTED (-4)

typedef void *ts_stream_t;

/* Library identity: "taseg_hip <version> gfx950". */
const char *ts_version(void);
/* Thread-local message describing the last non-TS_OK return. */
const char *ts_last_error(void);

/* Tuning values of the library (process-wide; the host side's options object - taseg_amd/options.py - pushes its fields when it
 * loads the library; the library itself reads no environment variable).  0 is every key's default.
 *   TS_OPT_GATHER_POSITIONS        != 0: pass 2 with K position registers per lane instead of LDS lists
 *   TS_OPT_WGRAD_WGS               workgroup target of the weight gradient's chunking (64 .. 8192; 0 = 512)
 *   TS_OPT_EVAL_TAIL_SEPARATE      != 0: the evaluation block's BatchNorm tail as a launch of its own
 *   TS_OPT_CLASS_FINISH_ROWS[_HALF] rows from which a class plan's finish runs inside the product (0 = never)
 *   TS_OPT_DEBUG_BN_ABLATE         timing diagnostics of csrc/bn.hip (bit field)
 *   TS_OPT_KMAP_FULL_PROBE         != 0: submanifold kernel maps on all 27 probes
 * ts_set_option returns TS_ERR_INVALID_ARGUMENT for an unknown key. */
enum {
  TS_OPT_GATHER_POSITIONS = 0,
  TS_OPT_WGRAD_WGS = 1,
  TS_OPT_EVAL_TAIL_SEPARATE = 2,
  TS_OPT_CLASS_FINISH_ROWS = 3,
  TS_OPT_CLASS_FINISH_ROWS_HALF = 4,
  TS_OPT_DEBUG_BN_ABLATE = 5,
  TS_OPT_KMAP_FULL_PROBE = 6,
  TS_OPT_COUNT = 7
};
int ts_set_option(int32_t key, int64_t value);
int64_t ts_get_option(int32_t key);

/* ------------------------------------------------------------------------ */
/* 1. The ten entry points of torchsparse.backend                           */
/*    (backend/pybind_cuda.cpp:18-39)                                       */
/* ------------------------------------------------------------------------ */

/* hash_cuda (backend/hash/hash_cuda.cu:10-23,67-73):
 * out[i] = fold60(FNV-1a-64 over (uint32)x,y,z,b).  coords [n,4], out [n]. */
int ts_hash(const int32_t *coords, int64_t n, int64_t *out, ts_stream_t stream);

/* kernel_hash_cuda (backend/hash/hash_cuda.cu:27-55,75-84):
 * out[k*n + i] = hash(x+ox[k], y+oy[k], z+oz[k], b).  offsets [K,3], out [K,n].
 * The row's own batch index is used (CUDA semantics, hash_cuda.cu:46), not
 * row 0's as in the CPU twin (hash_cpu.cpp:29). */
int ts_kernel_hash(const int32_t *coords, int64_t n, const int32_t *offsets,
                   int32_t n_offsets, int64_t *out, ts_stream_t stream);

/* hash_query_cuda (backend/others/query_cuda.cu:9-56):
 * out[q] = ref_idx[j] + 1 where ref_hash[j] == query[q], else 0.
 * ref_idx == NULL means arange(n_ref) (nn/functional/query.py:18-20).
 * Duplicate reference keys resolve to the smallest j (the CPU twin's
 * dense_hash_map::insert keeps the first, others/query_cpu.cpp:20-24).
 * Keys must not be -1 (reserved as the empty slot). */
size_t ts_hash_query_workspace_bytes(int64_t n_ref);
int ts_hash_query(const int64_t *query, int64_t n_query, const int64_t *ref_hash,
                  const int64_t *ref_idx, int64_t n_ref, int64_t *out, void *ws,
                  size_t ws_bytes, ts_stream_t stream);

/* count_cuda (backend/others/count_cuda.cu:10-31):
 * out[idx[i]]++ for idx[i] >= 0; out [n_out] is zeroed here first. */
int ts_count(const int32_t *idx, int64_t n, int32_t *out, int64_t n_out,
             ts_stream_t stream);

/* voxelize_forward_cuda (backend/voxelize/voxelize_cuda.cu:12-25,43-60):
 * out[idx[i], :] += feat[i, :] / counts[idx[i]]; out [m,c] is zeroed here. */
int ts_voxelize_forward(const float *feat, const int32_t *idx, const int32_t *counts,
                        int64_t n, int32_t c, int64_t m, float *out,
                        ts_stream_t stream);
/* voxelize_backward_cuda (voxelize_cuda.cu:28-41,62-80):
 * grad_feat[i, :] = grad_out[idx[i], :] / counts[idx[i]] (0 for skipped rows). */
int ts_voxelize_backward(const float *grad_out, const int32_t *idx,
                         const int32_t *counts, int64_t n, int32_t c, int64_t m,
                         float *grad_feat, ts_stream_t stream);

/* devoxelize_forward_cuda (backend/devoxelize/devoxelize_cuda.cu:11-33,61-78):
 * out[i,:] = sum_{k<8} w[i,k] * feat[idx[i,k],:]  (idx<0 contributes 0). */
int ts_devoxelize_forward(const float *feat, const int32_t *idx, const float *weight,
                          int64_t n, int32_t c, int64_t m, float *out,
                          ts_stream_t stream);
/* devoxelize_backward_cuda (devoxelize_cuda.cu:37-57,82-98): the exact adjoint,
 * grad_feat[idx[i,k],:] += w[i,k] * grad_out[i,:]; grad_feat [m,c] zeroed here. */
int ts_devoxelize_backward(const float *grad_out, const int32_t *idx,
                           const float *weight, int64_t n, int32_t c, int64_t m,
                           float *grad_feat, ts_stream_t stream);

/* convolution_forward_cuda (backend/convolution/convolution_cuda.cu:53-165):
 * out[o,:] = sum_k sum_{(i,o) in map_k} in[i,:] @ kernel[k]   (out is overwritten).
 * nbmap [P,2] int32 rows (in_idx, out_idx) grouped by offset k in order;
 * nbsizes_host [K] int32 on the HOST, exactly as the reference passes it
 * (nn/functional/conv.py:56).  transpose swaps the two map columns
 * (convolution_cuda.cu:21,34).  kernel is [K, c_in, c_out]. */
size_t ts_convolution_workspace_bytes(int64_t n_in, int64_t n_out, int32_t c_in,
                                      int32_t c_out, int32_t kernel_volume);
int ts_convolution_forward(const float *in_feat, int64_t n_in, int32_t c_in,
                           float *out_feat, int64_t n_out, int32_t c_out,
                           const float *kernel, int32_t kernel_volume,
                           const int32_t *nbmap, const int32_t *nbsizes_host,
                           int32_t transpose, void *ws, size_t ws_bytes,
                           ts_stream_t stream);
/* convolution_backward_cuda (convolution_cuda.cu:167-278):
 * grad_in = adjoint wrt in_feat, grad_kernel[k] = gather(in)^T @ gather(grad_out);
 * both outputs are overwritten.  grad_in may be NULL (input needs no grad). */
int ts_convolution_backward(const float *in_feat, int64_t n_in, int32_t c_in,
                            float *grad_in, const float *grad_out, int64_t n_out,
                            int32_t c_out, const float *kernel, float *grad_kernel,
                            int32_t kernel_volume, const int32_t *nbmap,
                            const int32_t *nbsizes_host, int32_t transpose, void *ws,
                            size_t ws_bytes, ts_stream_t stream);

/* ------------------------------------------------------------------------ */
/* 2. Rulebook construction (replaces the Python tensor-op sequences)        */
/* ------------------------------------------------------------------------ */

/* spdownsample (nn/functional/downsample.py:25-51), the branch taken when
 * stride[k] in {1, kernel_size[k]}:  c' = trunc(c / s) * s per axis, then the
 * unique rows in lexicographic (b, x, y, z) order (torch.unique(dim=0) of the
 * [b,x,y,z] permutation), returned as (x, y, z, b).
 * out_coords has room for n rows; *out_count (device int32) gets the number
 * of unique rows.  Supported range: 0 <= b < 1024, -2^17 <= x,y,z < 2^17
 * (checked on device; *out_count = -1 on violation). */
size_t ts_downsample_workspace_bytes(int64_t n);
int ts_downsample(const int32_t *coords, int64_t n, int32_t sx, int32_t sy, int32_t sz,
                  int32_t *out_coords, int32_t *out_count, void *ws, size_t ws_bytes,
                  ts_stream_t stream);

/* spdownsample (nn/functional/downsample.py:32-51), the OVERLAPPING-WINDOW branch
 * taken when some stride[k] is neither 1 nor kernel_size[k]: every row proposes
 * row + offset for the offsets of get_kernel_offsets(kernel_size, tensor_stride)
 * (nn/utils/kernel.py:19-20: arange(-k // 2 + 1, k // 2 + 1) * tensor_stride per
 * axis); a candidate is kept if on every axis it is a multiple of
 * stride * tensor_stride (:42) and not below the minimum of that axis over ALL
 * n rows, whatever their batch index (:34, :43); no upper bound (the TODO of :41
 * is reproduced).  Result: the unique kept rows in (b, x, y, z) order as
 * (x, y, z, b), like ts_downsample.
 * A row keeps at most cap = prod_a ceil(k_a / s_a) candidates and the result can
 * have MORE rows than the input: out_coords has room for cap * n rows.
 * Kernel sizes 1..5 and strides >= 1 per axis, cap * n < 2^31
 * (TS_ERR_INVALID_ARGUMENT otherwise).  *out_count and the coordinate range are
 * ts_downsample's (-1: a kept candidate outside the range; the far corner
 * (2^17 - 1, 2^17 - 1, 2^17 - 1) of batch 1023, whose key pads the unused slots,
 * counts as outside). */
size_t ts_downsample_windows_workspace_bytes(int64_t n, int32_t kx, int32_t ky, int32_t kz,
                                             int32_t sx, int32_t sy, int32_t sz);
int ts_downsample_windows(const int32_t *coords, int64_t n, int32_t kx, int32_t ky, int32_t kz,
                          int32_t sx, int32_t sy, int32_t sz, int32_t tx, int32_t ty, int32_t tz,
                          int32_t *out_coords, int32_t *out_count, void *ws, size_t ws_bytes,
                          ts_stream_t stream);

/* torch.unique(int64) + position lookup as used by initial_voxelize
 * (pcseg/model/segmentor/voxel/minkunet/utils.py:16-18):
 * uniq = ascending unique values of keys (non-negative, < 2^62),
 * inverse[i] = position of keys[i] in uniq (either output may be NULL),
 * *out_count (device int32) = number of unique values. */
size_t ts_unique_workspace_bytes(int64_t n);
int ts_unique_i64(const int64_t *keys, int64_t n, int64_t *uniq, int32_t *inverse,
                  int32_t *out_count, void *ws, size_t ws_bytes, ts_stream_t stream);

/* Kernel map construction: F.sphash(in) + F.sphash(out, offsets) +
 * F.sphashquery + the nonzero()/sum() compaction
 * (nn/functional/conv.py:156-176).
 *   nbr      [K, n_out] int32 : index of the input voxel at out_coords[j]+offsets[k], or -1
 *                               (== `results` of conv.py:166);
 *   nbr_t    [K, n_in]  int32 : the inverse table (output index j per (k, input i), or -1);
 *                               may be NULL;
 *   nbmaps   [K*n_out, 2] int32 capacity: rows (in_idx, out_idx) ordered by (k, out_idx)
 *                               (== conv.py:169-173); may be NULL together with nboffs;
 *   nbsizes  [K] int32        : hits per offset (== conv.py:168);
 *   nboffs   [K+1] int32      : exclusive prefix of nbsizes (nboffs[K] = P). */
size_t ts_build_kmap_workspace_bytes(int64_t n_in, int64_t n_out, int32_t n_offsets);
/*   ts_build_kmap_sym: the same tables, bit for bit, for a SUBMANIFOLD map (one coordinate set, K odd, offsets[K - 1 - k] =
 *   -offsets[k]: get_kernel_offsets of an odd kernel, nn/utils/kernel.py:11-32) on HALF the probes - offset k of voxel j finding r is
 *   offset K - 1 - k of r finding j.  Needs unique coordinates; a duplicate is detected on the device: nboffs[K] then reads -1 and
 *   the caller builds the map with ts_build_kmap.  Workspace: ts_build_kmap_workspace_bytes(n, n, K). */
/*   pos_out  [K, n_out] int32 : row of nbmaps holding the pair (k, j), or -1  (may be NULL);
 *   pos_in   [K, n_in]  int32 : row of nbmaps holding the pair of input i at offset k, or -1 (may be NULL). */
int ts_build_kmap(const int32_t *in_coords, int64_t n_in, const int32_t *out_coords,
                  int64_t n_out, const int32_t *offsets, int32_t n_offsets, int32_t *nbr,
                  int32_t *nbr_t, int32_t *nbmaps, int32_t *nbsizes, int32_t *nboffs,
                  int32_t *pos_out, int32_t *pos_in, void *ws, size_t ws_bytes,
                  ts_stream_t stream);
int ts_build_kmap_sym(const int32_t *coords, int64_t n, const int32_t *offsets, int32_t K, int32_t *nbr, int32_t *nbr_t, int32_t *nbmaps,
                      int32_t *nbsizes, int32_t *nboffs, int32_t *pos_out, int32_t *pos_in, void *ws, size_t ws_bytes, ts_stream_t stream);

/* Neighbour table from an explicit rulebook (the reference-form entry points
 * above go through this): nbr[k, col_out] = col_in for every pair of offset k.
 * nboffs [K+1] device prefix of the pair counts. */
int ts_nbr_from_nbmaps(const int32_t *nbmaps, const int32_t *nboffs, int32_t n_offsets,
                       int32_t col_in, int64_t n_rows, int32_t *nbr, ts_stream_t stream);

/* calc_ti_weights + the 8-corner lookup of voxel_to_point
 * (pcseg/.../minkunet/utils.py:72-82, nn/functional/devoxelize.py:10-48):
 * for point p (float [n,4] = x,y,z,b) and voxel grid `vox_coords` at stride s,
 * idx[i,k] = voxel at floor(p/s)*s + off_k (off = get_kernel_offsets(2, s), x
 * outermost) or -1, weight[i,k] = trilinear weight, masked and renormalised. */
size_t ts_trilinear_workspace_bytes(int64_t n_vox);
int ts_trilinear_map(const float *points, int64_t n_points, const int32_t *vox_coords,
                     int64_t n_vox, int32_t stride, int32_t *idx, float *weight, void *ws,
                     size_t ws_bytes, ts_stream_t stream);

/* ------------------------------------------------------------------------ */
/* 3. Sparse convolution on the neighbour table (the production kernels)     */
/* ------------------------------------------------------------------------ */

/* Output-stationary gather -> MFMA -> write-once convolution.
 *   out[j, :] = sum_k  in[nbr[k, j], :] @ W_k          (rows with nbr<0 skipped)
 * weight_transposed == 0: W_k = kernel[k]      ([c_in, c_out], forward);
 * weight_transposed == 1: W_k = kernel[k]^T    (kernel is [K, c_out, c_in]; this
 *                         is dgrad: in = grad_out, nbr = the inverse table).
 * out is overwritten; every row j < n_out is written exactly once. */
int ts_conv_nbr(const float *in_feat, int64_t n_in, int32_t c_in, const float *kernel,
                int32_t kernel_volume, int32_t weight_transposed, const int32_t *nbr,
                float *out_feat, int64_t n_out, int32_t c_out, ts_stream_t stream);

/* Weight gradient:  grad_kernel[k] = sum_{pairs p of k} a[pa_p, :]^T b[pb_p, :]
 * with (pa, pb) = nbmaps columns (col_a, 1-col_a); a is [*, c_a], b is [*, c_b],
 * grad_kernel [K, c_a, c_b] is overwritten (zeroed then accumulated).
 * n_pairs = nboffs[K], the rulebook length, known to the host (it sizes the grid). */
int ts_conv_wgrad(const float *a_feat, int32_t c_a, const float *b_feat, int32_t c_b,
                  const int32_t *nbmaps, const int32_t *nboffs, int32_t kernel_volume,
                  int32_t col_a, int64_t n_pairs, float *grad_kernel,
                  ts_stream_t stream);
/* The same weight gradient with run-to-run identical bits (the reference's grad_kernel[k] = in_buf^T . out_grad_buf,
 * convolution_cuda.cu:259-263, is one GEMM per offset and therefore deterministic; ts_conv_wgrad combines the partial
 * tiles of its pair chunks with float atomics): every workgroup stores its partial tile into `ws`, a second launch adds
 * the tiles of each offset in ascending chunk order.  ws >= ts_conv_wgrad_workspace_bytes(...), 16-byte aligned.
 * ts_conv_wgrad_f16_det: IEEE-half operands, float32 accumulation and result (the AMP path). */
size_t ts_conv_wgrad_workspace_bytes(int64_t n_pairs, int32_t c_a, int32_t c_b, int32_t kernel_volume);
int ts_conv_wgrad_det(const float *a_feat, int32_t c_a, const float *b_feat, int32_t c_b, const int32_t *nbmaps,
                      const int32_t *nboffs, int32_t kernel_volume, int32_t col_a, int64_t n_pairs, float *grad_kernel,
                      void *ws, size_t ws_bytes, ts_stream_t stream);
int ts_conv_wgrad_f16_det(const void *a_feat, int32_t c_a, const void *b_feat, int32_t c_b, const int32_t *nbmaps,
                          const int32_t *nboffs, int32_t kernel_volume, int32_t col_a, int64_t n_pairs,
                          float *grad_kernel, void *ws, size_t ws_bytes, ts_stream_t stream);

/* Two-pass convolution on the rulebook itself (the default forward / dgrad path):
 *   pass 1  ts_conv_pair_gemm :  z[p, :] = feat[g_p, :] @ W_{k(p)}   for every pair p of nbmaps,
 *           g_p = nbmaps[p][gather_col], k(p) = the offset whose [nboffs[k], nboffs[k+1]) holds p;
 *           one dense MFMA GEMM over all pairs (row gather fused into the A-operand load);
 *   pass 2  ts_conv_gather_sum:  out[j, :] = sum_k z[pos[k, j], :]   (pos = pos_out or pos_in of
 *           ts_build_kmap; -1 entries skipped), k ascending - deterministic, no atomics.
 * Together they equal ts_conv_nbr / the reference's gather -> GEMM -> scatter
 * (convolution_cuda.cu:101-164) with the K per-offset launches collapsed into one.
 * weight_transposed as in ts_conv_nbr.  z has n_pairs rows of c_out floats (caller-allocated). */
int ts_conv_pair_gemm(const float *feat, int64_t n_rows, int32_t c_in, const float *kernel,
                      int32_t kernel_volume, int32_t weight_transposed, const int32_t *nbmaps,
                      const int32_t *nboffs, int64_t n_pairs, int32_t gather_col, float *z,
                      int32_t c_out, ts_stream_t stream);
int ts_conv_gather_sum(const float *z, int32_t c, const int32_t *pos, int32_t kernel_volume,
                       int64_t n_rows, int64_t n_pairs, float *out, ts_stream_t stream);

/* BatchNorm over the [n, c] feature matrix of a sparse tensor (the reference runs nn.BatchNorm1d / nn.SyncBatchNorm on
 * conv outputs, pcseg/.../minkunet/minkunet.py:23-29).  c must be a multiple of 4 (<= 1024), pointers 16-byte aligned. */
/* mean[c], invstd[c] from sums = double [2, c] (sum x, sum x^2; e.g. the all-reduced pack of ts_bn_sync_stats) over
 * `total` rows (*total_dev if non-NULL - the all-reduced count of SyncBN - else total_host) and the nn.BatchNorm
 * momentum update of the running buffers (unbiased variance; either may be NULL). */
int ts_bn_finalize(const double *sums, const double *total_dev, double total_host, int32_t c, float eps,
                   float momentum, float *running_mean, float *running_var, float *mean,
                   float *invstd, ts_stream_t stream);

/* Fused elementwise halves of a conv block (the reference chains BatchNorm -> [+ shortcut] -> ReLU as separate
 * modules, minkunet.py:42-51,117-129: one full pass over [n, c] each):
 *   ts_bn_act_forward          out = act((x - mean) * invstd * weight + bias [+ residual]),  act = relu if relu != 0;
 *                              mask (optional, uint8 [n * c / 4]) gets the 4 sign bits of every float4 of `out`
 *   ts_bn_act_backward         g = grad_out * (out > 0) through that mask (all ones if mask == NULL); with
 *                              sums = double [2, c] (sum g, sum g (x - mean); ts_bn_sync_backward_reduce, all-reduced):
 *                              grad_x = (g - sums[0]/N - (x - mean) invstd^2 sums[1]/N) invstd weight,
 *                              grad_residual = g (optional); N = *total_dev if non-NULL else total_host. */
int ts_bn_act_forward(const float *x, const float *residual, const float *mean, const float *invstd,
                      const float *weight, const float *bias, int64_t n, int32_t c, int32_t relu,
                      float *out, uint8_t *mask, ts_stream_t stream);
int ts_bn_act_backward(const float *grad_out, const uint8_t *mask, const float *x, const float *mean,
                       const float *invstd, const float *weight, const double *sums,
                       const double *total_dev, double total_host, int64_t n, int32_t c, float *grad_x,
                       float *grad_residual, ts_stream_t stream);

/* Single-process training BatchNorm (+ residual) (+ ReLU) in ONE call per direction - what nn.BatchNorm1d in
 * training mode followed by the residual add and ReLU of the MinkUNet blocks computes (R minkunet.py:42-51,
 * 110-129; torch/nn/functional.py batch_norm).  Reductions go through <= 512 float partial slices in `ws`
 * (ts_bn_train_workspace_bytes(c) bytes, 16-byte aligned; stream-ordered scratch) that a finish kernel adds in
 * double: no memset, no atomics, results independent of workgroup scheduling.
 *   forward : mean/invstd [C] (saved for backward), running_mean/var updated in place and
 *             *num_batches_tracked incremented (each may be NULL),
 *             out = act((x - mean) invstd weight + bias [+ residual]), mask = 4-bit ReLU sign per float4 (relu only)
 *   backward: grad_x, grad_residual (optional, = masked grad_out), grad_weight [C], grad_bias [C] (optional)
 * SyncBatchNorm keeps using the split entry points above (the all-reduce sits between reduction and apply). */
size_t ts_bn_train_workspace_bytes(int32_t c);
int ts_bn_act_train_forward(const float *x, const float *residual, const float *weight, const float *bias,
                            float *running_mean, float *running_var, int64_t *num_batches_tracked, int64_t n,
                            int32_t c, float eps, float momentum, int32_t relu, float *mean, float *invstd,
                            float *out, uint8_t *mask, void *ws, size_t ws_bytes, ts_stream_t stream);
int ts_bn_act_train_backward(const float *grad_out, const uint8_t *mask, const float *x, const float *mean,
                             const float *invstd, const float *weight, int64_t n, int32_t c, float *grad_x,
                             float *grad_residual, float *grad_weight, float *grad_bias, void *ws, size_t ws_bytes,
                             ts_stream_t stream);

/* SyncBatchNorm reductions (the all-reduce over ranks happens between these and the elementwise entry points):
 *   ts_bn_sync_stats            pack[0..C) = sum x, pack[C..2C) = sum x^2, pack[2C] = n     (double [2C + 1])
 *   ts_bn_sync_backward_reduce  sums[0..C) = sum g, sums[C..2C) = sum g (x - mean), g = grad_out masked by the ReLU
 *                               mask when given; grad_weight / grad_bias [C] = this rank's parameter gradients
 * ws as for ts_bn_act_train_*. */
int ts_bn_sync_stats(const float *x, int64_t n, int32_t c, double *pack, void *ws, size_t ws_bytes, ts_stream_t stream);
int ts_bn_sync_backward_reduce(const float *grad_out, const uint8_t *mask, const float *x, const float *mean,
                               const float *invstd, int64_t n, int32_t c, double *sums, float *grad_weight,
                               float *grad_bias, void *ws, size_t ws_bytes, ts_stream_t stream);

/* Trilinear devoxelisation backward over runs of points that share their 8-corner index tuple (the points of one
 * interpolation cell).  Same result as ts_devoxelize_backward up to float summation order; the corner
 * contributions of a run are accumulated in registers and added to grad_feat once per run.
 *   ts_devox_order             order[n] = permutation grouping equal tuples (radix sort on 8 * first present corner
 *                              voxel + corner number; n_vox < 2^28); ws >= ts_devox_order_workspace_bytes(n)
 *   ts_devoxelize_backward_runs  grad_feat[m, c] (zeroed here) += runs; `order` may be NULL (natural order);
 *                              c % 4 == 0, 16-byte aligned rows */
/*   ts_devox_csr               inverse of a trilinear map: offsets[n_vox + 1] / entries[8 n] int32, the slots
 *                              (point * 8 + corner) with a non-zero weight onto voxel v in ascending order;
 *                              ws >= ts_devox_csr_workspace_bytes(n)
 *   ts_devoxelize_backward_csr grad_feat[v] = sum over the slots of v of weight[slot] * grad_out[point]: every row written
 *                              once, no fill, no atomics, fixed summation order (c % 4 == 0, 16-byte aligned rows) */
/*   ts_devoxelize_forward_ld / ts_devoxelize_backward_runs_ld / ts_devoxelize_backward_csr_ld: the same with the point-side
 *                              matrix `ld` floats per row (>= c, multiple of 4): the three devoxelisations of a
 *                              MinkUNet pass write into / read from column blocks of one [N, 480] matrix (no torch.cat of
 *                              z1 | z2 | z3 before the class head, no contiguous copies of its gradient slices) */
int ts_devoxelize_forward_ld(const float *feat, const int32_t *idx, const float *weight, int64_t n, int32_t c, int64_t m,
                             float *out, int64_t out_ld, ts_stream_t stream);
int ts_devoxelize_backward_runs_ld(const float *grad_out, int64_t go_ld, const int32_t *idx, const float *weight,
                                   const int32_t *order, int64_t n, int32_t c, int64_t m, float *grad_feat,
                                   ts_stream_t stream);
int ts_devoxelize_backward_csr_ld(const float *grad_out, int64_t go_ld, const float *weight, const int32_t *offsets,
                                  const int32_t *entries, int64_t n, int32_t c, int64_t m, float *grad_feat,
                                  ts_stream_t stream);

/* Cell-reduced form of the same adjoint for coarse strides (stride 16: ~700 contributions per voxel).  No reference
 * counterpart beyond devoxelize_backward_kernel (backend/devoxelize/devoxelize_cuda.cu:37-57), whose per-point
 * atomicAdds it replaces.  Plan (coordinates only, built once per batch):
 *   order      = ts_devox_order(idx): points of the same interpolation cell next to each other
 *   flags      = ts_devox_segments(idx, order, n, max_len): 1 where a segment (equal 8-corner tuple, <= max_len points)
 *                starts; seg_start = positions of the ones, then n
 *   offsets / entries = ts_devox_csr on the segments' tuples [n_seg, 8] with weight 1 on the present corners
 * ts_devoxelize_backward_cells_ld: stage 1 sums the weighted gradient rows of every segment per corner into part
 * [n_seg * 8, c] (every gradient row is read once), stage 2 gathers those rows per voxel along the inverse map.  Fixed
 * summation order, no atomics. */
int ts_devox_segments(const int32_t *idx, const int32_t *order, int64_t n, int32_t max_len, int32_t *flags,
                      ts_stream_t stream);
int ts_devoxelize_backward_cells_ld(const float *grad_out, int64_t go_ld, const float *weight, const int32_t *order,
                                    const int32_t *seg_start, int64_t n_seg, const int32_t *offsets,
                                    const int32_t *entries, int64_t n, int32_t c, int64_t m, float *part,
                                    float *grad_feat, ts_stream_t stream);
size_t ts_devox_csr_workspace_bytes(int64_t n);
int ts_devox_csr(const int32_t *idx, const float *weight, int64_t n, int64_t n_vox, int32_t *offsets, int32_t *entries,
                 void *ws, size_t ws_bytes, ts_stream_t stream);
int ts_devoxelize_backward_csr(const float *grad_out, const float *weight, const int32_t *offsets, const int32_t *entries,
                               int64_t n, int32_t c, int64_t m, float *grad_feat, ts_stream_t stream);
size_t ts_devox_order_workspace_bytes(int64_t n);
int ts_devox_order(const int32_t *idx, int64_t n, int64_t n_vox, int32_t *order, void *ws, size_t ws_bytes,
                   ts_stream_t stream);
int ts_devoxelize_backward_runs(const float *grad_out, const int32_t *idx, const float *weight, const int32_t *order,
                                int64_t n, int32_t c, int64_t m, float *grad_feat, ts_stream_t stream);
/* Half-storage forms for the AMP path (the reference's devoxelize op runs under `custom_fwd(cast_inputs=torch.half)`,
 * nn/functional/devoxelize.py:54): `void *` rows are IEEE half, leading dimensions in elements, sums in float32 and ONE
 * rounding at the store - the bits of the float32 entry points between a `.float()` of the inputs and a `.half()` of the
 * result, without those two passes.  C % 4 == 0, rows 8-byte aligned; `part` stays float32. */
int ts_devoxelize_forward_f16_ld(const void *feat, const int32_t *idx, const float *weight, int64_t n, int32_t c, int64_t m,
                                 void *out, int64_t out_ld, ts_stream_t stream);
int ts_devoxelize_backward_csr_f16_ld(const void *grad_out, int64_t go_ld, const float *weight, const int32_t *offsets,
                                      const int32_t *entries, int64_t n, int32_t c, int64_t m, void *grad_feat,
                                      ts_stream_t stream);
int ts_devoxelize_backward_cells_f16_ld(const void *grad_out, int64_t go_ld, const float *weight, const int32_t *order,
                                        const int32_t *seg_start, int64_t n_seg, const int32_t *offsets,
                                        const int32_t *entries, int64_t n, int32_t c, int64_t m, float *part,
                                        void *grad_feat, ts_stream_t stream);

/* TIAF image -> point gather (R pcseg/model/segmentor/voxel/minkunet/unet2d.py:180-214) on the NCHW stack:
 *   out[n, c] = feat[first_frame(b_n) + row_n / H, c, (row_n % H) >> shift, col_n >> shift]
 * feat [T, C, H >> shift, W >> shift] f32 (the stacked camera frames of all samples), pix [n, 2] f32 = (row, col) in
 * the sample's tall (T_b * H, W) image (truncated like the reference's `.long()`), pbatch [n] sample index,
 * frame_end [n_batch] cumulative frame counts (`offset_img`), shift = 0 (full scale) or 2 (the 1/4-scale map,
 * `row // 4, col // 4`).
 *   ts_image_plan            once per batch and scale: the points in RASTER order of their pixels - perm [n] (point index of the
 *                            i-th point of that order; stable: equal pixels keep index order), paddr [n] (pixel address
 *                            (frame * hs + r) * ws + c of that point, -1 if it falls outside its sample's frames: *err is then set
 *                            to 1 - the reference raises), run [n] (points on that pixel if i is the first of them, else 0)
 *   ts_image_gather_forward  out [n, C] rows in the original point order from one map of that scale (hw = hs * ws); lanes run
 *                            along the points of the raster order, one plane at a time, rows leave through an LDS transpose
 *   ts_image_gather_backward the adjoint as a segmented sum over the same order - no atomics, run-to-run identical: grad_feat
 *                            (n_feat = T * C * hw elements) += per-pixel sums, touching only pixels that have points;
 *                            accumulate == 0 zero-fills grad_feat first, != 0 adds into the gradient the map already has */
size_t ts_image_plan_workspace_bytes(int64_t n_pts);
int ts_image_plan(const float *pix, const int32_t *pbatch, const int32_t *frame_end, int64_t n_pts, int32_t n_batch, int32_t T, int32_t H,
                  int32_t W, int32_t shift, int32_t *perm, int32_t *paddr, int32_t *run, int32_t *err, void *ws, size_t ws_bytes,
                  ts_stream_t stream);
int ts_image_gather_forward(const float *feat, int32_t C, int64_t hw, const int32_t *perm, const int32_t *paddr, int64_t n_pts, float *out,
                            ts_stream_t stream);
int ts_image_gather_backward(const float *grad_out, int32_t C, int64_t hw, const int32_t *perm, const int32_t *paddr, const int32_t *run,
                             int64_t n_pts, float *grad_feat, int64_t n_feat, int32_t accumulate, ts_stream_t stream);

/* The same gather on a CHANNELS-LAST stack - feat [T, hs, ws, C] in memory, the layout the reference indexes (unet2d.py:183-187:
 * `permute(0, 2, 3, 1)` then row indexing) and the one the fp16 2-D convolutions produce: a pixel is one contiguous row of
 * C * elem_bytes bytes at row index paddr (ts_image_plan's pixel address), moved in 16-byte pieces by the threads of one row.
 *   ts_image_gather_rows_forward   out [n, C] in the original point order; a pure move: elements of elem_bytes = 1 / 2 / 4 / 8 bytes
 *   ts_image_gather_rows_backward  grad_feat [T, hs, ws, C] (n_feat elements) += per-pixel sums of grad_out [n, C]; half != 0: IEEE
 *                                  half rows and map (fp32 accumulation over the points of a pixel, one rounding into the map);
 *                                  every pixel row has one owner thread group: no atomics, run-to-run identical;
 *                                  accumulate as in ts_image_gather_backward */
int ts_image_gather_rows_forward(const void *feat, int32_t C, int32_t elem_bytes, const int32_t *perm, const int32_t *paddr, int64_t n_pts,
                                 void *out, ts_stream_t stream);
int ts_image_gather_rows_backward(const void *grad_out, int32_t C, int32_t half, const int32_t *perm, const int32_t *paddr,
                                  const int32_t *run, int64_t n_pts, void *grad_feat, int64_t n_feat, int32_t accumulate,
                                  ts_stream_t stream);

/* AvgPool2d(kernel 3, stride 2, padding 1, count_include_pad) of UNet2D's encoder blocks (R pcseg/model/segmentor/voxel/minkunet/
 * unet2d.py:58-62: `nn.AvgPool2d(kernel_size=kernel_size, stride=2, padding=1)`, kernel_size (3, 3)) on a channels-last stack:
 * x [T, H, W, C] -> y [T, Ho, Wo, C], Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1; fp32 accumulation, sum / 9.  half != 0: IEEE half.
 * The backward writes every element of grad_x (a gather over the <= 4 windows that hold a pixel: no atomics). */
int ts_avgpool3s2_rows_forward(const void *x, int32_t T, int32_t H, int32_t W, int32_t C, int32_t half, void *y, ts_stream_t stream);
int ts_avgpool3s2_rows_backward(const void *grad_y, int32_t T, int32_t H, int32_t W, int32_t C, int32_t half, void *grad_x,
                                ts_stream_t stream);

/* LeakyReLU -> BatchNorm2d (training) of UNet2D's blocks (unet2d.py:24-30,71,108: `bn(act(conv(x)))`, `nn.LeakyReLU()` slope 0.01) on
 * a channels-last stack seen as rows [N = T*H*W, C]: partial sums -> finish (double) -> elementwise pass, per direction.
 *   forward   out = (leaky(x) - mean) * invstd * weight + bias (+ residual [N, C], may be NULL: the block's `skip + y`, unet2d.py:31,64);
 *             mean / invstd [C] (statistics of the ACTIVATED values) kept for the backward; running_mean / running_var (momentum,
 *             unbiased variance) and num_batches_tracked updated when not NULL
 *   backward  grad_x with respect to the LeakyReLU's input, grad_weight / grad_bias [C] (may be NULL)
 * half != 0: IEEE half rows (C % 8 == 0), else float (C % 4 == 0); C <= 1024; ws >= ts_bn_train_workspace_bytes(c). */
int ts_leaky_bn_train_forward(const void *x, const float *weight, const float *bias, float *running_mean, float *running_var,
                              int64_t *num_batches_tracked, int64_t n, int32_t c, float eps, float momentum, float slope, int32_t half,
                              float *mean, float *invstd, const void *residual, void *out, void *ws, size_t ws_bytes, ts_stream_t stream);
int ts_leaky_bn_train_backward(const void *grad_out, const void *x, const float *mean, const float *invstd, const float *weight,
                               int64_t n, int32_t c, float slope, int32_t half, void *grad_x, float *grad_weight, float *grad_bias,
                               void *ws, size_t ws_bytes, ts_stream_t stream);

/* Max-voxelisation of point rows (Cylinder_TS: tools/utils/common/seg_utils.py:385-401, `torch_scatter.scatter_max(z.F, idx_query,
 * dim=0)[0]`).  feat [n, c], idx [n] int32 = voxel of every row (negative or >= m: the row takes no part), m voxels.
 *   forward   out [m, c] = per channel the maximum over the voxel's rows, arg [m, c] int32 = the SMALLEST row index that attains it;
 *             a voxel without rows gets 0 and -1.  The rows are grouped by voxel with the stable sort behind ts_devox_csr and walked
 *             in ascending order from the voxel's first row: no atomics, no zero-initialised maximum, every element of out / arg
 *             written once, run-to-run identical.  ws >= ts_voxelize_max_workspace_bytes(n, m)
 *   backward  grad_feat [n, c] = grad_out[idx[i], ch] where arg[idx[i], ch] == i, else 0 - a gather, every element written once
 * half != 0: IEEE half rows (c % 8 == 0), else float (c % 4 == 0); c <= 1024; 16-byte aligned rows. */
size_t ts_voxelize_max_workspace_bytes(int64_t n, int64_t m);
int ts_voxelize_max_forward(const void *feat, const int32_t *idx, int64_t n, int32_t c, int64_t m, int32_t half, void *out,
                            int32_t *arg, void *ws, size_t ws_bytes, ts_stream_t stream);
int ts_voxelize_max_backward(const void *grad_out, const int32_t *idx, const int32_t *arg, int64_t n, int32_t c, int64_t m,
                             int32_t half, void *grad_feat, ts_stream_t stream);

/* Mean-voxelisation of point rows with a fixed summation order (SPVCNN: fusion/spvcnn/utils.py:41-65 `point_to_voxel`).
 * feat [n, c], idx [n] int32 = voxel of every row (negative or >= m: the row takes no part), m voxels.
 *   ts_point_groups   the grouping one map needs, whatever is voxelised through it: offsets [m + 1], entries [n] int32 - the rows of
 *                     voxel v are entries[offsets[v] .. offsets[v + 1]) in ascending row order (the stable sort behind ts_devox_csr).
 *                     ws >= ts_point_groups_workspace_bytes(n)
 *   forward           out [m, c]: with cnt = the voxel's number of grouped rows, every term is feat[row] / (float)cnt in float32 (a
 *                     half row widened first).  The voxel's run is cut into pieces of P = ts_voxelize_mean_piece_rows() consecutive
 *                     rows counted from its first row; each piece is summed in ascending order, the piece sums are then added in
 *                     ascending piece order; a voxel of at most P rows is one sequential sum; a voxel without rows is a zero row; a
 *                     half result is rounded once at the store.  No atomics, no fill, every element written once, run-to-run
 *                     identical.  ws >= ts_voxelize_mean_workspace_bytes(n, c) (the full pieces' float32 sums)
 *   backward          grad_feat [n, c] = grad_out[idx[i]] / cnt, zeros for a row that took no part - a gather
 * half != 0: IEEE half rows (c % 8 == 0), else float (c % 4 == 0); c <= 1024; 16-byte aligned rows.
 * ts_voxelize_mean_set_piece_rows (16, 32 or 64) exists for the timing tool's comparison only: P is part of the rule. */
int32_t ts_voxelize_mean_piece_rows(void);
int ts_voxelize_mean_set_piece_rows(int32_t rows);
size_t ts_point_groups_workspace_bytes(int64_t n);
int ts_point_groups(const int32_t *idx, int64_t n, int64_t m, int32_t *offsets, int32_t *entries, void *ws, size_t ws_bytes,
                    ts_stream_t stream);
size_t ts_voxelize_mean_workspace_bytes(int64_t n, int32_t c);
int ts_voxelize_mean_forward(const void *feat, const int32_t *idx, const int32_t *offsets, const int32_t *entries, int64_t n,
                             int32_t c, int64_t m, int32_t half, void *out, void *ws, size_t ws_bytes, ts_stream_t stream);
int ts_voxelize_mean_backward(const void *grad_out, const int32_t *idx, const int32_t *offsets, int64_t n, int32_t c, int64_t m,
                              int32_t half, void *grad_feat, ts_stream_t stream);

/* The tail of SPVCNN's point branch (spvcnn.py:417-444) on rows [n, c] in one pass:
 *   out[i, :] = sum_k weight[i, k] vox[idx[i, k], :] + relu((y[i, :] - mean) invstd gamma + beta)
 * idx / weight [n, 8] = a ts_trilinear_map result over the m rows of vox; the sum runs over k = 0 .. 7 in k order in float32, a
 * corner with idx < 0 (or >= m) or weight 0 adds nothing (the arithmetic of ts_devoxelize_forward).  mask (optional, uint8
 * [n * c / 4], half: [n * c / 8]) gets the sign bits of the BatchNorm term - not of out - in the layout of ts_bn_act_forward, for
 * ts_bn_act_train_backward; mask == NULL with running statistics is the evaluation form.  half != 0: y, vox and out are IEEE half
 * (c % 8 == 0), else float (c % 4 == 0); c <= 1024; float arithmetic, one rounding at the store; 16-byte aligned rows and maps. */
int ts_point_tail_forward(const void *y, const void *vox, const int32_t *idx, const float *weight, const float *mean,
                          const float *invstd, const float *gamma, const float *beta, int64_t n, int32_t c, int64_t m, int32_t half,
                          void *out, uint8_t *mask, ts_stream_t stream);

/* RPVNet's range <-> point transfers (rpvnet.py:32-91) as maps the point <-> voxel kernels above already serve.  A feature map
 * [B, C, h, w] in channels-last memory is B h w rows of C: row b h w + y w + x.
 *   ts_range_plan   pxpy [n, 3] float = (batch, px, py), px and py in [-1, 1]; one call per resolution (batch, h, w), coordinates only.
 *                   pix [n] int32: the pixel row a point is averaged into by `point_to_range`,
 *                     x = (int32)(((px + 1) / 2) * (float)(w - 1)), y likewise with h - float32, one rounding per operation,
 *                     truncation (rpvnet.py:88).  ts_point_groups(pix, n, B h w) + ts_voxelize_mean_forward is the mean per pixel
 *                     (zeros for a pixel without points) with that kernel's summation rule; ts_voxelize_mean_backward the adjoint.
 *                   bidx int32 / bweight float [n, 8]: grid_sample's corners (bilinear, zeros padding, align_corners = False) in
 *                     the layout of ts_trilinear_map: ix = ((px + 1) w - 1) / 2, x0 = floor(ix), x1 = x0 + 1, columns 0 .. 3 =
 *                     nw, ne, sw, se with weights (x1 - ix)(y1 - iy), (ix - x0)(y1 - iy), (x1 - ix)(iy - y0), (ix - x0)(iy - y0) in
 *                     float32; a corner outside the map, and columns 4 .. 7: index -1, weight 0.  ts_devoxelize_forward over the
 *                     B h w rows is `range_to_point`; ts_devox_csr / ts_devox_order and ts_devoxelize_backward_* its adjoint.
 *                   err [1] int32 (caller-zeroed, OR-ed into): 1 a batch index that is no integer of [0, batch), 2 a non-finite
 *                     px / py, 4 px / py outside [-1, 1]; such a row takes no part either way (pix -1, all corners -1).  No host read.
 *   ts_range_point_tail_forward   ts_point_tail_forward with one more gathered operand, one pass:
 *                     out[i, :] = (sum_{k<8} weight[i, k] vox[idx[i, k], :] + sum_{j<4} bweight[i, j] pix[bidx[i, j], :])
 *                                 + relu((y[i, :] - mean) invstd gamma + beta)
 *                   over the m rows of vox and the mp rows of the map pix; the trilinear sum in k order, the bilinear sum in corner
 *                   order from its own zero, the two added, then the BatchNorm term (rpvnet.py:651 left to right).  mask, half, c and
 *                   alignment as ts_point_tail_forward. */
int ts_range_plan(const float *pxpy, int64_t n, int32_t batch, int32_t h, int32_t w, int32_t *pix, int32_t *bidx, float *bweight,
                  int32_t *err, ts_stream_t stream);
int ts_range_point_tail_forward(const void *y, const void *vox, const int32_t *idx, const float *weight, const void *pix,
                                const int32_t *bidx, const float *bweight, const float *mean, const float *invstd,
                                const float *gamma, const float *beta, int64_t n, int32_t c, int64_t m, int64_t mp, int32_t half,
                                void *out, uint8_t *mask, ts_stream_t stream);

/* RPVNet's inputs from a batch's point rows (SemkittiFusionDataset.get_range_image, semantickitti_fusion.py:64-114), two launches for
 * the whole batch.  feat [n, ld >= 5] float = x, y, z, reflectivity, ring per row; batch [n] int32; cut [B] float = the random cut of
 * every sample ((rand() - 0.5) * 2 pi, rounded to float as numpy does when it adds it).
 *   pxpy [n, 3] float   (batch, px, py): yaw = (float)atan2((double)y, -(double)x) + cut; yaw % 2 pi - pi; 0.5 (yaw / pi + 1) (W - 1)
 *                       in float32, rounded half-to-even to the column; the row is the rounded ring; px = 2 (column / (W - 1) - 0.5),
 *                       py likewise, in float64, cast once.  (numpy's own float32 arctan2 is not correctly rounded; this one is.)
 *   table [B, H, W] int32, pre-filled with -1: the LAST row index that lands on a pixel (integer atomicMax: order-free)
 *   image [B, 5, H, W] float: the winner's 25 (1 / depth - 0.4), 20 (reflectivity - 0.5) - float64 on the float32 depth quotient
 *                       and value, cast once - and x, y, z; a pixel without rows: -10, -10, 0, 0, 0
 *   err [1] int32, OR-ed into: 8 a ring above H - 1 or below 0, 16 a non-finite coordinate, 1 a batch index outside [0, B); such a
 *                       row takes no part and gets px = py = NaN, which ts_range_plan drops again. */
int ts_range_inputs(const float *feat, int64_t ld, const int32_t *batch, const float *cut, int64_t n, int32_t B, int32_t H, int32_t W,
                    float *pxpy, int32_t *table, float *image, int32_t *err, ts_stream_t stream);

/* The range-view family's data stage (LaserScan.do_range_projection, pcseg/data/dataset/semantickitti/laserscan.py:182-238, and
 * SemkittiRangeViewDataset.prepare_input_label_semantic_with_mask, semantickitti_rv.py:284-301), two launches for the whole batch.
 * feat [n, ld >= 4] float = x, y, z, remission per row; batch [n] int32; first [B] int32 = the first row of every scan (the rows of
 * a scan are consecutive); label [n] int32 or NULL (then label_rv is NULL too); fov_up / fov_down in degrees.
 *   per row, in the reference's float32 chain (numpy 2: Python scalars are weak), operation by operation:
 *     depth = sqrtf((x x + y y) + z z); yaw = -(float)atan2((double)y, (double)x); pitch = (float)asin((double)(z / depth));
 *     proj_x = 0.5f (yaw / (float)pi + 1.0f) W; proj_y = (1.0f - (pitch + (float)|fov_down|) / (float)fov) H; floor; clamp to
 *     [0, W - 1] / [0, H - 1].  (numpy's own float32 arctan2 / arcsin are not correctly rounded; these are.)
 *   proj_x, proj_y [n] int32, unproj_range [n] float in input order
 *   table [B, H, W] uint64, pre-filled with all ones: ONE atomicMin per row of (bits of depth) << 32 | (row - first[b]): the winner
 *     of a pixel is the row of smallest depth, the lowest index among equal depths - the reference's descending stable argsort
 *     followed by "last assignment wins" - in any arrival order
 *   scan_rv [B, 6, H, W] float = the winner's x / 50, y / 50, z / 3, remission, depth / 80 (float32 divisions), mask
 *   proj_range [B, H, W] float, proj_idx [B, H, W] int32 (index within the scan, -1: empty), label_rv [B, 1, H, W] int64
 *   a pixel without rows: -1 / 50, -1 / 50, -1 / 3, -1, -1 / 80, 0; range -1; index -1; label 0
 *   REPRODUCED: mask = (proj_idx > 0) (laserscan.py:238), so a pixel won by a scan's row 0 carries real values and mask 0
 *   err [1] int32, OR-ed into: 16 a non-finite coordinate, 32 depth == 0, 1 a batch index outside [0, B) or a row in front of its
 *     scan's first; such a row takes no part and gets proj_x = proj_y = -1, unproj_range = -1.  No host read. */
#define TS_RV_ERR_BATCH 1
#define TS_RV_ERR_PIXEL 2
#define TS_RV_ERR_NONFINITE 16
#define TS_RV_ERR_ORIGIN 32
int ts_rv_project(const float *feat, int64_t ld, const int32_t *batch, const int32_t *first, const int32_t *label, int64_t n,
                  int32_t B, int32_t H, int32_t W, double fov_up, double fov_down, int32_t *proj_x, int32_t *proj_y,
                  float *unproj_range, uint64_t *table, float *scan_rv, float *proj_range, int32_t *proj_idx, int64_t *label_rv,
                  int32_t *err, ts_stream_t stream);

/* The range-view family's kNN post-processing (KNN.forward, pcseg/model/segmentor/range/utils.py:300-341) for a whole batch in one
 * launch, one lane per point, selection and vote in registers.  proj_range [B, H, W] float, proj_class [B, H, W] int32 (the
 * per-pixel arg-max); unproj_range, px, py, batch [n]; weight [S S] float = 1 - gaussian as the reference computes it (:320).
 *   window slot s = (dy + pad) S + dx + pad, pad = (S - 1) / 2; a slot outside the image has range 0 and class 0 (F.unfold's zero
 *   padding: no wrap in azimuth); a range < 0 becomes +inf (:315); the centre slot's range is the point's own, its class stays the
 *   pixel's (:317); distance = fabsf(r - r_point) weight[s] (a NaN distance counts as +inf); the K smallest by ascending (distance,
 *   slot) - THE TIE RULE OF THIS LIBRARY, the reference's topk(sorted=False) states none; with cutoff > 0 a selected slot whose
 *   distance exceeds it votes for class nclasses (:330-333); label = 1 + the first maximum of the counts of classes 1 ..
 *   nclasses - 1 (:338), so a point whose votes are all unlabelled or cut off gets class 1; classes outside [0, nclasses] do not vote.
 *   S in {3, 5, 7}, 1 <= K <= S S, 2 <= nclasses <= 32: anything else returns TS_ERR_UNSUPPORTED.
 *   err [1] int32, OR-ed into: 2 a px / py outside the image, 1 a batch index outside [0, B); such a point gets label 0. */
int ts_rv_knn(const float *proj_range, const int32_t *proj_class, const float *unproj_range, const int32_t *px, const int32_t *py,
              const int32_t *batch, const float *weight, int64_t n, int32_t B, int32_t H, int32_t W, int32_t K, int32_t S,
              float cutoff, int32_t nclasses, int32_t *label, int32_t *err, ts_stream_t stream);

/* The range-view family's point augmentation (LaserScan.open_scan, laserscan.py:104-143) of a whole batch into a NEW cloud; the
 * input rows are never written.  feat [n, ld >= 4] float, batch [n] int32 ascending, label [n] int32 or NULL (then out_label is
 * NULL), first [B] int32 = the first input row of every cloud, params [B, TS_RV_AUG_RECORD] doubles
 *   { c, s, scale, tx, ty, tz, bits, flip }   bits: 1 rotate, 2 scale, 4 flip, 8 jitter ; flip: 0 .. 3 (1: x, 2: y, 3: both)
 * with c = cos, s = sin of the angle from the host.  drop [n_drop] int32 or NULL: the clouds' drop lists (np.unique of the
 * reference's draws: indices WITHIN the cloud), concatenated; drop_off [B + 1] int32 their offsets; keep [n] bytes, pre-filled with
 * ones by the caller.
 *   drop   one thread per list entry clears the row's keep byte (a duplicate would write the same value); an index outside its
 *          cloud sets TS_RV_ERR_DROP and is ignored.  Then the stable compaction of csrc/compact.h: the survivors keep their
 *          input order, no atomics; a cloud's first output row is the sum of the survivors before it, which the host knows from
 *          the lengths of the unique lists - no device read.
 *   arithmetic, in the reference's order, EVERY STEP rounded to float32 (it assigns back into its float32 array after each; this
 *          is not ts_stage_augment's single rounding):
 *     flip    sign changes of x and / or y
 *     scale   x, y (NOT z - reproduced) times (float)scale in float32: np.random.uniform returns a Python float, a weak scalar
 *     rotate  np.dot(float32 [n, 2], float64 2 x 2) is dgemm: X = fma(y, -s, x c), Y = fma(y, c, x s) in float64, rounded once
 *     jitter  (float)((double)v + t) per axis
 *     remission passes through; a step whose bit is clear is skipped: a record without bits returns the input's bits
 *   out [capacity >= n, 4] float (16-byte aligned), out_label [capacity] int32, out_sample [capacity] int64 and out_sample32
 *   [capacity] int32 (the survivors' clouds), counts [B] int64 (the survivors per cloud, on the device); rows past the survivors
 *   are not written.  At most TS_RV_MAX_CLOUDS clouds.  ws: ts_rv_augment_workspace_bytes(n, B) bytes.
 *   err [1] int32, OR-ed into: TS_RV_ERR_DROP, TS_RV_ERR_BATCH (a batch index outside [0, B): the row is dropped).  One launch for
 *   the drop lists and three for the compaction; no host read. */
#define TS_RV_ERR_DROP 64
#define TS_RV_AUG_RECORD 8
#define TS_RV_MAX_CLOUDS 64
size_t ts_rv_augment_workspace_bytes(int64_t n, int32_t B);
int ts_rv_augment(const float *feat, int64_t ld, const int32_t *batch, const int32_t *label, const int32_t *first, int64_t n,
                  int32_t B, const double *params, const int32_t *drop, const int32_t *drop_off, int64_t n_drop, uint8_t *keep,
                  float *out, int32_t *out_label, int64_t *out_sample, int32_t *out_sample32, int64_t capacity, int64_t *counts,
                  void *ws, size_t ws_bytes, int32_t *err, ts_stream_t stream);

/* The pixels of every class in every image: label [B, 1, H, W] int64, counts [B, TS_RV_CLASSES] int32 pre-filled with zeros and
 * added into.  Integer additions only: the result does not depend on their order.  A label outside [0, TS_RV_CLASSES) is not
 * counted.  One launch. */
#define TS_RV_CLASSES 32
int ts_rv_label_counts(const int64_t *label, int32_t B, int32_t H, int32_t W, int32_t *counts, ts_stream_t stream);

/* RangeShift, RangeMix, RangePaste and RangeUnion (SemkittiRangeViewDataset.__getitem__, semantickitti_rv.py:137-183;
 * sample_transform :304-320, MixTeacherSemkitti :360-1700, RangePaste :210-281, RangeUnion :197-207) of a batch of projected
 * images, one thread per output pixel, one launch.  scan_a [B, 6, H, W] float and label_a [B, 1, H, W] int64: the primaries;
 * scan_b, label_b: the partners, counts [B, TS_RV_CLASSES] int32 = ts_rv_label_counts(label_b) - all three NULL without partners,
 * then only the shift applies.  records [B, TS_RV_COMPOSE_RECORD] int32 on the device:
 *   { shift_a, shift_b, n_row_bounds, n_col_bounds, row_bounds[5], col_bounds[5], mixture, flags }   flags: 1 paste, 2 union
 * In the reference's order, for output pixel (y, x):
 *   shift   the primary is read at column (x + shift_a) mod W, the partner at (x + shift_b) mod W (0: none) - the partner is
 *           shifted before mix, paste and union see it
 *   mix     every colCrowR strategy is a checkerboard: cell row = the number of row bounds <= y, cell column = the number of
 *           column bounds <= x (the HOST computes the bounds with the reference's expressions; a bound at or beyond the size
 *           selects nothing, as the reference's empty slices); mixture 1 takes the primary where cell row + cell column is even,
 *           mixture 2 the partner there; 0: no mix
 *   paste   the pixel takes the partner when the partner's label there is one of 2 .. 8, 12, 16, 18, 19 and counts[b][label] > 20
 *   union   a pixel whose mask (channel 5) after mix and paste is 0 takes the partner - also a pixel won by a scan's row 0
 *           (the reproduced `proj_idx > 0`)
 * and ONE copy of the chosen pixel's six values and label to out_scan [B, 6, H, W], out_label [B, 1, H, W] (not in place).  A
 * record of zeros copies the primary bit for bit. */
#define TS_RV_COMPOSE_RECORD 16
int ts_rv_compose(const float *scan_a, const int64_t *label_a, const float *scan_b, const int64_t *label_b, const int32_t *counts,
                  const int32_t *records, int32_t B, int32_t H, int32_t W, float *out_scan, int64_t *out_label, ts_stream_t stream);

/* The gate of Cylinder_TS's ReconBlock (cylinder_ts.py:368-384) on rows [n, c]: out = x * (sigmoid(u) + sigmoid(v) + sigmoid(w)),
 * one pass; the backward forms grad_x, grad_u, grad_v, grad_w from grad_out and the four inputs in one pass.  float arithmetic;
 * half != 0: IEEE half storage (c % 8 == 0), else float (c % 4 == 0); 16-byte aligned pointers. */
int ts_sigmoid3_gate_forward(const void *x, const void *u, const void *v, const void *w, int64_t n, int32_t c, int32_t half,
                             void *out, ts_stream_t stream);
int ts_sigmoid3_gate_backward(const void *grad_out, const void *x, const void *u, const void *v, const void *w, int64_t n,
                              int32_t c, int32_t half, void *grad_x, void *grad_u, void *grad_v, void *grad_w,
                              ts_stream_t stream);

/* Dense 3 x 3 convolution, 32 -> 32 channels, stride 1, padding = dilation (1 or 2), on channels-last IEEE-half rows - the
 * full-resolution layers of UNet2D (unet2d.py:10-31,41-60: `nn.Conv2d(32, 32, (3, 3), padding=1)` and `dilation=2, padding=2`).
 *   ts_conv3x3c32_pack   the nn.Conv2d weight [co][ci][ky][kx] (half, any strides) -> the MFMA operand form the kernel keeps in
 *                        registers (ts_conv3x3c32_packed_bytes() bytes); mode 0: forward, mode 1: data gradient (taps mirrored,
 *                        channels swapped)
 *   ts_conv3x3c32_rows   y [T, H, W, 32] = conv(x [T, H, W, 32]) + bias [32] (float, may be NULL); with a mode-1 pack and
 *                        x = grad_y it returns grad_x.  fp32 accumulation, one rounding to half. */
size_t ts_conv3x3c32_packed_bytes(void);
int ts_conv3x3c32_pack(const void *weight, int64_t s_co, int64_t s_ci, int64_t s_ky, int64_t s_kx, int32_t mode, void *packed,
                       ts_stream_t stream);
int ts_conv3x3c32_rows(const void *x, const void *packed, const float *bias, int32_t T, int32_t H, int32_t W, int32_t dilation, void *y,
                       ts_stream_t stream);
/*   ts_conv3x3c32_wgrad  grad_weight [co][ci][ky][kx] (half, the element strides of the weight it belongs to) = sum over pixels of
 *                        x[t, y + (ky - 1) D, x + (kx - 1) D, ci] grad_y[t, y, x, co]: partial [9][32][32] sums per workgroup (fp32, LDS
 *                        transposing reads feed the MFMAs), then their sum in index order - no atomics, run-to-run identical.
 *                        grad_bias [32] (float, may be NULL): the column sums of grad_y, in the same pass.
 *                        ws >= ts_conv3x3c32_wgrad_workspace_bytes(). */
size_t ts_conv3x3c32_wgrad_workspace_bytes(void);
int ts_conv3x3c32_wgrad(const void *x, const void *grad_y, int32_t T, int32_t H, int32_t W, int32_t dilation, void *grad_weight,
                        int64_t s_co, int64_t s_ci, int64_t s_ky, int64_t s_kx, float *grad_bias, void *ws, size_t ws_bytes,
                        ts_stream_t stream);

/* The 1 x 1, 32 -> 32 channel layers in front of UNet2D's blocks with the LeakyReLU behind them (unet2d.py:10-12,41-43:
 * `act1(conv1(x))`) on channels-last IEEE-half rows: y [n_pixels, 32] = LeakyReLU_slope(x W^T + bias) (leaky = 0: no activation;
 * with a mode-1 pack that is the data gradient).  ts_conv1x1c32_wgrad: weight [co][ci] and bias gradient from x and the gradient g at
 * the layer's output - the 3 x 3 weight gradient's pass, centre tap (same workspace). */
size_t ts_conv1x1c32_packed_bytes(void);
int ts_conv1x1c32_pack(const void *weight, int64_t s_co, int64_t s_ci, int32_t mode, void *packed, ts_stream_t stream);
int ts_conv1x1c32_rows(const void *x, const void *packed, const float *bias, int64_t n_pixels, int32_t leaky, float slope, void *y,
                       ts_stream_t stream);
int ts_conv1x1c32_wgrad(const void *x, const void *g, int32_t T, int32_t H, int32_t W, void *grad_weight, int64_t s_co, int64_t s_ci,
                        float *grad_bias, void *ws, size_t ws_bytes, ts_stream_t stream);

/* The same convolution (stride 1, padding 1, no dilation) with the channel counts opened up - UpBlock.conv1 of the decoder
 * (unet2d.py:81-115: 96 -> 96 channels at 1/2 scale, 56 -> 96 at full scale): input channels a multiple of 8 up to 96, output
 * channels a multiple of 8.  A persistent workgroup owns one 32-channel output block, its 9 x C_in/16 weight fragments in registers.
 *   ts_conv3x3_rows_packed_bytes(k, m)  bytes of the packed operand for k reduction channels (the channels of the call's input)
 *                                       and m result channels; 0 = the kernel does not take the layer
 *   ts_conv3x3_rows_pack                weight [c_out][c_in][3][3] (half, element strides) -> packed; mode 0 forward
 *                                       (k, m) = (c_in, c_out), mode 1 data gradient (k, m) = (c_out, c_in)
 *   ts_conv3x3_rows                     y [T, H, W, y_channels] = conv(x [T, H, W, x_channels]) + bias (float, may be NULL) */
size_t ts_conv3x3_rows_packed_bytes(int32_t k_channels, int32_t m_channels);
int ts_conv3x3_rows_pack(const void *weight, int32_t c_out, int32_t c_in, int64_t s_co, int64_t s_ci, int64_t s_ky, int64_t s_kx,
                         int32_t mode, void *packed, ts_stream_t stream);
int ts_conv3x3_rows(const void *x, int32_t x_channels, const void *packed, const float *bias, int32_t T, int32_t H, int32_t W, void *y,
                    int32_t y_channels, ts_stream_t stream);
/*   ts_conv3x3_wgrad                    grad_weight [c_out][c_in][3][3] (half, the weight's element strides) and grad_bias [c_out]
 *                                       (float, may be NULL) of the same layers (channel counts multiples of 8 up to 96) from x and
 *                                       grad_y: the 9 x c_in x c_out fp32 sums in the registers of persistent workgroups (96 x 96 in two
 *                                       passes over the input channels), partials added in a fixed order - run-to-run identical.
 *                                       ws >= ts_conv3x3_wgrad_workspace_bytes(c_in, c_out) (0: layer not taken). */
size_t ts_conv3x3_wgrad_workspace_bytes(int32_t c_in, int32_t c_out);
int ts_conv3x3_wgrad(const void *x, int32_t c_in, const void *grad_y, int32_t c_out, int32_t T, int32_t H, int32_t W, void *grad_weight,
                     int64_t s_co, int64_t s_ci, int64_t s_ky, int64_t s_kx, float *grad_bias, void *ws, size_t ws_bytes, ts_stream_t stream);

/* UpBlock's entry on channels-last rows (unet2d.py:98-108: PixelShuffle(2), Dropout2d, torch.cat((upA, skip), dim=1), Dropout2d) in one
 * pass:  cat [T, 2h, 2w, C/4 + Cs] = concat(PixelShuffle(2)(x [T, h, w, C]), skip [T, 2h, 2w, Cs]) * scale [T, C/4 + Cs]
 * (float, may be NULL: the two dropout masks folded into one factor per frame and channel).  half != 0: IEEE half (C a multiple of
 * 32, Cs of 8), else float (16 / 4).  _backward is the adjoint: grad_x and grad_skip from grad_cat with the same scale. */
int ts_shuffle_cat_rows_forward(const void *x, const void *skip, const float *scale, int32_t T, int32_t h, int32_t w, int32_t C, int32_t Cs,
                                int32_t half, void *cat, ts_stream_t stream);
int ts_shuffle_cat_rows_backward(const void *grad_cat, const float *scale, int32_t T, int32_t h, int32_t w, int32_t C, int32_t Cs,
                                 int32_t half, void *grad_x, void *grad_skip, ts_stream_t stream);

/* ---- fp16 storage / fp32 accumulation (the reference trains under AMP: conv.py:19 `custom_fwd(cast_inputs=half)`).
 * `void *` operands are IEEE half arrays.  Channel counts must be multiples of 32, K <= 63.
 *   ts_cast_weights_f16      w f32 [K, Ci, Co] -> w16 [K, Ci, Co] and / or w16t [K, Co, Ci] (either may be NULL)
 *   ts_conv_pair_gemm_f16    z[p, :] = feat[nbmaps[p][gather_col], :] @ W_k(p); `w_rows` [K, c_out, c_red] holds, per
 *                            offset, one row per OUTPUT column contiguous in the reduction index: w16t for the forward
 *                            pass (c_red = Ci), w16 for the input gradient (c_red = Co, c_out = Ci)
 *   ts_conv_gather_sum_f16   out[j, :] = sum_k z[pos[k, j], :]  (fp32 accumulation, k ascending) */
int ts_cast_weights_f16(const float *w, int32_t K, int32_t c_in, int32_t c_out, void *w16, void *w16t,
                        ts_stream_t stream);
int ts_conv_pair_gemm_f16(const void *feat, int64_t n_rows, int32_t c_red, const void *w_rows, int32_t K,
                          const int32_t *nbmaps, const int32_t *nboffs, int64_t n_pairs, int32_t gather_col, void *z,
                          int32_t c_out, ts_stream_t stream);
/*   ts_conv_pair_gemm_f16_nat  ts_conv_pair_gemm_f16 with the weight in its natural layout w [K, c_red, c_out] (the forward
 *                              pass reads the half copy of kernel [K, C_in, C_out] in place; fragments come from the
 *                              transposing LDS load, no transposed copy of the weight exists) */
int ts_conv_pair_gemm_f16_nat(const void *feat, int64_t n_rows, int32_t c_red, const void *w, int32_t K,
                              const int32_t *nbmaps, const int32_t *nboffs, int64_t n_pairs, int32_t gather_col, void *z,
                              int32_t c_out, ts_stream_t stream);

int ts_conv_gather_sum_f16(const void *z, int32_t c, const int32_t *pos, int32_t K, int64_t n_rows, int64_t n_pairs,
                           void *out, ts_stream_t stream);
/*   ts_conv_wgrad_f16        grad_kernel[k] (fp32 [K, c_a, c_b], zeroed here) = sum_pairs a[pa]^T b[pb], half rows in,
 *                            fp32 accumulation (MFMA fragments via ds_read_b64_tr_b16), chunk partials by float atomics */
int ts_conv_wgrad_f16(const void *a_feat, int32_t c_a, const void *b_feat, int32_t c_b, const int32_t *nbmaps,
                      const int32_t *nboffs, int32_t K, int32_t col_a, int64_t n_pairs, float *grad_kernel,
                      ts_stream_t stream);

/* Half-storage forms of ts_bn_act_train_*: x / residual / out / grad_* are IEEE half [n, c] (c % 8 == 0), the mask is
 * one byte per 8 elements; statistics, affine parameters, their gradients and all arithmetic are fp32. */
int ts_bn_act_train_forward_f16(const void *x, const void *residual, const float *weight, const float *bias,
                                float *running_mean, float *running_var, int64_t *num_batches_tracked, int64_t n,
                                int32_t c, float eps, float momentum, int32_t relu, float *mean, float *invstd,
                                void *out, uint8_t *mask, void *ws, size_t ws_bytes, ts_stream_t stream);
int ts_bn_act_train_backward_f16(const void *grad_out, const uint8_t *mask, const void *x, const float *mean,
                                 const float *invstd, const float *weight, int64_t n, int32_t c, void *grad_x,
                                 void *grad_residual, float *grad_weight, float *grad_bias, void *ws, size_t ws_bytes,
                                 ts_stream_t stream);

/* Flat-buffer optimizer step of the training loop (R/train.py:399-417: GradScaler.unscale_ -> clip_grad_norm_ ->
 * SGD step -> GradScaler.update), decided on the device - no host read.  `state` = float[8] on the device:
 * [0] loss scale, [1] growth tracker, [2] gradient multiplier (clip coefficient / scale), [3] skip flag, [4] total norm.
 *   ts_sgd_grad_stats  *sumsq += sum g^2 (double), *nonfinite |= any non-finite        (call once per bucket)
 *   ts_sgd_decide      norm of the unscaled gradients, clip coefficient min(1, max_norm / (norm + 1e-6)), skip flag,
 *                      loss-scale update (amp != 0; as GradScaler, the scale is not grown past the largest float);
 *                      clears sumsq / nonfinite for the next step
 *   ts_sgd_apply       d = g * state[2] + wd * p; m = first_step ? d : momentum * m + d; p -= lr * m   (skipped if flagged) */
int ts_sgd_grad_stats(const float *grad, int64_t n, double *sumsq, int32_t *nonfinite, ts_stream_t stream);
int ts_sgd_decide(double *sumsq, int32_t *nonfinite, float *state, float max_norm, float growth, float backoff,
                  int32_t growth_interval, int32_t amp, ts_stream_t stream);
int ts_sgd_apply(float *param, const float *grad, float *momentum_buf, int64_t n, const float *state, float lr,
                 float momentum, float weight_decay, int32_t first_step, ts_stream_t stream);

/* ts_sgd_apply per parameter slot of a bucket, one launch (what FlatSGD.step() issues).  Device tables:
 *   slots[n_slots]      one record per parameter of the bucket, ascending offsets; every slot starts on a 16-element
 *                       boundary and the padding up to the next slot holds zeros in all three buckets
 *   tile_first[n_tiles] n_tiles = ceil(n / TS_SGD_TILE): index of the slot that holds element t * TS_SGD_TILE
 *   flags               NULL with one process: a slot with `unused` set is left untouched, bit for bit.  Else the
 *                       reducer's all-reduced "some rank had a gradient" array: such a slot is skipped only when
 *                       flags[flag_index] == 0
 *   groups[n_groups]    hyper-parameters per group, or NULL (n_groups 1): then every slot takes lr / momentum /
 *                       weight_decay / nesterov from the arguments
 * Per element ts_sgd_apply's arithmetic (the same bits for one group without Nesterov); with nesterov
 * p -= lr * (d + momentum * m_new).  n % 4 == 0, the three buckets 16-byte aligned. */
#define TS_SGD_TILE 4096
typedef struct TsSgdSlot {
  int64_t offset;      /* first element of the slot in the bucket */
  int64_t count;       /* elements of the parameter (the slot is padded to the next multiple of 16) */
  int32_t group;       /* index into groups */
  int32_t unused;      /* != 0: this rank has no gradient for the parameter this step */
  int32_t flag_index;  /* index into flags */
  int32_t reserved;
} TsSgdSlot;
typedef struct TsSgdGroup {
  float lr, momentum, weight_decay;
  int32_t nesterov;
} TsSgdGroup;
int ts_sgd_apply_segments(float *param, const float *grad, float *momentum_buf, int64_t n, const float *state,
                          const TsSgdSlot *slots, int32_t n_slots, const int32_t *tile_first, int64_t n_tiles,
                          const float *flags, const TsSgdGroup *groups, int32_t n_groups, float lr, float momentum,
                          float weight_decay, int32_t nesterov, int32_t first_step, ts_stream_t stream);

/* Flat-buffer AdamW step (torch.optim.AdamW: decoupled weight decay, no amsgrad) on the same buckets, slot records,
 * tile list and flags as ts_sgd_apply_segments.  ts_sgd_grad_stats and ts_sgd_decide come first; of their `state` only
 * [2] (gradient multiplier gs) and [3] (skip flag) are read.
 *   ts_adamw_prepare   one thread per slot, arithmetic in double.  Writes nothing when state[3] != 0 and nothing for a
 *                      skipped slot (`unused` set and, with flags, flags[flag_index] == 0).  Else t = ++step[s] and, from
 *                      groups[slots[s].group] = (lr, beta1, beta2, eps, weight_decay) - the CURRENT values -, coef[s]:
 *                        decay = (float)(1 - lr wd)   w1 = (float)(1 - beta1)   b2 = (float)beta2   w2 = (float)(1 - beta2)
 *                        neg_step_size = (float)(-(lr / (1 - beta1^t)))   bc2_sqrt = (float)sqrt(1 - beta2^t)
 *                        eps = (float)eps   live = 1 | (wd != 0 ? 2 : 0)
 *   ts_adamw_apply_segments   per element of a slot that is not skipped, every operation rounded to float on its own:
 *                        g' = g gs;  p1 = p decay (left out when live bit 1 is clear, as torch leaves out the mul_)
 *                        d = g' - m;  m' = w1 < 0.5 ? m + w1 d : g' - d (1 - w1)        (ATen's lerp)
 *                        v' = b2 v + (w2 g') g';  den = sqrtf(v') / bc2_sqrt + eps;  p' = p1 + (neg_step_size m') / den
 *                      with correctly rounded sqrtf and division.  The padding between slots (zeros in all four
 *                      buckets) stays zero because eps > 0: the caller must refuse eps <= 0.  A skipped step and a skipped
 *                      slot keep every bit of p, m, v.  n % 4 == 0, the four buckets 16-byte aligned,
 *                      n_tiles = ceil(n / TS_SGD_TILE). */
typedef struct TsAdamwGroup {
  double lr, beta1, beta2, eps, weight_decay;
} TsAdamwGroup;
typedef struct TsAdamwCoef {
  float decay, w1, b2, w2, neg_step_size, bc2_sqrt, eps;
  int32_t live;
} TsAdamwCoef;
int ts_adamw_prepare(const TsSgdSlot *slots, int32_t n_slots, const float *flags, const float *state,
                     const TsAdamwGroup *groups, int32_t n_groups, int32_t *step, TsAdamwCoef *coef, ts_stream_t stream);
int ts_adamw_apply_segments(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                            const float *state, const TsSgdSlot *slots, int32_t n_slots, const int32_t *tile_first,
                            int64_t n_tiles, const float *flags, const TsAdamwCoef *coef, ts_stream_t stream);

/* Half-storage forms of the SyncBatchNorm halves (ts_bn_sync_stats, ts_bn_act_forward, ts_bn_sync_backward_reduce,
 * ts_bn_act_backward): activations / gradients IEEE half [n, c] (c % 8 == 0), mask one byte per 8 elements, everything
 * else as in the fp32 forms.  ts_bn_act_backward_f16 needs 2 c floats of 16-byte aligned scratch. */
int ts_bn_sync_stats_f16(const void *x, int64_t n, int32_t c, double *pack, void *ws, size_t ws_bytes, ts_stream_t stream);
int ts_bn_act_forward_f16(const void *x, const void *residual, const float *mean, const float *invstd,
                          const float *weight, const float *bias, int64_t n, int32_t c, int32_t relu, void *out,
                          uint8_t *mask, ts_stream_t stream);
int ts_bn_sync_backward_reduce_f16(const void *grad_out, const uint8_t *mask, const void *x, const float *mean,
                                   const float *invstd, int64_t n, int32_t c, double *sums, float *grad_weight,
                                   float *grad_bias, void *ws, size_t ws_bytes, ts_stream_t stream);
int ts_bn_act_backward_f16(const void *grad_out, const uint8_t *mask, const void *x, const float *mean,
                           const float *invstd, const float *weight, const double *sums, const double *total_dev,
                           double total_host, int64_t n, int32_t c, void *grad_x, void *grad_residual, void *ws,
                           size_t ws_bytes, ts_stream_t stream);

/* SyncBatchNorm with the statistics all-reduce issued by the library on the CALLER'S stream (csrc/rccl.hip): RCCL is
 * bound at run time with dlopen (ts_rccl_load: path of the librccl.so the host framework already uses), the library
 * owns one communicator per SyncBatchNorm group (ts_rccl_unique_id on one rank, the 128-byte id distributed by the
 * host, ts_rccl_comm_init collectively), and one call per direction runs local sliced sums -> ncclAllReduce of
 * [2C + 1] / [2C] doubles -> elementwise pass.  Replaces nn.SyncBatchNorm (minkunet.py:23-25; torch/nn/modules/
 * _functions.py SyncBatchNorm) whose collectives go through the process group's own stream.
 * pack [2C + 1] / sums [2C]: double scratch; pack[2C] afterwards holds the global row count (= total_dev of the
 * backward call).  half = 1: IEEE-half activations / gradients.  ws as ts_bn_train_workspace_bytes(c). */
int ts_rccl_load(const char *librccl_path);
int ts_rccl_unique_id(void *id128);
int ts_rccl_comm_init(const void *id128, int32_t nranks, int32_t rank, void **comm);
int ts_rccl_comm_destroy(void *comm);
int ts_rccl_allreduce_f64(void *comm, double *buf, int64_t count, ts_stream_t stream);
int ts_bn_sync_forward(void *comm, const void *x, const void *residual, const float *weight, const float *bias,
                       float *running_mean, float *running_var, int64_t *num_batches_tracked, int64_t n, int32_t c,
                       float eps, float momentum,
                       int32_t relu, int32_t half, double *pack, float *mean, float *invstd, void *out, uint8_t *mask,
                       void *ws, size_t ws_bytes, ts_stream_t stream);
int ts_bn_sync_backward(void *comm, const void *grad_out, const uint8_t *mask, const void *x, const float *mean,
                        const float *invstd, const float *weight, const double *total_dev, int64_t n, int32_t c,
                        int32_t half, double *sums, void *grad_x, void *grad_residual, float *grad_weight,
                        float *grad_bias, void *ws, size_t ws_bytes, ts_stream_t stream);

/* One call per direction for conv -> BatchNorm(train) [+ residual] [-> ReLU], the unit of the MinkUNet family
 * (minkunet.py:31-129: BasicConvolutionBlock, BasicDeconvolutionBlock, the two halves of ResidualBlock).  Chains the
 * launches of ts_conv_pair_gemm / ts_conv_gather_sum (or the _f16 forms, half = 1) and ts_bn_act_train_* (comm == NULL)
 * or ts_bn_sync_* (comm = a ts_rccl_comm_init communicator) on `stream`; Z, the gradient w.r.t. the convolution output
 * and the transposed half weight live in `ws` (ts_conv_block_workspace_bytes).  Arguments: csrc/block.hip.
 * SyncBatchNorm with the all-reduce run by the CALLER (torch.distributed on its own communicator): comm = (void *)1 makes
 * the call stop after the local sums (forward: convolution + `pack`; backward: `sums`), the caller all-reduces that buffer
 * over its ranks and calls again with the same arguments and comm = (void *)2, which runs what is left (forward: statistics +
 * elementwise pass; backward: elementwise pass + weight gradient + input gradient).  ts_bn_sync_forward / _backward take the
 * same two values.
 *
 * `opts` (may be NULL) names everything a block call may use beyond the rulebook - explicitly, per call (round 4: it replaces
 * the thread-local one-shot hints ts_conv_class_hint / ts_conv_block_addend_hint and, for the block calls, ts_conv_planes_hint;
 * nothing a call leaves behind can steer another call):
 *   fwd_plan / dgrad_plan  class-sorted plans of THIS block's kernel map (ts_conv_class_plan) for the forward product and the
 *                          input gradient, or NULL for pair GEMM + pass 2.  A plan is used only if it fits the call: K, its row
 *                          count = the rows the product writes, channel counts the class kernels take, and map_id == the
 *                          call's nboffs pointer (the identity of the kernel map it was built from) - otherwise the two passes.
 *                          Plans with `rows` (direct, one group: the 2x2x2 strided / transposed maps) store the result rows
 *                          themselves: no Z, no pass 2.  Submanifold 3x3x3 maps use ONE plan for both directions (mirror = 1:
 *                          the input gradient takes the slice of offset K-1-k).
 *   planes                 fp32: the pre-split bf16 planes of `kernel` (ts_conv_split_planes), kept in step by the caller
 *   w16_current            half: the w16 buffer already holds the cast of `kernel` (the call casts nothing)
 *   addend                 backward only: [n_dgrad_rows, c_in] in grad_feat's storage type, 16-byte aligned, added in the
 *                          grad_feat store (the gradient reaching the block's input along a residual connection,
 *                          minkunet.py:117-129) - one rounding like a separate sum of the two */
typedef struct TsClassPlan {
  const int32_t *src, *tile_info, *n_tiles;
  const int32_t *pos;      /* [groups][n]: pass-2 plans */
  const int32_t *rows;     /* [m_pad]: direct plans (groups == 1) */
  int64_t n, m_pad;
  int64_t z_rows;          /* host copy of 128 * listed tiles (profile records only), or 0 */
  int32_t K, groups, mirror;
  const void *map_id;      /* nboffs pointer of the kernel map the plan was built from */
} TsClassPlan;
typedef struct TsConvBlockOpts {
  const TsClassPlan *fwd_plan, *dgrad_plan;
  const void *planes;
  int32_t w16_current;
  const void *addend;
  /* backward only: the weight gradient on a second stream.  wgrad_stream != NULL: the gradient w.r.t. the convolution output is
   * written into wgrad_ws (>= ts_conv_block_wgrad_ws_bytes) instead of the call's own workspace, and the weight gradient - partial
   * tiles + ordered sum, deterministic as before - is enqueued on wgrad_stream behind an event of the caller's stream; the input
   * gradient follows on the caller's stream without waiting for it.  wgrad_slot (0 .. 7) names the ring slot wgrad_ws belongs to:
   * a later call with the same slot first waits (on the caller's stream) for the slot's previous weight gradient.  grad_kernel is
   * complete on wgrad_stream: the caller joins the streams (ts_stream_join) before it reads the weight gradients. */
  ts_stream_t wgrad_stream;
  void *wgrad_ws;
  size_t wgrad_ws_bytes;
  int32_t wgrad_slot;
  /* wgrad_deferred != 0: the call only marks the point on its stream where the output gradient exists and leaves the weight
   * gradient to a ts_conv_block_wgrad_side call with the same arguments - from any host thread, so that its launches need not
   * come from the thread that issues the step */
  int32_t wgrad_deferred;
  /* natural != 0: a 1x1x1 convolution on the identity rulebook (K = 1, pair p = (p, p), n_pairs = n_out: conv.py:135-140's
   * `feats.matmul(weight)` as a block) - the pair GEMM's rows ARE the result rows: the product is written straight into the
   * convolution output / the input gradient, no Z, no pass 2, no position table read (pos may be any valid pointer); the shortcut
   * branch of a residual block (minkunet.py:105-111) as one call per direction.  Not combined with class plans or an addend. */
  int32_t natural;
} TsConvBlockOpts;
size_t ts_conv_block_workspace_bytes(int64_t n_pairs, int64_t n_rows_max, int32_t c_in, int32_t c_out, int32_t K,
                                     int32_t half);
size_t ts_conv_block_wgrad_ws_bytes(int64_t n_pairs, int64_t n_out, int32_t c_in, int32_t c_out, int32_t K, int32_t half);
/* `waiter` waits for everything enqueued on `other` so far (one event; no host synchronisation) */
int ts_stream_join(ts_stream_t waiter, ts_stream_t other);
int ts_conv_block_wgrad_side(const void *feat, int64_t n_feat_rows, int32_t c_in, int32_t K, const int32_t *nbmaps,
                             const int32_t *nboffs, int64_t n_pairs, int32_t wgrad_col_a, int64_t n_out, int32_t c_out, int32_t half,
                             float *grad_kernel, int32_t chunk_order, void *wgrad_ws, size_t wgrad_ws_bytes, int32_t slot,
                             ts_stream_t side_stream);
int ts_set_device(int32_t device);      /* hipSetDevice for a host thread the caller created */
/* The evaluation tail of the segmentors for a whole batch (R/pcseg/model/segmentor/voxel/minkunet/minkunet.py:435-455, minkunet_ms.py:
 * 433-458: per scene `out[scene mask][inverse_map of the scene]`, arg-max) without the per-scene loop of boolean masks:
 *   ts_scene_counts  counts [3][n_scenes] int64 = rows per scene of the voxel / point / label batch-index arrays (int32, `stride`
 *                    elements apart: the last column of an [N, 4] coordinate matrix is stride 4); *flags: bit 0 an index outside
 *                    0 .. n_scenes - 1, bit 1 an array that is not grouped by scene in ascending order (the caller then sorts).
 *                    counts and flags are zero-filled by the call.  n_scenes <= 64.
 *   ts_unvoxelise    for arrays grouped by scene: mapped [n_pts, C] (same type as logits; may be NULL) = logits[start of the point's
 *                    scene + inv[p], :], pred [n_pts] int64 (may be NULL) = index of the row's first maximum; *flags |= 4 where inv[p]
 *                    lies outside its scene (the reference's indexing raises).  counts = ts_scene_counts' first n_scenes entries. */
int ts_scene_counts(const int32_t *b_vox, int64_t stride_vox, int64_t n_vox, const int32_t *b_pts, int64_t stride_pts, int64_t n_pts,
                    const int32_t *b_lab, int64_t stride_lab, int64_t n_lab, int32_t n_scenes, int64_t *counts, int32_t *flags,
                    ts_stream_t stream);
int ts_unvoxelise(const void *logits, int32_t half, int32_t C, const int64_t *counts, int32_t n_scenes, const int32_t *b_pts,
                  int64_t stride_pts, const int64_t *inv, int64_t n_pts, void *mapped, int64_t *pred, int32_t *flags, ts_stream_t stream);
/* Evaluation on the device (R/train.py:35-52, 465-540: fast_hist over the scans of a batch; the summed votes of one scan, their
 * arg-max and the label payload) behind ts_scene_counts, for index arrays grouped by scene.  With cnt_v / cnt_p / cnt_l = its counts:
 * the KEPT points of scene s are its points in array order (those with point_mask != 0 where ts_eval_rows ran), K_s of them,
 * m_s = min(K_s, max(num_points[s], 0)); kept point j < m_s reads logits row start_v[s] + inv[p].
 *   ts_eval_rows       (point_mask given) rows [n_pts] int32: per kept point, scene-major, inv[p] (-1 where it is negative or above
 *                      2^31 - 1); kept [n_scenes] int64 = K_s.  Stable compaction in three launches, no atomics for order.
 *   ts_eval_confusion  hist [C, C] int64 += 1 at (l, arg-max of the row) for kept point j < m_s of scene s with label l =
 *                      labels[start_l[s] + j] in 0 .. C - 1 (labels of label_bytes 1 unsigned, 4 or 8 signed); the call ADDS.
 *                      pred (optional, int32, pred_cap rows >= sum m_s are written at most): the arg-max, scene-major.  One launch.
 *   ts_eval_votes      the scenes are the votes of ONE scan, n = m_s for all s: total[j, c] = ((x_0 + x_1) + x_2) + ... in float32 in
 *                      vote order, x_v = (float)logits[row of (v, j), c]; label [cap] (label_bytes 4: uint32, 1: uint8) = first
 *                      maximum of total[j]; sums (optional) [cap, C] float32 = total; top3 (optional, C >= 3) [cap, 3] float32 = the
 *                      three largest sums, descending; *n_out = n.  cap >= n_pts / n_scenes holds every n.  One launch.
 * Either inv (no mask) or rows + kept (ts_eval_rows), the other NULL.  scene_flags: the int ts_scene_counts wrote.  num_points
 * [n_scenes] int64, num_points_ms (optional) likewise.  *flags is OR-ed into and never cleared: bits 0 and 1 ts_scene_counts', bit 2
 * (4) an inverse map entry outside its scene (the row is skipped), bit 3 (8) min(cnt_l, num_points) != m_s for a scene (it
 * contributes nothing), bit 4 (16) votes of unequal m_s (nothing is written), bit 5 (32) num_points_ms[s] != cnt_p[s].  The arg-max
 * is the first maximum, a NaN wins (ts_unvoxelise).  No index addresses a load before it has been range-checked; n_pts = 0 is valid. */
size_t ts_eval_rows_workspace_bytes(int64_t n_pts, int32_t n_scenes);
int ts_eval_rows(const uint8_t *point_mask, const int32_t *b_pts, int64_t stride_pts, const int64_t *inv, int64_t n_pts,
                 int32_t n_scenes, int32_t *rows, int64_t *kept, void *ws, size_t ws_bytes, ts_stream_t stream);
int ts_eval_confusion(const void *logits, int32_t half, int32_t C, int64_t n_vox, const int64_t *counts, const int32_t *scene_flags,
                      int32_t n_scenes, const int64_t *inv, const int32_t *rows, const int64_t *kept, int64_t n_pts,
                      const void *labels, int32_t label_bytes, int64_t n_lab, const int64_t *num_points,
                      const int64_t *num_points_ms, int64_t *hist, int32_t *pred, int64_t pred_cap, int32_t *flags,
                      ts_stream_t stream);
int ts_eval_votes(const void *logits, int32_t half, int32_t C, int64_t n_vox, const int64_t *counts, const int32_t *scene_flags,
                  int32_t n_scenes, const int64_t *inv, const int32_t *rows, const int64_t *kept, int64_t n_pts,
                  const int64_t *num_points, const int64_t *num_points_ms, void *label, int32_t label_bytes, float *sums,
                  float *top3, int64_t cap, int64_t *n_out, int32_t *flags, ts_stream_t stream);
/* The same two reductions for a model whose logits rows are NOT grouped by scene and whose points find their row through the hash of
 * their cell (Cylinder_TS, R/pcseg/model/segmentor/voxel/cylinder3d/cylinder_ts.py:244-260: rows in ascending-hash order over the
 * batch): grows [n_pts] int64 names the GLOBAL logits row of every point (-1 = the lookup found none) in place of the per-scene
 * inverse map, and labels [n_pts] are aligned with the points (no batch column of their own).  counts / scene_flags: what
 * ts_scene_counts wrote ([3][n_scenes]; only the POINT row is read - call it with the points' batch column, int32 with a stride,
 * grouped by scene in ascending order, and n_vox = n_lab = 0).  The kept points of scene s are its first m_s = min(cnt_p[s],
 * max(num_points[s], 0)) points; no mask, no num_points_ms.
 *   ts_eval_confusion_rows  hist += 1 at (labels[p], arg-max of logits[grows[p]]) for every kept point whose label lies in 0 .. C - 1;
 *                           pred (optional) as in ts_eval_confusion; m_out (optional) [n_scenes] int64 = m_s.  One launch.
 *   ts_eval_votes_rows      as ts_eval_votes: the scenes are the votes of one scan, equal m_s; label / sums / top3 / n_out.  One launch.
 * Flags: bits 0, 1 and 4 as above (bits 2, 3 and 5 cannot rise); bit 6 (64) a point's row is negative or >= n_vox: the point
 * contributes nothing (confusion: not tallied, its pred is 0; votes: its term of the sum is left out).  Every row and position is
 * range-checked before it addresses a load; n_pts = 0 is valid (grows, labels may be NULL). */
int ts_eval_confusion_rows(const void *logits, int32_t half, int32_t C, int64_t n_vox, const int64_t *counts,
                           const int32_t *scene_flags, int32_t n_scenes, const int64_t *grows, int64_t n_pts, const void *labels,
                           int32_t label_bytes, const int64_t *num_points, int64_t *hist, int32_t *pred, int64_t pred_cap,
                           int64_t *m_out, int32_t *flags, ts_stream_t stream);
int ts_eval_votes_rows(const void *logits, int32_t half, int32_t C, int64_t n_vox, const int64_t *counts, const int32_t *scene_flags,
                       int32_t n_scenes, const int64_t *grows, int64_t n_pts, const int64_t *num_points, void *label,
                       int32_t label_bytes, float *sums, float *top3, int64_t cap, int64_t *n_out, int32_t *flags,
                       ts_stream_t stream);
/* Column concatenation / slicing of row-major feature matrices - torchsparse.cat (TS/torchsparse/operators.py:10-17: torch.cat of
 * the feature matrices along dim 1, the skip connections of the decoder, R/pcseg/model/segmentor/voxel/minkunet/minkunet.py:403-416)
 * and its gradient, for callers that chain block calls without tensors (the stage programs of csrc/fastpath/stage_program.h).
 * Widths and pitches in BYTES (any element size); 16-byte vector copies when every pointer, pitch and width allows, else 4 / 2 / 1.
 *   ts_cat_cols   dst[r] = a[r] | b[r]   (dst pitch = a_bytes + b_bytes), one launch
 *   ts_copy_cols  dst[r, 0:width] = src[r, offset : offset + width]   (src rows src_pitch apart, dst rows dst_pitch apart) */
int ts_cat_cols(const void *a, int64_t a_bytes, const void *b, int64_t b_bytes, int64_t rows, void *dst, ts_stream_t stream);
int ts_copy_cols(const void *src, int64_t src_pitch, int64_t offset, int64_t width, int64_t rows, void *dst, int64_t dst_pitch,
                 ts_stream_t stream);
int ts_conv_block_forward(const void *feat, int64_t n_feat_rows, int32_t c_in, const float *kernel, int32_t K,
                          const int32_t *nbmaps, const int32_t *nboffs, int64_t n_pairs, int32_t gather_col,
                          const int32_t *pos, int64_t n_out, int32_t c_out, const void *residual, const float *bn_weight,
                          const float *bn_bias, float *running_mean, float *running_var, int64_t *num_batches_tracked,
                          float eps, float momentum, int32_t relu, int32_t half, void *comm, double *pack, void *conv_out,
                          float *mean, float *invstd, void *out, uint8_t *mask, void *w16, const TsConvBlockOpts *opts,
                          void *ws, size_t ws_bytes, ts_stream_t stream);
/* evaluation form (module in eval mode, no graph): out = act((conv(feat) - mean) * invstd * bn_weight + bn_bias [+ residual]) with the
 * caller's mean / invstd (running_mean, 1 / sqrt(running_var + eps)); the same convolution as the training forward (opts->fwd_plan,
 * planes, w16_current), then one elementwise pass - no statistics, nothing kept for a backward pass */
int ts_conv_block_eval(const void *feat, int64_t n_feat_rows, int32_t c_in, const float *kernel, int32_t K,
                       const int32_t *nbmaps, const int32_t *nboffs, int64_t n_pairs, int32_t gather_col, const int32_t *pos,
                       int64_t n_out, int32_t c_out, const void *residual, const float *bn_weight, const float *bn_bias,
                       const float *mean, const float *invstd, int32_t relu, int32_t half, void *out, void *w16,
                       const TsConvBlockOpts *opts, void *ws, size_t ws_bytes, ts_stream_t stream);
int ts_conv_block_backward(const void *grad_out, const uint8_t *mask, const void *conv_out, const float *mean,
                           const float *invstd, const float *bn_weight, const double *total_dev, void *comm, double *sums,
                           int64_t n_out, int32_t c_out, int32_t half, const void *feat, int64_t n_feat_rows, int32_t c_in,
                           const void *weights, int32_t K, const int32_t *nbmaps, const int32_t *nboffs, int64_t n_pairs,
                           int32_t dgrad_gather_col, const int32_t *pos_dgrad, int64_t n_dgrad_rows, int32_t wgrad_col_a,
                           void *grad_feat, void *grad_residual, float *grad_kernel, float *grad_bn_weight,
                           float *grad_bn_bias, const TsConvBlockOpts *opts, void *ws, size_t ws_bytes, ts_stream_t stream);

/* Per-launch timing inside ts_conv_block_*: while enabled, every pair-GEMM / gather-sum / weight-gradient launch of the
 * block calls is bracketed by HIP events on the caller's stream.  ts_prof_collect waits for them and writes one record
 * of 9 doubles per launch: kind (0 pair GEMM, 1 gather-sum, 2 weight gradient), milliseconds, pairs, c_red, c_out, K,
 * rows, bytes per element, weight-transposed flag; returns the number of records (-1: HIP error).  ts_prof_reserve
 * creates events ahead of time (two per bracketed launch) so that none is created inside a timed region. */
void ts_prof_enable(int32_t on);
int ts_prof_reserve(int64_t n_events);
int64_t ts_prof_collect(double *records, int64_t capacity);
/* microseconds an event pair measures with nothing between its two records (median of `reps` pairs back to back on
 * `stream`): the bracket's own share of every per-launch figure above */
int ts_prof_empty_bracket_us(int32_t reps, ts_stream_t stream, double *out_us);

/* Debug / cross-check implementation selector: 0 = MFMA kernels (default; full-tile fp32 GEMMs run on the bf16 matrix
 * pipe through the exact three-way operand split of csrc/conv_pairs_s.hip), 5 = the same with v_mfma_f32_16x16x4_f32,
 * 1 = scalar reference kernels (one thread per output element, atomics),
 * 2 = MFMA kernels with the guarded generic staging code even where the unguarded full-tile variants apply,
 * 3 / 4 = full-tile pair GEMM with one workgroup per tile everywhere / persistent workgroups everywhere
 *         (default: persistent for the forward weight layout only),
 * 11 / 13 = with pre-split weight planes at hand (ts_conv_planes_hint) take the direct-rows pair GEMM on 96-column tiles
 *         as well / never (default: on 128-column tiles),
 * 14 = the default choice everywhere, but the fp32 class GEMM's plain launch runs one workgroup per tile instead of the
 *         persistent walk (same bits: the A/B parent and the bit oracle of the walk),
 * 15 = as 14, but with the walk's kernel (two gathered slices in flight), launched with a workgroup per tile. */
void ts_set_conv_impl(int32_t impl);

/* Lovasz-softmax with classes = 'present' around ONE sort (R/tools/utils/common/lovasz_losses.py:158-227: lovasz_softmax_flat,
 * lovasz_grad, flatten_probas' ignore handling), forward value and gradient in one pass.
 *   ts_lovasz_errors  errors[c, p] = |(labels[p] == c) - probas[p, c]| where labels[p] != ignore, else 0 (class-major [C, P])
 *   caller            errors_sorted, perm = sort(errors, dim 1, descending)            (perm int64, as torch.sort returns it)
 *   ts_lovasz_grad    loss[0] = mean over the classes present of dot(errors_sorted_c, lovasz_grad(fg_sorted_c));
 *                     grad_probas[p, c] = d loss / d probas[p, c] (every element written; rows with the ignored label 0), stored
 *                     [P, C], or [C, P] when class_major != 0 (what ts_ce_lovasz_backward reads: the scatter through perm then
 *                     stays inside one class's 4 P bytes at a time)
 * probas [P, C] float32 row-major, labels [P] int64 (`ignore` = a value no label takes when nothing is ignored),
 * C <= 64.  ws >= ts_lovasz_workspace_bytes(P, C).  Rows with the ignored label keep their place with zero error and
 * zero foreground (same value as dropping them, no host read of their number). */
int ts_lovasz_errors(const float *probas, const int64_t *labels, int64_t ignore, int64_t n_points, int32_t n_classes,
                     float *errors, ts_stream_t stream);
size_t ts_lovasz_workspace_bytes(int64_t n_points, int32_t n_classes);
int ts_lovasz_grad(const float *errors_sorted, const int64_t *perm, const int64_t *labels, int64_t ignore, int64_t n_points,
                   int32_t n_classes, float *loss, float *grad_probas, int32_t class_major, void *ws, size_t ws_bytes,
                   ts_stream_t stream);

/* The segmentors' training loss, CE + Lovasz (R/pcseg/loss/__init__.py:40-44, 118-133: nn.CrossEntropyLoss(ignore_index,
 * label_smoothing) + lovasz_softmax(softmax(logits), ignore)), around the one sort:
 *   ts_softmax_ce_forward  one pass over logits [P, C] (C <= 32): probas [P, C], the Lovasz error matrix [C, P] (what
 *                          ts_lovasz_errors writes) and partials [ceil(P / 256), 3] doubles (sum -logp[y], sum -sum_c logp_c, rows)
 *   ts_ce_lovasz_finish    out4 = { w_ce ce + w_lov lovasz, ce, lovasz, rows that count }; ce = (1 - eps) nll / n + eps smooth / (n C)
 *                          (torch's label-smoothed mean over the rows whose label is not ignored); lovasz = ts_lovasz_grad's
 *                          loss scalar (device pointer) or NULL
 *   ts_ce_lovasz_backward  grad_logits [P, C] from probas, labels, grad_probas (= ts_lovasz_grad's in CLASS-MAJOR form [C, P], or
 *                          NULL) and the upstream gradient scalar (device pointer) */
int ts_softmax_ce_forward(const float *logits, const int64_t *labels, int64_t ignore, int64_t n_points, int32_t n_classes,
                          float *probas, float *errors, double *partials, ts_stream_t stream);
int ts_ce_lovasz_finish(const double *partials, int64_t n_points, int32_t n_classes, float smoothing, float w_ce, float w_lov,
                        const float *lovasz, float *out4, ts_stream_t stream);
int ts_ce_lovasz_backward(const float *probas, const int64_t *labels, int64_t ignore, const float *grad_probas,
                          const float *out4, const float *grad_out, int64_t n_points, int32_t n_classes, float smoothing,
                          float w_ce, float w_lov, float *grad_logits, ts_stream_t stream);

/* Pre-split weight planes for the fp32 pair GEMMs (csrc/conv_pairs_s.hip) - an optional accelerator of
 * ts_conv_pair_gemm (one-shot hint below) and ts_conv_block_forward / _backward (TsConvBlockOpts.planes), no counterpart in the reference (its
 * convolution_forward_cuda, backend/convolution/convolution_cuda.cu:101-164, multiplies fp32 operands in cuBLAS).
 * The fp32 kernels evaluate a product on the bf16 matrix pipe through the exact split x = h + m + l of both operands;
 * for a weight that split is the same in every workgroup of every launch until the optimizer changes the weight.
 *   planes: 3 * K * c_in * c_out bf16 (16-byte aligned): h | m | l, each in the layout of W [K, c_in, c_out] (the forward
 *           product and the input gradient read the same planes); c_in * c_out % 8 == 0.
 *   ts_conv_split_planes[_batch]  write them (one launch per 16 weights): call after every update of the weight.
 *   ts_conv_planes_hint           one-shot and per thread: the NEXT ts_conv_pair_gemm made by this thread may read
 *           `planes` in place of `w` if its weight pointer is `w` and its shapes are (K, c_in, c_out); that call clears
 *           the hint whether it used it or not (the block calls take their planes as an argument and clear any hint).  Results are bit-identical with and without planes; keeping them in
 *           step with the weight is the caller's contract (taseg_amd/planes.py does it for the modules). */
typedef struct TsPlaneJob {
  const float *w;
  void *planes;
  int32_t K, c_in, c_out;
} TsPlaneJob;
int ts_conv_split_planes(const float *w, int32_t K, int32_t c_in, int32_t c_out, void *planes, ts_stream_t stream);
int ts_conv_split_planes_batch(const TsPlaneJob *jobs, int32_t n_jobs, ts_stream_t stream);
void ts_conv_planes_hint(const float *w, const void *planes, int32_t K, int32_t c_in, int32_t c_out);
/* The half-storage counterpart: job.planes = w16 [K, c_in, c_out] IEEE half (what ts_cast_weights_f16 writes), 16 weights
 * per launch.  A ts_conv_block_forward(half = 1) call with opts->w16_current takes its w16 argument as already cast and
 * launches no cast of its own (torch.autocast casts the weight in every call: conv.py:19). */
int ts_cast_weights_f16_batch(const TsPlaneJob *jobs, int32_t n_jobs, ts_stream_t stream);

/* Class-sorted implicit GEMM (csrc/conv_class.hip) - pass 1 of a convolution with the sums of up to nine offsets kept in the
 * accumulators.  The K offsets are cut into `groups` groups of K / groups <= 9; per group the destination rows are sorted by
 * their neighbour mask and cut into 128-row tiles; a workgroup owns a tile and walks the offsets of the tile's union mask.
 * Same product as convolution_forward_cuda / convolution_backward_cuda (backend/convolution/convolution_cuda.cu:101-278) on the
 * rulebook ts_build_kmap gave; another summation order than ts_conv_pair_gemm + ts_conv_gather_sum (1e-6-close, deterministic).
 *   submanifold 3x3x3 maps: groups = 3 (one z-plane of the kernel each): Z' has one row per (output row, z-plane) instead of one
 *     per rulebook pair (about 2 N instead of 6.5 N rows on a LiDAR scan), pass 2 is ts_conv_gather_sum with K = 3 and the
 *     plan's position table `pos`.  The map is its own transpose with the offsets reversed, so the SAME plan serves the input
 *     gradient (wt = 1, mirror = 1: slice K-1-k, transposed).
 *   2x2x2 strided maps (and their transposed use, convolution_cuda.cu:21,34): groups = 1, a DIRECT plan (`rows` instead of `pos`):
 *     all offsets of a destination row sit in one tile, the sums ARE the result and are stored straight into the destination
 *     rows - no Z, no pass 2.  Two plans per map: destination = coarse rows (nbr = the map's own table: strided forward,
 *     transposed input gradient) and destination = fine rows (nbr = ts_conv_nbr_transposed: transposed forward, strided input
 *     gradient; every fine row has exactly one pair); mirror = 0.  Rows without any neighbour are written as zeros.
 *   ts_conv_class_rows2(n, groups)  m_pad = groups * roundup(n, 128): slots of src / rows of Z' (ts_conv_class_rows: groups = 3)
 *   ts_conv_class_plan      nbr [K][n] -> src [K / groups][m_pad] (input row of (group offset, slot) or -1), tile_info
 *                           [m_pad / 128][2], n_tiles [2] (device: listed tiles, and their (tile, offset) steps - 128 * steps
 *                           row-products against the rulebook's P pairs says what the plan costs: mask-sorted LiDAR rows give
 *                           ~1.1 P, rows with unrelated masks up to 3.7 P), and exactly one of pos [groups][n] (row of Z' per
 *                           (group, destination) or -1) and rows [m_pad] (destination row per slot or -1; groups == 1)
 *   ts_conv_nbr_transposed  nbr_t [K][n_in] of a kernel map from its pos_in table and rulebook
 *   ts_conv_class_gemm      wt = 0: feat = input rows, kernel [K, c_red, c_out]; wt = 1: the transposed product (feat = output
 *                           gradients [*, c_red], kernel [K, c_out, c_red] as stored; mirror selects the slice K-1-k);
 *                           rows == NULL: zp [m_pad, c_out]; rows != NULL: zp [n, c_out] = the result
 *   ts_conv_class_conv      the WHOLE convolution on a three-group plan, out [n, c_out] (+ addend [n, c_out], optional): every row
 *                           is its own centre neighbour, so the centre group's tiles hold every output row exactly once - they
 *                           run as a second launch of the product, add the other two groups' Z' rows of their rows (pass 2's
 *                           additions in pass 2's order: the same bits as ts_conv_class_gemm + ts_conv_gather_sum) and store the
 *                           result rows; no pass-2 launch, the centre group's third of Z' is never written.  zp [m_pad, c_out]
 *                           is scratch for the outer groups' rows. */
int64_t ts_conv_class_rows(int64_t n);
int64_t ts_conv_class_rows2(int64_t n, int32_t groups);
size_t ts_conv_class_plan_workspace_bytes(int64_t n);
int ts_conv_class_plan(const int32_t *nbr, int64_t n, int32_t K, int32_t groups, int32_t *src, int32_t *tile_info,
                       int32_t *n_tiles, int32_t *pos, int32_t *rows, void *ws, size_t ws_bytes, ts_stream_t stream);
/* the direct plan of a strided map's one-pair-per-destination direction (destination = its input rows) straight from the rulebook,
 * without a sort (slot p = pair p; needs n_pairs == number of destination rows); ws >= 4 * ceil(n_pairs / 128) bytes */
int ts_conv_class_plan_pairs(const int32_t *nbmaps, const int32_t *nboffs, int32_t K, int64_t n_pairs, int32_t *src,
                             int32_t *tile_info, int32_t *n_tiles, int32_t *rows, void *ws, size_t ws_bytes, ts_stream_t stream);
int ts_conv_nbr_transposed(const int32_t *pos_in, const int32_t *nbmaps, int32_t K, int64_t n_in, int32_t *nbr_t,
                           ts_stream_t stream);
int32_t ts_conv_class_supported(int32_t c_red, int32_t c_out);
int ts_conv_class_gemm(const float *feat, int32_t c_red, const float *kernel, int32_t K, int32_t groups, int32_t c_out,
                       const int32_t *src, int64_t m_pad, const int32_t *tile_info, const int32_t *n_tiles, int32_t wt,
                       int32_t mirror, const int32_t *rows, float *zp, ts_stream_t stream);
/* With the weight's pre-split planes at hand (ts_conv_planes_hint(kernel, planes, K, C_in, C_out) right before the call, or
 * TsConvBlockOpts.planes of a block call) ts_conv_class_gemm runs persistent workgroups that walk the tile list (workgroup `slot`
 * of G takes tile round * G + slot, the slot order reversed every other round) and read the weight slices from the planes;
 * G = min(m_pad / 128, ts_conv_class_walk_slots(c_out, wt)) per column tile: what the chip holds of the instantiation that serves
 * c_out columns.  A call with a bare weight, and ts_set_conv_impl(14), run one workgroup per tile, which splits the fp32 weight
 * slice itself: the same bits. */
int32_t ts_conv_class_walk_slots(int32_t c_out, int32_t wt);
/* ... with the job the block calls let ride on the launch: dw [side_k][cacb] = per offset k the ascending sum of the weight-gradient
 * partial tiles part[c + k][cacb] over the chunks c = nboffs[k] / chunk .. (nboffs[k + 1] - 1) / chunk of its pairs (zeros where an
 * offset has none); cacb a multiple of 4, part and dw 16-byte aligned */
int ts_conv_class_gemm_wsum(const float *feat, int32_t c_red, const float *kernel, int32_t K, int32_t groups, int32_t c_out,
                            const int32_t *src, int64_t m_pad, const int32_t *tile_info, const int32_t *n_tiles, int32_t wt,
                            int32_t mirror, const int32_t *rows, float *zp, const float *part, const int32_t *side_nboffs, float *dw,
                            int32_t side_k, int32_t chunk, int64_t cacb, ts_stream_t stream);
/* does finishing inside the product beat pass 2 on a map of n rows (measured thresholds; what the block calls use) */
int32_t ts_conv_class_finish_pays(int64_t n, int32_t half);
int ts_conv_class_conv(const float *feat, int32_t c_red, const float *kernel, int32_t K, int32_t groups, int32_t c_out,
                       const int32_t *src, int64_t m_pad, const int32_t *tile_info, const int32_t *n_tiles, int32_t wt,
                       int32_t mirror, const int32_t *pos, int64_t n, const float *addend, float *zp, float *out,
                       ts_stream_t stream);
/* half storage (torch.autocast): feat / zp / out / addend IEEE half, w = the half weight [K, C_in, C_out] as stored */
int ts_conv_class_gemm_f16(const void *feat, int32_t c_red, const void *w, int32_t K, int32_t groups, int32_t c_out,
                           const int32_t *src, int64_t m_pad, const int32_t *tile_info, const int32_t *n_tiles, int32_t wt,
                           int32_t mirror, const int32_t *rows, void *zp, ts_stream_t stream);
int ts_conv_class_conv_f16(const void *feat, int32_t c_red, const void *w, int32_t K, int32_t groups, int32_t c_out,
                           const int32_t *src, int64_t m_pad, const int32_t *tile_info, const int32_t *n_tiles, int32_t wt,
                           int32_t mirror, const int32_t *pos, int64_t n, const void *addend, void *zp, void *out,
                           ts_stream_t stream);

/* Diagnostic: while `stamps` (device memory, 16 x uint64 per workgroup, `capacity` workgroups) is set, the 96- / 128-
 * column fp32 pair GEMMs run an instrumented instantiation whose workgroups leave shader-clock stamps of their phases
 * (tools/phase_probe.py); NULL switches back to the product kernels. */
void ts_debug_phase_stamps(unsigned long long *stamps, int64_t capacity);

/* ------------------------------------------------------------------------ */
/* 4. Host-side data stage moved on device                                   */
/* ------------------------------------------------------------------------ */

/* Dataset voxelisation, first half (pcseg/data/dataset/semantickitti/semantickitti_voxel.py:119-120,
 * semantickitti_voxel_ms.py:127-130,151): c = int32(round_half_even(p / voxel_size)) in float32, then
 * c -= shift.  points [n, point_stride] float32 (x, y, z first); batch_idx [n] int32 or NULL (= 0).
 * shift_in [n_batch,3] given: subtract it.  shift_in NULL: the per-batch minimum is computed into
 * mins_out [n_batch,3] and subtracted (pc_ -= pc_.min(0)).  out_coords [n,4] = (x, y, z, b). */
int ts_voxel_coords(const float *points, int64_t n, int32_t point_stride, float voxel_size,
                    const int32_t *batch_idx, int32_t n_batch, const int32_t *shift_in,
                    int32_t *mins_out, int32_t *out_coords, ts_stream_t stream);

/* Dataset voxelisation, second half: sparse_quantize(coords, return_index, return_inverse)
 * (torchsparse utils/quantize.py:9-46 == np.unique of the ravel key).  coords [n,4] int32 (x,y,z,b):
 *   out_index   [<=n] : for voxel v (ascending (b,x,y,z)) the index of its FIRST point in input order;
 *   out_inverse [n]   : voxel id of every point (global over the batch);
 *   *out_count        : number of voxels (-1 if a coordinate is outside [-2^17, 2^17) or b >= 1024). */
/* out [n_seg, 3] = per-segment minimum of (x, y, z) of points [n, point_stride] whose segment index is seg[i] (int64, 0 ..
 * n_seg - 1 <= 63): the current scan's minimum every fused cloud of a batch is clamped to (semantickitti_voxel_ms.py:121-124),
 * all samples in one launch */
int ts_segment_min3(const float *points, int64_t n, int32_t point_stride, const int64_t *seg, int32_t n_seg, float *out,
                    ts_stream_t stream);
/* The batched data stage (csrc/stage.hip, taseg_amd/data/stage.py::voxelize_batch_ms): the per-point decisions and the layout of
 * the fused clouds of a WHOLE batch (semantickitti_ms.py:303-308, semantickitti_voxel_ms.py:121-212; nuscenes_ms.py:320-328).
 *   ts_stage_keep_flags   keep[i] = pre_keep[i] (optional) AND table[scan_idx[i]][cls[i] (neg_col where cls[i] < 0)] AND
 *                         xyz(i) >= lo[sample] ; sample[i] = sample_of_scan[scan_idx[i]]  (table [n_scans, table_cols] bytes)
 *   ts_stage_layout       the fused clouds sample-major, current scan first: pts [n_cur + n_kept, f], lab, sample (int64 and
 *                         int32), is_cur, from the current points (cur_b ascending, cur_start [B + 1] their cumulative counts), the
 *                         history rows and the ascending indices idx [n_kept] of the kept ones (kept_start [B + 1] cumulative)
 *   ts_stage_split_voxels after ts_sparse_quantize on the batch: vox [m, 4] = coords4[index], start [B + 1] first voxel of every
 *                         sample, offset [B] cumulative voxel counts, inverse_local[i] = inverse[i] - start[row_sample[i]] */
int ts_stage_keep_flags(const float *points, int64_t n, int32_t point_stride, const uint8_t *pre_keep, const int32_t *scan_idx,
                        const int64_t *cls, const uint8_t *table, int32_t n_scans, int32_t table_cols, int32_t neg_col,
                        const int64_t *sample_of_scan, const float *lo, int32_t n_samples, uint8_t *keep, int64_t *sample,
                        ts_stream_t stream);
int ts_stage_layout(const float *cur, const int64_t *cur_lab, const int64_t *cur_b, int64_t n_cur, const float *hist,
                    const int64_t *hist_lab, const int64_t *hist_b, const int64_t *idx, int64_t n_kept, int32_t f,
                    const int64_t *cur_start, const int64_t *kept_start, float *pts, int64_t *lab, int64_t *sample, int32_t *sample32,
                    uint8_t *is_cur, ts_stream_t stream);
int ts_stage_split_voxels(const int32_t *coords4, const int32_t *index, int64_t m, const int32_t *inverse,
                          const int64_t *row_sample, int64_t n, int32_t n_samples, int32_t *vox, int64_t *start, int32_t *offset,
                          int64_t *inverse_local, ts_stream_t stream);
/* Point augmentation of the data stage (tools/utils/common/seg_utils.py:102-166 aug_points_ms, :43-100 aug_points; applied by
 * semantickitti_voxel_ms.py:90-119 before the clamp and both voxelisations): the xyz columns of points [n, point_stride] float32,
 * the other columns passed through; sample_idx [n] int32 or NULL (= 0) selects one of n_samples parameter records of
 * TS_AUG_RECORD doubles { c, s, scale, tx, ty, tz, bits, flip } (c = cos theta, s = sin theta from the host):
 *   bit 1   X = x*c + y*(-s) ; Y = x*s + y*c ; Z = z        (np.dot(xyz, rot_mat): dgemm's fused-multiply-add chain in k
 *                                                             order, X = fma(z, 0, fma(y, -s, x*c)) ... as ts_fuse_sweeps)
 *   bit 2   (X, Y, Z) *= scale                               (bit 16 too: in float32, numpy's float32 array * Python float when
 *                                                             the cloud has not been rotated into float64 before)
 *   bit 4   flip 1: X = -X ; 2: Y = -Y ; 3: both
 *   bit 8   (X, Y, Z) += (tx, ty, tz)
 * in float64 with ONE rounding to float32 at the end; a step whose bit is clear is skipped, a record without bits returns the
 * input bit for bit.  out == points (in place) or a non-overlapping [n, point_stride] array. */
#define TS_AUG_RECORD 8
int ts_stage_augment(const float *points, int64_t n, int32_t point_stride, const int32_t *sample_idx, const double *params,
                     int32_t n_samples, float *out, ts_stream_t stream);
/* Scan mixing of the training recipe (csrc/mix.hip; taseg_amd/data/mix.py draws the parameters): PolarMix
 * (semantickitti_ms.py:188-237 calling PolarMix_semantickitti.py:10-96; nuscenes_ms.py:168-214 calling PolarMix_nuscenes.py) and
 * LaserMix (semantickitti_ms.py:153-186 calling LaserMix_semantickitti.py:11-114 `lasermix_aug`; :116-219 `lasermix_aug_`) as a
 * stable partition of the rows of two clouds.  n_jobs jobs (samples), their rows concatenated job-major in points [n_rows,
 * point_stride >= 3] / labels [n_rows], cloud 1 (n1 rows) before cloud 2 (n2 rows); every job owns ceil((n1 + n2) / 256) blocks
 * of the grid (n_blocks in all).  keep [n_rows] bytes or NULL: a row whose byte is 0 does not exist (the class-step filter of the
 * fused clouds, semantickitti_ms.py:143).  records [n_jobs, TS_MIX_RECORD] doubles:
 *   0 kind (0 none: cloud 1 as it is, 1 LaserMix, 2 PolarMix)   1 alpha  2 beta  3 swap  4 paste   (PolarMix_semantickitti.py:61-91)
 *   5 .. 8 cos / sin of Omega[0], cos / sin of Omega[1]          9 rotated copies carry all columns after xyz (SemanticKITTI
 *   :54) or only column 3, zeros behind it (PolarMix_nuscenes.py:53)
 *   10 inclination in degrees (lasermix_aug_)  11 number of band thresholds  12 .. 16 the thresholds, descending
 *   17 n1  18 n2  19 first row  20 instance classes  21 first block  22 blocks
 * classes [n_jobs, TS_MIX_MAX_CLASSES] int32: the job's instance classes in list order (PolarMix_semantickitti.py:37).
 * Rules: yaw = (float)(-atan2((double)y, (double)x)); in the sector iff swap and (float)alpha < yaw < (float)beta.  PolarMix writes
 * cloud 1 without its sector rows | cloud 2's sector rows | cloud 2's instance rows by class, file order within a class | that
 * block rotated by Omega[0] | by Omega[1] (np.dot with [[c, s, 0], [-s, c, 0], [0, 0, 1]]: the ROTATE arithmetic of
 * ts_stage_augment).  LaserMix: inc = atan2(z, sqrt(x*x + y*y)) in float64 (/ pi * 180 under field 10), band = number of
 * thresholds with inc <= threshold; bands 0, 2, 4 come from cloud 1, bands 1, 3, 5 from cloud 2, written in band order.
 * out [capacity, point_stride], out_labels, out_job (the job of every row): the jobs' results one after the other, job j at rows
 * sum(totals[0 .. j)) ... ; totals [n_jobs] int64 the rows of every job (read them once per batch).  capacity bounds every store:
 * n1 + n2 * (swap + 3 * paste) per PolarMix job, n1 + n2 per LaserMix job.  No atomics: the same bits every run. */
#define TS_MIX_RECORD 24
#define TS_MIX_MAX_CLASSES 16
size_t ts_stage_mix_workspace_bytes(int64_t n_rows, int64_t n_blocks, int32_t n_jobs);
int ts_stage_mix(const float *points, int64_t n_rows, int32_t point_stride, const int64_t *labels, const uint8_t *keep,
                 const double *records, const int32_t *classes, int32_t n_jobs, int64_t n_blocks, float *out, int64_t *out_labels,
                 int32_t *out_job, int64_t capacity, int64_t *totals, void *ws, size_t ws_bytes, ts_stream_t stream);
/* The clamp of the fused clouds as one stable compaction for a whole batch (csrc/compact.hip): nuscenes_voxel_ms.py:122-125 /
 * semantickitti_voxel_ms.py:121-124, `point_ms[(point_ms[:, :3] >= point[:, :3].min(0)).all(1)]`, where the current scan is no
 * prefix of the fused cloud (after ts_stage_mix) and ts_stage_keep_flags / ts_stage_layout do not apply.  points [n, point_stride
 * >= 3] float32, labels [n] int64, sample [n] int32 ASCENDING (the out_job of ts_stage_mix), lo [n_samples, 3] float32 (the
 * minimum of every sample's single-frame cloud, ts_segment_min3), 1 <= n_samples <= TS_CLAMP_MAX_SAMPLES.  Row i survives iff
 * x >= lo[s][0] && y >= lo[s][1] && z >= lo[s][2] with s = sample[i] - a NaN on either side fails, as numpy's `>=`; a row whose
 * sample is outside [0, n_samples) does not survive.  out [n, point_stride], out_labels [n], out_sample [n] int64, out_sample32
 * [n] int32: the surviving rows in input order (the rows behind them are not written); counts [n_samples] int64 the survivors of
 * every sample - the caller reads them once per batch, the output holds sum(counts) rows.  Three launches (counts per block of 256
 * rows from wave ballots, the shared scan, the scatter by rank); no atomics: the same bits every run. */
#define TS_CLAMP_MAX_SAMPLES 64
size_t ts_stage_clamp_compact_workspace_bytes(int64_t n, int32_t n_samples);
int ts_stage_clamp_compact(const float *points, int64_t n, int32_t point_stride, const int64_t *labels, const int32_t *sample,
                           const float *lo, int32_t n_samples, float *out, int64_t *out_labels, int64_t *out_sample,
                           int32_t *out_sample32, int64_t *counts, void *ws, size_t ws_bytes, ts_stream_t stream);
/* Both fused clouds of the mask-distillation recipe's batch from ONE pass over the pose-fused, un-filtered history
 * (csrc/kd_stage.hip; taseg_amd/data/kd.py): semantickitti_ms_kd.py:141-147 - the student's cloud `raw_data_ms` (history filtered
 * by the pseudo labels under FLEXIBLE_STEPS) and the teacher's `raw_data_ms_gt` (the same history filtered by the annotations under
 * FLEXIBLE_STEPS_GT), the masks of :332-344, `append_time_flag` :280-284 - and semantickitti_voxel_ms_kd.py:125-132, both clouds
 * clamped to the current scan's minimum.  It replaces ts_stage_keep_flags -> nonzero -> searchsorted -> ts_stage_layout, run once
 * per cloud.  cur [n_cur, cur_stride >= 4] float32 the current scans of all samples one after the other (columns 0 .. 3 are
 * read), cur_labels [n_cur] int64, cur_start [n_samples + 1] int64 their cumulative row counts; hist [n_hist, 4] float32 the
 * history rows, their samples ASCENDING, hist_labels [n_hist] int64, scan_idx [n_hist] int32; cls_a / cls_b [n_hist] int64 the
 * class column of either rule (negative: column neg_col); table_a / table_b [n_scans, table_cols] bytes; sample_of_scan [n_scans]
 * int64; lo [n_samples, 3] float32 (ts_segment_min3 of the current scans), 1 <= n_samples <= TS_STAGE_PAIR_MAX_SAMPLES.
 * History row i belongs to cloud A iff table_a[scan_idx[i]][cls_a[i]] != 0 and x >= lo[s][0] && y >= lo[s][1] && z >= lo[s][2]
 * with s = sample_of_scan[scan_idx[i]] - a NaN on either side fails, as numpy's `>=`; a row whose sample is outside [0,
 * n_samples) belongs to neither - and to cloud B iff the same holds with table_b / cls_b.
 * out_a / out_b [capacity, 5] float32: the clouds sample-major, each sample's current scan first, its kept history behind it in
 * input order; column 4 is 1 on a current row and 0 on a history row.  Cloud A carries labels and the is-current byte
 * (`point_mask`), both carry the sample index as int64 and int32.  counts [n_samples, 3] int64: kept history rows of A, of B, and
 * the history rows that pass B's step rule BEFORE the clamp (the reference's `num_points_ms_gt` is never updated after it,
 * semantickitti_voxel_ms_kd.py:88, :132) - the caller reads them once per batch; cloud A holds n_cur + sum(counts[:, 0]) rows,
 * cloud B n_cur + sum(counts[:, 1]), the rows behind them are not written.  capacity >= n_cur + n_hist bounds every store.  Three
 * launches (counts per block of 256 rows from wave ballots; one block per cloud scanning the block counts beside a few summing
 * the per-sample counts; the scatter by rank of history and current rows);
 * no atomics: the same bits every run. */
#define TS_STAGE_PAIR_MAX_SAMPLES 64
size_t ts_stage_layout_pair_workspace_bytes(int64_t n_hist, int32_t n_samples);
int ts_stage_layout_pair(const float *cur, int64_t n_cur, int32_t cur_stride, const int64_t *cur_labels, const int64_t *cur_start,
                         const float *hist, int64_t n_hist, const int64_t *hist_labels, const int32_t *scan_idx,
                         const int64_t *cls_a, const int64_t *cls_b, const uint8_t *table_a, const uint8_t *table_b,
                         int32_t n_scans, int32_t table_cols, int32_t neg_col, const int64_t *sample_of_scan, const float *lo,
                         int32_t n_samples, float *out_a, int64_t *out_labels_a, int64_t *out_sample_a, int32_t *out_sample32_a,
                         uint8_t *out_is_cur_a, float *out_b, int64_t *out_sample_b, int32_t *out_sample32_b, int64_t capacity,
                         int64_t *counts, void *ws, size_t ws_bytes, ts_stream_t stream);
/* Moving-object augmentation of the SMSA recipe (csrc/moving.hip; taseg_amd/data/moving.py draws the parameters):
 * semantickitti_ms_ms.py:305-351 `static2moving` and :353-384 `moving2static`, called at :152-163 for the sample and at :198-207 /
 * :248-257 for its mix partner, on the current scan and the pose-fused UN-FILTERED history rows, before the class-step mask
 * (:165), the mix and the augmentation.  Rows of a call, for any number of clouds (samples and partners): points [n_rows,
 * point_stride >= 2], the n_cur current rows of all clouds first, the history rows behind them; labels [n_rows] the FULL uint32
 * labels (instance << 16 | raw class) as int64; cloud [n_rows] int32; delta [n_rows] int32 the frame offset of a history row
 * (time_flag_ms, -1 = the previous frame; not read for current rows).
 * ts_stage_moving_stats: cand [>= cap] int64 = the candidates, i.e. the distinct full labels of a cloud's current rows with raw
 * class 18, 20, 253 or 255 (np.unique at :306-307 / :354-355), ascending per cloud, the clouds' tables one after the other;
 * cand_start [n_clouds + 1] int32 on the DEVICE (nothing about the tables is read on the host; at most cap <=
 * TS_MOVING_MAX_CANDIDATES are used).  Per candidate k:
 *   counts [cap, 3] int32   rows of the instance in the current scan (:362), in the history (:315), at delta -1 (:368)
 *   stats  [cap, TS_MOVING_STATS] float32
 *          0 .. 3  min x, max x, min y, max y over the history rows (:320; +inf / -inf without one)
 *          4       mean of the history y (:321)          5, 6  mean x, y of the history rows at delta -1 (:368-370)
 *          7, 8    mean x, y of the current rows (:367-370)
 * Every mean is numpy's `column.mean()` of a strided float32 column over the instance's rows IN ROW ORDER: pieces of 8192 terms,
 * each summed by numpy's pairwise rule in float32 (fewer than 8 terms sequentially from 0; up to 128 eight running sums over groups
 * of 8 combined ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), the remainder sequentially; above, split at n / 2 rounded down
 * to a multiple of 8), the pieces' sums added in order to 0, / (float)n; 0.f / 0.f = NaN without a row, as numpy.
 * matched [1] int64: the rows that belong to a candidate; when it exceeds cap_rows (the capacity of the ordered list the means are
 * taken from) the means are NaN and the caller must enlarge cap_rows.  Counts and min / max use integer atomics (exact); no float
 * atomics: the same bits every run.
 * ts_stage_moving_apply (in place on `points`, a copy the caller owns): rec_labels [R] int64 the full labels of the instances
 * that move, ascending per cloud, rec_start [n_clouds + 1] int32, records [R, TS_MOVING_RECORD] doubles:
 *   0 kind   1 static2moving along x (:320-336)  2 static2moving along y (:338-344)  3 moving2static (:367-377)  0 nothing
 *   1 centre shift, signed (-center_shift for center_y > 4, +center_shift for center_y < -2, 0 none): y = y + (float)field
 *     on the history and the current rows (kind 1)
 *   2 shift_x / shift_y of kinds 1 / 2 (double): history x (kind 1) or y (kind 2) += (float)((double)delta * field)
 *   3, 4 shift_x, shift_y of kind 3 (float32 values): history x += (float)delta * shift_x, y likewise, float32 products
 *   5 the raw class the instance's rows get (258 / 259, :346-349; 31 / 32, :379-382)
 * out_labels [n_rows] int64 = lut[raw class after the rewrite] for EVERY row (lut: 260 entries, the 26-class map; 0 for a raw
 * class past the table). */
#define TS_MOVING_STATS 9
#define TS_MOVING_RECORD 8
#define TS_MOVING_MAX_CANDIDATES 1024
size_t ts_stage_moving_workspace_bytes(int64_t n_rows, int32_t cap, int64_t cap_rows);
int ts_stage_moving_stats(const float *points, int64_t n_rows, int64_t n_cur, int32_t point_stride, const int64_t *labels,
                          const int32_t *cloud, const int32_t *delta, const int64_t *cand, const int32_t *cand_start,
                          int32_t n_clouds, int32_t cap, int64_t cap_rows, int32_t *counts, float *stats, int64_t *matched, void *ws,
                          size_t ws_bytes, ts_stream_t stream);
int ts_stage_moving_apply(float *points, int64_t n_rows, int64_t n_cur, int32_t point_stride, const int64_t *labels,
                          const int32_t *cloud, const int32_t *delta, const int64_t *rec_labels, const int32_t *rec_start,
                          int32_t n_clouds, const double *records, const int64_t *lut, int64_t *out_labels, ts_stream_t stream);
size_t ts_quantize_workspace_bytes(int64_t n);
int ts_sparse_quantize(const int32_t *coords, int64_t n, int32_t *out_index, int32_t *out_inverse,
                       int32_t *out_count, void *ws, size_t ws_bytes, ts_stream_t stream);
/* The cylinder data stage (csrc/cylinder_stage.hip; taseg_amd/data/cylinder.py): pcseg/data/dataset/semantickitti/
 * semantickitti_cylinder.py:104-219 for a whole batch - two passes around one stable radix sort.
 * ts_cylinder_cells, one lane per row of points [n, point_stride >= 4] float32 (x, y, z, intensity, ...); sample_idx [n] int32 or
 * NULL (= 0); space = 9 doubles ON THE HOST { min[3], max[3], interval[3] }, interval = (max - min) / (grid - 1) formed in float64
 * by the caller as :149-151 forms it:
 *   rho = sqrt(x*x + y*y) in float32 (:20) ; phi = (float)atan2((double)y, (double)x) ; deg = phi / float32(pi) * 180 in float32
 *   (:21, :145: numpy keeps a float32 array float32 against a Python float).  phi is the ONE difference from the reference: numpy's
 *   float32 arctan2 is not correctly rounded, this is the float64 value rounded once, as ts_stage_mix takes its yaw.
 *   cell = (int)floor((clip(pol, min, max) - min) / interval) in float64 (:153): a value outside the space lands in the first or
 *   last cell of its axis, nothing is dropped.
 *   centre = (float)(((float)cell + 0.5f) * interval + min), product and sum in float64 (:156, :158)
 * cells [n, 4] int32 (x, y, z, sample; 16-byte aligned: the sort's input), point_coord [n, 4] int64 the same (32-byte aligned),
 * point_feature [n, 5 + point_stride] float32 = { centre[3], rho, deg, z, x, y, columns 3 .. } (:160).  A row with a non-finite
 * x, y or z gets cell 0 and stores TS_CYL_FLAG_NONFINITE to flags[0] (the reference would hand astype(int) a NaN).
 * ts_cylinder_voxels, :32-45 voxelize_with_label and the per-sample pieces of collate_batch (:176-219) for the batch: the 64-bit
 * key of ts_sparse_quantize carries the sample, so ONE stable sort orders every sample's voxels as torchsparse's sparse_quantize
 * does (ascending x, y, z) with a voxel's rows in input order; then head flags, their scan, the samples' first ranks, a scatter and
 * the vote.  labels [n] int64.  out_index [n] int32: out_index[v] = the FIRST row of voxel v (np.unique's return_index), voxels
 * sample-major; out_inverse [n] int64: the rank of the row's voxel INSIDE its sample (collate_batch concatenates the inverse maps
 * without an offset); voxel_label [n] int64: the class with the most rows among the voxel's rows whose label != ignore_label,
 * the LOWEST class on a tie (np.argmax), class 0 for a voxel of ignored rows only; the first m entries of either are written.
 * counts [n_samples + 1] int32: the voxels of every sample, then m.  flags [TS_CYL_FLAG_WORDS] int32, zeroed by the caller before
 * ts_cylinder_cells: flags[1] = TS_CYL_FLAG_LABEL where a label is neither ignore_label nor in [0, num_classes) (an IndexError
 * in the reference), flags[2] = TS_CYL_FLAG_RANGE where a sample index is outside [0, 1024).  The caller reads counts and flags
 * in one copy.  The vote gives every voxel 32 lanes, lane c counting class c in an integer register over the voxel's run of the
 * sorted order (1 <= num_classes <= 32): no [m, C] table, no atomics, no float arithmetic - the same bits every run. */
#define TS_CYL_FLAG_WORDS 3
#define TS_CYL_FLAG_NONFINITE 1
#define TS_CYL_FLAG_LABEL 2
#define TS_CYL_FLAG_RANGE 4
int ts_cylinder_cells(const float *points, int64_t n, int32_t point_stride, const int32_t *sample_idx, const double *space,
                      int32_t *cells, int64_t *point_coord, float *point_feature, int32_t *flags, ts_stream_t stream);
size_t ts_cylinder_voxels_workspace_bytes(int64_t n, int32_t n_samples);
int ts_cylinder_voxels(const int32_t *cells, const int64_t *labels, int64_t n, int32_t n_samples, int32_t num_classes,
                       int64_t ignore_label, int32_t *out_index, int64_t *out_inverse, int64_t *voxel_label, int32_t *counts,
                       int32_t *flags, void *ws, size_t ws_bytes, ts_stream_t stream);

/* fuse_multi_scan (pcseg/data/dataset/semantickitti/semantickitti_ms.py:403-417):
 * p' = ((p . R_t^T + t_t) - t_0) . R_0 for one history scan, in float32 with the
 * reference's summation order; points [n,4] (x,y,z,intensity), pose/pose0 are
 * 4x4 row-major float32 on the device; out [n,4]. */
int ts_fuse_scan(const float *points, int64_t n, const float *pose0, const float *pose,
                 float *out, ts_stream_t stream);
/* The same transform for the concatenated history scans of a sample: point i uses poses[scan_idx[i]]
 * (poses [n_scans, 4, 4] row-major).  Bit-identical to n_scans calls of ts_fuse_scan. */
int ts_fuse_scans(const float *points, const int32_t *scan_idx, int64_t n, const float *pose0, const float *poses,
                  int32_t n_scans, float *out, ts_stream_t stream);
/* the same for the history scans of a whole BATCH of samples: pose0s [n_scans, 4, 4] = the current-frame pose of the sample the
 * scan belongs to (one launch per batch instead of one per sample) */
int ts_fuse_scans_batch(const float *points, const int32_t *scan_idx, int64_t n, const float *pose0s, const float *poses,
                        int32_t n_scans, float *out, ts_stream_t stream);

/* nuScenes multi-scan fuse (pcseg/data/dataset/nuscenes/nuscenes_ms.py:280-318 per selected sweep, :348-373
 * transform_point): for point i of the concatenated sweeps, with s = sweep_idx[i] and params[s] = 28 doubles
 *   { A[9], a[3], flagA, B[9], b[3], flagB, dt, pad }:
 *   keep[i] = !(|x| < 1.0 && |y| < 1.5) on the RAW coordinates          (ego-box filter, :288 / :306)
 *   flagA:  p = f32(p . A^T); p = f32(p + a)                            (sweep -> its keyframe's lidar frame, :307-309)
 *   flagB:  p = f32(p . B + b)                                          (-> the current lidar frame, transform_point)
 *   out[i] = (p, intensity, f32(dt))                                    (:289 / :310)
 * Arithmetic in float64 with the fused-multiply-add chain numpy's matmul (dgemm) performs, rounded to float32 where
 * the reference stores into its float32 array.  points / out [n,5] float32; keep [n] uint8. */
int ts_fuse_sweeps(const float *points, const int32_t *sweep_idx, int64_t n, const double *params, int32_t n_sweeps,
                   float *out, uint8_t *keep, ts_stream_t stream);

/* TIAF camera projection of one scan (pcseg/data/dataset/semantickitti/semantickitti_ms_mm.py:411-461 get_fov_points,
 * the per-point part): for point i = (x, y, z, .)
 *   uvz = P . (x, y, z, 1)            P = P2 . Tr, 3x4 row-major float64; float64 FMA chain in k order (numpy's dgemm)
 *   keep[i] = x > 0  &&  0 < u < img_w  &&  0 < v < img_h  (u = uvz0 / uvz2, v = uvz1 / uvz2, float64)
 *                    &&  (int)v < crop_h  &&  (int)u < crop_w
 *   pix[i]  = ( float((int)v) + row_offset , float((int)u) )        row_offset = crop_h * frame index in the image stack
 * points [n,4] float32; pix [n,2] float32 (undefined where keep == 0); keep [n] uint8. */
int ts_project_fov(const float *points, int64_t n, const double *proj, int32_t img_w, int32_t img_h, int32_t crop_h,
                   int32_t crop_w, float row_offset, float *pix, uint8_t *keep, ts_stream_t stream);

/* nuScenes TIAF camera projection (pcseg/data/dataset/nuscenes/nuscenes_ms_mm.py:349-398 get_fov_points, the per-point
 * part): lidar frame -> ego -> global -> camera ego -> camera through the calibrated-sensor and ego-pose records of the lidar
 * and camera sample_data entries, pinhole projection with nuscenes-devkit's view_points, half-resolution pixel.
 *   cam[57] float64 = { M1[9] t1[3]  M2[9] t2[3]  t3[3] M3[9]  t4[3] M4[9]  K[9] }   (row-major 3x3; M3 / M4 = the TRANSPOSED
 *                       rotations of the camera's ego pose / calibrated sensor, as the reference applies them)
 *   p = M1 x + t1;  p = M2 p + t2;  p = M3 (p - t3);  p = M4 (p - t4)        every product an FMA chain in k order (dgemm)
 *   (u, v) = f32( (K p)[0,1] / (K p)[2] )
 *   keep[i] = p_z > 0  &&  0 < u < img_w  &&  0 < v < img_h  &&  ((int)v >> 1) >= crop_top
 *   pix[i]  = ( float(((int)v >> 1) - crop_top) + row_offset , float((int)u >> 1) )    row_offset = HEIGHT * image index
 * points [n,4] float32; pix [n,2] float32 (undefined where keep == 0); keep [n] uint8. */
int ts_project_cam(const float *points, int64_t n, const double *cam, int32_t img_w, int32_t img_h, int32_t crop_top,
                   float row_offset, float *pix, uint8_t *keep, ts_stream_t stream);

/* The camera side of the TIAF stage for a whole batch (csrc/tiaf_stage.hip; taseg_amd/data/tiaf.py).
 *
 * ts_tiaf_image_stack: the camera frames of one call straight into the planes the model reads
 * (semantickitti_ms_mm.py:428-452 `get_fov_points`, the image part - `image[..., [2,1,0]] / 255.`, IMAGE_FLIP :436-440 `np.fliplr` of
 * image and semantic map, the top-left crop with zero padding :443-452 - and semantickitti_voxel_ms_mm.py:245-248, the NCHW
 * permutation of collate_batch).  images / semantic / img_h / img_w / flips are HOST arrays of n_frames <= TS_TIAF_IMAGE_FRAMES
 * entries: device pointers to uint8 [h, w, 3] RGB images and (semantic may be NULL, so may an entry) float32 [h, w, 1] maps, their
 * sizes, a flip byte each (flips NULL: none); they reach the kernel BY VALUE in its argument block - nothing is uploaded.  table
 * [256] float32 on the device: i / 255 as the HOST rounds it (the device's division need not round as numpy's).  For frame t,
 * r < crop_h, q < crop_w, c < 3:
 *   out_image   [first + t][c][r][q] = r < min(crop_h, h) && q < min(crop_w, w) ? table[img[r][flip ? w - 1 - q : q][2 - c]] : 0
 *   out_semantic[first + t][0][r][q] = the semantic map at the same source pixel, or 0
 * so the flip acts on the full-width image BEFORE the crop: with w > crop_w a flipped frame shows the image's right part.
 * out_image [n_total, 3, crop_h, crop_w], out_semantic [n_total, 1, crop_h, crop_w] (or NULL) float32, first + n_frames <= n_total.
 * One launch; every output element of the frames is written exactly once (no fill pass); 16-byte stores and dword loads of the
 * image when crop_w % 4 == 0 and the outputs are 16-byte aligned; any h, w, crop_h, crop_w, any image alignment otherwise.
 *
 * ts_tiaf_fov_cloud: the FOV cloud of a whole batch as one stable compaction.  points [n_points, 4] float32: the rows of every
 * camera frame of every sample, sample-major, inside a sample NEWEST frame first (`raw_data_fov_ms.insert(0, ...)`, :369).  The
 * call works on n_rows VIRTUAL rows: frame [n_rows] int32 ASCENDING names the record of every virtual row, and virtual row i of
 * frame f reads point row records[f].src + (i - records[f].first) - frames of several samples (the votes of a TTA batch) may
 * read the same point rows.  records [n_frames <= TS_TIAF_MAX_FRAMES] TsTiafFrame on the device (their samples ascending), aug
 * [n_samples, TS_AUG_RECORD] doubles or NULL, lo [n_samples, 3] float32 - the minimum of the sample's AUGMENTED single-frame
 * cloud - or NULL, 1 <= n_samples <= TS_TIAF_MAX_SAMPLES.  Per virtual row, in this order:
 *   1  the projection and frustum test of ts_project_fov with the record's proj, img_w, img_h            (:416-426)
 *   2  col = flip ? img_w - 1 - col : col                                                                (:441)
 *   3  row < crop_h && col < crop_w, on the flipped column                                                (:454)
 *   4  fov_dist > 0: sqrt(x * x + y * y) <= fov_dist on the un-fused point, float32 multiply, add, sqrt   (:365-367)
 *   5  TS_TIAF_FUSE: the pose fuse of ts_fuse_scan with the record's pose0, pose                          (:368)
 *   6  aug: the arithmetic of ts_stage_augment on xyz with the sample's record    (semantickitti_voxel_ms_mm.py:92-124)
 *   7  lo: x >= lo[s][0] && y >= lo[s][1] && z >= lo[s][2], NaN on either side fails                      (... :132-133)
 * A row whose sample or point row is out of range does not survive.  out [capacity, 6] float32 = (x, y, z, intensity, row +
 * row_offset, col) of the survivors in input order, out_sample int64 / out_sample32 int32 their samples (the rows behind the
 * survivors are not written); counts [n_samples] int64 the survivors of every sample - the caller's one host read.  capacity >=
 * n_rows bounds every store.  Three launches (counts per block of 256 rows from wave ballots, the shared scan, the scatter by
 * rank - pass 3 recomputes the decision of pass 1 on the same bits); no atomics: the same bits every run. */
#define TS_TIAF_IMAGE_FRAMES 16
#define TS_TIAF_MAX_SAMPLES 64
#define TS_TIAF_MAX_FRAMES 1024
#define TS_TIAF_FLIP 1
#define TS_TIAF_FUSE 2
typedef struct TsTiafFrame {
  double proj[12];         /* P2 . Tr of the frame's sequence, 3 x 4 row-major */
  float pose0[16];         /* the pose of the sample's current frame, 4 x 4 row-major */
  float pose[16];          /* the frame's own pose */
  float row_offset;        /* crop_h * position of the frame in its sample's image stack */
  float fov_dist;          /* <= 0: off */
  int32_t sample;
  int32_t img_w, img_h;
  int32_t flags;           /* TS_TIAF_FLIP | TS_TIAF_FUSE */
  int32_t first;           /* the frame's first virtual row */
  int32_t src;             /* the point row it reads */
} TsTiafFrame;
int ts_tiaf_image_stack(const uint8_t *const *images, const float *const *semantic, const int32_t *img_h, const int32_t *img_w,
                        const uint8_t *flips, int32_t n_frames, const float *table, int32_t crop_h, int32_t crop_w, int64_t first,
                        int64_t n_total, float *out_image, float *out_semantic, ts_stream_t stream);
size_t ts_tiaf_fov_cloud_workspace_bytes(int64_t n_rows, int32_t n_samples);
int ts_tiaf_fov_cloud(const float *points, int64_t n_points, const int32_t *frame, int64_t n_rows, const TsTiafFrame *records,
                      int32_t n_frames, const double *aug, const float *lo, int32_t n_samples, int32_t crop_h, int32_t crop_w,
                      float *out, int64_t *out_sample, int32_t *out_sample32, int64_t capacity, int64_t *counts, void *ws,
                      size_t ws_bytes, ts_stream_t stream);

/* The camera side of the nuScenes TIAF stage for a whole batch (csrc/nusc_tiaf_stage.hip; taseg_amd/data/nuscenes_tiaf.py).
 *
 * ts_nusc_fov_cloud: the FOV cloud of a whole batch as one stable compaction over VIRTUAL rows, a virtual row being a (point row,
 * camera record) pair (nuscenes_ms_mm.py:297-305, 329-398 per keyframe and view; nuscenes_voxel_ms_mm.py:92-135 per sample).
 * points [n_points, 4] float32: the clouds of the batch's image keyframes, each in ITS keyframe's lidar frame - what ONE
 * ts_fuse_sweeps call over every keyframe's interval predecessors leaves (:246-295); labels [n_points] int64; pre_keep [n_points]
 * uint8 or NULL: that call's ego-box byte.  frame [n_rows] int32 ASCENDING names the record of every virtual row, and virtual row
 * i of record f reads point row records[f].src + (i - records[f].first) - the views of a keyframe, and the votes of a TTA batch,
 * read the same point rows.  records [n_frames <= TS_TIAF_MAX_FRAMES] TsNuscCamFrame on the device (their samples ascending; inside
 * a sample keyframe-major, view-minor: the order of the reference's loops), aug [n_samples, TS_AUG_RECORD] doubles or NULL, lo
 * [n_samples, 3] float32 - the minimum of the sample's AUGMENTED single-frame cloud - or NULL, 1 <= n_samples <=
 * TS_TIAF_MAX_SAMPLES.  Per virtual row, in this order:
 *   a  pre_keep[point row] != 0                                                                            (:288 / :306)
 *   b  paint_dist > 0: sqrt(x * x + y * y) <= paint_dist, float32 multiply, add, sqrt                      (:297-300)
 *   c  the camera chain, frustum test, half-resolution pixel and top-row cut of ts_project_cam with the record's cam, img_w,
 *      img_h, crop_top                                                                                     (:349-398)
 *   d  p = f32(p . B + b) with the record's move, as ts_fuse_sweeps' flagB - ALWAYS: the current keyframe's move is the
 *      rounded identity relative_transform(current, current) gives                                         (:305)
 *   e  aug: the arithmetic of ts_stage_augment on xyz with the sample's record          (nuscenes_voxel_ms_mm.py:92-125)
 *   f  lo: x >= lo[s][0] && y >= lo[s][1] && z >= lo[s][2], NaN on either side fails                       (... :133-135)
 * A row whose sample or point row is out of range does not survive.  out [capacity, 6] float32 = (x, y, z, intensity, row +
 * row_offset, col) of the survivors in input order, out_labels int64 their labels, out_sample int64 / out_sample32 int32 their
 * samples (the rows behind the survivors are not written); counts [n_samples] int64 the survivors of every sample - the caller's
 * one host read.  capacity >= n_rows bounds every store.  Three launches (counts per block of 256 rows from wave ballots, the
 * shared scan, the scatter by rank - pass 3 recomputes the decision of pass 1 on the same bits); no atomics: the same bits every
 * run.  A wave walks the records its rows name one after the other, so the 69 doubles of a record are read through a wave-uniform
 * address. */
typedef struct TsNuscCamFrame {
  double cam[57];          /* the camera chain, the layout of ts_project_cam */
  double move[12];         /* B[9] row-major, b[3]: relative_transform(current keyframe, the record's keyframe) */
  float row_offset;        /* HEIGHT * position of the image in its sample's stack */
  float paint_dist;        /* <= 0: off */
  int32_t sample;
  int32_t img_w, img_h;    /* the full-size camera image */
  int32_t crop_top;        /* rows cut from the top of the half-resolution image */
  int32_t first;           /* the record's first virtual row */
  int32_t src;             /* the point row it reads */
} TsNuscCamFrame;
size_t ts_nusc_fov_cloud_workspace_bytes(int64_t n_rows, int32_t n_samples);
int ts_nusc_fov_cloud(const float *points, const int64_t *labels, const uint8_t *pre_keep, int64_t n_points, const int32_t *frame,
                      int64_t n_rows, const TsNuscCamFrame *records, int32_t n_frames, const double *aug, const float *lo,
                      int32_t n_samples, float *out, int64_t *out_labels, int64_t *out_sample, int32_t *out_sample32,
                      int64_t capacity, int64_t *counts, void *ws, size_t ws_bytes, ts_stream_t stream);

/* BatchNorm (training) -> (+ residual) -> LeakyReLU(slope) on rows [N, C]: the range-view trunks' conv -> BN -> LeakyReLU and
 * conv -> BN -> `out += identity` -> LeakyReLU (R pcseg/model/segmentor/range/fidnet/model/semantic/fidnet.py:114-128).  The
 * ts_bn_act_train_* contract with a slope, on the same kernel family (csrc/bn.hip, the activation is a template parameter):
 *   forward   statistics of x; v = (x - mean) * invstd * weight + bias (+ residual); out = v > 0 ? v : v * slope, one rounding at a half
 *             store; mean / invstd [C] kept; running_mean / running_var / num_batches_tracked (may be NULL) updated; mask = one bit per
 *             element, set where the STORED value is > 0, in ts_bn_act_forward's layout (a byte per 16-byte chunk: 8 halves, or 4
 *             floats in the low 4 bits).  A stored 0 has taken the slope branch, as leaky_relu_backward decides it
 *   backward  g = grad_out * (bit ? 1 : slope); grad_x, grad_residual = g (may be NULL), grad_weight, grad_bias [C] (may be NULL)
 * half != 0: IEEE half rows (C % 8 == 0), else float (C % 4 == 0); C <= 1024; the mask is required; ws >= the size
 * ts_bn_train_workspace_bytes gives for c; pointers 16-byte aligned as for ts_bn_act_train_forward. */
int ts_bn_leaky_act_train_forward(const void *x, const void *residual, const float *weight, const float *bias, float *running_mean,
                                  float *running_var, int64_t *num_batches_tracked, int64_t n, int32_t c, float eps, float momentum,
                                  float slope, int32_t half, float *mean, float *invstd, void *out, uint8_t *mask, void *ws,
                                  size_t ws_bytes, ts_stream_t stream);
int ts_bn_leaky_act_train_backward(const void *grad_out, const uint8_t *mask, const void *x, const float *mean, const float *invstd,
                                   const float *weight, int64_t n, int32_t c, float slope, int32_t half, void *grad_x,
                                   void *grad_residual, float *grad_weight, float *grad_bias, void *ws, size_t ws_bytes,
                                   ts_stream_t stream);

/* The interpolation decoder of FIDNet / CENet (fidnet.py:300-311, cenet.py:233-243) on channels-last rows, one pass over the result:
 *   cat [T, H, W, Ca + Cb + 3 Cl] = concat(x [T, H, W, Ca], x1 [T, H, W, Cb], up(xk0), up(xk1), up(xk2)),  xk [T, hk[k], wk[k], Cl],
 * up = bilinear interpolation to H x W with align_corners = True, evaluated in float32 as ATen's device kernel evaluates it:
 *   scale = out > 1 ? (float)(in - 1) / (out - 1) : 0;  h1r = scale * (float)y;  h1 = (int)h1r;  h1p = h1 < in - 1;  h1lambda = h1r - h1;
 *   h0lambda = 1 - h1lambda (the same along the width);
 *   val = h0lambda * (w0lambda * v[h1][w1] + w1lambda * v[h1][w1 + w1p]) + h1lambda * (w0lambda * v[h1 + h1p][w1] + w1lambda * v[h1 + h1p][w1 + w1p])
 * every operation rounded on its own, one rounding at a half store.  res0 .. res2 [T, H, W, Cl] (may be NULL) receive the three
 * interpolated maps as well.  `tables` is what ts_fid_upcat_tables wrote for the same H, W, hk, wk (i0, lambda and the lower bounds
 * of i0 per level and axis; the size ts_fid_upcat_tables_bytes gives); hk, wk are HOST arrays of 3.
 *   backward  grad_x, grad_x1 = the slices of grad_cat; grad_xk[k] [T, hk, wk, Cl]: a coarse pixel (r, c) gathers the fine pixels of the
 *             rows [first_h[max(r - 1, 0)], first_h[r + 1]) and columns [first_w[max(c - 1, 0)], first_w[c + 1]) - no atomics, no fill.
 *             With g = grad_cat's slice (+ grad_res[k], may be NULL, one float sum), a fine pixel adds (ly[cy] * lx[cx]) * g for corner row
 *             cy = 0, 1 then corner column cx = 0, 1 where that corner is (r, c).  ORDER: fine row y goes to partial (y - y_lo) % S;
 *             a partial adds ascending y, then ascending x, then the corners, from 0; the result is partial 0 + partial 1 + ..;
 *             S = max(1, min(8, (H / hk) / 2, 256 / (Cl / V))), V = 4 (float) or 8 (half).  Two calls give the same bits.
 * half != 0: IEEE half (channel counts % 8), else float (% 4); each operand <= 1024 channels, else TS_ERR_UNSUPPORTED; 16-byte aligned. */
size_t ts_fid_upcat_tables_bytes(int32_t H, int32_t W);
int ts_fid_upcat_tables(int32_t H, int32_t W, const int32_t *hk, const int32_t *wk, void *tables, size_t tables_bytes, ts_stream_t stream);
int ts_fid_upcat_rows_forward(const void *x, const void *x1, const void *xk0, const void *xk1, const void *xk2, const void *tables,
                              int32_t T, int32_t H, int32_t W, const int32_t *hk, const int32_t *wk, int32_t Ca, int32_t Cb, int32_t Cl,
                              int32_t half, void *cat, void *res0, void *res1, void *res2, ts_stream_t stream);
int ts_fid_upcat_rows_backward(const void *grad_cat, const void *grad_res0, const void *grad_res1, const void *grad_res2,
                               const void *tables, int32_t T, int32_t H, int32_t W, const int32_t *hk, const int32_t *wk, int32_t Ca,
                               int32_t Cb, int32_t Cl, int32_t half, void *grad_x, void *grad_x1, void *grad_xk0, void *grad_xk1,
                               void *grad_xk2, ts_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TASEG_HIP_H_ */
