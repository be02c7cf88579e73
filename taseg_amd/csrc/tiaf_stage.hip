// The camera side of the TIAF data stage for a whole batch (taseg_amd/data/tiaf.py): see include/taseg_hip.h.
// Reference (numpy, one frame of one sample at a time): R/pcseg/data/dataset/semantickitti/semantickitti_ms_mm.py:407-461
// `get_fov_points` (projection, frustum test, IMAGE_FLIP :436-441, crop :443-457), :365-369 (FOV_DIST, pose fuse),
// semantickitti_voxel_ms_mm.py:92-124 (`aug_points_rgb_ms` on the FOV cloud), :132-133 (its clamp).
//
//   ts_tiaf_image_stack   up to TS_TIAF_IMAGE_FRAMES uint8 RGB frames -> the float32 NCHW planes the model reads, one launch: BGR /
//                         255 through the host's table, the flip, the top-left crop and the zero padding in the one store that
//                         writes every output element.  Frame pointers, sizes and flip bytes travel in the kernel arguments.
//   ts_tiaf_fov_cloud     projection -> flip -> crop test -> FOV_DIST -> pose fuse -> augmentation -> clamp per row, the survivors
//                         as one stable compaction: the one-cloud driver of csrc/compact.h (cp_compact) with tf_row as the row rule,
//                         one tally per sample; the projection, the pose fuse, the augmentation and the clamp inside tf_row are
//                         those of csrc/stage_rules.h.
#include "compact.h"
#include "stage_rules.h"

namespace {

// ------------------------------------------------------------------------------------------------ image stack
struct TfFrames {
  const unsigned char *img[TS_TIAF_IMAGE_FRAMES];
  const float *sem[TS_TIAF_IMAGE_FRAMES];
  int h[TS_TIAF_IMAGE_FRAMES], w[TS_TIAF_IMAGE_FRAMES];
  unsigned char flip[TS_TIAF_IMAGE_FRAMES];
};

// One lane per group of G output columns of one row of one frame (G = 4: W % 4 == 0 and 16-byte aligned planes -> four 16-byte
// stores per lane, a wave writes 1 KiB of every plane; G = 1: any W).  The source bytes of a group are 3 G neighbouring bytes,
// walked backwards under a flip.
template <int G>
__global__ __launch_bounds__(256) void tf_image_kernel(TfFrames f, const float *__restrict__ table, int H, int W, int64_t first,
                                                       float *__restrict__ out_img, float *__restrict__ out_sem) {
  const int t = blockIdx.z;
  const int r = blockIdx.y * blockDim.y + threadIdx.y;
  const int q0 = (blockIdx.x * blockDim.x + threadIdx.x) * G;
  if (r >= H || q0 >= W) return;
  const int h = f.h[t], w = f.w[t];
  const bool flip = f.flip[t] != 0;
  const unsigned char *__restrict__ src = f.img[t];
  const float *__restrict__ sem = f.sem[t];
  const int64_t plane = (int64_t)H * W;
  float *o = out_img + (first + t) * 3 * plane + (int64_t)r * W + q0;
  float v[3][G], s[G];
#pragma unroll
  for (int g = 0; g < G; ++g) v[0][g] = v[1][g] = v[2][g] = s[g] = 0.f;
  if (r < h) {
    const int cmax = min(W, w);
    const int64_t row = (int64_t)r * w;
    bool done = false;
    if (G == 4 && q0 + G <= cmax) {
      // the group's 12 source bytes lie in the four aligned dwords around them (rows of 3 w bytes start anywhere): four dword
      // loads and three byte-aligns instead of twelve byte loads - where the window stays inside the image (all but its first
      // and last group at most)
      const int c0 = flip ? w - G - q0 : q0;
      const uintptr_t at = (uintptr_t)(src + (row + c0) * 3), lo = at & ~(uintptr_t)3;
      if (lo >= (uintptr_t)src && lo + 16 <= (uintptr_t)src + (size_t)3 * h * w) {
        const uint32_t *p = reinterpret_cast<const uint32_t *>(lo);
        const uint32_t d0 = p[0], d1 = p[1], d2 = p[2], d3 = p[3], sh = (uint32_t)(at & 3);
        const uint32_t e[3] = {__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh),
                               __builtin_amdgcn_alignbyte(d3, d2, sh)};
        unsigned char bt[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) bt[k] = (unsigned char)(e[k >> 2] >> (8 * (k & 3)));
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const int px = flip ? G - 1 - g : g;          // the pixel of the group that lands in output column q0 + g
#pragma unroll
          for (int c = 0; c < 3; ++c) v[c][g] = table[bt[3 * px + 2 - c]];
        }
        if (out_sem && sem) {
#pragma unroll
          for (int g = 0; g < G; ++g) s[g] = sem[row + c0 + (flip ? G - 1 - g : g)];
        }
        done = true;
      }
    }
    if (!done) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int q = q0 + g;
        if (q < cmax) {
          const int col = flip ? w - 1 - q : q;
          const unsigned char *p = src + (row + col) * 3;
#pragma unroll
          for (int c = 0; c < 3; ++c) v[c][g] = table[p[2 - c]];
          if (out_sem && sem) s[g] = sem[row + col];
        }
      }
    }
  }
  if (G == 4) {
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<float4 *>(o + c * plane) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
    if (out_sem) *reinterpret_cast<float4 *>(out_sem + (first + t) * plane + (int64_t)r * W + q0) = make_float4(s[0], s[1], s[2], s[3]);
  } else {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if (q0 + g >= W) break;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c * plane + g] = v[c][g];
      if (out_sem) out_sem[(first + t) * plane + (int64_t)r * W + q0 + g] = s[g];
    }
  }
}

// ------------------------------------------------------------------------------------------------ FOV cloud
struct TfRule : CpRule {
  typedef float Row[6];
  const float4 *pts;
  const int *frame;
  const TsTiafFrame *rec;
  const double *aug;       // [n_samples, TS_AUG_RECORD] or NULL
  const float *lo;         // [n_samples, 3] or NULL
  float *out;              // [capacity, 6]
  int64_t n_points;
  int n_frames, crop_h, crop_w;

  __device__ __forceinline__ bool keeps(int64_t i, bool in, Row &o, int *sample) const;
  __device__ __forceinline__ void store(int64_t dst, int64_t, const Row &o) const {
    float2 *d = reinterpret_cast<float2 *>(out + dst * 6);    // rows of 24 bytes: 8-byte aligned
    d[0] = make_float2(o[0], o[1]);
    d[1] = make_float2(o[2], o[3]);
    d[2] = make_float2(o[4], o[5]);
  }
};

// Does virtual row i survive, and as which output row?  o = (x, y, z, intensity, row + row_offset, col); *sample its sample.
__device__ __forceinline__ bool tf_row(const TfRule &r, int64_t i, float (&o)[6], int *sample) {
  const int f = min(max(r.frame[i], 0), r.n_frames - 1);
  const TsTiafFrame *__restrict__ R = r.rec + f;
  const int b = R->sample;
  *sample = b;
  const int64_t srow = (int64_t)R->src + (i - (int64_t)R->first);
  if (b < 0 || b >= r.n_samples || srow < 0 || srow >= r.n_points) return false;
  const float4 p = r.pts[srow];
  // 1  ts_project_fov
  int row, col;
  if (!sr_project_fov(R->proj, p.x, p.y, p.z, R->img_w, R->img_h, row, col)) return false;
  // 2  IMAGE_FLIP (:441), 3  the crop test on the flipped column (:454)
  if (R->flags & TS_TIAF_FLIP) col = R->img_w - 1 - col;
  if (!(row < r.crop_h && col < r.crop_w)) return false;
  // 4  FOV_DIST on the un-fused x, y: float32 multiply, add, sqrt (:365-367; build.py compiles this file with -ffp-contract=off)
  if (R->fov_dist > 0.f) {
    const float radius = __fsqrt_rn(__fadd_rn(__fmul_rn(p.x, p.x), __fmul_rn(p.y, p.y)));
    if (!(radius <= R->fov_dist)) return false;
  }
  float q[3] = {p.x, p.y, p.z};
  // 5  ts_fuse_scan, 6  ts_stage_augment, 7  the clamp of ts_stage_clamp_compact
  if (R->flags & TS_TIAF_FUSE) sr_fuse_pose(R->pose, R->pose0, q[0], q[1], q[2]);
  if (r.aug) sr_augment(r.aug + (int64_t)TS_AUG_RECORD * b, q[0], q[1], q[2]);
  if (r.lo && !sr_clamp_keeps(q[0], q[1], q[2], r.lo, b)) return false;
  o[0] = q[0];
  o[1] = q[1];
  o[2] = q[2];
  o[3] = p.w;
  o[4] = __fadd_rn((float)row, R->row_offset);
  o[5] = (float)col;
  return true;
}

__device__ __forceinline__ bool TfRule::keeps(int64_t i, bool in, Row &o, int *sample) const {
  *sample = -1;
  return in && tf_row(*this, i, o, sample);
}

}  // namespace

extern "C" int ts_tiaf_image_stack(const uint8_t *const *images, const float *const *semantic, const int32_t *img_h,
                                   const int32_t *img_w, const uint8_t *flips, int32_t n_frames, const float *table, int32_t crop_h,
                                   int32_t crop_w, int64_t first, int64_t n_total, float *out_image, float *out_semantic,
                                   ts_stream_t stream) {
  TS_REQUIRE(n_frames >= 0 && n_frames <= TS_TIAF_IMAGE_FRAMES && crop_h > 0 && crop_w > 0 && first >= 0 &&
                 first + n_frames <= n_total && (int64_t)crop_h * crop_w < (int64_t)1 << 30 && crop_h <= 65535 * 4,
             TS_ERR_INVALID_ARGUMENT, "ts_tiaf_image_stack: bad sizes");
  if (n_frames == 0) return TS_OK;
  TS_REQUIRE(images && img_h && img_w && table && out_image, TS_ERR_INVALID_ARGUMENT, "ts_tiaf_image_stack: null pointer");
  TS_REQUIRE(((((uintptr_t)out_image) | ((uintptr_t)out_semantic) | ((uintptr_t)table)) & 3) == 0, TS_ERR_INVALID_ARGUMENT,
             "ts_tiaf_image_stack: table and outputs must be 4-byte aligned");
  TfFrames f;
  for (int t = 0; t < TS_TIAF_IMAGE_FRAMES; ++t) {
    const bool in = t < n_frames;
    f.img[t] = in ? images[t] : nullptr;
    f.sem[t] = in && semantic && out_semantic ? semantic[t] : nullptr;
    f.h[t] = in ? img_h[t] : 0;
    f.w[t] = in ? img_w[t] : 0;
    f.flip[t] = in && flips ? flips[t] : 0;
    if (in) {
      TS_REQUIRE(f.img[t] && f.h[t] > 0 && f.w[t] > 0 && (int64_t)f.h[t] * f.w[t] < (int64_t)1 << 30, TS_ERR_INVALID_ARGUMENT,
                 "ts_tiaf_image_stack: frame %d: null image or bad size", t);
      TS_REQUIRE((((uintptr_t)f.sem[t]) & 3) == 0, TS_ERR_INVALID_ARGUMENT, "ts_tiaf_image_stack: frame %d: semantic map not aligned", t);
    }
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(64, 4, 1);
  if ((crop_w & 3) == 0 && ((((uintptr_t)out_image) | ((uintptr_t)out_semantic)) & 15) == 0) {
    const dim3 grid((unsigned)ts_cdiv(crop_w / 4, 64), (unsigned)ts_cdiv(crop_h, 4), (unsigned)n_frames);
    tf_image_kernel<4><<<grid, block, 0, st>>>(f, table, crop_h, crop_w, first, out_image, out_semantic);
  } else {
    const dim3 grid((unsigned)ts_cdiv(crop_w, 64), (unsigned)ts_cdiv(crop_h, 4), (unsigned)n_frames);
    tf_image_kernel<1><<<grid, block, 0, st>>>(f, table, crop_h, crop_w, first, out_image, out_semantic);
  }
  TS_CHECK_LAUNCH("ts_tiaf_image_stack");
  return TS_OK;
}

extern "C" size_t ts_tiaf_fov_cloud_workspace_bytes(int64_t n_rows, int32_t n_samples) { return cp_compact_bytes(n_rows, n_samples); }

extern "C" int ts_tiaf_fov_cloud(const float *points, int64_t n_points, const int32_t *frame, int64_t n_rows,
                                 const TsTiafFrame *records, int32_t n_frames, const double *aug, const float *lo, int32_t n_samples,
                                 int32_t crop_h, int32_t crop_w, float *out, int64_t *out_sample, int32_t *out_sample32,
                                 int64_t capacity, int64_t *counts, void *ws, size_t ws_bytes, ts_stream_t stream) {
  static_assert(TS_TIAF_MAX_SAMPLES == TS_WAVE, "cp_count_kernel keeps one LDS counter per (wave, sample)");
  static_assert(sizeof(TsTiafFrame) == 256, "the frame record is 256 bytes (taseg_amd/data/tiaf.py FRAME_DTYPE)");
  TS_REQUIRE(n_points >= 0 && n_rows >= 0 && n_rows < (int64_t)1 << 30 && n_points < (int64_t)1 << 30 && n_frames >= 1 &&
                 n_frames <= TS_TIAF_MAX_FRAMES && n_samples >= 1 && n_samples <= TS_TIAF_MAX_SAMPLES && crop_h > 0 && crop_w > 0 &&
                 capacity >= n_rows,
             TS_ERR_INVALID_ARGUMENT, "ts_tiaf_fov_cloud: bad sizes");
  TS_REQUIRE(records && counts && ws && ((uintptr_t)ws & 3) == 0 && ((uintptr_t)records & 7) == 0 && ((uintptr_t)aug & 7) == 0,
             TS_ERR_INVALID_ARGUMENT, "ts_tiaf_fov_cloud: null or misaligned pointer");
  TS_REQUIRE(n_rows == 0 || (points && frame && out && out_sample && out_sample32), TS_ERR_INVALID_ARGUMENT,
             "ts_tiaf_fov_cloud: null pointer");
  TS_REQUIRE((((uintptr_t)points) & 15) == 0 && (((uintptr_t)out) & 7) == 0, TS_ERR_INVALID_ARGUMENT,
             "ts_tiaf_fov_cloud: points must be 16-byte, out 8-byte aligned");
  const TfRule r = {{n_rows, capacity, n_samples, out_sample, out_sample32}, (const float4 *)points, frame, records, aug, lo, out,
                    n_points, n_frames, crop_h, crop_w};
  return cp_compact(r, "ts_tiaf_fov_cloud", counts, ws, ws_bytes, (hipStream_t)stream);
}
