// The camera side of the nuScenes TIAF data stage for a whole batch (taseg_amd/data/nuscenes_tiaf.py): see include/taseg_hip.h.
// Reference (numpy, one view of one keyframe of one sample at a time): R/pcseg/data/dataset/nuscenes/nuscenes_ms_mm.py:297-305
// (PAINT_DIST, the move into the current lidar frame), :329-398 `get_fov_points`, nuscenes_voxel_ms_mm.py:92-125
// (`aug_points_rgb_ms` on the FOV cloud), :133-135 (its clamp).
//
//   ts_nusc_fov_cloud     ego-box byte -> PAINT_DIST -> camera chain, frustum, half-resolution pixel, top rows cut -> move ->
//                         augmentation -> clamp per virtual row, the survivors as one stable compaction: the one-cloud driver of
//                         csrc/compact.h (cp_compact) with nf_wave / nf_row as the row rule, one tally per sample; the projection, the move, the
//                         augmentation and the clamp inside nf_row are those of csrc/stage_rules.h.
//
// A record carries 69 doubles.  Read through a per-lane pointer they would occupy 138 VGPRs of every lane; the rows of a record
// are contiguous, so a wave holds one record, or a few at a boundary: nf_wave walks the wave's distinct records one after the
// other and reads each through a wave-uniform pointer - scalar loads into SGPRs.
#include "compact.h"
#include "stage_rules.h"

namespace {

struct NfRule : CpRule {
  struct Row {
    float o[5];                    // x, y, z, row + row_offset, col
    int64_t srow;                  // the point row it read: store takes the intensity and the label from there
  };
  const float4 *pts;
  const int64_t *labels;
  const unsigned char *pre_keep;   // [n_points] or NULL
  const int *frame;
  const TsNuscCamFrame *rec;
  const double *aug;               // [n_samples, TS_AUG_RECORD] or NULL
  const float *lo;                 // [n_samples, 3] or NULL
  float *out;                      // [capacity, 6]
  int64_t *out_labels;             // [capacity]
  int64_t n_points;
  int n_frames;

  __device__ __forceinline__ bool keeps(int64_t i, bool in, Row &row, int *sample) const;
  __device__ __forceinline__ void store(int64_t dst, int64_t, const Row &row) const {
    float2 *d = reinterpret_cast<float2 *>(out + dst * 6);    // rows of 24 bytes: 8-byte aligned
    d[0] = make_float2(row.o[0], row.o[1]);
    d[1] = make_float2(row.o[2], pts[row.srow].w);            // (a survivor's srow is in [0, n_points))
    d[2] = make_float2(row.o[3], row.o[4]);
    out_labels[dst] = labels[row.srow];
  }
};

typedef const __attribute__((address_space(4))) TsNuscCamFrame *NfRecord;      // a record read through scalar loads

// Does virtual row i of record *R (a wave-uniform pointer) survive, and as which output row?  o = (x, y, z, row + row_offset,
// col), *srow the point row it read - NfRule::store takes the intensity and the label from there.
__device__ __forceinline__ bool nf_row(const NfRule &r, NfRecord R, int64_t i, float (&o)[5], int64_t *srow) {
#pragma clang fp contract(off)  // (build.py compiles this file with -ffp-contract=off, as pointops.hip: __fmul_rn / __fadd_rn keep
                                // their roundings)
  const int b = R->sample;
  const int64_t s = (int64_t)R->src + (i - (int64_t)R->first);
  *srow = s;
  if (b < 0 || b >= r.n_samples || s < 0 || s >= r.n_points) return false;
  if (r.pre_keep && !r.pre_keep[s]) return false;                                       // a
  const float4 p = r.pts[s];
  if (R->paint_dist > 0.f) {                                                            // b
    const float radius = __fsqrt_rn(__fadd_rn(__fmul_rn(p.x, p.x), __fmul_rn(p.y, p.y)));
    if (!(radius <= R->paint_dist)) return false;
  }
  int row, col;
  if (!sr_project_cam(R->cam, p.x, p.y, p.z, R->img_w, R->img_h, R->crop_top, row, col)) return false;   // c
  float q[3] = {p.x, p.y, p.z};
  sr_move(R->move, q);                                                                  // d
  if (r.aug) sr_augment(r.aug + (int64_t)TS_AUG_RECORD * b, q[0], q[1], q[2]);          // e
  if (r.lo && !sr_clamp_keeps(q[0], q[1], q[2], r.lo, b)) return false;                 // f
  o[0] = q[0];
  o[1] = q[1];
  o[2] = q[2];
  o[3] = __fadd_rn((float)row, R->row_offset);
  o[4] = (float)col;
  return true;
}

// nf_row for every lane of the wave (every lane of the wave calls it; `in`: the lane has a row): one round per distinct record of
// the wave, the record's index made wave-uniform so that its fields are scalar loads.  *sample: the row's sample, -1 without one.
__device__ __forceinline__ bool nf_wave(const NfRule &r, int64_t i, bool in, float (&o)[5], int *sample, int64_t *srow) {
  const int f = in ? min(max(r.frame[i], 0), r.n_frames - 1) : -1;
  bool keep = false;
  *sample = -1;
  *srow = 0;
  unsigned long long rem = __ballot(in);
  while (rem) {                                         // (rem is wave-uniform: every lane takes every round)
    const int f0 = __builtin_amdgcn_readfirstlane(__shfl(f, __ffsll((long long)rem) - 1));
    const bool mine = in && f == f0;                    // true for the lane f0 came from: every round retires a lane
    if (mine) {
      // (under f == f0 the compiler puts the lane's own f back into the address: the first-lane read of the finished pointer is
      //  what it cannot undo - every active lane holds the same pointer here.  The constant address space - the table is not
      //  written while the kernel runs - is what makes a load through a uniform address a scalar load.)
      const uintptr_t at = (uintptr_t)(r.rec + f0);
      const NfRecord R = (NfRecord)(((uintptr_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(at >> 32)) << 32) |
                                    (uintptr_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)at));
      *sample = R->sample;
      keep = nf_row(r, R, i, o, srow);
    }
    rem &= ~__ballot(mine);
  }
  return keep;
}

__device__ __forceinline__ bool NfRule::keeps(int64_t i, bool in, Row &row, int *sample) const {
  return nf_wave(*this, i, in, row.o, sample, &row.srow);
}

}  // namespace

extern "C" size_t ts_nusc_fov_cloud_workspace_bytes(int64_t n_rows, int32_t n_samples) { return cp_compact_bytes(n_rows, n_samples); }

extern "C" int ts_nusc_fov_cloud(const float *points, const int64_t *labels, const uint8_t *pre_keep, int64_t n_points,
                                 const int32_t *frame, int64_t n_rows, const TsNuscCamFrame *records, int32_t n_frames,
                                 const double *aug, const float *lo, int32_t n_samples, float *out, int64_t *out_labels,
                                 int64_t *out_sample, int32_t *out_sample32, int64_t capacity, int64_t *counts, void *ws,
                                 size_t ws_bytes, ts_stream_t stream) {
  static_assert(TS_TIAF_MAX_SAMPLES == TS_WAVE, "cp_count_kernel keeps one LDS counter per (wave, sample)");
  static_assert(sizeof(TsNuscCamFrame) == 584, "the camera record is 584 bytes (taseg_amd/data/nuscenes_tiaf.py CAM_FRAME_DTYPE)");
  TS_REQUIRE(n_points >= 0 && n_rows >= 0 && n_rows < (int64_t)1 << 30 && n_points < (int64_t)1 << 30 && n_frames >= 1 &&
                 n_frames <= TS_TIAF_MAX_FRAMES && n_samples >= 1 && n_samples <= TS_TIAF_MAX_SAMPLES && capacity >= n_rows,
             TS_ERR_INVALID_ARGUMENT, "ts_nusc_fov_cloud: bad sizes");
  TS_REQUIRE(records && counts && ws && ((uintptr_t)ws & 3) == 0 && ((uintptr_t)records & 7) == 0 && ((uintptr_t)aug & 7) == 0 &&
                 ((uintptr_t)lo & 3) == 0,
             TS_ERR_INVALID_ARGUMENT, "ts_nusc_fov_cloud: null or misaligned pointer");
  TS_REQUIRE(n_rows == 0 || (points && labels && frame && out && out_labels && out_sample && out_sample32), TS_ERR_INVALID_ARGUMENT,
             "ts_nusc_fov_cloud: null pointer");
  TS_REQUIRE((((uintptr_t)points) & 15) == 0 && (((uintptr_t)out) & 7) == 0 && (((uintptr_t)labels) & 7) == 0 &&
                 (((uintptr_t)out_labels) & 7) == 0,
             TS_ERR_INVALID_ARGUMENT, "ts_nusc_fov_cloud: points must be 16-byte, out and the labels 8-byte aligned");
  const NfRule r = {{n_rows, capacity, n_samples, out_sample, out_sample32}, (const float4 *)points, labels, pre_keep, frame, records,
                    aug, lo, out, out_labels, n_points, n_frames};
  return cp_compact(r, "ts_nusc_fov_cloud", counts, ws, ws_bytes, (hipStream_t)stream);
}
