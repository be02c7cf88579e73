// Kernels of the RPVNet segmentor (reference pcseg/model/segmentor/fusion/rpvnet/rpvnet.py): the range <-> point transfers and the
// three-way hand-over of the point branch.
//   * ts_range_plan: per resolution of the range branch, the pixel every point is averaged into (`point_to_range`, rpvnet.py:73-91)
//     and the four bilinear corners `F.grid_sample` reads for it (`range_to_point`, rpvnet.py:32-51), written in the [n, 8] layout
//     of ts_trilinear_map - so the mean is ts_voxelize_mean_forward over B h w "voxels", the bilinear read is ts_devoxelize_forward
//     and both adjoints are the kernels those have already: fixed order, no atomics.
//   * ts_range_point_tail_forward: z.F = voxel_to_point(x).F + range_to_point(r) + relu(BN(Linear(z_prev.F))) (rpvnet.py:648-704) in
//     one pass over the rows - launch_point_tail<true> of point_tail.h: the shared kernel with the range operand compiled in.
// Compiled with -ffp-contract=off (csrc/build.py): tests/rpvnet_ref.py restates the plan operation by operation, bit for bit.
#include "point_tail.h"

namespace {

// One thread per point.  pxpy [n, 3] = (batch, px, py), px and py in [-1, 1].
//   pixel   x = (int)(((px + 1) / 2) * (float)(w - 1)), y likewise with h: float32, one rounding per operation, truncation - the
//           tensor expression of rpvnet.py:88 (not `round`: columns whose product lands a hair below an integer fall one pixel short,
//           as the reference's do)
//   corners ix = ((px + 1) * w - 1) / 2, x0 = floor(ix), x1 = x0 + 1; weights (x1 - ix)(y1 - iy), (ix - x0)(y1 - iy),
//           (x1 - ix)(iy - y0), (ix - x0)(iy - y0) for nw, ne, sw, se: grid_sample's bilinear mode, zeros padding,
//           align_corners = False; a corner outside the map: index -1, weight 0
// A row whose batch index is no integer of [0, B), or whose px / py is not finite or outside [-1, 1], takes no part (pix -1, all
// corners -1) and ORs a bit into *err (an integer vector atomic: order-free): 1 batch, 2 non-finite, 4 outside [-1, 1].
__global__ __launch_bounds__(256) void range_plan_kernel(const float *__restrict__ pxpy, int64_t n, int B, int h, int w,
                                                         int *__restrict__ pix, int *__restrict__ bidx, float *__restrict__ bw,
                                                         int *__restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float bf = pxpy[3 * i], px = pxpy[3 * i + 1], py = pxpy[3 * i + 2];
  int flag = 0;
  int b = 0;
  if (!(bf >= 0.f && bf < (float)B) || bf != truncf(bf)) flag |= 1;
  else b = (int)bf;
  if (!isfinite(px) || !isfinite(py)) flag |= 2;
  else if (px < -1.f || px > 1.f || py < -1.f || py > 1.f) flag |= 4;
  int id[4] = {-1, -1, -1, -1};
  float wt[4] = {0.f, 0.f, 0.f, 0.f};
  int p = -1;
  if (flag == 0) {
    const int base = b * h * w;
    const int x = (int)(((px + 1.f) / 2.f) * (float)(w - 1)), y = (int)(((py + 1.f) / 2.f) * (float)(h - 1));
    p = base + y * w + x;
    const float ix = ((px + 1.f) * (float)w - 1.f) / 2.f, iy = ((py + 1.f) * (float)h - 1.f) / 2.f;
    const float fx0 = floorf(ix), fy0 = floorf(iy), fx1 = fx0 + 1.f, fy1 = fy0 + 1.f;
    const int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
    const float wx0 = fx1 - ix, wx1 = ix - fx0, wy0 = fy1 - iy, wy1 = iy - fy0;
    const bool inx0 = x0 >= 0 && x0 < w, inx1 = x1 >= 0 && x1 < w, iny0 = y0 >= 0 && y0 < h, iny1 = y1 >= 0 && y1 < h;
    if (inx0 && iny0) { id[0] = base + y0 * w + x0; wt[0] = wx0 * wy0; }
    if (inx1 && iny0) { id[1] = base + y0 * w + x1; wt[1] = wx1 * wy0; }
    if (inx0 && iny1) { id[2] = base + y1 * w + x0; wt[2] = wx0 * wy1; }
    if (inx1 && iny1) { id[3] = base + y1 * w + x1; wt[3] = wx1 * wy1; }
  } else {
    atomicOr(err, flag);
  }
  pix[i] = p;
  *(int4 *)(bidx + i * 8) = make_int4(id[0], id[1], id[2], id[3]);
  *(int4 *)(bidx + i * 8 + 4) = make_int4(-1, -1, -1, -1);
  *(float4 *)(bw + i * 8) = make_float4(wt[0], wt[1], wt[2], wt[3]);
  *(float4 *)(bw + i * 8 + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
}

}  // namespace

extern "C" int ts_range_plan(const float *pxpy, int64_t n, int32_t batch, int32_t h, int32_t w, int32_t *pix, int32_t *bidx,
                             float *bweight, int32_t *err, ts_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  TS_REQUIRE(n >= 0 && n < (1LL << 30) && batch > 0 && h > 0 && w > 0 && (int64_t)batch * h * w < (1LL << 31) - 1,
             TS_ERR_INVALID_ARGUMENT, "ts_range_plan: bad sizes");
  if (n == 0) return TS_OK;
  TS_REQUIRE(pxpy && pix && bidx && bweight && err, TS_ERR_INVALID_ARGUMENT, "ts_range_plan: null pointer");
  TS_REQUIRE(aligned16(bidx, bweight), TS_ERR_INVALID_ARGUMENT, "ts_range_plan: maps must be 16-byte aligned");
  range_plan_kernel<<<(unsigned)ts_cdiv(n, (int64_t)256), 256, 0, stream>>>(pxpy, n, batch, h, w, pix, bidx, bweight, err);
  TS_CHECK_LAUNCH("ts_range_plan");
  return TS_OK;
}

extern "C" int ts_range_point_tail_forward(const void *y, const void *vox, const int32_t *idx, const float *weight, const void *pix,
                                           const int32_t *bidx, const float *bweight, const float *mean, const float *invstd,
                                           const float *gamma, const float *beta, int64_t n, int32_t c, int64_t m, int64_t mp,
                                           int32_t half, void *out, uint8_t *mask, ts_stream_t stream_) {
  return launch_point_tail<true>("ts_range_point_tail_forward", y, vox, idx, weight, pix, bidx, bweight, mp, mean, invstd, gamma, beta,
                                 n, c, m, half, out, mask, (hipStream_t)stream_);
}
