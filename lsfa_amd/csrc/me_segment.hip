// A segment's network inputs from its macroblock rows in one launch: for every non-key frame f = 1..F of every chain, the `motion_vector`
// and `res_diff` that lsfa_mv_identity, lsfa_mv_accumulate (frames 1..f), lsfa_mv_field, lsfa_mv_residual and lsfa_transform_mv_res build
// frame by frame - without the accumulated source map, the field, the residual or the owner map ever existing.
//
// Two facts carry it ("Motion estimation"):
//   * transform_mv_res reads at most 16 source pixels per output element (2 x 2 padded positions, each 2 x 2 source pixels): about 38 K of
//     the 600 K pixels of a 1000 x 600 frame;
//   * the rows of lsfa_mv_estimate[_chain] partition the frame into their destination blocks, so the "last writer" of a pixel is the block
//     that contains it and accu_f[p] is a walk back through the per-block vectors of frames f, f - 1, .. 1:
//         q = p;  for k = f .. 1:  q' = q + (src - dst) of frame k's row at block (q.y >> 4, q.x >> 4);  q = q' if q' is inside the frame
//     (a source outside the frame is not written by the accumulation either; the estimator never produces one, and for rows that are not
//     the estimator's the rule keeps every read inside the frames and the table).  Then mv = p - q and res = cur[p] - key[q].
// The arithmetic behind the walk is transform_mv_res_kernel's (mv_res_kernels.h): the first resize in float32, everything after it in
// float64, one rounding at the end.
//
// segment_inputs_kernel: four lanes per output cell (frame, chain, Y, X), one per padded position of the second resize.  A lane walks its
// 2 x 2 source pixels together (four independent chains of dependent loads) and keeps what the five output channels read of them: the
// two vector components and the residual's channels 1 and 2 (the in-place loop never reads the first resize's channel 0).  The four
// padded values of a channel meet through __shfl; lane c & 3 stores channel c.  The vector table is read through the cache (172 KB for
// nine 1000 x 600 frames, every row of it read by the sixteen walks that start inside its block or pass through it).
#include "common.h"
#include "mv_res_kernels.h"

using namespace lsfa;

namespace {

constexpr int kThreads = 256;

struct SegmentArgs {
  MvResArgs r;
  int n_chains, n_frames;
  int mbw, blocks;              // macroblocks per row / per frame
  long long frame_stride;       // bytes between two BGR frames
};

// one step of the walk for source pixel (x, y): frame k's row of the block that contains it
__device__ __forceinline__ void walk_step(const int* __restrict__ rows_k, const SegmentArgs& a, int& x, int& y) {
  const int* row = rows_k + (size_t)((y >> 4) * a.mbw + (x >> 4)) * 7;
  const long long nx = (long long)x + ((long long)row[3] - (long long)row[5]), ny = (long long)y + ((long long)row[4] - (long long)row[6]);
  if (nx >= 0 && nx < a.r.W && ny >= 0 && ny < a.r.H) { x = (int)nx; y = (int)ny; }
}

__global__ __launch_bounds__(kThreads) void segment_inputs_kernel(const int* __restrict__ mvs, const unsigned char* __restrict__ bgr, SegmentArgs a,
                                                                  float* __restrict__ out_mv, float* __restrict__ out_res) {
  const MvResArgs& r = a.r;
  const int plane = r.oh * r.ow;
  const int cells = a.n_frames * a.n_chains * plane;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  const bool live = (t >> 2) < cells;
  const int cell = live ? (t >> 2) : cells - 1;       // lanes past the end compute the last cell again and store nothing: every lane reaches the shuffles
  const int j = t & 3;
  const int fc = cell / plane, pos = cell - fc * plane, Y = pos / r.ow, X = pos - Y * r.ow;
  const int fi = fc / a.n_chains, c = fc - fi * a.n_chains, f = fi + 1;       // frame-major: out[f - 1][c]

  const ResizeTap tx = resize_tap(X, r.pw, r.inv_rcnn), ty = resize_tap(Y, r.ph, r.inv_rcnn);
  const int py = (j & 2) ? ty.i1 : ty.i0, px = (j & 1) ? tx.i1 : tx.i0;       // this lane's padded position

  // the first resize there: motion vector x, y and residual channels 1, 2 (0.0 in the padding)
  double first[4] = {0.0, 0.0, 0.0, 0.0};
  if (py < r.h1 && px < r.w1) {
    const ResizeTap sx = resize_tap(px, r.W, r.inv_scale), sy = resize_tap(py, r.H, r.inv_scale);
    const int x0[4] = {sx.i0, sx.i1, sx.i0, sx.i1}, y0[4] = {sy.i0, sy.i0, sy.i1, sy.i1};
    int qx[4], qy[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) { qx[s] = x0[s]; qy[s] = y0[s]; }
    const int* rows_c = mvs + (size_t)c * a.n_frames * a.blocks * 7;
    for (int k = f; k >= 1; --k) {
      const int* rows_k = rows_c + (size_t)(k - 1) * a.blocks * 7;
#pragma unroll
      for (int s = 0; s < 4; ++s) walk_step(rows_k, a, qx[s], qy[s]);
    }
    const unsigned char* key = bgr + (size_t)c * (a.n_frames + 1) * (size_t)a.frame_stride;
    const unsigned char* cur = key + (size_t)f * (size_t)a.frame_stride;
    float src[4][4];       // [channel][source pixel]
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const size_t o = ((size_t)y0[s] * r.W + x0[s]) * 3, k = ((size_t)qy[s] * r.W + qx[s]) * 3;
      src[0][s] = resize_source(x0[s] - qx[s], r.mv_sign);
      src[1][s] = resize_source(y0[s] - qy[s], r.mv_sign);
      src[2][s] = resize_source((int)cur[o + 1] - (int)key[k + 1], 1.f);
      src[3][s] = resize_source((int)cur[o + 2] - (int)key[k + 2], 1.f);
    }
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) first[ch] = (double)resize_blend(src[ch][0], src[ch][1], src[ch][2], src[ch][3], sx, sy);
  }
  // the five padded maps at this position: motion vectors 0, 1; the residual after its in-place loop 0, 1, 2
  const double padded[5] = {first[0], first[1], padded_res(r, 0, first[1 + padded_res_source(0)]), padded_res(r, 1, first[1 + padded_res_source(1)]),
                            padded_res(r, 2, first[1 + padded_res_source(2)])};
  const int lane0 = (int)(threadIdx.x & 63u) & ~3;
  float* mv_o = out_mv + (size_t)fc * 2 * plane + pos;
  float* res_o = out_res + (size_t)fc * 3 * plane + pos;
#pragma unroll
  for (int ch = 0; ch < 5; ++ch) {
    const double p00 = __shfl(padded[ch], lane0, 64), p01 = __shfl(padded[ch], lane0 + 1, 64);
    const double p10 = __shfl(padded[ch], lane0 + 2, 64), p11 = __shfl(padded[ch], lane0 + 3, 64);
    double v = second_resize(p00, p01, p10, p11, tx, ty);
    if (live && j == (ch & 3)) {
      if (ch < 2) { v *= r.mv_mul; mv_o[ch * plane] = (float)v; }
      else res_o[(ch - 2) * plane] = (float)v;
    }
  }
}

}  // namespace

extern "C" int lsfa_mv_segment_inputs(const int* mvs, const unsigned char* bgr, long long frame_stride, int n_chains, int n_frames, int width, int height,
                                      double im_scale, int h1, int w1, int rcnn_stride, const double* pixel_means_bgr_host, double pixel_scale,
                                      float* out_mv, float* out_res, int out_h, int out_w, void* stream) {
  LSFA_REQUIRE(mvs && bgr && pixel_means_bgr_host && out_mv && out_res, "lsfa_mv_segment_inputs: NULL argument");
  LSFA_REQUIRE(width > 0 && height > 0 && (long)width * height < (1L << 30), "lsfa_mv_segment_inputs: bad frame size %d x %d", width, height);
  LSFA_REQUIRE(n_chains >= 1 && n_frames >= 1, "lsfa_mv_segment_inputs: %d chains of %d frames: both counts must be at least 1", n_chains, n_frames);
  LSFA_REQUIRE(frame_stride >= (long long)width * height * 3, "lsfa_mv_segment_inputs: frame stride %lld does not hold a %d x %d x 3 frame", frame_stride,
               width, height);
  LSFA_REQUIRE(h1 > 0 && w1 > 0 && rcnn_stride > 0 && im_scale > 0.0, "lsfa_mv_segment_inputs: bad shape: h1 %d, w1 %d, rcnn_stride %d, im_scale %g", h1, w1,
               rcnn_stride, im_scale);
  SegmentArgs a;
  a.r = mv_res_args(height, width, im_scale, h1, w1, rcnn_stride, pixel_means_bgr_host, pixel_scale, true);
  if (a.r.oh != out_h || a.r.ow != out_w) {
    set_error("lsfa_mv_segment_inputs: outputs are %d x %d, the padded %d x %d map gives %d x %d", out_h, out_w, a.r.ph, a.r.pw, a.r.oh, a.r.ow);
    return LSFA_EINVAL;
  }
  a.n_chains = n_chains; a.n_frames = n_frames;
  a.mbw = ceil_div(width, 16);
  a.blocks = a.mbw * ceil_div(height, 16);
  a.frame_stride = frame_stride;
  const long cells = (long)n_frames * n_chains * a.r.oh * a.r.ow;
  LSFA_REQUIRE(cells < (1L << 28), "lsfa_mv_segment_inputs: %ld output cells exceed one launch", cells);
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_MV_ESTIMATE, s);
  hipLaunchKernelGGL(segment_inputs_kernel, dim3((unsigned)ceil_div((int)(cells * 4), kThreads)), dim3(kThreads), 0, s, mvs, bgr, a, out_mv, out_res);
  LSFA_LAUNCH_CHECK("lsfa_mv_segment_inputs");
  return LSFA_OK;
}
