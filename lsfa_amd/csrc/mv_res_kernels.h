// transform_mv_res (lib/utils/image.py:202-228) as device functions, stated once for mv.hip (full-resolution motion-vector and residual maps
// in memory) and me_segment.hip (the same maps computed on demand from a segment's macroblock rows).  An output element depends on 2 x 2
// padded positions and each of those on 2 x 2 source pixels: the first resize's four values in float32 (mul, mul, add: the two passes'
// roundings), everything behind them in float64, one rounding to float32 at the end.  oracle/np_ref.py::transform_mv_res is the same
// arithmetic statement by statement.  (ResizeTap, resize_tap and resize_blend: resize_kernels.h)
#pragma once
#include <cmath>

#include "resize_kernels.h"

namespace lsfa {

struct MvResArgs {
  int H, W;             // the decoded frame
  int h1, w1;           // cvRound(H im_scale), cvRound(W im_scale): the first resize's output
  int ph, pw;           // padded to the stride
  int oh, ow;           // cvRound(ph / stride), cvRound(pw / stride): the network's feature grid
  double inv_scale;     // 1. / im_scale
  double inv_rcnn;      // 1. / (1. / stride)
  double mv_mul;        // im_scale * (1. / stride)
  double m0, m1, m2, pixel_scale;       // pixel_means in B, G, R order
  float mv_sign;        // -1: the motion vectors are negated first (`motion_vector = - motion_vector`, image.py:54)
};

// everything of MvResArgs that follows from the caller's arguments; the caller compares oh / ow with its output's shape
inline MvResArgs mv_res_args(int H, int W, double im_scale, int h1, int w1, int rcnn_stride, const double* pixel_means_bgr_host, double pixel_scale,
                             bool negate_mv) {
  MvResArgs a;
  a.H = H; a.W = W; a.h1 = h1; a.w1 = w1;
  a.ph = (h1 + rcnn_stride - 1) / rcnn_stride * rcnn_stride;
  a.pw = (w1 + rcnn_stride - 1) / rcnn_stride * rcnn_stride;
  const double rcnn_scale = 1.0 / (double)rcnn_stride;
  a.oh = (int)nearbyint((double)a.ph * rcnn_scale);        // cvRound (ties to even); a multiple of the stride divides exactly
  a.ow = (int)nearbyint((double)a.pw * rcnn_scale);
  a.inv_scale = 1.0 / im_scale;
  a.inv_rcnn = 1.0 / rcnn_scale;
  a.mv_mul = im_scale * rcnn_scale;
  a.m0 = pixel_means_bgr_host[0]; a.m1 = pixel_means_bgr_host[1]; a.m2 = pixel_means_bgr_host[2];
  a.pixel_scale = pixel_scale;
  a.mv_sign = negate_mv ? -1.f : 1.f;
  return a;
}

// a source value as the first resize reads it
// (sign: the reference negates the decoder's motion vectors before the transform, image.py:54 - exact, applied to the source values)
template <typename T>
__device__ __forceinline__ float resize_source(T v, float sign) { return (float)v * sign; }

template <typename T>
__device__ __forceinline__ float first_resize(const T* __restrict__ src, int H, int W, int C, int c, int y, int x, double inv_scale, float sign = 1.f) {
  const ResizeTap tx = resize_tap(x, W, inv_scale), ty = resize_tap(y, H, inv_scale);
  const float s00 = resize_source(src[((size_t)ty.i0 * W + tx.i0) * C + c], sign), s01 = resize_source(src[((size_t)ty.i0 * W + tx.i1) * C + c], sign);
  const float s10 = resize_source(src[((size_t)ty.i1 * W + tx.i0) * C + c], sign), s11 = resize_source(src[((size_t)ty.i1 * W + tx.i1) * C + c], sign);
  return resize_blend(s00, s01, s10, s11, tx, ty);
}

// the first resize's channel that channel c of the padded residual is computed from: the in-place loop rewrites channel 0 from channel 2
// and then channel 2 from the NEW channel 0, so the first resize's channel 0 is never read
__device__ __forceinline__ int padded_res_source(int c) { return c == 1 ? 1 : 2; }

// channel c of the padded residual AFTER the in-place loop, from v = the first resize's channel padded_res_source(c) there (0.0 in the
// padding):  i = 0: p0 = (p2 - mean[2]) scale;  i = 1: p1 = (p1 - mean[1]) scale;  i = 2: p2 = (p0 - mean[0]) scale with the NEW p0
__device__ __forceinline__ double padded_res(const MvResArgs& a, int c, double v) {
  if (c == 1) return (v - a.m1) * a.pixel_scale;
  const double p0 = (v - a.m2) * a.pixel_scale;
  return c == 0 ? p0 : (p0 - a.m0) * a.pixel_scale;
}

// value of padded map `which` (0: motion vectors, channel c; 1: the residual AFTER the in-place loop, channel c) at (y, x), float64
template <typename T>
__device__ __forceinline__ double padded_value(const T* __restrict__ mv, const T* __restrict__ res, const MvResArgs& a, int which, int c, int y, int x) {
  const bool inside = y < a.h1 && x < a.w1;
  if (which == 0) return inside ? (double)first_resize(mv, a.H, a.W, 2, c, y, x, a.inv_scale, a.mv_sign) : 0.0;
  return padded_res(a, c, inside ? (double)first_resize(res, a.H, a.W, 3, padded_res_source(c), y, x, a.inv_scale) : 0.0);
}

// the second resize (1 / stride, CV_64F) of one output element from its 2 x 2 padded values (row i0: p00, p01; row i1: p10, p11)
__device__ __forceinline__ double second_resize(double p00, double p01, double p10, double p11, const ResizeTap& tx, const ResizeTap& ty) {
  const double ax = (double)tx.a, bx = (double)(1.f - tx.a), ay = (double)ty.a, by = (double)(1.f - ty.a);      // `1.f - fx` in float, used in double
  const double h0 = p00 * bx + p01 * ax;
  const double h1 = p10 * bx + p11 * ax;
  return h0 * by + h1 * ay;
}

}  // namespace lsfa
