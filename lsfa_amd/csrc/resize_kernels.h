// The tap, weight and `transform` arithmetic of the frame intake, stated once for mv.hip (packed BGR / float frames, motion vectors,
// residuals) and yuvfmt.hip (taps read from YUV planes).  OpenCV 3.2's HResizeLinear / VResizeLinear<float, float, float> as restated in
// oracle/np_ref.py; the precisions of `transform` follow lib/utils/image.py:296-308 (see lsfa_image_resize_transform in lsfa_hip.h).
#pragma once
#include <hip/hip_runtime.h>

namespace lsfa {

struct ResizeTap { int i0, i1; float a; };

// resize.cpp: `fx = (float)((dx + 0.5) * scale_x - 0.5); sx = cvFloor(fx); fx -= sx;` with scale = 1. / f; taps clamped into the image
__device__ __forceinline__ ResizeTap resize_tap(int d, int src_n, double inv_f) {
  const float f = (float)(((double)d + 0.5) * inv_f - 0.5);
  int s0 = (int)floorf(f);
  float a = f - (float)s0;
  if (s0 < 0) { s0 = 0; a = 0.f; }
  if (s0 >= src_n - 1) { s0 = src_n - 1; a = 0.f; }
  ResizeTap t;
  t.i0 = s0;
  t.i1 = min(s0 + 1, src_n - 1);
  t.a = a;
  return t;
}

// the four source values (row i0: s00, s01; row i1: s10, s11) of one output element through both passes, in float32
__device__ __forceinline__ float resize_blend(float s00, float s01, float s10, float s11, const ResizeTap& tx, const ResizeTap& ty) {
  const float bx = 1.f - tx.a, by = 1.f - ty.a;
  const float h0 = s00 * bx + s01 * tx.a;          // the horizontal pass of the two rows, rounded to float like the work buffer
  const float h1 = s10 * bx + s11 * tx.a;
  return h0 * by + h1 * ty.a;
}

// `transform` of one resized (or padding) pixel into the three planes of `data`: plane 0 = R - mean[2], plane 1 = G - mean[1],
// plane 2 = B - mean[0] (m0, m1, m2 = pixel_means in B, G, R order), times pixel_scale
__device__ __forceinline__ void resize_transform_store(float* __restrict__ o, long plane, float b, float g, float r, double m0, double m1, double m2,
                                                       double pixel_scale, int sub_f64) {
  if (sub_f64) {
    // stride > 0: `resize` copied the float32 frame into np.zeros(...) - a float64 image (image.py:288-293) - so `transform` subtracts in float64
    // and the executor rounds once
    o[0] = (float)(((double)r - m2) * pixel_scale);
    o[plane] = (float)(((double)g - m1) * pixel_scale);
    o[2 * plane] = (float)(((double)b - m0) * pixel_scale);
    return;
  }
  // stride == 0: a float32 image minus a Python float is a float32 subtraction (the mean rounded to float32 first); the product with pixel_scale is float64
  const float tr = r - (float)m2, tg = g - (float)m1, tb = b - (float)m0;
  o[0] = (float)((double)tr * pixel_scale);
  o[plane] = (float)((double)tg * pixel_scale);
  o[2 * plane] = (float)((double)tb * pixel_scale);
}

}  // namespace lsfa
