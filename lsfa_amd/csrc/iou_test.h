// "Does this pair of boxes suppress?" decided exactly without dividing, in float32 (devIoU > thresh,
// nms_kernel.cu:30-38, multi_proposal.cu:252-260) and in float64 (numpy's `ovr <= thresh` survives,
// lib/nms/nms.py:71).  Shared by nms_kernels.h, nms.hip, proposal.hip and detpost.hip.
//
// fl(inter / uni) > thresh with uni > 0 and 0 < thresh:
//   v = inter - thresh*uni (exact) and d = fma(-thresh, uni, inter) = fl(v) have the same sign;
//   v <= 0            =>  inter/uni <= thresh           => the rounded quotient is <= thresh (rounding is monotone)
//   v >= thresh*uni*u =>  inter/uni >= thresh*(1 + u)   => >= the number after thresh (u = 2^-23 / 2^-52), so the quotient is > thresh
// and d >= thresh*uni*2u implies the second case.  The sliver in between (and non-positive or NaN unions, and
// thresholds outside (1e-30, 1e30) / (1e-300, 1e300)) takes the division.  Callers start `unsure` at !t.fast,
// test it wave-wide and redo with *_div what they decided with *_fast.
// -ffp-contract=off is the parity contract: the fma stands where the test needs it and nowhere else, and a pair's
// value does not depend on which of the two boxes is called the row (max, min, + of two areas are symmetric).
#pragma once
#include <math.h>

#include <hip/hip_runtime.h>

namespace lsfa {

struct IouTest {
  float thresh;
  float thresh_eps;   // thresh * 2^-22
  int fast;
};

static inline IouTest make_iou_test(float thresh) {
  IouTest t;
  t.thresh = thresh;
  t.thresh_eps = thresh * 2.384185791015625e-07f;
  t.fast = (thresh > 1e-30f && thresh < 1e30f) ? 1 : 0;
  return t;
}

__device__ __forceinline__ float box_area(const float4& b) { return (b.z - b.x + 1) * (b.w - b.y + 1); }

__device__ __forceinline__ bool iou_exceeds_fast(const float4& a, float Sa, const float4& b, float Sb, const IouTest& t,
                                                 bool& unsure) {
  const float left = fmaxf(a.x, b.x), right = fminf(a.z, b.z);
  const float top = fmaxf(a.y, b.y), bottom = fminf(a.w, b.w);
  const float width = fmaxf(right - left + 1, 0.f), height = fmaxf(bottom - top + 1, 0.f);
  const float interS = width * height;
  const float uni = Sa + Sb - interS;
  const float d = fmaf(-t.thresh, uni, interS);
  const bool pos = d > 0.f, clear = d >= t.thresh_eps * uni;
  unsure = unsure || !(uni > 0.f) || (pos && !clear);
  return pos && clear;
}
__device__ __forceinline__ bool iou_exceeds_div(const float4& a, float Sa, const float4& b, float Sb, const IouTest& t) {
  const float left = fmaxf(a.x, b.x), right = fminf(a.z, b.z);
  const float top = fmaxf(a.y, b.y), bottom = fminf(a.w, b.w);
  const float width = fmaxf(right - left + 1, 0.f), height = fmaxf(bottom - top + 1, 0.f);
  const float interS = width * height;
  return interS / (Sa + Sb - interS) > t.thresh;
}

// ---- float64: a pair suppresses when NOT (ovr <= thresh), so a NaN quotient suppresses as in numpy ----
struct IouTest64 { double thresh, thresh_eps; int fast; };   // thresh_eps = thresh * 2^-51
static inline IouTest64 make_iou_test64(double thresh) {
  IouTest64 t;
  t.thresh = thresh;
  t.thresh_eps = thresh * 4.440892098500626e-16;   // 2^-51
  t.fast = (thresh > 1e-300 && thresh < 1e300) ? 1 : 0;
  return t;
}

struct Box64 { double x1, y1, x2, y2; };

__device__ __forceinline__ double box_area(const Box64& b) { return (b.x2 - b.x1 + 1) * (b.y2 - b.y1 + 1); }

__device__ __forceinline__ double box_inter(const Box64& a, const Box64& b) {
  const double w = fmax(0.0, fmin(a.x2, b.x2) - fmax(a.x1, b.x1) + 1), h = fmax(0.0, fmin(a.y2, b.y2) - fmax(a.y1, b.y1) + 1);
  return w * h;
}
__device__ __forceinline__ bool iou_exceeds_fast(const Box64& a, double Sa, const Box64& b, double Sb, const IouTest64& t,
                                                 bool& unsure) {
  const double inter = box_inter(a, b);
  const double uni = Sa + Sb - inter;
  const double d = fma(-t.thresh, uni, inter);
  const bool pos = d > 0.0, clear = d >= t.thresh_eps * uni;
  unsure = unsure || !(uni > 0.0) || (pos && !clear);
  return pos && clear;
}
__device__ __forceinline__ bool iou_exceeds_div(const Box64& a, double Sa, const Box64& b, double Sb, const IouTest64& t) {
  const double inter = box_inter(a, b);
  return !(inter / (Sa + Sb - inter) <= t.thresh);
}

}  // namespace lsfa
