// What the YUV intake's kernels (yuvfmt.hip) convert into, whatever the format: a converted pixel and its clamp, the table of the three
// matrices, and the two output forms of the plane kernels - the packed BGR frame (plus the packed Y plane) and the network's `data`.  A
// kernel template takes one of the two as `Out` and calls px (one pixel) or quad (four adjacent pixels).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lsfa {

struct Bgr { int b, g, r; };

// v >> DOWN clipped to 0..255, clamped BEFORE the shift: the same number (v < 0 gives 0, v >= 256 << DOWN gives 255, >> is monotonic), and
// the ONLY form a channel that reaches BgrOut::quad may be computed in.  Shift-then-saturate, min(max(v >> DOWN, 0), 255), is what the
// gfx950 back end folds, together with quad's `b | g << 8`, into v_ashr_pk_u8_i32.  That instruction writes the low half of its
// destination and the back end uses the result as a whole dword: wherever the register held a negative value before (a clipped blue),
// bytes 2 and 3 of the stored dword came out as 0xFF on the device - DESIGN.md "Other chroma formats".
template <int DOWN>
__device__ __forceinline__ int clip_down(int v) { return min(max(v, 0), (256 << DOWN) - 1) >> DOWN; }

// {o, cy, rv, gu, gv, bu} per matrix, in 8-bit units: BT.601 limited, BT.709 limited, BT.601 full range (include/lsfa_hip.h)
constexpr int kYuvMatrix[3][6] = {{16, 298, 409, 100, 208, 516}, {16, 298, 459, 55, 136, 541}, {0, 256, 359, 88, 183, 454}};

// the packed (N, H, W, 3) uint8 BGR frame and, optionally, the 8-bit Y plane with the pitch removed
struct BgrOut {
  unsigned char* bgr;
  unsigned char* y_packed;      // may be nullptr
  long hw;
  __device__ __forceinline__ void px(long n, long pix, const Bgr& c, int Y) const {
    unsigned char* o = bgr + (n * hw + pix) * 3;
    o[0] = (unsigned char)c.b; o[1] = (unsigned char)c.g; o[2] = (unsigned char)c.r;
    if (y_packed) y_packed[n * hw + pix] = (unsigned char)Y;
  }
  // pix % 4 == 0, hw % 4 == 0, both bases dword aligned: twelve bytes as three dwords, b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
  __device__ __forceinline__ void quad(long n, long pix, const Bgr (&c)[4], uint32_t ydw) const {
    uint32_t* o = reinterpret_cast<uint32_t*>(bgr + (n * hw + pix) * 3);
    o[0] = (uint32_t)c[0].b | ((uint32_t)c[0].g << 8) | ((uint32_t)c[0].r << 16) | ((uint32_t)c[1].b << 24);
    o[1] = (uint32_t)c[1].g | ((uint32_t)c[1].r << 8) | ((uint32_t)c[2].b << 16) | ((uint32_t)c[2].g << 24);
    o[2] = (uint32_t)c[2].r | ((uint32_t)c[3].b << 8) | ((uint32_t)c[3].g << 16) | ((uint32_t)c[3].r << 24);
    if (y_packed) *reinterpret_cast<uint32_t*>(y_packed + n * hw + pix) = ydw;
  }
};

// `data` (N, 3, H, W) float32: image_transform_u8_kernel's arithmetic (stem.hip) - subtraction and product in float64, one rounding
struct DataOut {
  float* out;
  long hw;
  double m0, m1, m2, scale;     // pixel_means in B, G, R order
  __device__ __forceinline__ void px(long n, long pix, const Bgr& c, int) const {
    float* o = out + n * 3 * hw + pix;
    o[0] = (float)(((double)c.r - m2) * scale);
    o[hw] = (float)(((double)c.g - m1) * scale);
    o[2 * hw] = (float)(((double)c.b - m0) * scale);
  }
  // pix % 4 == 0, hw % 4 == 0, the base 16-byte aligned: one float4 per plane
  __device__ __forceinline__ void quad(long n, long pix, const Bgr (&c)[4], uint32_t) const {
    float* o = out + n * 3 * hw + pix;
    *reinterpret_cast<float4*>(o) = make_float4((float)(((double)c[0].r - m2) * scale), (float)(((double)c[1].r - m2) * scale),
                                                (float)(((double)c[2].r - m2) * scale), (float)(((double)c[3].r - m2) * scale));
    *reinterpret_cast<float4*>(o + hw) = make_float4((float)(((double)c[0].g - m1) * scale), (float)(((double)c[1].g - m1) * scale),
                                                     (float)(((double)c[2].g - m1) * scale), (float)(((double)c[3].g - m1) * scale));
    *reinterpret_cast<float4*>(o + 2 * hw) = make_float4((float)(((double)c[0].b - m0) * scale), (float)(((double)c[1].b - m0) * scale),
                                                         (float)(((double)c[2].b - m0) * scale), (float)(((double)c[3].b - m0) * scale));
  }
};

}  // namespace lsfa
