// 10-bit YUV 4:2:0 intake: what HEVC Main10, VP9 profile 2 and AV1 10-bit decode to - the VCN engines' P010 / P016 surfaces and libav's
// yuv420p10le - straight to the packed uint8 BGR frame, the 8-bit luma plane the search reads and the network's `data`, like yuv.hip does
// for 8-bit planes.  Samples are 16-bit little-endian words; everything behind the intake stays 8-bit.
//
// NOT a port of anything in the reference.  The conversion is DEFINED by the specification below (include/lsfa_hip.h; DESIGN.md "YUV intake",
// "10-bit planes"; tests/ref_yuv10.py states it in numpy).  Integer arithmetic, one answer per input, every 16-bit word is defined input:
//   a sample is s = (w >> shift) & 1023: shift = 6 is P010 (the value in the high ten bits, the low six ignored), shift = 0 is yuv420p10le /
//   I010 (the value in the low ten bits, the high six masked);
//   pixel (x, y) takes Y[y][x] and the chroma sample (x >> 1, y >> 1); chroma planes are ceil(W / 2) x ceil(H / 2);
//   C = Y - 4 o, D = U - 512, E = V - 512 with the 8-bit table's o and coefficients (yuv_out.h), e.g. matrix 0:
//   R = clip((298 C + 409 E + 512) >> 10)  G = clip((298 C - 100 D - 208 E + 512) >> 10)  B = clip((298 C + 516 D + 512) >> 10)
//   - the 8-bit formulas with rounding constant 512 and shift 10: converted in ten bits, rounded once; |intermediate| < 2^20;
//   y_packed = min(255, (Y + 2) >> 2).
// Planes that are exactly 4 x an 8-bit plane give yuv.hip's BGR and Y bit for bit.
// Out of scope: 12-bit and P016's low bits as signal, interpolated chroma, HDR transfer functions, rocDecode.  NV21, 4:2:2, 4:4:4: yuvfmt.hip.
//
// Bandwidth kernels in yuv.hip's shape.  yuv420p10_quad_kernel gives a thread four horizontally adjacent pixels of two rows: two 8-byte Y
// loads, one 8-byte load of two U, V pairs (two 4-byte loads for planar chroma) - every chroma sample is read once - and yuv_out.h's quad
// stores.  yuv420p10_words_kernel is the element-wise form (a thread per pixel, 2-byte loads) for bases, pitches or strides that are not
// 8-byte aligned (4-byte for planar chroma), W % 4 != 0 and an odd H; the host picks one of the two per launch.  The resize form gathers
// and converts its four taps per output pixel and shares resize_kernels.h.
#include "common.h"
#include "resize_kernels.h"
#include "yuv_out.h"

using namespace lsfa;

namespace {

constexpr int kThreads = 256;

struct Yuv10Planes {
  const unsigned char* y;
  const unsigned char* u;       // v == nullptr: interleaved U, V words (P010's layout)
  const unsigned char* v;
  long long y_pitch, y_stride, c_pitch, c_stride;       // bytes: row to row, frame to frame; all even
  int N, H, W;
  int shift;                    // 6: the sample in the high ten bits; 0: in the low ten
  int o, cy, rv, gu, gv, bu;    // the matrix' row of kYuvMatrix, o in 10-bit units
};

__device__ __forceinline__ int sample10(const Yuv10Planes& p, uint32_t w) { return (int)((w >> p.shift) & 1023u); }

__device__ __forceinline__ int luma8(int Y) { return min(255, (Y + 2) >> 2); }

__device__ __forceinline__ Bgr yuv10_to_bgr(const Yuv10Planes& p, int Y, int U, int V) {
  const int c = p.cy * (Y - p.o) + 512, d = U - 512, e = V - 512;
  Bgr o;
  o.r = clip255((c + p.rv * e) >> 10);
  o.g = clip255((c - p.gu * d - p.gv * e) >> 10);
  o.b = clip255((c + p.bu * d) >> 10);
  return o;
}

__device__ __forceinline__ uint32_t word_at(const unsigned char* base, long byte_offset) {
  return *reinterpret_cast<const uint16_t*>(base + byte_offset);
}

// pixel (x, y) of frame n, 2-byte loads; *luma receives its Y reduced to 8 bits
__device__ __forceinline__ Bgr yuv10_pixel(const Yuv10Planes& p, long n, int y, int x, int* luma) {
  const int Y = sample10(p, word_at(p.y, n * p.y_stride + (long)y * p.y_pitch + 2L * x));
  const long co = n * p.c_stride + (long)(y >> 1) * p.c_pitch;
  int U, V;
  if (p.v) { U = sample10(p, word_at(p.u, co + 2L * (x >> 1))); V = sample10(p, word_at(p.v, co + 2L * (x >> 1))); }
  else { U = sample10(p, word_at(p.u, co + 4L * (x >> 1))); V = sample10(p, word_at(p.u, co + 4L * (x >> 1) + 2)); }
  *luma = luma8(Y);
  return yuv10_to_bgr(p, Y, U, V);
}

// W % 4 == 0, H % 2 == 0, Y and interleaved chroma base / pitch / stride 8-byte aligned, planar chroma 4-byte aligned: the host checks
template <class Out>
__global__ __launch_bounds__(kThreads) void yuv420p10_quad_kernel(Yuv10Planes p, Out out) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  const int w4 = p.W >> 2, h2 = p.H >> 1;
  const long per = (long)w4 * h2;
  if (i >= p.N * per) return;
  const long n = i / per, r = i - n * per;
  const int ry = (int)(r / w4), qx = (int)(r - (long)ry * w4);
  const unsigned char* yr = p.y + n * p.y_stride + (long)(2 * ry) * p.y_pitch + 8L * qx;
  const uint2 yd[2] = {*reinterpret_cast<const uint2*>(yr), *reinterpret_cast<const uint2*>(yr + p.y_pitch)};
  const long co = n * p.c_stride + (long)ry * p.c_pitch;
  int U[2], V[2];
  if (p.v) {
    const uint32_t u = *reinterpret_cast<const uint32_t*>(p.u + co + 4L * qx), v = *reinterpret_cast<const uint32_t*>(p.v + co + 4L * qx);
    U[0] = sample10(p, u & 0xffffu); U[1] = sample10(p, u >> 16);
    V[0] = sample10(p, v & 0xffffu); V[1] = sample10(p, v >> 16);
  } else {
    const uint2 uv = *reinterpret_cast<const uint2*>(p.u + co + 8L * qx);       // U0 V0 | U1 V1
    U[0] = sample10(p, uv.x & 0xffffu); V[0] = sample10(p, uv.x >> 16);
    U[1] = sample10(p, uv.y & 0xffffu); V[1] = sample10(p, uv.y >> 16);
  }
#pragma unroll
  for (int row = 0; row < 2; ++row) {
    const int Y[4] = {sample10(p, yd[row].x & 0xffffu), sample10(p, yd[row].x >> 16), sample10(p, yd[row].y & 0xffffu), sample10(p, yd[row].y >> 16)};
    Bgr c[4];
    uint32_t ydw = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      c[k] = yuv10_to_bgr(p, Y[k], U[k >> 1], V[k >> 1]);
      ydw |= (uint32_t)luma8(Y[k]) << (8 * k);
    }
    out.quad(n, (long)(2 * ry + row) * p.W + 4 * qx, c, ydw);
  }
}

template <class Out>
__global__ __launch_bounds__(kThreads) void yuv420p10_words_kernel(Yuv10Planes p, Out out) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  const long hw = (long)p.H * p.W;
  if (i >= p.N * hw) return;
  const long n = i / hw, pix = i - n * hw;
  const int y = (int)(pix / p.W), x = (int)(pix - (long)y * p.W);
  int Y;
  const Bgr c = yuv10_pixel(p, n, y, x, &Y);
  out.px(n, pix, c, Y);
}

// lsfa_image_resize_transform's is_u8 = 1 kernel with the taps converted from the planes: a thread per output pixel, the three channels together
__global__ __launch_bounds__(kThreads) void resize_transform_yuv420p10_kernel(Yuv10Planes p, int h1, int w1, int ph, int pw, double inv_scale, double m0,
                                                                              double m1, double m2, double pixel_scale, int sub_f64,
                                                                              float* __restrict__ out) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  const long plane = (long)ph * pw;
  if (i >= p.N * plane) return;
  const int n = (int)(i / plane);
  const long r = i - n * plane;
  const int y = (int)(r / pw), x = (int)(r - (long)y * pw);
  float b = 0.f, g = 0.f, rr = 0.f;
  if (y < h1 && x < w1) {
    const ResizeTap tx = resize_tap(x, p.W, inv_scale), ty = resize_tap(y, p.H, inv_scale);
    int Y;
    const Bgr s00 = yuv10_pixel(p, n, ty.i0, tx.i0, &Y), s01 = yuv10_pixel(p, n, ty.i0, tx.i1, &Y);
    const Bgr s10 = yuv10_pixel(p, n, ty.i1, tx.i0, &Y), s11 = yuv10_pixel(p, n, ty.i1, tx.i1, &Y);
    b = resize_blend((float)s00.b, (float)s01.b, (float)s10.b, (float)s11.b, tx, ty);
    g = resize_blend((float)s00.g, (float)s01.g, (float)s10.g, (float)s11.g, tx, ty);
    rr = resize_blend((float)s00.r, (float)s01.r, (float)s10.r, (float)s11.r, tx, ty);
  }
  resize_transform_store(out + (size_t)n * 3 * plane + r, plane, b, g, rr, m0, m1, m2, pixel_scale, sub_f64);
}

int fill_planes(const char* who, Yuv10Planes& p, const void* y, long long y_pitch, long long y_frame_stride, const void* u_or_uv, const void* v,
                long long c_pitch, long long c_frame_stride, int N, int H, int W, int matrix, int shift) {
  LSFA_REQUIRE(y && u_or_uv, "%s: NULL plane", who);
  LSFA_REQUIRE(N > 0 && H > 0 && W > 0 && H <= (1 << 16) && W <= (1 << 16) && (long long)N * H * W < (1LL << 36), "%s: bad shape: %d frames of %d x %d", who,
               N, W, H);
  LSFA_REQUIRE(matrix >= 0 && matrix <= 2, "%s: matrix %d is not 0 (BT.601 limited), 1 (BT.709 limited) or 2 (BT.601 full range)", who, matrix);
  LSFA_REQUIRE(shift == 0 || shift == 6, "%s: shift %d is not 6 (P010: the sample in the high ten bits) or 0 (yuv420p10le: in the low ten)", who, shift);
  LSFA_REQUIRE(((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(u_or_uv) | reinterpret_cast<uintptr_t>(v)) & 1u) == 0,
               "%s: a plane of 16-bit words starts at an odd address", who);
  LSFA_REQUIRE((((unsigned long long)y_pitch | (unsigned long long)y_frame_stride | (unsigned long long)c_pitch | (unsigned long long)c_frame_stride) & 1u) == 0,
               "%s: pitches and frame strides are bytes between 16-bit words and must be even: Y %lld / %lld, chroma %lld / %lld", who, y_pitch,
               y_frame_stride, c_pitch, c_frame_stride);
  LSFA_REQUIRE(y_pitch >= 2LL * W, "%s: Y pitch %lld is below the row's %lld bytes", who, y_pitch, 2LL * W);
  const int cw = (W + 1) / 2, need = v ? 2 * cw : 4 * cw;
  LSFA_REQUIRE(c_pitch >= need, "%s: chroma pitch %lld is below the %s row's %d bytes", who, c_pitch, v ? "planar" : "interleaved", need);
  p.y = static_cast<const unsigned char*>(y); p.u = static_cast<const unsigned char*>(u_or_uv); p.v = static_cast<const unsigned char*>(v);
  p.y_pitch = y_pitch; p.y_stride = y_frame_stride; p.c_pitch = c_pitch; p.c_stride = c_frame_stride;
  p.N = N; p.H = H; p.W = W;
  p.shift = shift;
  const int* m = kYuvMatrix[matrix];
  p.o = 4 * m[0]; p.cy = m[1]; p.rv = m[2]; p.gu = m[3]; p.gv = m[4]; p.bu = m[5];
  return LSFA_OK;
}

// may the launch take yuv420p10_quad_kernel?  (the outputs' alignment is the caller's part)
bool quad_ok(const Yuv10Planes& p) {
  if ((p.W & 3) || (p.H & 1)) return false;
  if ((reinterpret_cast<uintptr_t>(p.y) | (uintptr_t)p.y_pitch | (uintptr_t)p.y_stride) & 7u) return false;
  const uintptr_t cm = p.v ? 3u : 7u;
  return ((reinterpret_cast<uintptr_t>(p.u) | reinterpret_cast<uintptr_t>(p.v) | (uintptr_t)p.c_pitch | (uintptr_t)p.c_stride) & cm) == 0;
}

template <class Out>
void launch(const Yuv10Planes& p, const Out& out, bool quad, hipStream_t s) {
  if (quad) {
    const long total = (long)p.N * (p.H >> 1) * (p.W >> 2);
    hipLaunchKernelGGL(yuv420p10_quad_kernel<Out>, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, p, out);
  } else {
    const long total = (long)p.N * p.H * p.W;
    hipLaunchKernelGGL(yuv420p10_words_kernel<Out>, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, p, out);
  }
}

}  // namespace

extern "C" int lsfa_yuv420p10_to_bgr_u8(const void* y, long long y_pitch, long long y_frame_stride, const void* u_or_uv, const void* v, long long c_pitch,
                                        long long c_frame_stride, int N, int H, int W, int matrix, int shift, unsigned char* bgr,
                                        unsigned char* y_packed, void* stream) {
  Yuv10Planes p;
  if (int rc = fill_planes("lsfa_yuv420p10_to_bgr_u8", p, y, y_pitch, y_frame_stride, u_or_uv, v, c_pitch, c_frame_stride, N, H, W, matrix, shift)) return rc;
  LSFA_REQUIRE(bgr, "lsfa_yuv420p10_to_bgr_u8: NULL output");
  BgrOut out;
  out.bgr = bgr; out.y_packed = y_packed; out.hw = (long)H * W;
  const bool quad = quad_ok(p) && ((reinterpret_cast<uintptr_t>(bgr) | reinterpret_cast<uintptr_t>(y_packed)) & 3u) == 0;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_STEM, s);
  launch(p, out, quad, s);
  LSFA_LAUNCH_CHECK("lsfa_yuv420p10_to_bgr_u8");
  return LSFA_OK;
}

extern "C" int lsfa_image_transform_yuv420p10(const void* y, long long y_pitch, long long y_frame_stride, const void* u_or_uv, const void* v,
                                              long long c_pitch, long long c_frame_stride, int N, int H, int W, int matrix, int shift,
                                              const double* pixel_means_bgr_host, double pixel_scale, float* data_nchw, void* stream) {
  Yuv10Planes p;
  if (int rc = fill_planes("lsfa_image_transform_yuv420p10", p, y, y_pitch, y_frame_stride, u_or_uv, v, c_pitch, c_frame_stride, N, H, W, matrix, shift))
    return rc;
  LSFA_REQUIRE(pixel_means_bgr_host && data_nchw, "lsfa_image_transform_yuv420p10: NULL argument");
  LSFA_REQUIRE((reinterpret_cast<uintptr_t>(data_nchw) & 3u) == 0, "lsfa_image_transform_yuv420p10: the output is not float aligned");
  DataOut out;
  out.out = data_nchw; out.hw = (long)H * W;
  out.m0 = pixel_means_bgr_host[0]; out.m1 = pixel_means_bgr_host[1]; out.m2 = pixel_means_bgr_host[2];
  out.scale = pixel_scale;
  const bool quad = quad_ok(p) && (reinterpret_cast<uintptr_t>(data_nchw) & 15u) == 0;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_STEM, s);
  launch(p, out, quad, s);
  LSFA_LAUNCH_CHECK("lsfa_image_transform_yuv420p10");
  return LSFA_OK;
}

extern "C" int lsfa_image_resize_transform_yuv420p10(const void* y, long long y_pitch, long long y_frame_stride, const void* u_or_uv, const void* v,
                                                     long long c_pitch, long long c_frame_stride, int N, int H, int W, int matrix, int shift,
                                                     double im_scale, int h1, int w1, int stride, const double* pixel_means_bgr_host,
                                                     double pixel_scale, float* data_nchw, int out_h, int out_w, void* stream) {
  Yuv10Planes p;
  if (int rc = fill_planes("lsfa_image_resize_transform_yuv420p10", p, y, y_pitch, y_frame_stride, u_or_uv, v, c_pitch, c_frame_stride, N, H, W, matrix,
                           shift))
    return rc;
  LSFA_REQUIRE(pixel_means_bgr_host && data_nchw, "lsfa_image_resize_transform_yuv420p10: NULL argument");
  LSFA_REQUIRE((reinterpret_cast<uintptr_t>(data_nchw) & 3u) == 0, "lsfa_image_resize_transform_yuv420p10: the output is not float aligned");
  LSFA_REQUIRE(h1 > 0 && w1 > 0 && h1 <= (1 << 16) && w1 <= (1 << 16) && stride >= 0 && stride <= (1 << 16) && im_scale > 0.0,
               "lsfa_image_resize_transform_yuv420p10: bad shape");
  const int ph = stride > 0 ? (h1 + stride - 1) / stride * stride : h1, pw = stride > 0 ? (w1 + stride - 1) / stride * stride : w1;
  if (ph != out_h || pw != out_w) {
    set_error("lsfa_image_resize_transform_yuv420p10: output is %d x %d, the resized %d x %d frame padded to %d gives %d x %d", out_h, out_w, h1, w1,
              stride, ph, pw);
    return LSFA_EINVAL;
  }
  const long total = (long)N * ph * pw;
  LSFA_REQUIRE(total < (1L << 36), "lsfa_image_resize_transform_yuv420p10: output too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_STEM, s);
  hipLaunchKernelGGL(resize_transform_yuv420p10_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, p, h1, w1, ph, pw,
                     1.0 / im_scale, pixel_means_bgr_host[0], pixel_means_bgr_host[1], pixel_means_bgr_host[2], pixel_scale, stride > 0 ? 1 : 0, data_nchw);
  LSFA_LAUNCH_CHECK("lsfa_image_resize_transform_yuv420p10");
  return LSFA_OK;
}
