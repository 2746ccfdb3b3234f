// YUV 4:2:0 intake: the planes a decoder hands over (libav, the VCN engines, a raw .yuv dump) - a full-resolution Y plane and half-resolution
// chroma, semi-planar (NV12: U, V interleaved) or planar (I420), each with its own row pitch - straight to the packed BGR frame
// lsfa_mv_residual reads, to the luma plane lsfa_mv_estimate searches and to the network's `data`, without a host-side colour conversion and
// with 1.5 instead of 3 bytes per pixel uploaded.
//
// NOT a port of anything in the reference: there swscale converts inside the coviar loader, on the CPU.  The conversion is DEFINED by the
// specification below (include/lsfa_hip.h; DESIGN.md "YUV intake"; tests/ref_yuv.py states it in numpy) - parity with swscale or OpenCV,
// which carry options such as chroma siting and bilinear chroma, is unpinned and not claimed.  Integer arithmetic, one answer per input:
//   pixel (x, y) takes Y[y][x] and the chroma sample (x >> 1, y >> 1) (nearest neighbour); chroma planes are ceil(W / 2) x ceil(H / 2);
//   C = Y - o, D = U - 128, E = V - 128;  >> is arithmetic;  clip clamps to 0..255;
//   matrix 0 (BT.601 limited)  o = 16  R = clip((298 C + 409 E + 128) >> 8)  G = clip((298 C - 100 D - 208 E + 128) >> 8)  B = clip((298 C + 516 D + 128) >> 8)
//   matrix 1 (BT.709 limited)  o = 16  R = clip((298 C + 459 E + 128) >> 8)  G = clip((298 C -  55 D - 136 E + 128) >> 8)  B = clip((298 C + 541 D + 128) >> 8)
//   matrix 2 (BT.601 full)     o = 0   R = clip((256 C + 359 E + 128) >> 8)  G = clip((256 C -  88 D - 183 E + 128) >> 8)  B = clip((256 C + 454 D + 128) >> 8)
// Out of scope: interpolated chroma, any binding to rocDecode.  10-bit samples (P010, yuv420p10le): yuv10.hip.  NV21, 4:2:2, 4:4:4: yuvfmt.hip.
//
// Bandwidth kernels.  yuv420_quad_kernel gives a thread four horizontally adjacent pixels of two rows: two Y dwords, one dword holding two
// U, V pairs (two half-words for I420) - every chroma sample is read once - and, for `data`, six 16-byte stores.  yuv420_bytes_kernel is the
// byte-wise form (a thread per pixel) for bases or pitches that are not aligned, W % 4 != 0 and an odd last row; the host picks one of the
// two per launch.  The resize form gathers its four taps per output pixel like resize_transform_kernel (mv.hip) and shares its tap and
// weight arithmetic (resize_kernels.h).  The two output forms of the plane kernels (BgrOut, DataOut) are yuv_out.h's, shared with yuv10.hip.
#include "common.h"
#include "resize_kernels.h"
#include "yuv_out.h"

using namespace lsfa;

namespace {

constexpr int kThreads = 256;

struct YuvPlanes {
  const unsigned char* y;
  const unsigned char* u;       // v == nullptr: interleaved U, V (NV12)
  const unsigned char* v;
  long long y_pitch, y_stride, c_pitch, c_stride;       // bytes: row to row, frame to frame
  int N, H, W;
  int o, cy, rv, gu, gv, bu;    // the matrix' row of the table above
};

__device__ __forceinline__ Bgr yuv_to_bgr(const YuvPlanes& p, int Y, int U, int V) {
  const int c = p.cy * (Y - p.o) + 128, d = U - 128, e = V - 128;
  Bgr o;
  o.r = clip255((c + p.rv * e) >> 8);
  o.g = clip255((c - p.gu * d - p.gv * e) >> 8);
  o.b = clip255((c + p.bu * d) >> 8);
  return o;
}

// pixel (x, y) of frame n, byte loads; *luma receives its Y
__device__ __forceinline__ Bgr yuv_pixel(const YuvPlanes& p, long n, int y, int x, int* luma) {
  const int Y = p.y[n * p.y_stride + (long)y * p.y_pitch + x];
  const long co = n * p.c_stride + (long)(y >> 1) * p.c_pitch;
  int U, V;
  if (p.v) { U = p.u[co + (x >> 1)]; V = p.v[co + (x >> 1)]; }
  else { U = p.u[co + 2 * (x >> 1)]; V = p.u[co + 2 * (x >> 1) + 1]; }
  *luma = Y;
  return yuv_to_bgr(p, Y, U, V);
}

// W % 4 == 0, H % 2 == 0, Y base / pitch / stride dword aligned, chroma dword (NV12) or half-word (I420) aligned: the host checks
template <class Out>
__global__ __launch_bounds__(kThreads) void yuv420_quad_kernel(YuvPlanes p, Out out) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  const int w4 = p.W >> 2, h2 = p.H >> 1;
  const long per = (long)w4 * h2;
  if (i >= p.N * per) return;
  const long n = i / per, r = i - n * per;
  const int ry = (int)(r / w4), qx = (int)(r - (long)ry * w4);
  const unsigned char* yr = p.y + n * p.y_stride + (long)(2 * ry) * p.y_pitch + 4 * qx;
  const uint32_t yd[2] = {*reinterpret_cast<const uint32_t*>(yr), *reinterpret_cast<const uint32_t*>(yr + p.y_pitch)};
  const long co = n * p.c_stride + (long)ry * p.c_pitch;
  int U[2], V[2];
  if (p.v) {
    const uint32_t u = *reinterpret_cast<const uint16_t*>(p.u + co + 2 * qx), v = *reinterpret_cast<const uint16_t*>(p.v + co + 2 * qx);
    U[0] = (int)(u & 255u); U[1] = (int)(u >> 8);
    V[0] = (int)(v & 255u); V[1] = (int)(v >> 8);
  } else {
    const uint32_t uv = *reinterpret_cast<const uint32_t*>(p.u + co + 4 * qx);       // U0 V0 U1 V1
    U[0] = (int)(uv & 255u); V[0] = (int)((uv >> 8) & 255u);
    U[1] = (int)((uv >> 16) & 255u); V[1] = (int)(uv >> 24);
  }
#pragma unroll
  for (int row = 0; row < 2; ++row) {
    Bgr c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = yuv_to_bgr(p, (int)((yd[row] >> (8 * k)) & 255u), U[k >> 1], V[k >> 1]);
    out.quad(n, (long)(2 * ry + row) * p.W + 4 * qx, c, yd[row]);
  }
}

template <class Out>
__global__ __launch_bounds__(kThreads) void yuv420_bytes_kernel(YuvPlanes p, Out out) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  const long hw = (long)p.H * p.W;
  if (i >= p.N * hw) return;
  const long n = i / hw, pix = i - n * hw;
  const int y = (int)(pix / p.W), x = (int)(pix - (long)y * p.W);
  int Y;
  const Bgr c = yuv_pixel(p, n, y, x, &Y);
  out.px(n, pix, c, Y);
}

// lsfa_image_resize_transform's is_u8 = 1 kernel with the taps converted from the planes: a thread per output pixel, the three channels together
__global__ __launch_bounds__(kThreads) void resize_transform_yuv420_kernel(YuvPlanes p, int h1, int w1, int ph, int pw, double inv_scale, double m0,
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
    const Bgr s00 = yuv_pixel(p, n, ty.i0, tx.i0, &Y), s01 = yuv_pixel(p, n, ty.i0, tx.i1, &Y);
    const Bgr s10 = yuv_pixel(p, n, ty.i1, tx.i0, &Y), s11 = yuv_pixel(p, n, ty.i1, tx.i1, &Y);
    b = resize_blend((float)s00.b, (float)s01.b, (float)s10.b, (float)s11.b, tx, ty);
    g = resize_blend((float)s00.g, (float)s01.g, (float)s10.g, (float)s11.g, tx, ty);
    rr = resize_blend((float)s00.r, (float)s01.r, (float)s10.r, (float)s11.r, tx, ty);
  }
  resize_transform_store(out + (size_t)n * 3 * plane + r, plane, b, g, rr, m0, m1, m2, pixel_scale, sub_f64);
}

int fill_planes(const char* who, YuvPlanes& p, const unsigned char* y, long long y_pitch, long long y_frame_stride, const unsigned char* u_or_uv,
                const unsigned char* v, long long c_pitch, long long c_frame_stride, int N, int H, int W, int matrix) {
  LSFA_REQUIRE(y && u_or_uv, "%s: NULL plane", who);
  LSFA_REQUIRE(N > 0 && H > 0 && W > 0 && H <= (1 << 16) && W <= (1 << 16) && (long long)N * H * W < (1LL << 36), "%s: bad shape: %d frames of %d x %d", who,
               N, W, H);
  LSFA_REQUIRE(matrix >= 0 && matrix <= 2, "%s: matrix %d is not 0 (BT.601 limited), 1 (BT.709 limited) or 2 (BT.601 full range)", who, matrix);
  LSFA_REQUIRE(y_pitch >= W, "%s: Y pitch %lld is below the row's %d bytes", who, y_pitch, W);
  const int cw = (W + 1) / 2, need = v ? cw : 2 * cw;
  LSFA_REQUIRE(c_pitch >= need, "%s: chroma pitch %lld is below the %s row's %d bytes", who, c_pitch, v ? "I420" : "NV12", need);
  p.y = y; p.u = u_or_uv; p.v = v;
  p.y_pitch = y_pitch; p.y_stride = y_frame_stride; p.c_pitch = c_pitch; p.c_stride = c_frame_stride;
  p.N = N; p.H = H; p.W = W;
  const int* m = kYuvMatrix[matrix];
  p.o = m[0]; p.cy = m[1]; p.rv = m[2]; p.gu = m[3]; p.gv = m[4]; p.bu = m[5];
  return LSFA_OK;
}

// may the launch take yuv420_quad_kernel?  (the outputs' alignment is the caller's part)
bool quad_ok(const YuvPlanes& p) {
  if ((p.W & 3) || (p.H & 1)) return false;
  if ((reinterpret_cast<uintptr_t>(p.y) | (uintptr_t)p.y_pitch | (uintptr_t)p.y_stride) & 3u) return false;
  const uintptr_t cm = p.v ? 1u : 3u;
  return ((reinterpret_cast<uintptr_t>(p.u) | reinterpret_cast<uintptr_t>(p.v) | (uintptr_t)p.c_pitch | (uintptr_t)p.c_stride) & cm) == 0;
}

template <class Out>
void launch(const YuvPlanes& p, const Out& out, bool quad, hipStream_t s) {
  if (quad) {
    const long total = (long)p.N * (p.H >> 1) * (p.W >> 2);
    hipLaunchKernelGGL(yuv420_quad_kernel<Out>, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, p, out);
  } else {
    const long total = (long)p.N * p.H * p.W;
    hipLaunchKernelGGL(yuv420_bytes_kernel<Out>, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, p, out);
  }
}

}  // namespace

extern "C" int lsfa_yuv420_to_bgr_u8(const unsigned char* y, long long y_pitch, long long y_frame_stride, const unsigned char* u_or_uv,
                                     const unsigned char* v, long long c_pitch, long long c_frame_stride, int N, int H, int W, int matrix,
                                     unsigned char* bgr, unsigned char* y_packed, void* stream) {
  YuvPlanes p;
  if (int rc = fill_planes("lsfa_yuv420_to_bgr_u8", p, y, y_pitch, y_frame_stride, u_or_uv, v, c_pitch, c_frame_stride, N, H, W, matrix)) return rc;
  LSFA_REQUIRE(bgr, "lsfa_yuv420_to_bgr_u8: NULL output");
  BgrOut out;
  out.bgr = bgr; out.y_packed = y_packed; out.hw = (long)H * W;
  const bool quad = quad_ok(p) && ((reinterpret_cast<uintptr_t>(bgr) | reinterpret_cast<uintptr_t>(y_packed)) & 3u) == 0;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_STEM, s);
  launch(p, out, quad, s);
  LSFA_LAUNCH_CHECK("lsfa_yuv420_to_bgr_u8");
  return LSFA_OK;
}

extern "C" int lsfa_image_transform_yuv420(const unsigned char* y, long long y_pitch, long long y_frame_stride, const unsigned char* u_or_uv,
                                           const unsigned char* v, long long c_pitch, long long c_frame_stride, int N, int H, int W, int matrix,
                                           const double* pixel_means_bgr_host, double pixel_scale, float* data_nchw, void* stream) {
  YuvPlanes p;
  if (int rc = fill_planes("lsfa_image_transform_yuv420", p, y, y_pitch, y_frame_stride, u_or_uv, v, c_pitch, c_frame_stride, N, H, W, matrix)) return rc;
  LSFA_REQUIRE(pixel_means_bgr_host && data_nchw, "lsfa_image_transform_yuv420: NULL argument");
  LSFA_REQUIRE((reinterpret_cast<uintptr_t>(data_nchw) & 3u) == 0, "lsfa_image_transform_yuv420: the output is not float aligned");
  DataOut out;
  out.out = data_nchw; out.hw = (long)H * W;
  out.m0 = pixel_means_bgr_host[0]; out.m1 = pixel_means_bgr_host[1]; out.m2 = pixel_means_bgr_host[2];
  out.scale = pixel_scale;
  const bool quad = quad_ok(p) && (reinterpret_cast<uintptr_t>(data_nchw) & 15u) == 0;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_STEM, s);
  launch(p, out, quad, s);
  LSFA_LAUNCH_CHECK("lsfa_image_transform_yuv420");
  return LSFA_OK;
}

extern "C" int lsfa_image_resize_transform_yuv420(const unsigned char* y, long long y_pitch, long long y_frame_stride, const unsigned char* u_or_uv,
                                                  const unsigned char* v, long long c_pitch, long long c_frame_stride, int N, int H, int W, int matrix,
                                                  double im_scale, int h1, int w1, int stride, const double* pixel_means_bgr_host, double pixel_scale,
                                                  float* data_nchw, int out_h, int out_w, void* stream) {
  YuvPlanes p;
  if (int rc = fill_planes("lsfa_image_resize_transform_yuv420", p, y, y_pitch, y_frame_stride, u_or_uv, v, c_pitch, c_frame_stride, N, H, W, matrix))
    return rc;
  LSFA_REQUIRE(pixel_means_bgr_host && data_nchw, "lsfa_image_resize_transform_yuv420: NULL argument");
  LSFA_REQUIRE(h1 > 0 && w1 > 0 && h1 <= (1 << 16) && w1 <= (1 << 16) && stride >= 0 && stride <= (1 << 16) && im_scale > 0.0,
               "lsfa_image_resize_transform_yuv420: bad shape");
  const int ph = stride > 0 ? (h1 + stride - 1) / stride * stride : h1, pw = stride > 0 ? (w1 + stride - 1) / stride * stride : w1;
  if (ph != out_h || pw != out_w) {
    set_error("lsfa_image_resize_transform_yuv420: output is %d x %d, the resized %d x %d frame padded to %d gives %d x %d", out_h, out_w, h1, w1, stride,
              ph, pw);
    return LSFA_EINVAL;
  }
  const long total = (long)N * ph * pw;
  LSFA_REQUIRE(total < (1L << 36), "lsfa_image_resize_transform_yuv420: output too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_STEM, s);
  hipLaunchKernelGGL(resize_transform_yuv420_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, p, h1, w1, ph, pw,
                     1.0 / im_scale, pixel_means_bgr_host[0], pixel_means_bgr_host[1], pixel_means_bgr_host[2], pixel_scale, stride > 0 ? 1 : 0, data_nchw);
  LSFA_LAUNCH_CHECK("lsfa_image_resize_transform_yuv420");
  return LSFA_OK;
}
