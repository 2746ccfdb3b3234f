// YUV intake: the frames a decoder, a capture card or a camera hands over - libav, the VCN engines, a raw .yuv dump - straight to the packed
// uint8 BGR frame lsfa_mv_residual reads, to the 8-bit luma plane lsfa_mv_estimate searches and to the network's `data`, without a host-side
// colour conversion.  ONE conversion and one kernel set behind all nine exports: the three lsfa_*yuv420* (8-bit NV12 / I420) and the three
// lsfa_*yuv420p10* (P010 / yuv420p10le) are lsfa_yuv_to_bgr_u8, lsfa_image_transform_yuv and lsfa_image_resize_transform_yuv at a format code.
//
// NOT a port of anything in the reference: there swscale converts inside the coviar loader, on the CPU.  The conversion is DEFINED by the
// specification (include/lsfa_hip.h, "YUV 4:2:0 intake", "10-bit YUV 4:2:0 intake", "YUV intake, other chroma formats"; DESIGN.md "YUV
// intake"; tests/ref_yuv.py, ref_yuv10.py and ref_yuvfmt.py state it in numpy) - parity with swscale or OpenCV, which carry options such as
// chroma siting and bilinear chroma, is unpinned and not claimed.  Integer arithmetic, one answer per input, every byte and word defined input:
//   C = Y - o, D = U - 128, E = V - 128;  >> is arithmetic;  clip clamps to 0..255;
//   matrix 0 (BT.601 limited)  o = 16  R = clip((298 C + 409 E + 128) >> 8)  G = clip((298 C - 100 D - 208 E + 128) >> 8)  B = clip((298 C + 516 D + 128) >> 8)
//   matrix 1 (BT.709 limited)  o = 16  R = clip((298 C + 459 E + 128) >> 8)  G = clip((298 C -  55 D - 136 E + 128) >> 8)  B = clip((298 C + 541 D + 128) >> 8)
//   matrix 2 (BT.601 full)     o = 0   R = clip((256 C + 359 E + 128) >> 8)  G = clip((256 C -  88 D - 183 E + 128) >> 8)  B = clip((256 C + 454 D + 128) >> 8)
//   ten-bit samples in 16-bit little-endian words, s = (w >> shift) & 1023: C = Y - 4 o, D = U - 512, E = V - 512, the same coefficients,
//   rounding constant 512 and >> 10 - converted in ten bits, rounded once, |intermediate| < 2^20; y_packed = min(255, (Y + 2) >> 2).  Planes
//   that are exactly 4 x an 8-bit plane give the 8-bit BGR and Y bit for bit.
// format = sub | layout << 4 | sample << 8:
//   sub     0: 4:2:0 (sx, sy) = (1, 1)   1: 4:2:2 (1, 0)   2: 4:4:4 (0, 0); pixel (x, y) takes Y[y][x] and the chroma sample (x >> sx, y >> sy),
//           nearest neighbour; chroma planes are ceil(W / 2^sx) x ceil(H / 2^sy)
//   layout  0: two planes U, V   1: one interleaved plane U, V   2: one interleaved plane V, U   3: packed Y0 U Y1 V   4: packed U Y0 V Y1
//           (3 and 4: sub = 1, sample = 0 only; the row is ceil(W / 2) four-byte groups in the `y` plane, no chroma planes)
//   sample  0: bytes   1: words, the value in the low ten bits (shift 0: yuv420p10le / I010)   2: in the high ten (shift 6: P010 / P016 surfaces)
// Out of scope: interpolated or sited chroma, packed 10-bit (v210, Y210, Y410), 12-bit and P016's low bits as signal, 4:1:1 / 4:1:0, YVYU,
// alpha, BT.2020 / HDR transfer, RGB, any binding to rocDecode.
//
// Bandwidth kernels, two per output form; the host picks one per launch.  Every format is reduced on the host to three sample addresses -
// the first Y, U and V with the bytes from a sample to the next of its kind - so the element-wise kernel (a thread per pixel, one- or
// two-byte loads) and the resize kernel take layout and subsampling at run time and know nothing of them; only bytes or words is compiled
// in.  yuvfmt_quad_kernel is compiled per format: a thread takes four horizontally adjacent pixels (of two rows for 4:2:0, of one row
// otherwise) and reads every chroma sample once - 4:2:0 two Y dwords and one dword of two U, V pairs (two half-words for planar chroma),
// 4:2:2 semi-planar one Y dword and one dword of two pairs, packed one 8-byte load of four whole pixels, 4:4:4 one Y dword and eight chroma
// bytes, words twice that - and stores through yuv_out.h's quad forms (for `data`, three 16-byte stores a row).  It needs W % 4 == 0, for
// 4:2:0 an even H, and every base, pitch and frame stride a multiple of the load it feeds.  The resize form gathers and converts its four
// taps per output pixel like resize_transform_kernel (mv.hip) and shares its tap and weight arithmetic (resize_kernels.h).
#include "common.h"
#include "resize_kernels.h"
#include "yuv_out.h"

using namespace lsfa;

namespace {

constexpr int kThreads = 256;

struct FmtPlanes {
  const unsigned char* y;       // the Y of pixel (0, 0)
  const unsigned char* u;       // the U and the V of chroma sample (0, 0): two planes, one interleaved plane or the packed plane itself
  const unsigned char* v;
  long long y_pitch, y_stride, c_pitch, c_stride;       // bytes: row to row, frame to frame
  int N, H, W;
  int sx, sy;                   // pixel (x, y) takes chroma sample (x >> sx, y >> sy)
  int y_step, c_step;           // bytes from a sample to the next of its kind in a row
  int words, shift;             // words: 16-bit words, the sample (w >> shift) & 1023; else bytes
  int o, cy, rv, gu, gv, bu;    // the matrix' row of kYuvMatrix, o in the sample's units
  int key;                      // host only: sub | layout << 4 | words << 8, what yuvfmt_quad_kernel is compiled for
  int quad;                     // host only: the geometry allows yuvfmt_quad_kernel (the outputs' alignment is the caller's part)
};

// the one conversion; clip_down (yuv_out.h) and nothing else clamps a channel
template <bool WORDS>
__device__ __forceinline__ Bgr fmt_to_bgr(const FmtPlanes& p, int Y, int U, int V) {
  constexpr int half = WORDS ? 512 : 128, down = WORDS ? 10 : 8;
  const int c = p.cy * (Y - p.o) + half, d = U - half, e = V - half;
  Bgr o;
  o.r = clip_down<down>(c + p.rv * e);
  o.g = clip_down<down>(c - p.gu * d - p.gv * e);
  o.b = clip_down<down>(c + p.bu * d);
  return o;
}

template <bool WORDS>
__device__ __forceinline__ int fmt_luma8(int Y) { return WORDS ? min(255, (Y + 2) >> 2) : Y; }

template <bool WORDS>
__device__ __forceinline__ int sample_at(const FmtPlanes& p, const unsigned char* a) {
  if constexpr (WORDS) return (int)(((uint32_t)*reinterpret_cast<const uint16_t*>(a) >> p.shift) & 1023u);
  else return (int)*a;
}

// pixel (x, y) of frame n, one load per sample; *luma receives its Y as 8 bits.  The layout and the subsampling are run-time values (the
// three addresses and their steps); bytes or words is compiled in, so that the loads of a thread are issued together and not one per branch
template <bool WORDS>
__device__ __forceinline__ Bgr fmt_pixel(const FmtPlanes& p, long n, int y, int x, int* luma) {
  const int Y = sample_at<WORDS>(p, p.y + n * p.y_stride + (long)y * p.y_pitch + (long)p.y_step * x);
  const long co = n * p.c_stride + (long)(y >> p.sy) * p.c_pitch + (long)p.c_step * (x >> p.sx);
  const int U = sample_at<WORDS>(p, p.u + co), V = sample_at<WORDS>(p, p.v + co);
  *luma = fmt_luma8<WORDS>(Y);
  return fmt_to_bgr<WORDS>(p, Y, U, V);
}

// BYTES (2, 4, 8 or 16, the address a multiple of it) as one load into dwords
template <int BYTES>
__device__ __forceinline__ void load_raw(const unsigned char* a, uint32_t (&r)[4]) {
  if constexpr (BYTES == 2) {
    r[0] = *reinterpret_cast<const uint16_t*>(a);
  } else if constexpr (BYTES == 4) {
    r[0] = *reinterpret_cast<const uint32_t*>(a);
  } else if constexpr (BYTES == 8) {
    const uint2 t = *reinterpret_cast<const uint2*>(a);
    r[0] = t.x; r[1] = t.y;
  } else {
    static_assert(BYTES == 16, "a load of 2, 4, 8 or 16 bytes");
    const uint4 t = *reinterpret_cast<const uint4*>(a);
    r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
  }
}

// sample k of what load_raw read
template <bool WORDS>
__device__ __forceinline__ int raw_sample(const FmtPlanes& p, const uint32_t (&r)[4], int k) {
  if constexpr (WORDS) return (int)((((r[k >> 1] >> (16 * (k & 1))) & 0xffffu) >> p.shift) & 1023u);
  else return (int)((r[k >> 2] >> (8 * (k & 3))) & 255u);
}

// W % 4 == 0, H % 2 == 0 where SY, every base / pitch / stride a multiple of the load it feeds (fill_planes' `quad`): the host checks
template <int SX, int SY, int LAYOUT, bool WORDS, class Out>
__global__ __launch_bounds__(kThreads) void yuvfmt_quad_kernel(FmtPlanes p, Out out) {
  constexpr int B = WORDS ? 2 : 1, ROWS = 1 << SY, NC = 4 >> SX;       // bytes per sample, rows per thread, chroma samples per four pixels
  constexpr bool PACKED = LAYOUT >= 3;
  static_assert(!PACKED || (SX == 1 && SY == 0 && !WORDS), "packed is 4:2:2 of bytes");
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  const int w4 = p.W >> 2, hr = p.H >> SY;
  const long per = (long)w4 * hr;
  if (i >= p.N * per) return;
  const long n = i / per, r = i - n * per;
  const int ry = (int)(r / w4), qx = (int)(r - (long)ry * w4);
  uint32_t yraw[ROWS][4] = {};
  int U[NC], V[NC];
  if constexpr (PACKED) {       // Y0 U Y1 V | Y2 U Y3 V (3) or U Y0 V Y1 | U Y2 V Y3 (4): four whole pixels in eight bytes
    load_raw<8>((LAYOUT == 3 ? p.y : p.y - 1) + n * p.y_stride + (long)ry * p.y_pitch + 8L * qx, yraw[0]);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      U[j] = raw_sample<false>(p, yraw[0], 4 * j + (LAYOUT == 3 ? 1 : 0));
      V[j] = raw_sample<false>(p, yraw[0], 4 * j + (LAYOUT == 3 ? 3 : 2));
    }
  } else {
    const unsigned char* yr = p.y + n * p.y_stride + (long)(ROWS * ry) * p.y_pitch + (long)(4 * B) * qx;
#pragma unroll
    for (int row = 0; row < ROWS; ++row) load_raw<4 * B>(yr + row * p.y_pitch, yraw[row]);
    const long co = n * p.c_stride + (long)ry * p.c_pitch;
    if constexpr (LAYOUT == 0) {
      uint32_t ur[4] = {}, vr[4] = {};
      load_raw<NC * B>(p.u + co + (long)(NC * B) * qx, ur);
      load_raw<NC * B>(p.v + co + (long)(NC * B) * qx, vr);
#pragma unroll
      for (int j = 0; j < NC; ++j) { U[j] = raw_sample<WORDS>(p, ur, j); V[j] = raw_sample<WORDS>(p, vr, j); }
    } else {                    // U V U V .. (1) or V U V U .. (2)
      uint32_t cr[4] = {};
      load_raw<2 * NC * B>((LAYOUT == 1 ? p.u : p.v) + co + (long)(2 * NC * B) * qx, cr);
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        U[j] = raw_sample<WORDS>(p, cr, 2 * j + (LAYOUT == 2 ? 1 : 0));
        V[j] = raw_sample<WORDS>(p, cr, 2 * j + (LAYOUT == 1 ? 1 : 0));
      }
    }
  }
#pragma unroll
  for (int row = 0; row < ROWS; ++row) {
    Bgr c[4];
    uint32_t ydw = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int Y = PACKED ? raw_sample<false>(p, yraw[0], 2 * k + (LAYOUT == 4 ? 1 : 0)) : raw_sample<WORDS>(p, yraw[row], k);
      c[k] = fmt_to_bgr<WORDS>(p, Y, U[k >> SX], V[k >> SX]);
      ydw |= (uint32_t)fmt_luma8<WORDS>(Y) << (8 * k);
    }
    out.quad(n, (long)(ROWS * ry + row) * p.W + 4 * qx, c, ydw);
  }
}

template <bool WORDS, class Out>
__global__ __launch_bounds__(kThreads) void yuvfmt_elems_kernel(FmtPlanes p, Out out) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  const long hw = (long)p.H * p.W;
  if (i >= p.N * hw) return;
  const long n = i / hw, pix = i - n * hw;
  const int y = (int)(pix / p.W), x = (int)(pix - (long)y * p.W);
  int Y;
  const Bgr c = fmt_pixel<WORDS>(p, n, y, x, &Y);
  out.px(n, pix, c, Y);
}

// lsfa_image_resize_transform's is_u8 = 1 kernel with the taps converted from the planes: a thread per output pixel, the three channels together
template <bool WORDS>
__global__ __launch_bounds__(kThreads) void resize_transform_yuvfmt_kernel(FmtPlanes p, int h1, int w1, int ph, int pw, double inv_scale, double m0,
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
    const Bgr s00 = fmt_pixel<WORDS>(p, n, ty.i0, tx.i0, &Y), s01 = fmt_pixel<WORDS>(p, n, ty.i0, tx.i1, &Y);
    const Bgr s10 = fmt_pixel<WORDS>(p, n, ty.i1, tx.i0, &Y), s11 = fmt_pixel<WORDS>(p, n, ty.i1, tx.i1, &Y);
    b = resize_blend((float)s00.b, (float)s01.b, (float)s10.b, (float)s11.b, tx, ty);
    g = resize_blend((float)s00.g, (float)s01.g, (float)s10.g, (float)s11.g, tx, ty);
    rr = resize_blend((float)s00.r, (float)s01.r, (float)s10.r, (float)s11.r, tx, ty);
  }
  resize_transform_store(out + (size_t)n * 3 * plane + r, plane, b, g, rr, m0, m1, m2, pixel_scale, sub_f64);
}

// with the 4:2:0 name of each: what a message of the 8-bit 4:2:0 exports calls its two layouts
const char* const kLayoutName[5] = {"planar (I420's)", "interleaved U, V (NV12's)", "interleaved V, U (NV21's)", "packed YUYV", "packed UYVY"};

int fill_planes(const char* who, FmtPlanes& p, const void* y, long long y_pitch, long long y_frame_stride, const void* u_or_uv, const void* v,
                long long c_pitch, long long c_frame_stride, int N, int H, int W, int matrix, int format) {
  const int sub = format & 15, layout = (format >> 4) & 15, sample = (format >> 8) & 15;
  LSFA_REQUIRE(format >= 0 && format < (1 << 12) && sub <= LSFA_YUV_444 && layout <= LSFA_YUV_UYVY && sample <= LSFA_YUV_HI10,
               "%s: format 0x%x is not sub (0..2) | layout (0..4) << 4 | sample (0..2) << 8", who, (unsigned)format);
  const bool packed = layout >= LSFA_YUV_YUYV, words = sample != LSFA_YUV_U8;
  LSFA_REQUIRE(!packed || (sub == LSFA_YUV_422 && !words), "%s: format 0x%x: the packed layouts exist only as 4:2:2 of bytes", who, (unsigned)format);
  LSFA_REQUIRE(N > 0 && H > 0 && W > 0 && H <= (1 << 16) && W <= (1 << 16) && (long long)N * H * W < (1LL << 36), "%s: bad shape: %d frames of %d x %d", who,
               N, W, H);
  LSFA_REQUIRE(matrix >= 0 && matrix <= 2, "%s: matrix %d is not 0 (BT.601 limited), 1 (BT.709 limited) or 2 (BT.601 full range)", who, matrix);
  LSFA_REQUIRE(y, "%s: NULL plane", who);
  if (packed) {
    LSFA_REQUIRE(!u_or_uv && !v && c_pitch == 0 && c_frame_stride == 0,
                 "%s: a %s frame is one plane: both chroma pointers must be NULL and the chroma pitch %lld and frame stride %lld zero", who,
                 kLayoutName[layout], c_pitch, c_frame_stride);
  } else {
    LSFA_REQUIRE(u_or_uv, "%s: NULL plane", who);
    LSFA_REQUIRE((layout == LSFA_YUV_PLANAR) == (v != nullptr), "%s: layout %d (%s) goes with %s", who, layout, kLayoutName[layout],
                 layout == LSFA_YUV_PLANAR ? "two chroma planes: v is NULL" : "one chroma plane: v must be NULL");
  }
  const int B = words ? 2 : 1;
  if (words) {
    LSFA_REQUIRE(((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(u_or_uv) | reinterpret_cast<uintptr_t>(v)) & 1u) == 0,
                 "%s: a plane of 16-bit words starts at an odd address", who);
    LSFA_REQUIRE((((unsigned long long)y_pitch | (unsigned long long)y_frame_stride | (unsigned long long)c_pitch | (unsigned long long)c_frame_stride) & 1u) == 0,
                 "%s: pitches and frame strides are bytes between 16-bit words and must be even: Y %lld / %lld, chroma %lld / %lld", who, y_pitch,
                 y_frame_stride, c_pitch, c_frame_stride);
  }
  const int sx = sub == LSFA_YUV_444 ? 0 : 1, sy = sub == LSFA_YUV_420 ? 1 : 0;
  const int cw = (W + (1 << sx) - 1) >> sx;
  const long long y_row = packed ? 4LL * cw : (long long)B * W;
  LSFA_REQUIRE(y_pitch >= y_row, "%s: %s pitch %lld is below the row's %lld bytes", who, packed ? kLayoutName[layout] : "Y", y_pitch, y_row);
  const unsigned char* yb = static_cast<const unsigned char*>(y);
  const unsigned char* cb = static_cast<const unsigned char*>(u_or_uv);
  if (packed) {
    p.y = yb + (layout == LSFA_YUV_UYVY ? 1 : 0); p.u = yb + (layout == LSFA_YUV_UYVY ? 0 : 1); p.v = p.u + 2;
    p.y_step = 2; p.c_step = 4;
    c_pitch = y_pitch; c_frame_stride = y_frame_stride;
  } else {
    const int c_row = (layout == LSFA_YUV_PLANAR ? 1 : 2) * B * cw;
    LSFA_REQUIRE(c_pitch >= c_row, "%s: chroma pitch %lld is below the %s row's %d bytes", who, c_pitch, kLayoutName[layout], c_row);
    p.y = yb; p.y_step = B;
    if (layout == LSFA_YUV_PLANAR) { p.u = cb; p.v = static_cast<const unsigned char*>(v); p.c_step = B; }
    else { p.u = cb + (layout == LSFA_YUV_VU ? B : 0); p.v = cb + (layout == LSFA_YUV_VU ? 0 : B); p.c_step = 2 * B; }
  }
  p.y_pitch = y_pitch; p.y_stride = y_frame_stride; p.c_pitch = c_pitch; p.c_stride = c_frame_stride;
  p.N = N; p.H = H; p.W = W;
  p.sx = sx; p.sy = sy;
  p.words = words ? 1 : 0; p.shift = sample == LSFA_YUV_HI10 ? 6 : 0;
  const int* m = kYuvMatrix[matrix];
  p.o = (words ? 4 : 1) * m[0]; p.cy = m[1]; p.rv = m[2]; p.gu = m[3]; p.gv = m[4]; p.bu = m[5];
  p.key = sub | layout << 4 | p.words << 8;
  // the loads of yuvfmt_quad_kernel: four Y samples (packed: four pixels); 4 >> sx samples of a chroma plane, twice that of an interleaved one
  const uintptr_t y_load = packed ? 8 : 4 * B, c_load = packed ? 8 : (uintptr_t)((layout == LSFA_YUV_PLANAR ? 1 : 2) * (4 >> sx) * B);
  p.quad = (W & 3) == 0 && (sy == 0 || (H & 1) == 0) &&
           ((reinterpret_cast<uintptr_t>(y) | (uintptr_t)y_pitch | (uintptr_t)y_frame_stride) & (y_load - 1)) == 0 &&
           ((reinterpret_cast<uintptr_t>(u_or_uv) | reinterpret_cast<uintptr_t>(v) | (uintptr_t)c_pitch | (uintptr_t)c_frame_stride) & (c_load - 1)) == 0;
  return LSFA_OK;
}

template <int SX, int SY, int LAYOUT, bool WORDS, class Out>
void launch_quad(const FmtPlanes& p, const Out& out, hipStream_t s) {
  const long total = (long)p.N * (p.H >> SY) * (p.W >> 2);
  auto quad_kernel = yuvfmt_quad_kernel<SX, SY, LAYOUT, WORDS, Out>;
  hipLaunchKernelGGL(quad_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, p, out);
}

template <class Out>
void launch(const FmtPlanes& p, const Out& out, bool quad, hipStream_t s) {
  if (!quad) {
    const long total = (long)p.N * p.H * p.W;
    auto elems_kernel = p.words ? yuvfmt_elems_kernel<true, Out> : yuvfmt_elems_kernel<false, Out>;
    hipLaunchKernelGGL(elems_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, p, out);
    return;
  }
  switch (p.key) {
#define LSFA_FMT(sub, sx, sy, layout)                                                               \
  case sub | layout << 4: launch_quad<sx, sy, layout, false>(p, out, s); break;                     \
  case sub | layout << 4 | 1 << 8: launch_quad<sx, sy, layout, true>(p, out, s); break;
    LSFA_FMT(0, 1, 1, 0) LSFA_FMT(0, 1, 1, 1) LSFA_FMT(0, 1, 1, 2)
    LSFA_FMT(1, 1, 0, 0) LSFA_FMT(1, 1, 0, 1) LSFA_FMT(1, 1, 0, 2)
    LSFA_FMT(2, 0, 0, 0) LSFA_FMT(2, 0, 0, 1) LSFA_FMT(2, 0, 0, 2)
#undef LSFA_FMT
    case 1 | 3 << 4: launch_quad<1, 0, 3, false>(p, out, s); break;
    case 1 | 4 << 4: launch_quad<1, 0, 4, false>(p, out, s); break;
  }
}

// ---- the three host bodies, one per output form.  `who` is the export that was called: every message names it ---------------------------
int to_bgr(const char* who, const void* y, long long y_pitch, long long y_frame_stride, const void* u_or_uv, const void* v, long long c_pitch,
           long long c_frame_stride, int N, int H, int W, int matrix, int format, unsigned char* bgr, unsigned char* y_packed, void* stream) {
  FmtPlanes p;
  if (int rc = fill_planes(who, p, y, y_pitch, y_frame_stride, u_or_uv, v, c_pitch, c_frame_stride, N, H, W, matrix, format)) return rc;
  LSFA_REQUIRE(bgr, "%s: NULL output", who);
  BgrOut out;
  out.bgr = bgr; out.y_packed = y_packed; out.hw = (long)H * W;
  const bool quad = p.quad && ((reinterpret_cast<uintptr_t>(bgr) | reinterpret_cast<uintptr_t>(y_packed)) & 3u) == 0;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_STEM, s);
  launch(p, out, quad, s);
  LSFA_LAUNCH_CHECK(who);
  return LSFA_OK;
}

int transform(const char* who, const void* y, long long y_pitch, long long y_frame_stride, const void* u_or_uv, const void* v, long long c_pitch,
              long long c_frame_stride, int N, int H, int W, int matrix, int format, const double* pixel_means_bgr_host, double pixel_scale,
              float* data_nchw, void* stream) {
  FmtPlanes p;
  if (int rc = fill_planes(who, p, y, y_pitch, y_frame_stride, u_or_uv, v, c_pitch, c_frame_stride, N, H, W, matrix, format)) return rc;
  LSFA_REQUIRE(pixel_means_bgr_host && data_nchw, "%s: NULL argument", who);
  LSFA_REQUIRE((reinterpret_cast<uintptr_t>(data_nchw) & 3u) == 0, "%s: the output is not float aligned", who);
  DataOut out;
  out.out = data_nchw; out.hw = (long)H * W;
  out.m0 = pixel_means_bgr_host[0]; out.m1 = pixel_means_bgr_host[1]; out.m2 = pixel_means_bgr_host[2];
  out.scale = pixel_scale;
  const bool quad = p.quad && (reinterpret_cast<uintptr_t>(data_nchw) & 15u) == 0;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_STEM, s);
  launch(p, out, quad, s);
  LSFA_LAUNCH_CHECK(who);
  return LSFA_OK;
}

int resize_transform(const char* who, const void* y, long long y_pitch, long long y_frame_stride, const void* u_or_uv, const void* v,
                     long long c_pitch, long long c_frame_stride, int N, int H, int W, int matrix, int format, double im_scale, int h1, int w1,
                     int stride, const double* pixel_means_bgr_host, double pixel_scale, float* data_nchw, int out_h, int out_w, void* stream) {
  FmtPlanes p;
  if (int rc = fill_planes(who, p, y, y_pitch, y_frame_stride, u_or_uv, v, c_pitch, c_frame_stride, N, H, W, matrix, format)) return rc;
  LSFA_REQUIRE(pixel_means_bgr_host && data_nchw, "%s: NULL argument", who);
  LSFA_REQUIRE((reinterpret_cast<uintptr_t>(data_nchw) & 3u) == 0, "%s: the output is not float aligned", who);
  LSFA_REQUIRE(h1 > 0 && w1 > 0 && h1 <= (1 << 16) && w1 <= (1 << 16) && stride >= 0 && stride <= (1 << 16) && im_scale > 0.0, "%s: bad shape", who);
  const int ph = stride > 0 ? (h1 + stride - 1) / stride * stride : h1, pw = stride > 0 ? (w1 + stride - 1) / stride * stride : w1;
  LSFA_REQUIRE(ph == out_h && pw == out_w, "%s: output is %d x %d, the resized %d x %d frame padded to %d gives %d x %d", who, out_h, out_w, h1, w1,
               stride, ph, pw);
  const long total = (long)N * ph * pw;
  LSFA_REQUIRE(total < (1L << 36), "%s: output too large", who);
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_STEM, s);
  auto resize_kernel = p.words ? resize_transform_yuvfmt_kernel<true> : resize_transform_yuvfmt_kernel<false>;
  hipLaunchKernelGGL(resize_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, p, h1, w1, ph, pw,
                     1.0 / im_scale, pixel_means_bgr_host[0], pixel_means_bgr_host[1], pixel_means_bgr_host[2], pixel_scale, stride > 0 ? 1 : 0, data_nchw);
  LSFA_LAUNCH_CHECK(who);
  return LSFA_OK;
}

// the 4:2:0 exports say their layout by `v` (NULL: one interleaved U, V plane) and, the 10-bit ones, their sample by `shift`
int format_420(const void* v, int sample) { return LSFA_YUV_FORMAT(LSFA_YUV_420, v ? LSFA_YUV_PLANAR : LSFA_YUV_UV, sample); }
int sample_10(int shift) { return shift == 6 ? LSFA_YUV_HI10 : LSFA_YUV_LO10; }
int check_shift(const char* who, int shift) {
  LSFA_REQUIRE(shift == 0 || shift == 6, "%s: shift %d is not 6 (P010: the sample in the high ten bits) or 0 (yuv420p10le: in the low ten)", who, shift);
  return LSFA_OK;
}

}  // namespace

// ---- the nine exports: the three of a format code, then the 4:2:0 ones as forwards to them -------------------------------------------------
extern "C" int lsfa_yuv_to_bgr_u8(const void* y, long long y_pitch, long long y_frame_stride, const void* u_or_uv, const void* v, long long c_pitch,
                                  long long c_frame_stride, int N, int H, int W, int matrix, int format, unsigned char* bgr, unsigned char* y_packed,
                                  void* stream) {
  return to_bgr("lsfa_yuv_to_bgr_u8", y, y_pitch, y_frame_stride, u_or_uv, v, c_pitch, c_frame_stride, N, H, W, matrix, format, bgr, y_packed, stream);
}

extern "C" int lsfa_image_transform_yuv(const void* y, long long y_pitch, long long y_frame_stride, const void* u_or_uv, const void* v, long long c_pitch,
                                        long long c_frame_stride, int N, int H, int W, int matrix, int format, const double* pixel_means_bgr_host,
                                        double pixel_scale, float* data_nchw, void* stream) {
  return transform("lsfa_image_transform_yuv", y, y_pitch, y_frame_stride, u_or_uv, v, c_pitch, c_frame_stride, N, H, W, matrix, format,
                   pixel_means_bgr_host, pixel_scale, data_nchw, stream);
}

extern "C" int lsfa_image_resize_transform_yuv(const void* y, long long y_pitch, long long y_frame_stride, const void* u_or_uv, const void* v,
                                               long long c_pitch, long long c_frame_stride, int N, int H, int W, int matrix, int format, double im_scale,
                                               int h1, int w1, int stride, const double* pixel_means_bgr_host, double pixel_scale, float* data_nchw,
                                               int out_h, int out_w, void* stream) {
  return resize_transform("lsfa_image_resize_transform_yuv", y, y_pitch, y_frame_stride, u_or_uv, v, c_pitch, c_frame_stride, N, H, W, matrix, format,
                          im_scale, h1, w1, stride, pixel_means_bgr_host, pixel_scale, data_nchw, out_h, out_w, stream);
}

extern "C" int lsfa_yuv420_to_bgr_u8(const unsigned char* y, long long y_pitch, long long y_frame_stride, const unsigned char* u_or_uv,
                                     const unsigned char* v, long long c_pitch, long long c_frame_stride, int N, int H, int W, int matrix,
                                     unsigned char* bgr, unsigned char* y_packed, void* stream) {
  return to_bgr("lsfa_yuv420_to_bgr_u8", y, y_pitch, y_frame_stride, u_or_uv, v, c_pitch, c_frame_stride, N, H, W, matrix,
                format_420(v, LSFA_YUV_U8), bgr, y_packed, stream);
}

extern "C" int lsfa_image_transform_yuv420(const unsigned char* y, long long y_pitch, long long y_frame_stride, const unsigned char* u_or_uv,
                                           const unsigned char* v, long long c_pitch, long long c_frame_stride, int N, int H, int W, int matrix,
                                           const double* pixel_means_bgr_host, double pixel_scale, float* data_nchw, void* stream) {
  return transform("lsfa_image_transform_yuv420", y, y_pitch, y_frame_stride, u_or_uv, v, c_pitch, c_frame_stride, N, H, W, matrix,
                   format_420(v, LSFA_YUV_U8), pixel_means_bgr_host, pixel_scale, data_nchw, stream);
}

extern "C" int lsfa_image_resize_transform_yuv420(const unsigned char* y, long long y_pitch, long long y_frame_stride, const unsigned char* u_or_uv,
                                                  const unsigned char* v, long long c_pitch, long long c_frame_stride, int N, int H, int W, int matrix,
                                                  double im_scale, int h1, int w1, int stride, const double* pixel_means_bgr_host, double pixel_scale,
                                                  float* data_nchw, int out_h, int out_w, void* stream) {
  return resize_transform("lsfa_image_resize_transform_yuv420", y, y_pitch, y_frame_stride, u_or_uv, v, c_pitch, c_frame_stride, N, H, W, matrix,
                          format_420(v, LSFA_YUV_U8), im_scale, h1, w1, stride, pixel_means_bgr_host, pixel_scale, data_nchw, out_h, out_w, stream);
}

extern "C" int lsfa_yuv420p10_to_bgr_u8(const void* y, long long y_pitch, long long y_frame_stride, const void* u_or_uv, const void* v, long long c_pitch,
                                        long long c_frame_stride, int N, int H, int W, int matrix, int shift, unsigned char* bgr,
                                        unsigned char* y_packed, void* stream) {
  if (int rc = check_shift("lsfa_yuv420p10_to_bgr_u8", shift)) return rc;
  return to_bgr("lsfa_yuv420p10_to_bgr_u8", y, y_pitch, y_frame_stride, u_or_uv, v, c_pitch, c_frame_stride, N, H, W, matrix,
                format_420(v, sample_10(shift)), bgr, y_packed, stream);
}

extern "C" int lsfa_image_transform_yuv420p10(const void* y, long long y_pitch, long long y_frame_stride, const void* u_or_uv, const void* v,
                                              long long c_pitch, long long c_frame_stride, int N, int H, int W, int matrix, int shift,
                                              const double* pixel_means_bgr_host, double pixel_scale, float* data_nchw, void* stream) {
  if (int rc = check_shift("lsfa_image_transform_yuv420p10", shift)) return rc;
  return transform("lsfa_image_transform_yuv420p10", y, y_pitch, y_frame_stride, u_or_uv, v, c_pitch, c_frame_stride, N, H, W, matrix,
                   format_420(v, sample_10(shift)), pixel_means_bgr_host, pixel_scale, data_nchw, stream);
}

extern "C" int lsfa_image_resize_transform_yuv420p10(const void* y, long long y_pitch, long long y_frame_stride, const void* u_or_uv, const void* v,
                                                     long long c_pitch, long long c_frame_stride, int N, int H, int W, int matrix, int shift,
                                                     double im_scale, int h1, int w1, int stride, const double* pixel_means_bgr_host,
                                                     double pixel_scale, float* data_nchw, int out_h, int out_w, void* stream) {
  if (int rc = check_shift("lsfa_image_resize_transform_yuv420p10", shift)) return rc;
  return resize_transform("lsfa_image_resize_transform_yuv420p10", y, y_pitch, y_frame_stride, u_or_uv, v, c_pitch, c_frame_stride, N, H, W, matrix,
                          format_420(v, sample_10(shift)), im_scale, h1, w1, stride, pixel_means_bgr_host, pixel_scale, data_nchw, out_h, out_w, stream);
}

