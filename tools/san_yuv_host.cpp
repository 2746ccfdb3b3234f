// Host-side sanitiser run of lsfa_amd/csrc/yuvfmt.hip, the one intake source: the kernel source itself, compiled for the host with the
// launches run as loops (tools/host_hip/hip/hip_runtime.h), on the cases tools/san_yuv_cases.py writes from tests/ref_yuvfmt.py, ref_yuv.py
// and ref_yuv10.py - lsfa_*_yuv on every geometry of tests/test_yuvfmt_gpu.py, all 29 formats and all three matrices; the six 4:2:0
// exports (lsfa_*yuv420*, lsfa_*yuv420p10*) on the geometries of tests/test_yuv_gpu.py and tests/test_yuv10_gpu.py, both layouts, both
// alignments.  Every buffer is allocated at exactly its promised size, so a load or store one byte outside it, or a wide access off its
// alignment, ends the run; every output must equal the reference bit for bit; the kernel each launch picked is checked too, and every
// refusal must come back as LSFA_EINVAL without a launch.  No GPU, no library, nothing loaded into python:
//   python tools/san_yuv_cases.py cases.bin &&
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I tools/host_hip -I include -I lsfa_amd/csrc \
//       tools/san_yuv_host.cpp -o san_yuv_host && ./san_yuv_host cases.bin
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "common.h"

thread_local dim3 blockIdx, threadIdx, gridDim;
const char* host_last_kernel = "";

// what runtime.hip gives the library
namespace lsfa {
static char last_error[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(last_error, sizeof last_error, fmt, ap);
  va_end(ap);
}
int hip_fail(hipError_t e, const char* what) { set_error("%s: launch failed", what); return (int)e; }
ProfScope::ProfScope(int, hipStream_t stream) : stream_(stream), slot_(-1) {}
ProfScope::~ProfScope() {}
}  // namespace lsfa

#include "yuvfmt.hip"

static int failures = 0;

static void fail(long id, const char* what) {
  printf("FAIL case %ld: %s (%s)\n", id, what, lsfa::last_error);
  ++failures;
}

// an allocation of exactly `off + n` bytes; the object starts `off` bytes in.  n == 0: no object at all
struct Exact {
  unsigned char* base;
  unsigned char* p;
  Exact(size_t off, size_t n) : base(n ? (unsigned char*)malloc(off + n) : nullptr), p(n ? base + off : nullptr) {}
  ~Exact() { free(base); }
};

static bool read_exact(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

// the three exports of a case's entry on the plane arguments: 0 lsfa_*_yuv at the format, 1 lsfa_*yuv420* (the layout is said by v),
// 2 lsfa_*yuv420p10* (and the sample by shift s).  o: the output of the refusals below
struct Planes { const void* y; long long yp, yfs; const void* c; const void* v; long long cp, cfs; int N, H, W, m, f; unsigned char* o; int entry, s; };

static int shift_of(int format) { return (format >> 8) == LSFA_YUV_HI10 ? 6 : 0; }
static const unsigned char* u8(const void* p) { return static_cast<const unsigned char*>(p); }

static int to_bgr(const Planes& k, unsigned char* bgr, unsigned char* yp) {
  if (k.entry == 1) return lsfa_yuv420_to_bgr_u8(u8(k.y), k.yp, k.yfs, u8(k.c), u8(k.v), k.cp, k.cfs, k.N, k.H, k.W, k.m, bgr, yp, nullptr);
  if (k.entry == 2) return lsfa_yuv420p10_to_bgr_u8(k.y, k.yp, k.yfs, k.c, k.v, k.cp, k.cfs, k.N, k.H, k.W, k.m, k.s, bgr, yp, nullptr);
  return lsfa_yuv_to_bgr_u8(k.y, k.yp, k.yfs, k.c, k.v, k.cp, k.cfs, k.N, k.H, k.W, k.m, k.f, bgr, yp, nullptr);
}

static int transform(const Planes& k, const double* means, double scale, float* data) {
  if (k.entry == 1) return lsfa_image_transform_yuv420(u8(k.y), k.yp, k.yfs, u8(k.c), u8(k.v), k.cp, k.cfs, k.N, k.H, k.W, k.m, means, scale, data, nullptr);
  if (k.entry == 2)
    return lsfa_image_transform_yuv420p10(k.y, k.yp, k.yfs, k.c, k.v, k.cp, k.cfs, k.N, k.H, k.W, k.m, k.s, means, scale, data, nullptr);
  return lsfa_image_transform_yuv(k.y, k.yp, k.yfs, k.c, k.v, k.cp, k.cfs, k.N, k.H, k.W, k.m, k.f, means, scale, data, nullptr);
}

static int resize(const Planes& k, double im_scale, int h1, int w1, int stride, const double* means, double scale, float* data, int ph, int pw) {
  if (k.entry == 1)
    return lsfa_image_resize_transform_yuv420(u8(k.y), k.yp, k.yfs, u8(k.c), u8(k.v), k.cp, k.cfs, k.N, k.H, k.W, k.m, im_scale, h1, w1, stride, means, scale,
                                              data, ph, pw, nullptr);
  if (k.entry == 2)
    return lsfa_image_resize_transform_yuv420p10(k.y, k.yp, k.yfs, k.c, k.v, k.cp, k.cfs, k.N, k.H, k.W, k.m, k.s, im_scale, h1, w1, stride, means,
                                                 scale, data, ph, pw, nullptr);
  return lsfa_image_resize_transform_yuv(k.y, k.yp, k.yfs, k.c, k.v, k.cp, k.cfs, k.N, k.H, k.W, k.m, k.f, im_scale, h1, w1, stride, means, scale, data, ph,
                                         pw, nullptr);
}

int main(int argc, char** argv) {
  FILE* f = fopen(argc > 1 ? argv[1] : "san_yuv_cases.bin", "rb");
  if (!f) { printf("no case file\n"); return 2; }
  long cases = 0, quads = 0, per_entry[3] = {0, 0, 0}, quads_per_entry[3] = {0, 0, 0};
  for (;; ++cases) {
    long long h[22];
    double d[5];
    if (fread(h, sizeof h, 1, f) != 1) break;
    if (fread(d, sizeof d, 1, f) != 1) { fail(cases, "short file"); break; }
    const int H = (int)h[0], W = (int)h[1], N = (int)h[2], format = (int)h[3], chroma = (int)h[4], matrix = (int)h[5];
    const long long y_pitch = h[6], y_fs = h[7], c_pitch = h[8], c_fs = h[9];
    const size_t y_off = (size_t)h[10], y_bytes = (size_t)h[11], c_off = (size_t)h[12], c_bytes = (size_t)h[13], out_off = (size_t)h[14];
    const int stride = (int)h[15], h1 = (int)h[16], w1 = (int)h[17], ph = (int)h[18], pw = (int)h[19], expect_quad = (int)h[20], entry = (int)h[21];
    if (entry < 0 || entry > 2) { fail(cases, "bad entry"); break; }
    const size_t px = (size_t)N * H * W, rpx = (size_t)N * 3 * ph * pw;
    Exact y(y_off, y_bytes), c(c_off, chroma >= 1 ? c_bytes : 0), v(c_off, chroma == 2 ? c_bytes : 0);
    std::vector<unsigned char> want_bgr(px * 3), want_yp(px);
    std::vector<float> want_data(px * 3), want_rdata(rpx);
    if (!read_exact(f, y.p, y_bytes) || !read_exact(f, c.p, chroma >= 1 ? c_bytes : 0) || !read_exact(f, v.p, chroma == 2 ? c_bytes : 0) ||
        !read_exact(f, want_bgr.data(), px * 3) || !read_exact(f, want_yp.data(), px) || !read_exact(f, want_data.data(), px * 12) ||
        !read_exact(f, want_rdata.data(), rpx * 4)) {
      fail(cases, "short file");
      break;
    }
    const Planes k = {y.p, y_pitch, y_fs, c.p, v.p, c_pitch, c_fs, N, H, W, matrix, format, nullptr, entry, shift_of(format)};
    ++per_entry[entry];
    // BGR + y_packed, then BGR alone
    {
      Exact bgr(out_off, px * 3), yp(out_off ? 4 : 0, px), bgr2(out_off, px * 3);
      if (to_bgr(k, bgr.p, yp.p) != LSFA_OK) fail(cases, "to_bgr refused");
      const bool quad = strstr(host_last_kernel, "quad") != nullptr;
      quads += quad;
      quads_per_entry[entry] += quad;
      if (quad != (expect_quad != 0)) fail(cases, quad ? "to_bgr took the quad kernel" : "to_bgr took the element-wise kernel");
      if (memcmp(bgr.p, want_bgr.data(), px * 3)) fail(cases, "bgr differs");
      if (memcmp(yp.p, want_yp.data(), px)) fail(cases, "y_packed differs");
      if (to_bgr(k, bgr2.p, nullptr) != LSFA_OK) fail(cases, "to_bgr refused");
      if (memcmp(bgr2.p, want_bgr.data(), px * 3)) fail(cases, "bgr without y_packed differs");
    }
    {
      Exact data(out_off * 4, px * 12);
      if (transform(k, d + 1, d[4], (float*)data.p) != LSFA_OK) fail(cases, "transform refused");
      if ((strstr(host_last_kernel, "quad") != nullptr) != (expect_quad != 0)) fail(cases, "transform took the other kernel");
      if (memcmp(data.p, want_data.data(), px * 12)) fail(cases, "data differs");
    }
    {
      Exact rdata(0, rpx * 4);
      if (resize(k, d[0], h1, w1, stride, d + 1, d[4], (float*)rdata.p, ph, pw) != LSFA_OK) fail(cases, "resize refused");
      if (memcmp(rdata.p, want_rdata.data(), rpx * 4)) fail(cases, "resized data differs");
    }
  }
  fclose(f);
  // the refusals: nothing may be launched (host_last_kernel stays) and nothing dereferenced
  {
    alignas(16) static unsigned char plane[64];
    alignas(16) static unsigned char out[256];
    static const double means[3] = {0, 0, 0};
    host_last_kernel = "none";
    const int nv16 = LSFA_YUV_FORMAT(LSFA_YUV_422, LSFA_YUV_UV, LSFA_YUV_U8), yuyv = LSFA_YUV_FORMAT(LSFA_YUV_422, LSFA_YUV_YUYV, LSFA_YUV_U8);
    const int p210 = LSFA_YUV_FORMAT(LSFA_YUV_422, LSFA_YUV_UV, LSFA_YUV_HI10), i422 = LSFA_YUV_FORMAT(LSFA_YUV_422, LSFA_YUV_PLANAR, LSFA_YUV_U8);
    const int nv12 = LSFA_YUV_FORMAT(LSFA_YUV_420, LSFA_YUV_UV, LSFA_YUV_U8);
    typedef Planes Call;
    const Call ok = {plane, 8, 0, plane, nullptr, 8, 0, 1, 2, 4, 0, nv16, out}, okp = {plane, 8, 0, nullptr, nullptr, 0, 0, 1, 2, 4, 0, yuyv, out};
    const Call okw = {plane, 8, 0, plane, nullptr, 8, 0, 1, 2, 4, 0, p210, out}, okpl = {plane, 8, 0, plane, plane, 8, 0, 1, 2, 4, 0, i422, out};
    // the 4:2:0 exports: NV12 bytes through lsfa_*yuv420*, P010 words through lsfa_*yuv420p10*
    const Call ok8 = {plane, 8, 0, plane, nullptr, 8, 0, 1, 2, 4, 0, nv12, out, 1, 0}, ok10 = {plane, 8, 0, plane, nullptr, 8, 0, 1, 2, 4, 0, nv12, out, 2, 6};
    Call b;
    int refused = 0, tried = 0;
    auto three = [&](const Call& k, int expect) {
      return (to_bgr(k, k.o, nullptr) == expect) + (transform(k, means, 1.0, (float*)k.o) == expect) +
             (resize(k, 1.0, 2, 4, 0, means, 1.0, (float*)k.o, 2, 4) == expect);
    };
#define TRY(from, change) do { b = from; change; ++tried; refused += three(b, LSFA_EINVAL); } while (0)
    TRY(ok, b.y = nullptr); TRY(ok, b.c = nullptr); TRY(ok, b.o = nullptr); TRY(ok, b.N = 0); TRY(ok, b.H = 0); TRY(ok, b.W = -1); TRY(ok, b.m = 3);
    TRY(ok, b.m = -1); TRY(ok, b.yp = 3); TRY(ok, b.cp = 3); TRY(ok, b.yp = 0); TRY(ok, b.yp = -8); TRY(ok, b.v = plane);
    TRY(ok, b.f = 3); TRY(ok, b.f = 5 << 4 | 1); TRY(ok, b.f = 3 << 8 | 1); TRY(ok, b.f = 1 << 12 | nv16); TRY(ok, b.f = -1); TRY(ok, b.f = 15);
    TRY(okp, b.f = LSFA_YUV_FORMAT(LSFA_YUV_420, LSFA_YUV_YUYV, LSFA_YUV_U8)); TRY(okp, b.f = LSFA_YUV_FORMAT(LSFA_YUV_444, LSFA_YUV_UYVY, LSFA_YUV_U8));
    TRY(okp, b.f = LSFA_YUV_FORMAT(LSFA_YUV_422, LSFA_YUV_YUYV, LSFA_YUV_LO10)); TRY(okp, b.f = LSFA_YUV_FORMAT(LSFA_YUV_422, LSFA_YUV_UYVY, LSFA_YUV_HI10));
    TRY(okp, b.y = nullptr); TRY(okp, b.c = plane); TRY(okp, b.v = plane); TRY(okp, b.cp = 8); TRY(okp, b.cfs = 16); TRY(okp, b.yp = 7); TRY(okp, b.o = nullptr);
    TRY(okp, b.W = 5);          // three groups: 12 bytes
    TRY(okpl, b.v = nullptr); TRY(okpl, b.cp = 1); TRY(okpl, b.f = LSFA_YUV_FORMAT(LSFA_YUV_444, LSFA_YUV_PLANAR, LSFA_YUV_U8); b.cp = 3);
    TRY(ok, b.f = LSFA_YUV_FORMAT(LSFA_YUV_444, LSFA_YUV_VU, LSFA_YUV_U8); b.cp = 7);
    TRY(okw, b.y = plane + 1); TRY(okw, b.c = plane + 1); TRY(okw, b.yp = 9); TRY(okw, b.cp = 9); TRY(okw, b.yfs = 17); TRY(okw, b.cfs = -3); TRY(okw, b.yp = 6);
    TRY(okw, b.cp = 6); TRY(okw, b.f = LSFA_YUV_FORMAT(LSFA_YUV_422, LSFA_YUV_PLANAR, LSFA_YUV_LO10); b.v = plane + 1; b.cp = 4);
    TRY(ok8, b.y = nullptr); TRY(ok8, b.c = nullptr); TRY(ok8, b.o = nullptr); TRY(ok8, b.N = 0); TRY(ok8, b.H = 0); TRY(ok8, b.H = -3); TRY(ok8, b.W = 0);
    TRY(ok8, b.m = 3); TRY(ok8, b.m = -1); TRY(ok8, b.yp = 3); TRY(ok8, b.cp = 3); TRY(ok8, b.yp = 0); TRY(ok8, b.yp = -8); TRY(ok8, b.v = plane; b.cp = 1);
    TRY(ok10, b.y = nullptr); TRY(ok10, b.c = nullptr); TRY(ok10, b.o = nullptr); TRY(ok10, b.N = 0); TRY(ok10, b.H = 0); TRY(ok10, b.W = -1); TRY(ok10, b.m = 3);
    TRY(ok10, b.m = -1); TRY(ok10, b.s = 2); TRY(ok10, b.s = 10); TRY(ok10, b.s = -6); TRY(ok10, b.y = plane + 1); TRY(ok10, b.c = plane + 1);
    TRY(ok10, b.v = plane + 1); TRY(ok10, b.yp = 9); TRY(ok10, b.cp = 9); TRY(ok10, b.yfs = 17); TRY(ok10, b.cfs = -3); TRY(ok10, b.yp = 6); TRY(ok10, b.cp = 6);
    TRY(ok10, b.v = plane; b.cp = 2);
#undef TRY
    if (refused != 3 * tried || strcmp(host_last_kernel, "none")) { printf("FAIL refusals: %d of %d, last launch %s\n", refused, 3 * tried, host_last_kernel); ++failures; }
    printf("%d of %d refusals as declared\n", refused, 3 * tried);
    // ... and the six calls they were made from are taken
    int taken = three(ok, LSFA_OK) + three(okp, LSFA_OK) + three(okw, LSFA_OK) + three(okpl, LSFA_OK) + three(ok8, LSFA_OK) + three(ok10, LSFA_OK);
    if (taken != 18) { printf("FAIL: %d of 18 well-formed calls taken (%s)\n", taken, lsfa::last_error); ++failures; }
  }
  const char* const names[3] = {"lsfa_*_yuv", "lsfa_*yuv420*", "lsfa_*yuv420p10*"};
  for (int e = 0; e < 3; ++e) {
    printf("%s: %ld cases (%ld through the quad kernel)\n", names[e], per_entry[e], quads_per_entry[e]);
    if (per_entry[e] == 0 || quads_per_entry[e] == 0 || quads_per_entry[e] == per_entry[e]) { printf("FAIL: %s did not see both kernels\n", names[e]); ++failures; }
  }
  printf("%ld cases (%ld through the quad kernel), %d failures\n", cases, quads, failures);
  return failures || cases == 0 ? 1 : 0;
}
