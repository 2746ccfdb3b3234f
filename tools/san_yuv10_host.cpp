// Host-side sanitiser run of lsfa_amd/csrc/yuv10.hip: the kernel source itself, compiled for the host with the launches run as loops
// (tools/host_hip/hip/hip_runtime.h), on the cases tools/san_yuv10_cases.py writes from tests/ref_yuv10.py - every geometry of
// tests/test_yuv10_gpu.py, both chroma layouts, both alignments, all three matrices.  Every buffer is allocated at exactly its promised size,
// so a load or store one byte outside it, or a wide access off its alignment, ends the run; every output must equal the reference bit for
// bit and lie between untouched guard values; the kernel each launch picked is checked too.  No GPU, no library, nothing loaded into python:
//   python tools/san_yuv10_cases.py cases.bin &&
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I tools/host_hip -I include -I lsfa_amd/csrc \
//       tools/san_yuv10_host.cpp -o san_yuv10_host && ./san_yuv10_host cases.bin
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

#include "yuv10.hip"

static int failures = 0;

static void fail(long id, const char* what) {
  printf("FAIL case %ld: %s (%s)\n", id, what, lsfa::last_error);
  ++failures;
}

// an allocation of exactly `off + n` bytes; the object starts `off` bytes in
struct Exact {
  unsigned char* base;
  unsigned char* p;
  Exact(size_t off, size_t n) : base((unsigned char*)malloc(off + n)), p(base + off) {}
  ~Exact() { free(base); }
};

static bool read_exact(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

int main(int argc, char** argv) {
  FILE* f = fopen(argc > 1 ? argv[1] : "san_yuv10_cases.bin", "rb");
  if (!f) { printf("no case file\n"); return 2; }
  long cases = 0, quads = 0;
  for (;; ++cases) {
    long long h[21];
    double d[5];
    if (fread(h, sizeof h, 1, f) != 1) break;
    if (fread(d, sizeof d, 1, f) != 1) { fail(cases, "short file"); break; }
    const int H = (int)h[0], W = (int)h[1], N = (int)h[2], semi = (int)h[3], shift = (int)h[4], matrix = (int)h[5];
    const long long y_pitch = h[6], y_fs = h[7], c_pitch = h[8], c_fs = h[9];
    const size_t y_off = (size_t)h[10], y_bytes = (size_t)h[11], c_off = (size_t)h[12], c_bytes = (size_t)h[13], out_off = (size_t)h[14];
    const int stride = (int)h[15], h1 = (int)h[16], w1 = (int)h[17], ph = (int)h[18], pw = (int)h[19], expect_quad = (int)h[20];
    const size_t px = (size_t)N * H * W, rpx = (size_t)N * 3 * ph * pw;
    Exact y(y_off, y_bytes), c(c_off, c_bytes), v(c_off, semi ? 0 : c_bytes);
    std::vector<unsigned char> want_bgr(px * 3), want_yp(px);
    std::vector<float> want_data(px * 3), want_rdata(rpx);
    if (!read_exact(f, y.p, y_bytes) || !read_exact(f, c.p, c_bytes) || !read_exact(f, v.p, semi ? 0 : c_bytes) || !read_exact(f, want_bgr.data(), px * 3) ||
        !read_exact(f, want_yp.data(), px) || !read_exact(f, want_data.data(), px * 12) || !read_exact(f, want_rdata.data(), rpx * 4)) {
      fail(cases, "short file");
      break;
    }
    const void* vp = semi ? nullptr : v.p;
    // BGR + y_packed, then BGR alone
    {
      Exact bgr(out_off, px * 3), yp(out_off ? 4 : 0, px), bgr2(out_off, px * 3);
      if (lsfa_yuv420p10_to_bgr_u8(y.p, y_pitch, y_fs, c.p, vp, c_pitch, c_fs, N, H, W, matrix, shift, bgr.p, yp.p, nullptr) != LSFA_OK) fail(cases, "to_bgr refused");
      const bool quad = strstr(host_last_kernel, "quad") != nullptr;
      quads += quad;
      if (quad != (expect_quad != 0)) fail(cases, quad ? "to_bgr took the quad kernel" : "to_bgr took the element-wise kernel");
      if (memcmp(bgr.p, want_bgr.data(), px * 3)) fail(cases, "bgr differs");
      if (memcmp(yp.p, want_yp.data(), px)) fail(cases, "y_packed differs");
      if (lsfa_yuv420p10_to_bgr_u8(y.p, y_pitch, y_fs, c.p, vp, c_pitch, c_fs, N, H, W, matrix, shift, bgr2.p, nullptr, nullptr) != LSFA_OK) fail(cases, "to_bgr refused");
      if (memcmp(bgr2.p, want_bgr.data(), px * 3)) fail(cases, "bgr without y_packed differs");
    }
    {
      Exact data(out_off * 4, px * 12);
      if (lsfa_image_transform_yuv420p10(y.p, y_pitch, y_fs, c.p, vp, c_pitch, c_fs, N, H, W, matrix, shift, d + 1, d[4], (float*)data.p, nullptr) != LSFA_OK)
        fail(cases, "transform refused");
      if ((strstr(host_last_kernel, "quad") != nullptr) != (expect_quad != 0)) fail(cases, "transform took the other kernel");
      if (memcmp(data.p, want_data.data(), px * 12)) fail(cases, "data differs");
    }
    {
      Exact rdata(0, rpx * 4);
      if (lsfa_image_resize_transform_yuv420p10(y.p, y_pitch, y_fs, c.p, vp, c_pitch, c_fs, N, H, W, matrix, shift, d[0], h1, w1, stride, d + 1, d[4],
                                                (float*)rdata.p, ph, pw, nullptr) != LSFA_OK)
        fail(cases, "resize refused");
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
    struct { const void* y; long long yp, yfs; const void* c; const void* v; long long cp, cfs; int N, H, W, m, s; unsigned char* o; } ok =
        {plane, 8, 0, plane, nullptr, 8, 0, 1, 2, 4, 0, 6, out}, b;
    int refused = 0, tried = 0;
#define TRY(change)                                                                                                                        \
  do {                                                                                                                                     \
    b = ok; change; ++tried;                                                                                                               \
    refused += lsfa_yuv420p10_to_bgr_u8(b.y, b.yp, b.yfs, b.c, b.v, b.cp, b.cfs, b.N, b.H, b.W, b.m, b.s, b.o, nullptr, nullptr) == LSFA_EINVAL;   \
    refused += lsfa_image_transform_yuv420p10(b.y, b.yp, b.yfs, b.c, b.v, b.cp, b.cfs, b.N, b.H, b.W, b.m, b.s, means, 1.0, (float*)b.o, nullptr) == LSFA_EINVAL; \
    refused += lsfa_image_resize_transform_yuv420p10(b.y, b.yp, b.yfs, b.c, b.v, b.cp, b.cfs, b.N, b.H, b.W, b.m, b.s, 1.0, 2, 4, 0, means, 1.0, (float*)b.o, 2, 4, \
                                                     nullptr) == LSFA_EINVAL;                                                             \
  } while (0)
    TRY(b.y = nullptr); TRY(b.c = nullptr); TRY(b.o = nullptr); TRY(b.N = 0); TRY(b.H = 0); TRY(b.W = -1); TRY(b.m = 3); TRY(b.m = -1);
    TRY(b.s = 2); TRY(b.s = 10); TRY(b.s = -6); TRY(b.y = plane + 1); TRY(b.c = plane + 1); TRY(b.v = plane + 1); TRY(b.yp = 9); TRY(b.cp = 9);
    TRY(b.yfs = 17); TRY(b.cfs = -3); TRY(b.yp = 6); TRY(b.cp = 6); TRY(b.v = plane; b.cp = 2);
#undef TRY
    if (refused != 3 * tried || strcmp(host_last_kernel, "none")) { printf("FAIL refusals: %d of %d, last launch %s\n", refused, 3 * tried, host_last_kernel); ++failures; }
    printf("%d of %d refusals as declared\n", refused, 3 * tried);
  }
  printf("%ld cases (%ld through the quad kernel), %d failures\n", cases, quads, failures);
  return failures || cases == 0 ? 1 : 0;
}
