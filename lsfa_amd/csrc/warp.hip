// Bilinear feature warp (GridGenerator 'warp' + BilinearSampler) with the fused key-path (x scale_map) and
// cur-path (+ rnet_conv0(res_diff) [bn] + small-net feature) epilogues.  Kernels: warp_kernels.h.
// See include/lsfa_hip.h for the reference interfaces it replaces.
//
// Four entry points, two host paths: warp_nchw (the gather kernel and, without bn, the LDS-staged one) and warp_cl (channels-last maps).
#include <atomic>
#include <type_traits>

#include "warp_kernels.h"

namespace {

using namespace lsfa;
using namespace lsfa::warp;

// Run-time flags -> template parameters: with_flags(f, b0, b1, ..) calls f(std::true_type or std::false_type for b0, for b1, ..).  Every
// kernel choice below goes through it, so an operand that is given and the epilogue step that reads it cannot come apart.
template <class F> void with_flags(F&& f) { f(); }
template <class F, class... Bs> void with_flags(F&& f, bool b, Bs... rest) {
  if (b) with_flags([&](auto... t) { f(std::true_type{}, t...); }, rest...);
  else with_flags([&](auto... t) { f(std::false_type{}, t...); }, rest...);
}

inline bool aligned(const void* p, size_t a) { return p == nullptr || ((uintptr_t)p % a) == 0; }

std::atomic<int> g_variant{0};       // lsfa_warp_set_variant: 0 auto, 1 gather kernel only, 2 staged kernel wherever it applies

// What both layouts ask of their arguments.
int check_args(const char* who, const float* feat, int feat_n, const float* flow, int N, int C, int H, int W, const float* res, int res_c,
               const float* res_w, const float* res_b, const float* out) {
  LSFA_REQUIRE(feat && flow && out, "%s: feat, flow and out must be non-NULL", who);
  LSFA_REQUIRE(N > 0 && C > 0 && H > 1 && W > 1, "%s: bad shape N=%d C=%d H=%d W=%d", who, N, C, H, W);
  LSFA_REQUIRE(feat_n >= 1 && N % feat_n == 0, "%s: feat batch %d must divide N=%d", who, feat_n, N);
  if (res) {
    LSFA_REQUIRE(res_w && res_b, "%s: res given without res_w/res_b", who);
    if (res_c < 1 || res_c > kResMax) {
      set_error("%s: res_c=%d not in [1,%d]", who, res_c, kResMax);
      return LSFA_ENOTSUP;
    }
  }
  return LSFA_OK;
}

constexpr int kStages = 3;

// The staged kernel's instance for the operands given: f(kernel).  rc3: the frame path's residual has 3 channels (rnet_conv0); those
// instances keep 3 values per pixel and unroll the dot product.
template <int THREADS, int NPAIR, int NDMA, class F>
void staged_instance(bool has_mul, bool has_add, bool has_res, bool rc3, F&& f) {
  with_flags([&](auto M, auto A, auto R, auto RC3) {
    if constexpr (R.value || !RC3.value) f(warp_staged_kernel<THREADS, NPAIR, NDMA, kStages, M.value, A.value, R.value, RC3.value ? 3 : 0>);
  }, has_mul, has_add, has_res, has_res && rc3);
}

// The staged kernel (warp_kernels.h, round 3) for one (THREADS, NPAIR, NDMA) configuration; returns false when the shape does not fit it.
template <int THREADS, int NPAIR, int NDMA>
bool launch_staged(hipStream_t s, StagedArgs a) {
  const int HW = a.H * a.W;
  constexpr int kRegion = THREADS * NDMA * 4;
  a.guard = (2 * a.W + 6 + 3) & ~3;
  // the lanes cover the plane; the DMA pass covers its chunks; the farthest tap (plane start + <= 3 floats of shift + H*W + 2W + 1, taken
  // and discarded for a flow that leaves the map at the bottom right) stays inside the slot
  if (HW > 2 * THREADS * NPAIR || (3 + HW + 3) / 4 > THREADS * NDMA || 3 + HW + 2 * a.W + 2 > kRegion + a.guard) return false;
  const int ops = (a.mul ? 1 : 0) + (a.add ? 1 : 0);
  const size_t lds_bytes = (size_t)kStages * (2 * a.guard + (1 + ops) * kRegion) * 4;
  if (lds_bytes > 160 * 1024) return false;
  // all twelve instances on the configuration's first use (not each on its own: the first use of one may come inside a graph capture)
  static lsfa::PerDeviceOnce attr;
  attr.run([] {
    for (int i = 0; i < 16; ++i)
      if (!(i & 8) || (i & 4))
        staged_instance<THREADS, NPAIR, NDMA>(i & 1, i & 2, i & 4, i & 8, [](auto* kernel) {
          (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        });
  });
  staged_instance<THREADS, NPAIR, NDMA>(a.mul != nullptr, a.add != nullptr, a.res != nullptr, a.res_c == 3, [&](auto* kernel) {
    hipLaunchKernelGGL(kernel, dim3(a.N * (a.C / a.cg)), dim3(THREADS), lds_bytes, s, a);
  });
  return true;
}

// lsfa_warp_bilinear (bn_s == NULL) and lsfa_warp_bilinear_bn (mul == NULL).  bn_s / bn_t: the small net's `bn_before_fuse`
// (resnet_v1_101_flownet_rfcn.py:231-235, :243-246), warp_conv_feat_bn between the warp and the addend.  The BatchNorm's shift does not
// commute with the warp's zero padding (a tap outside the map contributes 0, not 0 * s + t), so it cannot be folded into the key feature; it
// is an epilogue step instead: r = warp + rnet_conv0(res); r = r * bn_scale[c]; r = r + bn_shift[c]; r = r + add.  Only the gather kernel
// has it: a call with bn neither tries the staged kernel nor consults the variant switch.
int warp_nchw(const char* who, const float* feat, int feat_n, const float* flow, int N, int C, int H, int W, const float* mul, const float* add,
              const float* res, int res_c, const float* res_w, const float* res_b, const float* bn_s, const float* bn_t, float* out, void* stream) {
  if (int rc = check_args(who, feat, feat_n, flow, N, C, H, W, res, res_c, res_w, res_b, out)) return rc;
  LSFA_REQUIRE(N <= 65535, "%s: N=%d exceeds grid.z", who, N);
  LSFA_REQUIRE(!(mul && bn_s), "%s: no kernel takes mul together with bn", who);
  hipStream_t s = (hipStream_t)stream;
  const int HW = H * W;
  ProfScope prof(LSFA_OP_WARP, s);
  // round 3: planes staged in LDS by DMA (warp_staged_kernel) wherever the shape allows it: whole planes of 1,024 .. 4,096 even
  // pixels, 16-byte aligned maps whose images end on a 16-byte boundary, channel runs that divide C.  Same bits as warp_kernel.
  const int variant = bn_s ? 1 : g_variant.load();
  if (variant != 1 && HW % 2 == 0 && (HW >= 1024 || variant == 2) && ((size_t)C * HW) % 4 == 0 && aligned(feat, 16) && aligned(mul, 16) &&
      aligned(add, 16) && aligned(flow, 8) && aligned(res, 8) && aligned(out, 8)) {
    StagedArgs a = {feat, feat_n, flow, N, C, H, W, mul, add, res, res_c, res_w, res_b, out, 1, 0};
    const long planes = (long)N * C;
    // many planes: 4-wave workgroups of 8 channels, two or three to a CU (5.1-5.35 TB/s at 32 maps); few (one map = 1,024 planes):
    // 10-wave workgroups of 4 channels, one per CU and a short prologue (8.4 us against 9.1)
    bool done = false;
    auto run_len = [&](int want) { int g = want; while (g > 1 && C % g) g >>= 1; return g; };
    if (planes >= 4096) { a.cg = run_len(8); done = launch_staged<256, 5, 3>(s, a); }
    if (!done) { a.cg = run_len(planes >= 4096 ? 8 : 4); done = launch_staged<640, 2, 1>(s, a); }
    if (!done) { a.cg = run_len(planes >= 4096 ? 8 : 4); done = launch_staged<512, 4, 2>(s, a); }
    if (done) {
      LSFA_LAUNCH_CHECK(who);
      return LSFA_OK;
    }
  }
  if (variant == 2) { set_error("%s: the staged kernel does not take this shape / alignment", who); return LSFA_ENOTSUP; }
  int vec = (HW % 4 == 0) ? 4 : (HW % 2 == 0) ? 2 : 1;
  const size_t al = sizeof(float) * vec;
  if (!(aligned(flow, al) && aligned(mul, al) && aligned(add, al) && aligned(res, al) && aligned(out, al))) vec = 1;
  const int gx = ceil_div(HW, kThreads * vec);
  // enough workgroups to cover 256 CUs several times over, while amortising the tap
  // computation over the channel run
  int cpb = 8;
  while (cpb > 1 && (long)gx * ceil_div(C, cpb) * N < 1024) cpb >>= 1;
  const dim3 grid(gx, ceil_div(C, cpb), N);
  auto gather = [&](auto V) {
    with_flags([&](auto M, auto A, auto R, auto B) {
      if constexpr (!(M.value && B.value))
        hipLaunchKernelGGL((warp_kernel<V.value, M.value, A.value, R.value, B.value>), grid, dim3(kThreads), 0, s, feat, feat_n, flow, C, H, W, mul,
                           add, res, res_c, res_w, res_b, out, cpb, bn_s, bn_t);
    }, mul != nullptr, add != nullptr, res != nullptr, bn_s != nullptr);
  };
  if (vec == 4) gather(std::integral_constant<int, 4>{});
  else if (vec == 2) gather(std::integral_constant<int, 2>{});
  else gather(std::integral_constant<int, 1>{});
  LSFA_LAUNCH_CHECK(who);
  return LSFA_OK;
}

// lsfa_warp_bilinear_cl and lsfa_warp_bilinear_bn_cl: warp_cl_kernel (warp_kernels.h, r6) with its amax_out.
int warp_cl(const char* who, const float* feat_cl, int feat_n, const float* flow, int N, int C, int H, int W, const float* add_cl, const float* res,
            int res_c, const float* res_w, const float* res_b, const float* bn_s, const float* bn_t, float* out_cl, unsigned* amax_out, int amax_c0,
            void* stream) {
  if (int rc = check_args(who, feat_cl, feat_n, flow, N, C, H, W, res, res_c, res_w, res_b, out_cl)) return rc;
  LSFA_REQUIRE(C % 4 == 0, "%s: bad shape N=%d C=%d (a multiple of 4) H=%d W=%d", who, N, C, H, W);
  LSFA_REQUIRE(amax_c0 >= 0 && amax_c0 < C && amax_c0 % 4 == 0, "%s: amax_c0=%d must be a multiple of 4 in [0, C)", who, amax_c0);
  LSFA_REQUIRE(aligned(feat_cl, 16) && aligned(add_cl, 16) && aligned(out_cl, 16), "%s: maps must be 16-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  const long P = (long)N * H * W;
  LSFA_REQUIRE(P * C < (1L << 31), "%s: map of 2^31 elements or more", who);
  long per = P / 1536;                     // ~6 workgroups per CU; a run of pixels amortises the quad's residual weights
  if (per < 1) per = 1;
  if (per > 16) per = 16;
  const dim3 grid((unsigned)((P + per - 1) / per));
  ProfScope prof(LSFA_OP_WARP, s);
  with_flags([&](auto A, auto R, auto B) {
    hipLaunchKernelGGL((warp_cl_kernel<A.value, R.value, B.value>), grid, dim3(256), 0, s, feat_cl, feat_n, flow, N, C, H, W, add_cl, res, res_c,
                       res_w, res_b, out_cl, amax_out, amax_c0, (int)per, bn_s, bn_t);
  }, add_cl != nullptr, res != nullptr, bn_s != nullptr);
  LSFA_LAUNCH_CHECK(who);
  return LSFA_OK;
}

}  // namespace

extern "C" int lsfa_warp_set_variant(int variant) {
  LSFA_REQUIRE(variant >= 0 && variant <= 2, "lsfa_warp_set_variant: unknown variant %d", variant);
  g_variant.store(variant);
  return LSFA_OK;
}

extern "C" int lsfa_warp_bilinear(const float* feat, int feat_n, const float* flow, int N, int C, int H,
                                  int W, const float* mul, const float* add, const float* res, int res_c,
                                  const float* res_w, const float* res_b, float* out, void* stream) {
  return warp_nchw("lsfa_warp_bilinear", feat, feat_n, flow, N, C, H, W, mul, add, res, res_c, res_w, res_b, nullptr, nullptr, out, stream);
}

extern "C" int lsfa_warp_bilinear_cl(const float* feat_cl, int feat_n, const float* flow, int N, int C, int H, int W, const float* add_cl,
                                     const float* res, int res_c, const float* res_w, const float* res_b, float* out_cl, unsigned* amax_out,
                                     int amax_c0, void* stream) {
  return warp_cl("lsfa_warp_bilinear_cl", feat_cl, feat_n, flow, N, C, H, W, add_cl, res, res_c, res_w, res_b, nullptr, nullptr, out_cl, amax_out,
                 amax_c0, stream);
}

extern "C" int lsfa_warp_bilinear_bn(const float* feat, int feat_n, const float* flow, int N, int C, int H, int W, const float* add, const float* res,
                                     int res_c, const float* res_w, const float* res_b, const float* bn_scale, const float* bn_shift, float* out,
                                     void* stream) {
  LSFA_REQUIRE(bn_scale && bn_shift, "lsfa_warp_bilinear_bn: bn_scale and bn_shift must be non-NULL");
  return warp_nchw("lsfa_warp_bilinear_bn", feat, feat_n, flow, N, C, H, W, nullptr, add, res, res_c, res_w, res_b, bn_scale, bn_shift, out, stream);
}

extern "C" int lsfa_warp_bilinear_bn_cl(const float* feat_cl, int feat_n, const float* flow, int N, int C, int H, int W, const float* add_cl,
                                        const float* res, int res_c, const float* res_w, const float* res_b, const float* bn_scale,
                                        const float* bn_shift, float* out_cl, unsigned* amax_out, int amax_c0, void* stream) {
  LSFA_REQUIRE(bn_scale && bn_shift, "lsfa_warp_bilinear_bn_cl: bn_scale and bn_shift must be non-NULL");
  return warp_cl("lsfa_warp_bilinear_bn_cl", feat_cl, feat_n, flow, N, C, H, W, add_cl, res, res_c, res_w, res_b, bn_scale, bn_shift, out_cl,
                 amax_out, amax_c0, stream);
}
