// fp32 implicit-GEMM convolution on channels-last maps with the fp32 matrix cores
// (v_mfma_f32_32x32x2_f32: exact fp32 products and sums, the chip's fp32 peak).
//
// What it is for: conv2 of the pre-activation ResNet units (3x3, stride 1 or 2, dilation d, folded
// bn3 bias + ReLU; dff_rfcn/symbols/resnet.py:70-101, sym_common.py:92-135) on (H*W, C) rows.  At
// LSFA's size the stage-3 instance is a SMALL GEMM — 2394 pixels x 256 channels x K = 2304 — for a
// 256-CU part: 600 output tiles of 32x32 for 1024 SIMDs.  An fp32 MFMA occupies its SIMD for 64
// cycles whatever else is resident, so the time is (tile-tasks per SIMD, rounded up) x (MFMAs per
// task) x 64 cycles, and the lever is the task count, not occupancy:
//   * a workgroup computes a 64-pixel x 64-channel tile with 4 waves (one 32x32 accumulator tile each:
//     16 VGPRs), K walked tap by tap in 64-channel chunks (32 when Cin % 64 != 0), staged through LDS,
//     double-buffered;
//   * gridDim.z splits the TAPS over workgroups (3 x 3 taps for a 3x3 kernel) when the tile grid alone
//     would leave SIMDs idle; the slices write fp32 partial tiles to the workspace and a second kernel
//     adds them in a fixed order and applies bias + ReLU — deterministic, unlike the library's atomic
//     split-K (its `gkgs` kernels) which also needs a zero-fill launch;
//   * the MFMA sums over k in any order we like, as long as A and B agree: a lane reads 4 consecutive
//     k of its row/column with ONE ds_read_b128 (lanes 0-31 take k = 8c..8c+3, lanes 32-63 take
//     8c+4..8c+7) and feeds 4 MFMAs from it; LDS rows are padded by 4 floats, which spreads the 16
//     lanes of a b128 group over all 64 banks.
// Zero padding is realised when a chunk is staged (out-of-map pixels load zeros).
// Weight layout (prepared once at bind time): w[co][tap][ci], i.e. K contiguous per output channel.
#include "common.h"

#include <stdlib.h>

#include <algorithm>

using namespace lsfa;

namespace {

constexpr int kBM = 64, kBN = 64;
constexpr int kThreads = 256;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ConvArgs {
  const float* x; const float* w; const float* bias; float* y; float* part;
  int N, H, W, Cin, Cout, kh, kw, stride, pad, dil, Ho, Wo, relu, taps_per_slice;
  // fused tail of a pre-activation unit's conv3 (resnet.py:93-101): y = conv + residual (in place allowed), and the
  // NEXT unit's bn1 + ReLU of that sum as a second output: y2 = max(y * scale2[c] + shift2[c], 0)
  const float* res; float* y2; const float* scale2; const float* shift2;
  int y_nchw;      // conv_reduce_kernel only: y / y2 / res are NCHW (the partial slices are always NHWC)
};

__device__ __forceinline__ void conv_epilogue(const ConvArgs& a, float v, size_t o, int ch, float bias, float sc2, float sh2) {
  v = v + bias;
  if (a.res) v = v + a.res[o];
  if (a.relu) v = fmaxf(v, 0.f);
  a.y[o] = v;
  if (a.y2) a.y2[o] = fmaxf(v * sc2 + sh2, 0.f);
  (void)ch;
}

// grid (ceil(P / 64), Cout / 64, slices); block 256.  P = N*Ho*Wo output pixels.  BK = channels per staged chunk
// (64 when Cin allows: 32 MFMAs per wave between barriers, long enough to cover the L2 latency of the next
// chunk's loads with the ~2 waves per SIMD these small grids leave; 32 otherwise).
template <int BK>
__global__ __launch_bounds__(kThreads) void conv_igemm_kernel(ConvArgs a) {
  constexpr int kLdk = BK + 4;                // padded LDS row (floats): conflict-free ds_read_b128 groups
  constexpr int NV = BK / 16;                 // float4 per thread and operand of a staged chunk
  __shared__ __attribute__((aligned(16))) float As[2][kBM * kLdk];
  __shared__ __attribute__((aligned(16))) float Bs[2][kBN * kLdk];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int P = a.N * a.Ho * a.Wo;
  const int m0 = blockIdx.x * kBM, n0 = blockIdx.y * kBN;
  const int taps = a.kh * a.kw;
  const int tap0 = blockIdx.z * a.taps_per_slice, tap1 = min(tap0 + a.taps_per_slice, taps);
  const int chunks_per_tap = a.Cin / BK;
  const int nchunks = (tap1 - tap0) * chunks_per_tap;

  // staging role of this thread: row (pixel of A / channel of B) and a (BK/4)-float column segment
  const int srow = tid >> 2, scol = (tid & 3) * (BK / 4);
  const int pix = m0 + srow;
  const bool pix_ok = pix < P;
  int py = 0, px = 0, pn = 0;
  if (pix_ok) { pn = pix / (a.Ho * a.Wo); const int r = pix - pn * a.Ho * a.Wo; py = r / a.Wo; px = r - py * a.Wo; }
  const float* wrow = a.w + ((size_t)(n0 + srow) * taps) * a.Cin + scol;

  // named registers: arrays (even with compile-time indices) and lambda captures ended up in scratch memory here
  float4 ra0, ra1, ra2, ra3, rb0, rb1, rb2, rb3;      // NV = 2 uses the first two of each
  ra2 = ra3 = rb2 = rb3 = make_float4(0.f, 0.f, 0.f, 0.f);
  float a_keep = 0.f;
#define LSFA_CONV_FETCH(chunk_)                                                                                        \
  {                                                                                                                    \
    const int t_ = (chunk_) / chunks_per_tap;                                                                          \
    const int tap = tap0 + t_;                                                                                         \
    const int ci0 = ((chunk_) - t_ * chunks_per_tap) * BK;                                                             \
    const int ty = tap / a.kw, tx = tap - ty * a.kw;                                                                   \
    const int iy = py * a.stride - a.pad + ty * a.dil, ix = px * a.stride - a.pad + tx * a.dil;                        \
    const bool ok = pix_ok && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;                                              \
    const float4* src = reinterpret_cast<const float4*>(a.x + (((size_t)pn * a.H + (ok ? iy : 0)) * a.W + (ok ? ix : 0)) * a.Cin + ci0 + scol); \
    const float4* wsrc = reinterpret_cast<const float4*>(wrow + (size_t)tap * a.Cin + ci0);                            \
    ra0 = src[0]; ra1 = src[1]; rb0 = wsrc[0]; rb1 = wsrc[1];                                                          \
    if (NV > 2) { ra2 = src[2]; ra3 = src[3]; rb2 = wsrc[2]; rb3 = wsrc[3]; }                                          \
    a_keep = ok ? 1.0f : 0.0f;   /* zero padding = the (clamped, valid) load times 0, applied when the chunk is */     \
                                 /* written to LDS: any use of the loaded value here would stall the wave before its MFMAs */ \
  }
#define LSFA_CONV_STASH(buf_)                                                                                          \
  {                                                                                                                    \
    float4* da = reinterpret_cast<float4*>(&As[buf_][srow * kLdk + scol]);                                             \
    float4* db = reinterpret_cast<float4*>(&Bs[buf_][srow * kLdk + scol]);                                             \
    da[0] = make_float4(ra0.x * a_keep, ra0.y * a_keep, ra0.z * a_keep, ra0.w * a_keep);                               \
    da[1] = make_float4(ra1.x * a_keep, ra1.y * a_keep, ra1.z * a_keep, ra1.w * a_keep);                               \
    db[0] = rb0; db[1] = rb1;                                                                                          \
    if (NV > 2) {                                                                                                      \
      da[2] = make_float4(ra2.x * a_keep, ra2.y * a_keep, ra2.z * a_keep, ra2.w * a_keep);                             \
      da[3] = make_float4(ra3.x * a_keep, ra3.y * a_keep, ra3.z * a_keep, ra3.w * a_keep);                             \
      db[2] = rb2; db[3] = rb3;                                                                                        \
    }                                                                                                                  \
  }

  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;

  LSFA_CONV_FETCH(0)
  LSFA_CONV_STASH(0)
  __syncthreads();
  const int arow = (wr * 32 + (lane & 31)) * kLdk + 4 * (lane >> 5);
  const int brow = (wc * 32 + (lane & 31)) * kLdk + 4 * (lane >> 5);
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    const int buf = chunk & 1;
    if (chunk + 1 < nchunks) LSFA_CONV_FETCH(chunk + 1)  // global loads in flight under the MFMAs
#pragma unroll
    for (int c = 0; c < BK / 8; ++c) {
      const float4 av = *reinterpret_cast<const float4*>(&As[buf][arow + 8 * c]);
      const float4 bv = *reinterpret_cast<const float4*>(&Bs[buf][brow + 8 * c]);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);   // keep every use of the freshly loaded registers behind the MFMAs
    if (chunk + 1 < nchunks) {
      LSFA_CONV_STASH(buf ^ 1)   // the other buffer: its last readers passed the barrier of the previous iteration
      __syncthreads();
    }
  }

#undef LSFA_CONV_FETCH
#undef LSFA_CONV_STASH
  // C/D layout of 32x32x2: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  const int ch = n0 + wc * 32 + (lane & 31);
  const float bias = (a.part == nullptr && a.bias) ? a.bias[ch] : 0.f;
  const float sc2 = (a.part == nullptr && a.y2) ? a.scale2[ch] : 0.f, sh2 = (a.part == nullptr && a.y2) ? a.shift2[ch] : 0.f;
  float* part = a.part ? a.part + (size_t)blockIdx.z * P * a.Cout : nullptr;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    const int p = m0 + wr * 32 + row;
    if (p < P) {
      const size_t o = (size_t)p * a.Cout + ch;
      if (part) part[o] = acc[r];
      else conv_epilogue(a, acc[r], o, ch, bias, sc2, sh2);
    }
  }
}

// the epilogue for the tap-split case: sum over slices of part, in slice order, then the same tail; float4 of channels per thread
__global__ __launch_bounds__(kThreads) void conv_reduce_kernel(ConvArgs a, long n4, int slices) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n4) return;
  const float4* part = reinterpret_cast<const float4*>(a.part);
  float4 s = part[i];
  for (int z = 1; z < slices; ++z) {
    const float4 v = part[(size_t)z * n4 + i];
    s.x = s.x + v.x; s.y = s.y + v.y; s.z = s.z + v.z; s.w = s.w + v.w;
  }
  const int c4 = a.Cout / 4;
  const int ch = (int)(i % c4) * 4;
  const float sv[4] = {s.x, s.y, s.z, s.w};
  float o1[4], o2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float v = sv[k] + (a.bias ? a.bias[ch + k] : 0.f);
    if (a.res) {
      size_t ro = (size_t)i * 4 + k;
      if (a.y_nchw) { const int hw = a.Ho * a.Wo; const long p = (i * 4) / a.Cout, pn = p / hw; ro = ((size_t)pn * a.Cout + ch + k) * hw + (p - pn * hw); }
      v = v + a.res[ro];
    }
    if (a.relu) v = fmaxf(v, 0.f);
    o1[k] = v;
    o2[k] = a.y2 ? fmaxf(v * a.scale2[ch + k] + a.shift2[ch + k], 0.f) : 0.f;
  }
  if (a.y_nchw) {
    const long p = (i * 4) / a.Cout;
    const int hw = a.Ho * a.Wo;
    const long pn = p / hw, pr = p - pn * hw;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const size_t o = ((size_t)pn * a.Cout + ch + k) * hw + pr;
      a.y[o] = o1[k];
      if (a.y2) a.y2[o] = o2[k];
    }
    return;
  }
  reinterpret_cast<float4*>(a.y)[i] = make_float4(o1[0], o1[1], o1[2], o1[3]);
  if (a.y2) reinterpret_cast<float4*>(a.y2)[i] = make_float4(o2[0], o2[1], o2[2], o2[3]);
}

int pick_slices(long tiles, int taps) {
  // one 4-wave workgroup per tile: below ~1 workgroup per CU the SIMDs idle, so cut the taps into 3 (3x3 kernels)
  if (taps % 3 == 0 && tiles * 4 < 1024) return 3;
  return 1;
}

}  // namespace

extern "C" size_t lsfa_conv_nhwc_workspace_bytes(int N, int H, int W, int Cout, int kh, int kw, int stride, int pad, int dil) {
  if (N <= 0 || H <= 0 || W <= 0 || Cout <= 0 || stride <= 0) return 0;
  const int Ho = (H + 2 * pad - dil * (kh - 1) - 1) / stride + 1, Wo = (W + 2 * pad - dil * (kw - 1) - 1) / stride + 1;
  const long P = (long)N * Ho * Wo;
  const int slices = pick_slices(((P + kBM - 1) / kBM) * (Cout / kBN), kh * kw);
  return slices > 1 ? align_up((size_t)slices * P * Cout * sizeof(float), 256) : 256;
}

extern "C" int lsfa_conv_nhwc_fused_fwd(const float* x, int N, int H, int W, int Cin, const float* w, const float* bias, int Cout,
                                        int kh, int kw, int stride, int pad, int dil, int relu, const float* residual, float* y,
                                        float* y2, const float* scale2, const float* shift2, void* ws, size_t ws_bytes,
                                        void* stream) {
  LSFA_REQUIRE(x && w && y, "lsfa_conv_nhwc_fwd: NULL argument");
  LSFA_REQUIRE(N > 0 && H > 0 && W > 0 && kh > 0 && kw > 0 && stride > 0 && pad >= 0 && dil > 0, "lsfa_conv_nhwc_fwd: bad shape");
  LSFA_REQUIRE(!y2 || (scale2 && shift2), "lsfa_conv_nhwc_fused_fwd: y2 given without scale2 / shift2");
  LSFA_REQUIRE(!y2 || y2 != y, "lsfa_conv_nhwc_fused_fwd: y2 must not alias y");
  if (Cin % 32 != 0 || Cout % kBN != 0) {
    set_error("lsfa_conv_nhwc_fwd: Cin=%d must be a multiple of %d and Cout=%d of %d", Cin, 32, Cout, kBN);
    return LSFA_ENOTSUP;
  }
  const int Ho = (H + 2 * pad - dil * (kh - 1) - 1) / stride + 1, Wo = (W + 2 * pad - dil * (kw - 1) - 1) / stride + 1;
  LSFA_REQUIRE(Ho > 0 && Wo > 0, "lsfa_conv_nhwc_fwd: empty output");
  const long P = (long)N * Ho * Wo;
  LSFA_REQUIRE(P * Cout < (1L << 31) && (long)N * H * W * Cin < (1L << 33), "lsfa_conv_nhwc_fwd: tensor too large");
  const int taps = kh * kw;
  const long tiles = ((P + kBM - 1) / kBM) * (Cout / kBN);
  const int slices = pick_slices(tiles, taps);
  if (slices > 1 && (!ws || ws_bytes < lsfa_conv_nhwc_workspace_bytes(N, H, W, Cout, kh, kw, stride, pad, dil))) {
    set_error("lsfa_conv_nhwc_fwd: workspace %zu < %zu bytes", ws_bytes, lsfa_conv_nhwc_workspace_bytes(N, H, W, Cout, kh, kw, stride, pad, dil));
    return LSFA_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  ConvArgs a = {x, w, bias, y, slices > 1 ? (float*)ws : nullptr, N, H, W, Cin, Cout, kh, kw, stride, pad, dil, Ho, Wo, relu,
                (taps + slices - 1) / slices, residual, y2, scale2, shift2, 0};
  ProfScope prof(LSFA_OP_CONV, s);
  const dim3 grid((unsigned)((P + kBM - 1) / kBM), Cout / kBN, slices);
  if (Cin % 64 == 0) hipLaunchKernelGGL(conv_igemm_kernel<64>, grid, dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL(conv_igemm_kernel<32>, grid, dim3(kThreads), 0, s, a);
  if (slices > 1) {
    const long n4 = P * Cout / 4;
    hipLaunchKernelGGL(conv_reduce_kernel, dim3((unsigned)((n4 + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a, n4, slices);
  }
  LSFA_LAUNCH_CHECK("lsfa_conv_nhwc_fwd");
  return LSFA_OK;
}

extern "C" int lsfa_conv_nhwc_fwd(const float* x, int N, int H, int W, int Cin, const float* w, const float* bias, int Cout,
                                  int kh, int kw, int stride, int pad, int dil, int relu, float* y, void* ws, size_t ws_bytes,
                                  void* stream) {
  return lsfa_conv_nhwc_fused_fwd(x, N, H, W, Cin, w, bias, Cout, kh, kw, stride, pad, dil, relu, nullptr, y, nullptr, nullptr,
                                  nullptr, ws, ws_bytes, stream);
}
