// The small net's channel-attention fuse (resnet_v1_101_flownet_rfcn.py:251-274, `concatv1` / `concatv2`) on channels-last maps:
//   global_pool (Pooling global_pool avg) -> s_feat_conv1 (1x1) + ReLU -> s_feat_conv2 (1x1) + sigmoid -> broadcast_mul + add.
// Three entry points (include/lsfa_hip.h): the per-image channel mean, the gate (both 1x1 convolutions on the pooled vector: GEMVs), and
// the gate's application to the map.  All three are deterministic (no float atomics) and give an image the same bits whatever the batch.
// Built with -ffp-contract=off: every product and sum below is rounded on its own unless the source says fmaf.
#include "common.h"

namespace {

constexpr int kMeanChunk = 16;       // pixels per partial sum of lsfa_channel_mean (fixed: part of the documented order)
constexpr int kMeanThreads = 256;    // one channel quad per thread: a workgroup covers 1,024 channels of a chunk
constexpr int kGateRowsPerWg = 4;    // one wave per output row
constexpr int kGateImages = 8;       // images a wave carries through one pass over a weight row

// partial[n][k][c] = (((0 + x[n, 16k]) + x[n, 16k + 1]) + ...) over the chunk's pixels in ascending order.  Channel c < C1 reads x1, else
// x2[c - C1]: the concatenation [x1 | x2] is never stored.
__global__ __launch_bounds__(kMeanThreads) void channel_mean_partial_kernel(const float* __restrict__ x1, int C1, const float* __restrict__ x2,
                                                                            int C2, int HW, int nchunks, float* __restrict__ partial) {
  const int C = C1 + C2;
  const int q = blockIdx.y * kMeanThreads + threadIdx.x;       // channel quad
  if (4 * q >= C) return;
  const int n = blockIdx.z, k = blockIdx.x;
  const int c = 4 * q;
  const float* src;
  int ld;
  if (c < C1) { src = x1 + (size_t)n * HW * C1 + c; ld = C1; }
  else { src = x2 + (size_t)n * HW * C2 + (c - C1); ld = C2; }
  const int p0 = k * kMeanChunk, p1 = min(p0 + kMeanChunk, HW);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p = p0; p < p1; ++p) {
    const float4 v = *reinterpret_cast<const float4*>(src + (size_t)p * ld);
    acc.x = acc.x + v.x; acc.y = acc.y + v.y; acc.z = acc.z + v.z; acc.w = acc.w + v.w;
  }
  *reinterpret_cast<float4*>(partial + ((size_t)n * nchunks + k) * C + c) = acc;
}

// mean[n][c] = ((((partial[n][0][c] + partial[n][1][c]) + ...) + partial[n][nchunks-1][c]) / HW
__global__ __launch_bounds__(256) void channel_mean_final_kernel(const float* __restrict__ partial, int N, int C, int HW, int nchunks,
                                                                 float* __restrict__ mean) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * C) return;
  const int n = i / C, c = i - n * C;
  const float* p = partial + (size_t)n * nchunks * C + c;
  float s = p[0];
  for (int k = 1; k < nchunks; ++k) s = s + p[(size_t)k * C];
  mean[i] = s / (float)HW;
}

// out[n][o] = act(dot(w[o, :], x[n, :]) + b[o]), one wave per row o, the row read once for kGateImages images at a time.
// dot: lane l accumulates k = 4(l + 64j) .. 4(l + 64j) + 3 for j = 0, 1, .. with fmaf in that order (acc = fmaf(w, x, acc), acc from 0),
// then the 64 lane sums are added by a butterfly over lane distance 32, 16, 8, 4, 2, 1 (every lane ends with the same sum), then + b[o].
// act 1: max(v, 0); act 2: 1 / (1 + exp(-v)) with exp correctly rounded (expf_cr).
__global__ __launch_bounds__(64 * kGateRowsPerWg) void gate_fc_kernel(const float* __restrict__ x, int N, int K, const float* __restrict__ w,
                                                                      const float* __restrict__ b, int O, int act, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int o = blockIdx.x * kGateRowsPerWg + (threadIdx.x >> 6);
  if (o >= O) return;                                     // (a whole wave: no lane of it takes part in a shuffle)
  const float* wr = w + (size_t)o * K;
  for (int n0 = 0; n0 < N; n0 += kGateImages) {
    float acc[kGateImages];
#pragma unroll
    for (int j = 0; j < kGateImages; ++j) acc[j] = 0.f;
    for (int k = 4 * lane; k < K; k += 256) {
      const float4 wv = *reinterpret_cast<const float4*>(wr + k);
#pragma unroll
      for (int j = 0; j < kGateImages; ++j) {
        if (n0 + j < N) {
          const float4 xv = *reinterpret_cast<const float4*>(x + (size_t)(n0 + j) * K + k);
          acc[j] = fmaf(wv.x, xv.x, acc[j]);
          acc[j] = fmaf(wv.y, xv.y, acc[j]);
          acc[j] = fmaf(wv.z, xv.z, acc[j]);
          acc[j] = fmaf(wv.w, xv.w, acc[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kGateImages; ++j) {
      float v = acc[j];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, 64);
      v = v + b[o];
      if (act == 1) v = fmaxf(v, 0.f);
      else if (act == 2) v = 1.0f / (1.0f + expf_cr(-v));
      if (lane == 0 && n0 + j < N) out[(size_t)(n0 + j) * O + o] = v;
    }
  }
}

// out = x * s[n, c] + y (two roundings) on (N, HW, C) maps, one channel quad per thread; max|out| over channels [c0, C) into amax_out.
__global__ __launch_bounds__(256) void gate_apply_kernel(const float* __restrict__ x, const float* __restrict__ s, const float* __restrict__ y,
                                                         int HW, int C, long total4, float* __restrict__ out, unsigned* __restrict__ amax_out,
                                                         int c0) {
  const int C4 = C >> 2;
  float mx = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
    const int q = (int)(i % C4);
    const int n = (int)(i / ((long)HW * C4));
    const float4 xv = reinterpret_cast<const float4*>(x)[i];
    const float4 yv = reinterpret_cast<const float4*>(y)[i];
    const float4 sv = *reinterpret_cast<const float4*>(s + (size_t)n * C + 4 * q);
    float4 o;
    o.x = xv.x * sv.x; o.x = o.x + yv.x;
    o.y = xv.y * sv.y; o.y = o.y + yv.y;
    o.z = xv.z * sv.z; o.z = o.z + yv.z;
    o.w = xv.w * sv.w; o.w = o.w + yv.w;
    reinterpret_cast<float4*>(out)[i] = o;
    if (4 * q >= c0) mx = fmaxf(mx, fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), fabsf(o.w))));
  }
  if (amax_out) {
    uint32_t m = __float_as_uint(mx);       // non-negative (fmaxf drops a NaN: a non-finite output shows in the consumer's own status)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(amax_out + ((blockIdx.x * 4 + (threadIdx.x >> 6)) & 255), m);
  }
}

inline bool aligned16(const void* p) { return p == nullptr || ((uintptr_t)p % 16) == 0; }

}  // namespace

extern "C" size_t lsfa_channel_mean_workspace_bytes(int N, int C, int HW) {
  if (N <= 0 || C <= 0 || HW <= 0) return 0;
  return (size_t)N * lsfa::ceil_div(HW, kMeanChunk) * C * sizeof(float);
}

extern "C" int lsfa_channel_mean(const float* x1, int C1, const float* x2, int C2, int N, int HW, float* mean, void* ws, size_t ws_bytes,
                                 void* stream) {
  using namespace lsfa;
  LSFA_REQUIRE(x1 && mean && ws, "lsfa_channel_mean: x1, mean and ws must be non-NULL");
  LSFA_REQUIRE(N > 0 && HW > 0 && C1 > 0 && C1 % 4 == 0 && C2 >= 0 && C2 % 4 == 0 && (C2 == 0 || x2),
               "lsfa_channel_mean: bad shape N=%d HW=%d C1=%d C2=%d (multiples of 4; x2 given when C2 > 0)", N, HW, C1, C2);
  LSFA_REQUIRE(N <= 65535, "lsfa_channel_mean: N=%d exceeds grid.z", N);
  LSFA_REQUIRE(aligned16(x1) && aligned16(x2) && aligned16(ws), "lsfa_channel_mean: maps and ws must be 16-byte aligned");
  const int C = C1 + C2;
  LSFA_REQUIRE(ws_bytes >= lsfa_channel_mean_workspace_bytes(N, C, HW), "lsfa_channel_mean: workspace of %zu bytes, %zu needed", ws_bytes,
               lsfa_channel_mean_workspace_bytes(N, C, HW));
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_AGG, s);
  const int nchunks = ceil_div(HW, kMeanChunk);
  float* partial = static_cast<float*>(ws);
  hipLaunchKernelGGL(channel_mean_partial_kernel, dim3(nchunks, ceil_div(C / 4, kMeanThreads), N), dim3(kMeanThreads), 0, s, x1, C1, x2, C2, HW,
                     nchunks, partial);
  hipLaunchKernelGGL(channel_mean_final_kernel, dim3(ceil_div(N * C, 256)), dim3(256), 0, s, partial, N, C, HW, nchunks, mean);
  LSFA_LAUNCH_CHECK("lsfa_channel_mean");
  return LSFA_OK;
}

extern "C" int lsfa_channel_gate(const float* m, int N, int K, const float* w1, const float* b1, int M, const float* w2, const float* b2,
                                 int O, float* hidden, float* gate, void* stream) {
  using namespace lsfa;
  LSFA_REQUIRE(m && w1 && b1 && w2 && b2 && hidden && gate, "lsfa_channel_gate: every pointer must be non-NULL");
  LSFA_REQUIRE(N > 0 && K > 0 && K % 4 == 0 && M > 0 && M % 4 == 0 && O > 0, "lsfa_channel_gate: bad shape N=%d K=%d M=%d O=%d (K, M multiples of 4)",
               N, K, M, O);
  LSFA_REQUIRE(aligned16(m) && aligned16(w1) && aligned16(w2) && aligned16(hidden), "lsfa_channel_gate: m, w1, w2, hidden must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_AGG, s);
  hipLaunchKernelGGL(gate_fc_kernel, dim3(ceil_div(M, kGateRowsPerWg)), dim3(64 * kGateRowsPerWg), 0, s, m, N, K, w1, b1, M, 1, hidden);
  hipLaunchKernelGGL(gate_fc_kernel, dim3(ceil_div(O, kGateRowsPerWg)), dim3(64 * kGateRowsPerWg), 0, s, hidden, N, M, w2, b2, O, 2, gate);
  LSFA_LAUNCH_CHECK("lsfa_channel_gate");
  return LSFA_OK;
}

extern "C" int lsfa_gate_apply(const float* x, const float* gate, const float* y, int N, int HW, int C, float* out, unsigned* amax_out, int amax_c0,
                               void* stream) {
  using namespace lsfa;
  LSFA_REQUIRE(x && gate && y && out, "lsfa_gate_apply: x, gate, y and out must be non-NULL");
  LSFA_REQUIRE(N > 0 && HW > 0 && C > 0 && C % 4 == 0, "lsfa_gate_apply: bad shape N=%d HW=%d C=%d (a multiple of 4)", N, HW, C);
  LSFA_REQUIRE(amax_c0 >= 0 && amax_c0 < C && amax_c0 % 4 == 0, "lsfa_gate_apply: amax_c0=%d must be a multiple of 4 in [0, C)", amax_c0);
  LSFA_REQUIRE(aligned16(x) && aligned16(gate) && aligned16(y) && aligned16(out), "lsfa_gate_apply: pointers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_AGG, s);
  const long total4 = (long)N * HW * (C / 4);
  long blocks = (total4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;        // grid-stride beyond 8 workgroups per CU
  hipLaunchKernelGGL(gate_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, gate, y, HW, C, total4, out, amax_out, amax_c0);
  LSFA_LAUNCH_CHECK("lsfa_gate_apply");
  return LSFA_OK;
}
