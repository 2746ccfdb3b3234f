// Ordered compaction and scans inside a workgroup of whole waves, shared by the overlay's plan and paint kernels (256 lanes), the tracker,
// Proposal's compact and select kernels and the detection post-processing (1024).
#pragma once
#include <hip/hip_runtime.h>

namespace lsfa {

// the position of this lane's kept item among the kept items of the workgroup's kWaves * 64, in lane order, and their number: ballot +
// popcount per wave, the wave counts through LDS (s_wave: kWaves ints).  Every lane of the workgroup calls it; s_wave is free again when
// it returns.
template <int kWaves>
__device__ __forceinline__ int prefix_block(bool keep, int* s_wave, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(keep);
  if (lane == 0) s_wave[wave] = __popcll(m);
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int c = s_wave[w];
    before += w < wave ? c : 0;
    all += c;
  }
  __syncthreads();
  *total = all;
  return before + __popcll(m & ((1ull << lane) - 1ull));
}

__device__ __forceinline__ int prefix_256(bool keep, int* s_wave, int* total) { return prefix_block<4>(keep, s_wave, total); }

// inclusive scan of one int per lane over the wave
__device__ __forceinline__ int wave_inclusive_scan(int v) {
  const int lane = threadIdx.x & 63;
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  return incl;
}

// the same for counts: exclusive scan of one int per thread over the workgroup's kWaves * 64, and the sum; wave_sums: kWaves ints of LDS,
// free again on return
template <int kWaves>
__device__ __forceinline__ int block_exclusive_scan(int v, int* wave_sums, int* total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int incl = wave_inclusive_scan(v);
  if (lane == 63) wave_sums[wid] = incl;
  __syncthreads();
  int base = 0, tot = 0;
  for (int i = 0; i < kWaves; ++i) {
    const int s = wave_sums[i];
    if (i < wid) base += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return base + incl - v;
}

}  // namespace lsfa
