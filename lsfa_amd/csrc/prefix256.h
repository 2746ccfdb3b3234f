// Ordered compaction inside a workgroup of whole waves, shared by the overlay's plan and paint kernels (256 lanes) and the tracker (1024).
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

}  // namespace lsfa
