// 32-bit order keys of float scores, shared by proposal.hip, detpost.hip and nms_kernels.h: sorting the keys
// ascending sorts the scores descending, as thrust::greater and numpy's argsort()[::-1] see them.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace lsfa {

// ascending-orderable image of a float, complemented: smaller key == larger score
__device__ __forceinline__ uint32_t desc_key(float score) {
  score = score + 0.0f;  // -0 -> +0, so that equal scores tie like thrust::greater sees them
  const uint32_t u = __float_as_uint(score);
  const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}
__device__ __forceinline__ float key_score(uint32_t key) {
  const uint32_t asc = ~key;
  const uint32_t u = (asc & 0x80000000u) ? (asc & 0x7fffffffu) : ~asc;
  return __uint_as_float(u);
}

constexpr int kKeyBins = 4096;

// 12-bit monotone image of an order key, larger score -> larger bin: 128 bins per octave of score over
// [2^-32, 1) (7 mantissa bits); everything below (negative scores, the -1 marks) lands in bin 0, everything
// above in 4095.  Monotone in the key, so "key order" never contradicts "bin order"; ties inside a bin are
// resolved exactly by whoever selects through the bins (proposal_rank_kernel, det_cap_kernel).
__device__ __forceinline__ int key_bin(uint32_t key) {
  const uint32_t asc = ~key;
  if (!(asc & 0x80000000u)) return 0;                     // negative float
  const int e7 = (int)((asc & 0x7fffffffu) >> 16);        // exponent + 7 mantissa bits of a positive float
  const int b = e7 - ((127 - 32) << 7);
  return b < 0 ? 0 : (b > kKeyBins - 1 ? kKeyBins - 1 : b);
}

}  // namespace lsfa
