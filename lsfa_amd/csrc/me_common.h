// What the motion searches share (me.hip: the full search; me_pyramid.hip: the pyramid's refinement): reads of a uint8 luma plane - a byte
// or four bytes at any position, 0 outside the frame, so that a staged window never holds anything but the frame and zeros -, the pieces
// of a macroblock's search both kernels use, and the host-side rules of their arguments.
#pragma once
#include "common.h"

namespace lsfa {

// cost = SAD + lambda * (|dx| + |dy|): with SAD <= 65,280 the full search's 64 lambda stays below 2^31 (its key and int32 arithmetic) and
// the refinement's 510 lambda below 2^34 (the top 37 bits of its key)
constexpr int kMaxLambda = (1 << 24);

// byte (gx, gy) of a plane, 0 outside the frame
__device__ __forceinline__ uint32_t plane_byte(const unsigned char* __restrict__ p, int W, int H, int gx, int gy) {
  return (gx >= 0 && gx < W && gy >= 0 && gy < H) ? (uint32_t)p[(size_t)gy * W + gx] : 0u;
}

// bytes (gx .. gx + 3, gy) of a plane as one little-endian dword, 0 outside the frame: two aligned dwords realigned where all four bytes
// are inside the frame and the second aligned dword ends inside the plane, byte loads otherwise (frame edges)
__device__ __forceinline__ uint32_t plane_dword(const unsigned char* __restrict__ p, int W, int H, long total, int gx, int gy) {
  if (gy >= 0 && gy < H && gx >= 0 && gx + 3 < W) {
    const long a = (long)gy * W + gx, base = a & ~3L;
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p + base);
    if ((a & 3L) == 0) return q[0];
    if (base + 8 <= total) return __builtin_amdgcn_alignbyte(q[1], q[0], (uint32_t)(a & 3L));
  }
  return plane_byte(p, W, H, gx, gy) | (plane_byte(p, W, H, gx + 1, gy) << 8) | (plane_byte(p, W, H, gx + 2, gy) << 16) |
         (plane_byte(p, W, H, gx + 3, gy) << 24);
}

// pair `pair` of n_chains stacks of n_frames + 1 planes `stride` bytes apart: frame f = 1..n_frames of chain c = pair / n_frames and the
// frame in front of it.  Signed: a negative stride is a stack stored in reverse
__device__ __forceinline__ void pair_planes(const unsigned char* __restrict__ luma, long long stride, int n_frames, int pair,
                                            const unsigned char*& cur, const unsigned char*& ref) {
  const int c = pair / n_frames, f = pair - c * n_frames + 1;
  cur = luma + ((long long)c * (n_frames + 1) + f) * stride;
  ref = cur - stride;
}

// byte mask of the covered columns per block dword of a block bw pixels wide (all ones for a block of full width)
__device__ __forceinline__ void covered_masks(int bw, uint32_t (&mask)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int nb = min(4, max(0, bw - 4 * k));
    mask[k] = nb >= 4 ? 0xFFFFFFFFu : ((1u << (8 * nb)) - 1u);
  }
}

// best becomes the smallest key of the wave, in every lane (in place: by value the refinement allocates its registers differently)
__device__ __forceinline__ void wave_min(unsigned long long& best) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long other = __shfl_xor(best, o, 64);
    best = other < best ? other : best;
  }
}

// the sum over `width` adjacent lanes (a power of two, the group aligned to it), in every lane of the group
template <int width>
__device__ __forceinline__ int lanes_sum(int v) {
#pragma unroll
  for (int o = width / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the row of the block at (x0, y0) with the vector (dx, dy)
__device__ __forceinline__ void store_row(int* __restrict__ row, int x0, int y0, int dx, int dy) {
  row[0] = -1; row[1] = 16; row[2] = 16;
  row[3] = x0 + 8 + dx; row[4] = y0 + 8 + dy; row[5] = x0 + 8; row[6] = y0 + 8;
}

// ---- host: the arguments every search shares, checked ----------------------------------------------------------------------------------------
// the frame and the cost's parameters
inline int me_frame_args(const char* who, int width, int height, int lambda, int max_sad) {
  LSFA_REQUIRE(width > 0 && height > 0 && (long)width * height < (1L << 30), "%s: bad frame size %d x %d", who, width, height);
  LSFA_REQUIRE(lambda >= 0 && lambda <= kMaxLambda, "%s: lambda %d is outside 0..%d", who, lambda, kMaxLambda);
  LSFA_REQUIRE(max_sad >= 0, "%s: max_sad %d is negative (0 switches it off)", who, max_sad);
  return LSFA_OK;
}

// ... and a stack of luma planes, what the chain exports take: n_chains * (n_frames + 1) planes (height, width) plane_stride bytes apart,
// luma 4-byte aligned at plane 0; a negative stride is a stack stored in reverse; |plane_stride| is a multiple of 4 that holds a plane.
// -> the macroblocks of a plane and the pairs of the stack, which fit one grid with a workgroup (or less) per block of every pair
inline int me_stack_args(const char* who, const unsigned char* luma, long long plane_stride, int n_chains, int n_frames, int width, int height,
                         int lambda, int max_sad, int* blocks, long* pairs) {
  if (const int rc = me_frame_args(who, width, height, lambda, max_sad)) return rc;
  LSFA_REQUIRE(n_chains >= 1 && n_frames >= 1, "%s: %d chains of %d frames: both counts must be at least 1", who, n_chains, n_frames);
  const long long total = (long long)width * height;
  // stated without |plane_stride| (the negation of LLONG_MIN overflows); below 2^36 the kernels' plane offsets stay inside 64 bits for every
  // stack that a memory can hold
  LSFA_REQUIRE((plane_stride >= total || plane_stride <= -total) && (plane_stride & 3) == 0 && plane_stride > -(1LL << 36) &&
                   plane_stride < (1LL << 36),
               "%s: plane stride %lld must hold a %d x %d plane, be a multiple of 4 and lie below 2^36", who, plane_stride, width, height);
  LSFA_REQUIRE((reinterpret_cast<uintptr_t>(luma) & 3u) == 0, "%s: the luma planes must be 4-byte aligned", who);
  *blocks = ceil_div(width, 16) * ceil_div(height, 16);
  *pairs = (long)n_chains * n_frames;
  LSFA_REQUIRE(*pairs <= ((1L << 31) - 1) / *blocks, "%s: %ld pairs of %d macroblocks exceed one grid", who, *pairs, *blocks);
  return LSFA_OK;
}

}  // namespace lsfa
