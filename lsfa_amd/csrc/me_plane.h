// Reads of a uint8 luma plane that the motion searches share (me.hip: the full search; me_pyramid.hip: the pyramid's refinement): a byte or
// four bytes at any position, 0 outside the frame, so that a staged window never holds anything but the frame and zeros.
#pragma once
#include "common.h"

namespace lsfa {

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

}  // namespace lsfa
