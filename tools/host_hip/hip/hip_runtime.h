// A stand-in for <hip/hip_runtime.h> that lets a plane kernel's source compile for the HOST with an ordinary C++ compiler: the qualifiers
// vanish, the built-in indices are thread-local variables, and hipLaunchKernelGGL runs the kernel as nested loops over a grid of up to two
// dimensions and one-dimensional blocks.  Only what tools/san_yuv_host.cpp needs; vector types keep the device's alignment so that a misaligned wide access is seen by the
// undefined-behaviour sanitiser.  Never part of the library's build.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#define __device__
#define __global__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)

using std::max;
using std::min;

struct dim3 {
  unsigned x, y, z;
  dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
struct alignas(8) uint2 { uint32_t x, y; };
struct alignas(16) uint4 { uint32_t x, y, z, w; };
struct alignas(16) float4 { float x, y, z, w; };
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }

typedef void* hipStream_t;
typedef enum { hipSuccess = 0, hipErrorUnknown = 999 } hipError_t;
inline hipError_t hipGetLastError() { return hipSuccess; }
inline hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }

extern thread_local dim3 blockIdx, threadIdx, gridDim;
extern const char* host_last_kernel;          // the text of the last launch's kernel argument

#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...)  \
  do {                                                               \
    const dim3 g__ = (grid), b__ = (block);                          \
    host_last_kernel = #kernel;                                      \
    gridDim = g__;                                                   \
    for (unsigned by__ = 0; by__ < g__.y; ++by__)                    \
      for (unsigned bx__ = 0; bx__ < g__.x; ++bx__)                  \
        for (unsigned tx__ = 0; tx__ < b__.x; ++tx__) {              \
          blockIdx.x = bx__;                                         \
          blockIdx.y = by__;                                         \
          threadIdx.x = tx__;                                        \
          kernel(__VA_ARGS__);                                       \
        }                                                            \
  } while (0)
