/* Just enough of CUDA's device-side vocabulary to compile the reference's sliced kernels for the host.
 * The slices are #included inside namespace ref, after this header, so that their unqualified calls of
 * min / max / round / floor / ceil / exp find the overloads below (the ones CUDA's headers give device code)
 * and not the C library's double versions.
 *
 * Declared substitution: exp(float) is the correctly rounded float exponential, (float)exp((double)x).
 * CUDA's own is documented to 2 ulp and has no bit-level statement. */
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include <pthread.h>

#define __global__
#define __device__
#define __shared__ static          /* one block runs at a time; its threads share the array */

namespace ref {

struct dim3 {
  unsigned x, y, z;
  dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
static thread_local dim3 blockIdx, threadIdx, blockDim, gridDim;

/* block-wide barrier of the emulated block (ref::run_block sets it up) */
static pthread_barrier_t* block_barrier = nullptr;
static inline void __syncthreads() { if (block_barrier) pthread_barrier_wait(block_barrier); }

/* CUDA's overload set: same-type forms, and the mixed float/double forms that promote to double */
static inline int min(int a, int b) { return a < b ? a : b; }
static inline int max(int a, int b) { return a > b ? a : b; }
static inline float min(float a, float b) { return fminf(a, b); }
static inline float max(float a, float b) { return fmaxf(a, b); }
static inline double min(double a, double b) { return fmin(a, b); }
static inline double max(double a, double b) { return fmax(a, b); }
static inline double min(float a, double b) { return fmin((double)a, b); }
static inline double max(float a, double b) { return fmax((double)a, b); }
static inline double min(double a, float b) { return fmin(a, (double)b); }
static inline double max(double a, float b) { return fmax(a, (double)b); }

static inline float round(float x) { return roundf(x); }      /* half away from zero */
static inline double round(double x) { return ::round(x); }
static inline float floor(float x) { return floorf(x); }
static inline double floor(double x) { return ::floor(x); }
static inline float ceil(float x) { return ceilf(x); }
static inline double ceil(double x) { return ::ceil(x); }
static inline float exp(float x) { return (float)::exp((double)x); }
static inline double exp(double x) { return ::exp(x); }

/* One emulated thread per (blockIdx.x, threadIdx.x) of a 1-D launch, in index order.  Every loop-style
 * kernel of the reference is launched with at least `count` threads, so each thread's grid-stride loop
 * runs its body at most once. */
template <typename F>
static void launch_1d(unsigned blocks, unsigned threads, F kernel) {
  gridDim = dim3(blocks);
  blockDim = dim3(threads);
  for (unsigned b = 0; b < blocks; ++b)
    for (unsigned t = 0; t < threads; ++t) {
      blockIdx = dim3(b);
      threadIdx = dim3(t);
      kernel();
    }
}

/* A 2-D grid of blocks that use __shared__ and __syncthreads(): `threads` host threads run one block at a
 * time between two barriers, each with its own threadIdx and the block's blockIdx. */
template <typename F>
struct block_job {
  F* kernel; dim3 grid; unsigned threads, tid; pthread_barrier_t* bar;
};
template <typename F>
static void* block_thread(void* p) {
  block_job<F>* j = (block_job<F>*)p;
  gridDim = j->grid;
  blockDim = dim3(j->threads);
  threadIdx = dim3(j->tid);
  for (unsigned by = 0; by < j->grid.y; ++by)
    for (unsigned bx = 0; bx < j->grid.x; ++bx) {
      blockIdx = dim3(bx, by);
      (*j->kernel)();
      pthread_barrier_wait(j->bar);      /* nobody refills the shared array while a neighbour still reads it */
    }
  return nullptr;
}
template <typename F>
static void launch_blocks(dim3 grid, unsigned threads, F kernel) {
  pthread_barrier_t bar;
  pthread_barrier_init(&bar, nullptr, threads);
  block_barrier = &bar;
  std::vector<pthread_t> th(threads);
  std::vector<block_job<F> > jobs(threads);
  for (unsigned t = 0; t < threads; ++t) {
    jobs[t].kernel = &kernel; jobs[t].grid = grid; jobs[t].threads = threads; jobs[t].tid = t; jobs[t].bar = &bar;
    pthread_create(&th[t], nullptr, block_thread<F>, &jobs[t]);
  }
  for (unsigned t = 0; t < threads; ++t) pthread_join(th[t], nullptr);
  block_barrier = nullptr;
  pthread_barrier_destroy(&bar);
}

}  // namespace ref
