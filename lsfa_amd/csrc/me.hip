// Block-matching motion estimation on decoded frames: the per-macroblock vectors that lsfa_mv_accumulate takes, computed from two uint8
// frames on the device instead of read out of a compressed stream.
//
// NOT a port of anything in the reference: there the vectors come from ffmpeg's MPEG-4 encoder (data/reencode_vid.sh: EPZS search, half-pel
// refinement, four vectors per macroblock) through libav's side data (external/data_loader_py2/coviar_data_loader.c).  Neither exists in this
// project, so the result is DEFINED by the specification below ("Motion estimation"; tests/ref_me.py states it in numpy) - parity
// with an encoder's search is unpinned and not claimed.  Integer arithmetic throughout, one answer per input:
//   luma  Y = (29 B + 150 G + 77 R + 128) >> 8;
//   block (bx, by) covers x in [16 bx, min(16 bx + 16, W)), y in [16 by, min(16 by + 16, H));
//   candidates (dx, dy) in [-R, R]^2, valid iff the covered rectangle shifted by (dx, dy) lies inside the frame;
//   SAD(dx, dy) = sum |Ycur(x, y) - Yref(x + dx, y + dy)| over the covered pixels;  cost = SAD + lambda (|dx| + |dy|);
//   the vector is the valid candidate smallest under (cost, |dx| + |dy|, dy, dx), compared lexicographically; with max_sad > 0 a winner whose
//   SAD exceeds it becomes (0, 0) (an intra block; the SAD output keeps the winner's);
//   row by * mbw + bx = {-1, 16, 16, 16 bx + 8 + dx, 16 by + 8 + dy, 16 bx + 8, 16 by + 8}: every block, zero vectors included.
// Out of scope: half-pel refinement, 8x8 partitions, B-frames, reading a real bitstream.
//
// me_search_kernel: one 256-lane workgroup per macroblock.  The block (16 x 16 bytes) and its search window ((16 + 2R) rows of 16 + 4G bytes,
// G = ceil((2R + 1) / 4)) are staged in LDS once; pixels outside the frame are staged as 0 and never reach a valid candidate's sum.  A lane
// keeps the block in 64 registers and takes work units (dy, g) = four horizontally adjacent candidates dx = -R + 4g + {0, 1, 2, 3}: per row
// five window dwords and four v_qsad_pk_u16_u8, each sliding one block dword over eight window bytes, accumulate the four SADs as packed
// 16-bit sums (a block's SAD is at most 256 * 255 = 65,280, so they cannot overflow).  Blocks cut by the right frame edge take the same walk
// with v_alignbyte_b32 + v_sad_u8 and a byte mask per block dword (their uncovered block bytes are staged as 0, the mask zeroes the
// window's); blocks cut by the bottom edge stop after their covered rows.  A candidate is one 64-bit key
//   cost << 21 | (|dx| + |dy|) << 14 | (dy + 32) << 7 | (dx + 32),
// whose integer order IS the total order above, so the argmin is a plain `min`: per lane, then __shfl_xor across the wave, then one LDS
// step across the four waves.  Invalid candidates are skipped by range arithmetic on (dx, dy), never by clamping addresses.
#include "common.h"
#include "me_common.h"      // shared with the pyramid's refinement (me_pyramid.hip): plane reads, masks, wave min, row store, argument rules

using namespace lsfa;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSearch = 32;
constexpr int kMaxGroups = (2 * kMaxSearch + 1 + 3) / 4;               // 17
constexpr int kMaxWinDwords = (16 + 2 * kMaxSearch) * (4 + kMaxGroups);   // 80 rows of 21 dwords

__global__ __launch_bounds__(kThreads) void luma_u8_kernel(const unsigned char* __restrict__ bgr, int n, unsigned char* __restrict__ luma) {
  // four pixels per thread: 12 source bytes = three aligned dwords in, one dword out (hipMalloc'ed planes are dword aligned; the host
  // side sends unaligned planes through the byte path)
  const int q = blockIdx.x * kThreads + threadIdx.x;
  const int p = q * 4;
  if (p >= n) return;
  if (p + 4 <= n) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(bgr) + (size_t)q * 3;
    const uint32_t a = s[0], b = s[1], c = s[2];       // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
    auto y = [](uint32_t B, uint32_t G, uint32_t R) { return (29u * B + 150u * G + 77u * R + 128u) >> 8; };
    const uint32_t y0 = y(a & 255u, (a >> 8) & 255u, (a >> 16) & 255u);
    const uint32_t y1 = y(a >> 24, b & 255u, (b >> 8) & 255u);
    const uint32_t y2 = y((b >> 16) & 255u, b >> 24, c & 255u);
    const uint32_t y3 = y((c >> 8) & 255u, (c >> 16) & 255u, c >> 24);
    reinterpret_cast<uint32_t*>(luma)[q] = y0 | (y1 << 8) | (y2 << 16) | (y3 << 24);
    return;
  }
  for (int i = p; i < n; ++i)
    luma[i] = (unsigned char)((29u * bgr[(size_t)i * 3] + 150u * bgr[(size_t)i * 3 + 1] + 77u * bgr[(size_t)i * 3 + 2] + 128u) >> 8);
}

__global__ __launch_bounds__(kThreads) void luma_u8_bytes_kernel(const unsigned char* __restrict__ bgr, int n, unsigned char* __restrict__ luma) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  luma[i] = (unsigned char)((29u * bgr[(size_t)i * 3] + 150u * bgr[(size_t)i * 3 + 1] + 77u * bgr[(size_t)i * 3 + 2] + 128u) >> 8);
}

// the four SADs of block dword k, `c`, against window bytes [i, i + 4), i = 0..3, of the 8 bytes {hi, lo}, added to acc
struct Sad4Packed {
  // two accumulators, alternating: two independent dependency chains instead of one of 64 instructions.  Their fields add up to at most
  // 65,280 together, so the 64-bit sum carries nothing from one field into the next
  unsigned long long acc0 = 0ull, acc1 = 0ull;
  __device__ __forceinline__ void add(uint32_t lo, uint32_t hi, uint32_t c, uint32_t /*mask*/, int k) {
    const unsigned long long w = ((unsigned long long)hi << 32) | lo;
    if ((k & 1) == 0) acc0 = __builtin_amdgcn_qsad_pk_u16_u8(w, c, acc0);
    else acc1 = __builtin_amdgcn_qsad_pk_u16_u8(w, c, acc1);
  }
  __device__ __forceinline__ int get(int i) const { return (int)(((acc0 + acc1) >> (16 * i)) & 0xFFFFull); }
};
struct Sad4Masked {
  uint32_t acc[4] = {0u, 0u, 0u, 0u};
  __device__ __forceinline__ void add(uint32_t lo, uint32_t hi, uint32_t c, uint32_t mask, int /*k*/) {
    acc[0] = __builtin_amdgcn_sad_u8(lo & mask, c, acc[0]);
    acc[1] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(hi, lo, 1u) & mask, c, acc[1]);
    acc[2] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(hi, lo, 2u) & mask, c, acc[2]);
    acc[3] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(hi, lo, 3u) & mask, c, acc[3]);
  }
  __device__ __forceinline__ int get(int i) const { return (int)acc[i]; }
};

struct MeArgs {
  int W, H, mbw, R, G, lambda, max_sad;
  long total;       // W * H: the planes' size in bytes
};

template <class Sad4, bool kFullHeight>
__device__ __forceinline__ unsigned long long search_units(const uint32_t* __restrict__ s_win, const uint32_t (&c)[16][4], const uint32_t (&mask)[4],
                                                           const MeArgs& a, int x0, int y0, int bw, int bh, int first_unit) {
  const int R = a.R, G = a.G, wsd = 4 + G, units = (2 * R + 1) * G;
  unsigned long long best = ~0ull;
  // keeps the whole-block instance a loop of its own: without a difference the optimiser folds it back into the guarded instance
  if (kFullHeight) asm volatile("; whole 16 x 16 block");
  for (int u = first_unit; u < units; u += kThreads) {
    const int dyi = u / G, g = u - dyi * G;
    const int dy = dyi - R;
    // rows of the covered rectangle shifted by dy stay inside the frame?  (uniform per unit; the columns are checked per candidate)
    if (y0 + dy < 0 || y0 + bh - 1 + dy > a.H - 1) continue;
    const uint32_t* w = s_win + dyi * wsd + g;
    Sad4 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      // bottom-edge blocks: covered rows only.  Whole-height blocks carry no guard: sixteen guarded rows are sixteen basic blocks, each
      // waiting for its own LDS reads; unguarded, the reads of all rows are issued ahead of the SADs
      if (kFullHeight || r < bh) {
        const uint32_t w0 = w[r * wsd], w1 = w[r * wsd + 1], w2 = w[r * wsd + 2], w3 = w[r * wsd + 3], w4 = w[r * wsd + 4];
        s.add(w0, w1, c[r][0], mask[0], 0);
        s.add(w1, w2, c[r][1], mask[1], 1);
        s.add(w2, w3, c[r][2], mask[2], 2);
        s.add(w3, w4, c[r][3], mask[3], 3);
      }
    }
    const int ady = dy < 0 ? -dy : dy;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int dx = -R + 4 * g + i;
      if (dx > R || x0 + dx < 0 || x0 + bw - 1 + dx > a.W - 1) continue;
      const int len = (dx < 0 ? -dx : dx) + ady;
      const unsigned long long cost = (unsigned long long)(s.get(i) + a.lambda * len);
      const unsigned long long key = (cost << 21) | ((unsigned long long)len << 14) | ((unsigned long long)(dy + 32) << 7) | (unsigned long long)(dx + 32);
      best = key < best ? key : best;
    }
  }
  return best;
}

// one workgroup's search: macroblock `blk` of the pair (cur, ref); the row goes to mvs[blk], the SAD to sad_out[blk].  `rot` only picks
// the wave the units are dealt out from first (it cannot change the result: the minimum is over all units)
__device__ __forceinline__ void me_search_block(const unsigned char* __restrict__ cur, const unsigned char* __restrict__ ref, const MeArgs& a,
                                                int* __restrict__ mvs, int* __restrict__ sad_out, int blk, unsigned rot) {
  __shared__ uint4 s_blk[16];                       // the block: 16 rows of 16 bytes, uncovered bytes 0
  __shared__ uint32_t s_win[kMaxWinDwords];         // the window: (16 + 2R) rows of 4 + G dwords, bytes outside the frame 0
  __shared__ unsigned long long s_best[kThreads / 64];
  const int tid = threadIdx.x;
  const int by = blk / a.mbw, bx = blk - by * a.mbw;
  const int x0 = 16 * bx, y0 = 16 * by;
  const int bw = min(16, a.W - x0), bh = min(16, a.H - y0);
  const int R = a.R, wsd = 4 + a.G, rows = 16 + 2 * R;

  if (tid < 64) {       // block dword (row tid / 4, dword tid % 4)
    const int r = tid >> 2, k = tid & 3;
    reinterpret_cast<uint32_t*>(s_blk)[tid] = plane_dword(cur, a.W, a.H, a.total, x0 + 4 * k, y0 + r);
  }
  for (int i = tid; i < rows * wsd; i += kThreads) {
    const int r = i / wsd, k = i - r * wsd;
    s_win[i] = plane_dword(ref, a.W, a.H, a.total, x0 - R + 4 * k, y0 - R + r);
  }
  __syncthreads();

  uint32_t c[16][4];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const uint4 v = s_blk[r];
    c[r][0] = v.x; c[r][1] = v.y; c[r][2] = v.z; c[r][3] = v.w;
  }
  uint32_t mask[4];
  covered_masks(bw, mask);
  // the units are dealt out from a different wave in each workgroup: the last, partly filled round then lands on different SIMDs
  const int first_unit = (tid + 64 * (int)(rot & 3u)) & (kThreads - 1);
  unsigned long long best;
  if (bw == 16 && bh == 16) best = search_units<Sad4Packed, true>(s_win, c, mask, a, x0, y0, bw, bh, first_unit);
  else if (bw == 16) best = search_units<Sad4Packed, false>(s_win, c, mask, a, x0, y0, bw, bh, first_unit);
  else best = search_units<Sad4Masked, false>(s_win, c, mask, a, x0, y0, bw, bh, first_unit);
  wave_min(best);
  if ((tid & 63) == 0) s_best[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int wv = 1; wv < kThreads / 64; ++wv) best = s_best[wv] < best ? s_best[wv] : best;
    // (0, 0) is always valid, so a key exists
    int dx = (int)(best & 127ull) - 32, dy = (int)((best >> 7) & 127ull) - 32;
    const int len = (int)((best >> 14) & 127ull);
    const int sad = (int)(best >> 21) - a.lambda * len;
    if (a.max_sad > 0 && sad > a.max_sad) { dx = 0; dy = 0; }
    store_row(mvs + (size_t)blk * 7, x0, y0, dx, dy);
    if (sad_out) sad_out[blk] = sad;
  }
}

__global__ __launch_bounds__(kThreads) void me_search_kernel(const unsigned char* __restrict__ cur, const unsigned char* __restrict__ ref, MeArgs a,
                                                             int* __restrict__ mvs, int* __restrict__ sad_out) {
  me_search_block(cur, ref, a, mvs, sad_out, (int)blockIdx.x, blockIdx.x);
}

// me_search_chain_kernel: the same search for every pair (frame f, frame f - 1), f = 1..n_frames, of n_chains stacks of n_frames + 1 planes in
// one grid: workgroup w is macroblock w % blocks of pair w / blocks, and the pair index only selects two base pointers (pair_planes: the
// stride is signed, a stack may be stored in reverse) and the pair's slice of the outputs.  The first-unit rotation follows the
// workgroup's index in the whole grid, as the single-pair kernel's does.
__global__ __launch_bounds__(kThreads) void me_search_chain_kernel(const unsigned char* __restrict__ luma, long long plane_stride, int n_frames, int blocks,
                                                                   MeArgs a, int* __restrict__ mvs, int* __restrict__ sad_out) {
  const int pair = (int)(blockIdx.x / (unsigned)blocks), blk = (int)(blockIdx.x - (unsigned)pair * (unsigned)blocks);
  const unsigned char *cur, *ref;
  pair_planes(luma, plane_stride, n_frames, pair, cur, ref);
  me_search_block(cur, ref, a, mvs + (size_t)pair * blocks * 7, sad_out ? sad_out + (size_t)pair * blocks : nullptr, blk, blockIdx.x);
}

}  // namespace

extern "C" int lsfa_luma_u8(const unsigned char* bgr, int width, int height, unsigned char* luma, void* stream) {
  LSFA_REQUIRE(bgr && luma, "lsfa_luma_u8: NULL argument");
  LSFA_REQUIRE(width > 0 && height > 0 && (long)width * height < (1L << 30), "lsfa_luma_u8: bad frame size %d x %d", width, height);
  const int n = width * height;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_MV_ESTIMATE, s);
  if (((reinterpret_cast<uintptr_t>(bgr) | reinterpret_cast<uintptr_t>(luma)) & 3u) == 0)
    hipLaunchKernelGGL(luma_u8_kernel, dim3(ceil_div(ceil_div(n, 4), kThreads)), dim3(kThreads), 0, s, bgr, n, luma);
  else
    hipLaunchKernelGGL(luma_u8_bytes_kernel, dim3(ceil_div(n, kThreads)), dim3(kThreads), 0, s, bgr, n, luma);
  LSFA_LAUNCH_CHECK("lsfa_luma_u8");
  return LSFA_OK;
}

namespace {

// the search's own arguments behind a frame me_frame_args has checked: what lsfa_mv_estimate and lsfa_mv_estimate_chain launch with
int me_args(const char* who, int width, int height, int search, int lambda, int max_sad, MeArgs* a) {
  LSFA_REQUIRE(search >= 1 && search <= kMaxSearch, "%s: search %d is outside 1..%d", who, search, kMaxSearch);
  a->W = width; a->H = height;
  a->mbw = ceil_div(width, 16);
  a->R = search;
  a->G = ceil_div(2 * search + 1, 4);
  a->lambda = lambda;
  a->max_sad = max_sad;
  a->total = (long)width * height;
  return LSFA_OK;
}

}  // namespace

extern "C" int lsfa_mv_estimate(const unsigned char* luma_cur, const unsigned char* luma_ref, int width, int height, int search, int lambda,
                                int max_sad, int* mvs, int* sad, void* stream) {
  const char* who = "lsfa_mv_estimate";
  LSFA_REQUIRE(luma_cur && luma_ref && mvs, "%s: NULL argument", who);
  MeArgs a;
  if (const int rc = me_frame_args(who, width, height, lambda, max_sad)) return rc;
  if (const int rc = me_args(who, width, height, search, lambda, max_sad, &a)) return rc;
  LSFA_REQUIRE(((reinterpret_cast<uintptr_t>(luma_cur) | reinterpret_cast<uintptr_t>(luma_ref)) & 3u) == 0, "%s: the luma planes must be 4-byte aligned", who);
  const int blocks = a.mbw * ceil_div(height, 16);
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_MV_ESTIMATE, s);
  hipLaunchKernelGGL(me_search_kernel, dim3(blocks), dim3(kThreads), 0, s, luma_cur, luma_ref, a, mvs, sad);
  LSFA_LAUNCH_CHECK(who);
  return LSFA_OK;
}

extern "C" int lsfa_mv_estimate_chain(const unsigned char* luma, long long plane_stride, int n_chains, int n_frames, int width, int height, int search,
                                      int lambda, int max_sad, int* mvs, int* sad, void* stream) {
  const char* who = "lsfa_mv_estimate_chain";
  LSFA_REQUIRE(luma && mvs, "%s: NULL argument", who);
  MeArgs a;
  int blocks;
  long pairs;
  if (const int rc = me_stack_args(who, luma, plane_stride, n_chains, n_frames, width, height, lambda, max_sad, &blocks, &pairs)) return rc;
  if (const int rc = me_args(who, width, height, search, lambda, max_sad, &a)) return rc;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_MV_ESTIMATE, s);
  hipLaunchKernelGGL(me_search_chain_kernel, dim3((unsigned)(pairs * blocks)), dim3(kThreads), 0, s, luma, plane_stride, n_frames, blocks, a, mvs, sad);
  LSFA_LAUNCH_CHECK(who);
  return LSFA_OK;
}
