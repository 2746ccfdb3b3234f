// Pyramid (coarse-to-fine) motion search: vectors beyond the full search's +-32 pixels at a fraction of its cost.  A second, separately
// specified mode beside the full search of me.hip; NOT the full search with a larger range (a coarse level can lock onto the wrong minimum,
// and a block whose true source is valid can have an ancestor whose shifted rectangle is not).  Like the full search it is defined by its
// own specification ("Pyramid search"; tests/ref_me_pyramid.py states it in numpy), integer arithmetic, one answer per input:
//   P_0 is the luma plane the full search reads; P_{k+1} is ceil(w_k / 2) x ceil(h_k / 2),
//     P_{k+1}[y][x] = (a + b + c + d + 2) >> 2 over P_k at (2x, 2y), (2x + 1, 2y), (2x, 2y + 1), (2x + 1, 2y + 1), coordinates clamped to
//     P_k; every level from the level below it, so the two roundings of P_2 are part of the specification;
//   the top level L is lsfa_mv_estimate[_chain] on P_L (16 x 16 blocks on P_L's own grid, max_sad = 0), bit for bit;
//   levels k = L - 1 .. 0: block (bx, by) of P_k's grid has the parent (bx >> 1, by >> 1) on level k + 1 with winner (pdx, pdy); its
//     candidates are (2 pdx + ex, 2 pdy + ey), (ex, ey) in [-r, r]^2, plus (0, 0); valid iff the covered rectangle shifted by the candidate
//     lies inside P_k ((0, 0) always is); cost = SAD + lambda (|dx| + |dy|) on the ABSOLUTE vector, the same lambda at every level; the
//     winner is the smallest under (cost, |dx| + |dy|, dy, dx); max_sad applies to the level-0 winner only; rows as the full search's.
//   Reach: R 2^L + r (2^L - 1) pixels per axis, at most 137.
//
// pyramid_kernel: one launch for every plane of a stack and both levels.  A 256-lane workgroup forms a 32 x 32 tile of P_1 from its
// 64 x 64 pixels of P_0 (a lane: four adjacent P_1 pixels, two dwords of two rows where the plane's rows are dword aligned, clamped byte
// loads otherwise), keeps the tile in LDS and forms its 16 x 16 tile of P_2 from THAT tile - never from P_0.  The clamped taps of a P_2
// pixel lie in the same tile (2x + 1 clamps to 2x).
//
// refine_chain_kernel: one WAVE per macroblock, four macroblocks per 256-lane workgroup, every pair of a segment in one grid.  A block has
// at most (2r + 1)^2 + 1 = 50 candidates, so a lane IS a candidate: the wave stages the block (64 dwords), the (16 + 2r)-row window around
// 2 (pdx, pdy) (six dwords a row) and the sixteen rows behind the zero candidate in LDS once, pixels outside the plane as 0 (they never
// reach a valid candidate's sum); a lane then walks its sixteen rows, five window dwords each, realigned to its own byte offset with
// v_alignbyte_b32 and summed with v_sad_u8 - with the byte masks of blocks cut by the right edge and without the rows below the bottom
// edge, as the full search does.  Arithmetic does not bound it (about 2 % of the full search's SADs at R = 16); the launch shape does:
// 2,394 waves per 1000 x 600 pair instead of 2,394 workgroups.  The key is the refinement's own,
//   cost << 27 | (|dx| + |dy|) << 18 | (dy + 256) << 9 | (dx + 256),
// whose integer order is the total order above for |dx|, |dy| <= 255 (nine-bit fields; the mode's reach is 137); a candidate beyond
// that - only a parent row that is not the mode's own can ask for one - is dropped like an invalid one.  The argmin is a `min` over the
// wave (__shfl_xor); lane 0 writes the row.
#include "common.h"
#include "me_common.h"

using namespace lsfa;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxRefine = 3;
constexpr int kWinStride = 7;                            // dwords from one staged row to the next: six staged, odd against bank conflicts
constexpr int kWinRows = 16 + 2 * kMaxRefine;            // 22
constexpr int kVecLimit = 255;                           // the key's nine-bit vector fields

struct PyramidArgs {
  int W, H, w1, h1, w2, h2;
  int levels, tiles_x;
  int rows_aligned;             // P_0's rows start on dword boundaries in every plane
  long long s0, s1, s2;         // bytes from plane to plane on levels 0, 1, 2
};

__device__ __forceinline__ uint32_t avg4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return (a + b + c + d + 2u) >> 2; }

__global__ __launch_bounds__(kThreads) void pyramid_kernel(const unsigned char* __restrict__ p0, PyramidArgs a, unsigned char* __restrict__ p1,
                                                           unsigned char* __restrict__ p2) {
  __shared__ uint32_t s_p1[32][9];       // the P_1 tile: 32 rows of 32 bytes (+ one dword of padding)
  const int tid = threadIdx.x;
  const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;
  const unsigned char* src = p0 + (size_t)blockIdx.y * (size_t)a.s0;
  const int row = tid >> 3, q = tid & 7;
  const int X = 32 * tx + 4 * q, Y = 32 * ty + row;          // this lane's four P_1 pixels (X .. X + 3, Y)
  const int ya = min(2 * Y, a.H - 1), yb = min(2 * Y + 1, a.H - 1);
  uint32_t v[4];
  if (a.rows_aligned && 2 * X + 7 < a.W) {
    const uint32_t* ra = reinterpret_cast<const uint32_t*>(src + (size_t)ya * a.W + 2 * X);
    const uint32_t* rb = reinterpret_cast<const uint32_t*>(src + (size_t)yb * a.W + 2 * X);
    const uint32_t a0 = ra[0], a1 = ra[1], b0 = rb[0], b1 = rb[1];
    v[0] = avg4(a0 & 255u, (a0 >> 8) & 255u, b0 & 255u, (b0 >> 8) & 255u);
    v[1] = avg4((a0 >> 16) & 255u, a0 >> 24, (b0 >> 16) & 255u, b0 >> 24);
    v[2] = avg4(a1 & 255u, (a1 >> 8) & 255u, b1 & 255u, (b1 >> 8) & 255u);
    v[3] = avg4((a1 >> 16) & 255u, a1 >> 24, (b1 >> 16) & 255u, b1 >> 24);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // clamped: a pixel past P_1's edge reads P_0's last column / row again and is neither stored nor read by P_2
      const int xa = min(2 * (X + i), a.W - 1), xb = min(2 * (X + i) + 1, a.W - 1);
      v[i] = avg4(src[(size_t)ya * a.W + xa], src[(size_t)ya * a.W + xb], src[(size_t)yb * a.W + xa], src[(size_t)yb * a.W + xb]);
    }
  }
  const uint32_t packed = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
  s_p1[row][q] = packed;
  if (Y < a.h1) {
    unsigned char* d = p1 + (size_t)blockIdx.y * (size_t)a.s1 + (size_t)Y * a.w1 + X;
    if ((a.w1 & 3) == 0 && X + 3 < a.w1) *reinterpret_cast<uint32_t*>(d) = packed;
    else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (X + i < a.w1) d[i] = (unsigned char)v[i];
    }
  }
  if (a.levels < 2) return;
  __syncthreads();
  if (tid < 64) {
    const int row2 = tid >> 2, q2 = tid & 3;
    const int X2 = 16 * tx + 4 * q2, Y2 = 16 * ty + row2;
    if (Y2 < a.h2) {
      const int la = min(2 * Y2, a.h1 - 1) - 32 * ty, lb = min(2 * Y2 + 1, a.h1 - 1) - 32 * ty;      // rows of the tile
      uint32_t u[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (X2 + i < a.w2) {
          const int ca = min(2 * (X2 + i), a.w1 - 1) - 32 * tx, cb = min(2 * (X2 + i) + 1, a.w1 - 1) - 32 * tx;
          auto at = [&](int r, int c) { return (s_p1[r][c >> 2] >> (8 * (c & 3))) & 255u; };
          u[i] = avg4(at(la, ca), at(la, cb), at(lb, ca), at(lb, cb));
        }
      }
      unsigned char* d = p2 + (size_t)blockIdx.y * (size_t)a.s2 + (size_t)Y2 * a.w2 + X2;
      if ((a.w2 & 3) == 0 && X2 + 3 < a.w2) *reinterpret_cast<uint32_t*>(d) = u[0] | (u[1] << 8) | (u[2] << 16) | (u[3] << 24);
      else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (X2 + i < a.w2) d[i] = (unsigned char)u[i];
      }
    }
  }
}

struct RefineArgs {
  int W, H, mbw, blocks;        // level k: the plane and its macroblock grid
  int pmbw, pblocks;            // level k + 1: macroblocks per row / per plane
  int r, lambda, max_sad, n_frames;
  long total;                   // W * H: a plane's size in bytes
  long long stride;             // bytes from plane to plane; negative for a stack stored in reverse
  long waves;                   // pairs * blocks: one wave each
};

__device__ __forceinline__ int clamp_vec(long long v) { return (int)(v < -1024 ? -1024 : (v > 1024 ? 1024 : v)); }

__global__ __launch_bounds__(kThreads) void refine_chain_kernel(const unsigned char* __restrict__ luma, const int* __restrict__ parent, RefineArgs a,
                                                                int* __restrict__ mvs, int* __restrict__ sad_out) {
  __shared__ uint32_t s_blk[kWaves][64];                                 // the block: 16 rows of 4 dwords, uncovered bytes 0
  __shared__ uint32_t s_win[kWaves][(kWinRows + 16) * kWinStride];       // the window's rows, then the 16 rows behind the zero candidate
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  long g = (long)blockIdx.x * kWaves + wave;
  const bool live = g < a.waves;
  if (!live) g = a.waves - 1;       // a wave past the end does the last block again and stores nothing: every wave reaches the barrier
  const int pair = (int)(g / a.blocks), blk = (int)(g - (long)pair * a.blocks);
  const unsigned char *cur, *ref;
  pair_planes(luma, a.stride, a.n_frames, pair, cur, ref);
  const int by = blk / a.mbw, bx = blk - by * a.mbw;
  const int x0 = 16 * bx, y0 = 16 * by;
  const int bw = min(16, a.W - x0), bh = min(16, a.H - y0);
  const int r = a.r, n = 2 * r + 1;

  const int* prow = parent + ((size_t)pair * a.pblocks + (size_t)((by >> 1) * a.pmbw + (bx >> 1))) * 7;
  // a row that is not the mode's own may carry anything: beyond +-1024 the candidates are dropped below in any case
  const int cx = 2 * clamp_vec((long long)prow[3] - (long long)prow[5]), cy = 2 * clamp_vec((long long)prow[4] - (long long)prow[6]);
  const int wx = x0 + cx - r, wy = y0 + cy - r;

  uint32_t* blk_s = s_blk[wave];
  uint32_t* win = s_win[wave];
  uint32_t* zero = win + kWinRows * kWinStride;
  {
    const int rr = lane >> 2, k = lane & 3;
    blk_s[lane] = plane_dword(cur, a.W, a.H, a.total, x0 + 4 * k, y0 + rr);
    zero[rr * kWinStride + k] = plane_dword(ref, a.W, a.H, a.total, x0 + 4 * k, y0 + rr);
    if (lane < 16) zero[lane * kWinStride + 4] = 0u;       // read as the fifth dword of a row at byte offset 0: never part of a sum
  }
  for (int i = lane; i < (16 + 2 * r) * 6; i += 64) {
    const int rr = i / 6, k = i - rr * 6;
    win[rr * kWinStride + k] = plane_dword(ref, a.W, a.H, a.total, wx + 4 * k, wy + rr);
  }
  __syncthreads();

  // a lane is a candidate: lanes 0 .. n^2 - 1 the refinement's, lane n^2 the zero vector, the rest idle (they walk the zero rows)
  int dx = 0, dy = 0, sh = 0;
  const uint32_t* w = zero;
  bool valid = lane <= n * n;
  if (lane < n * n) {
    const int eyi = lane / n, exi = lane - eyi * n;
    dx = cx - r + exi; dy = cy - r + eyi;
    w = win + eyi * kWinStride + (exi >> 2);
    sh = exi & 3;
  }
  valid = valid && x0 + dx >= 0 && x0 + bw - 1 + dx <= a.W - 1 && y0 + dy >= 0 && y0 + bh - 1 + dy <= a.H - 1 && dx >= -kVecLimit && dx <= kVecLimit &&
          dy >= -kVecLimit && dy <= kVecLimit;

  uint32_t mask[4];
  covered_masks(bw, mask);
  uint32_t acc0 = 0u, acc1 = 0u;       // two dependency chains
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    if (rr < bh) {       // uniform over the wave: blocks cut by the bottom edge stop after their covered rows
      const uint4 cb = reinterpret_cast<const uint4*>(blk_s)[rr];
      const uint32_t* wr = w + rr * kWinStride;
      const uint32_t w0 = wr[0], w1 = wr[1], w2 = wr[2], w3 = wr[3], w4 = wr[4];
      acc0 = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w1, w0, (uint32_t)sh) & mask[0], cb.x, acc0);
      acc1 = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w2, w1, (uint32_t)sh) & mask[1], cb.y, acc1);
      acc0 = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w3, w2, (uint32_t)sh) & mask[2], cb.z, acc0);
      acc1 = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w4, w3, (uint32_t)sh) & mask[3], cb.w, acc1);
    }
  }
  unsigned long long best = ~0ull;
  if (valid) {
    const unsigned long long len = (unsigned long long)((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy));
    const unsigned long long cost = (unsigned long long)(acc0 + acc1) + (unsigned long long)a.lambda * len;
    best = (cost << 27) | (len << 18) | ((unsigned long long)(dy + 256) << 9) | (unsigned long long)(dx + 256);
  }
  wave_min(best);
  if (lane == 0 && live) {
    // (0, 0) is always valid, so a key exists
    int bdx = (int)(best & 511ull) - 256, bdy = (int)((best >> 9) & 511ull) - 256;
    const long long len = (long long)((best >> 18) & 511ull);
    const int sad = (int)((long long)(best >> 27) - (long long)a.lambda * len);
    if (a.max_sad > 0 && sad > a.max_sad) { bdx = 0; bdy = 0; }
    store_row(mvs + (size_t)g * 7, x0, y0, bdx, bdy);
    if (sad_out) sad_out[g] = sad;
  }
}

}  // namespace

extern "C" int lsfa_luma_pyramid(const unsigned char* luma, long long plane_stride, int n_planes, int width, int height, int levels,
                                 unsigned char* level1, long long stride1, unsigned char* level2, long long stride2, void* stream) {
  LSFA_REQUIRE(levels == 1 || levels == 2, "lsfa_luma_pyramid: levels %d is outside 1..2", levels);
  LSFA_REQUIRE(luma && level1 && (levels == 1 || level2), "lsfa_luma_pyramid: NULL argument");
  LSFA_REQUIRE(width > 0 && height > 0 && (long)width * height < (1L << 30), "lsfa_luma_pyramid: bad frame size %d x %d", width, height);
  LSFA_REQUIRE(n_planes >= 1 && n_planes <= 65535, "lsfa_luma_pyramid: %d planes: 1..65535 in one launch", n_planes);
  PyramidArgs a;
  a.W = width; a.H = height;
  a.w1 = ceil_div(width, 2); a.h1 = ceil_div(height, 2);
  a.w2 = ceil_div(a.w1, 2); a.h2 = ceil_div(a.h1, 2);
  LSFA_REQUIRE(plane_stride >= (long long)width * height, "lsfa_luma_pyramid: plane stride %lld does not hold a %d x %d plane", plane_stride, width, height);
  LSFA_REQUIRE(stride1 >= (long long)a.w1 * a.h1 && (stride1 & 3) == 0,
               "lsfa_luma_pyramid: level 1 stride %lld must hold a %d x %d plane and be a multiple of 4", stride1, a.w1, a.h1);
  LSFA_REQUIRE(levels == 1 || (stride2 >= (long long)a.w2 * a.h2 && (stride2 & 3) == 0),
               "lsfa_luma_pyramid: level 2 stride %lld must hold a %d x %d plane and be a multiple of 4", stride2, a.w2, a.h2);
  LSFA_REQUIRE(((reinterpret_cast<uintptr_t>(level1) | (levels == 2 ? reinterpret_cast<uintptr_t>(level2) : 0)) & 3u) == 0,
               "lsfa_luma_pyramid: the output planes must be 4-byte aligned");
  a.levels = levels;
  a.tiles_x = ceil_div(a.w1, 32);
  a.rows_aligned = (width & 3) == 0 && (plane_stride & 3) == 0 && (reinterpret_cast<uintptr_t>(luma) & 3u) == 0;
  a.s0 = plane_stride; a.s1 = stride1; a.s2 = levels == 2 ? stride2 : 0;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_MV_ESTIMATE, s);
  hipLaunchKernelGGL(pyramid_kernel, dim3((unsigned)(a.tiles_x * ceil_div(a.h1, 32)), (unsigned)n_planes), dim3(kThreads), 0, s, luma, a, level1,
                     levels == 2 ? level2 : nullptr);
  LSFA_LAUNCH_CHECK("lsfa_luma_pyramid");
  return LSFA_OK;
}

extern "C" int lsfa_mv_refine_chain(const unsigned char* luma, long long plane_stride, int n_chains, int n_frames, int width, int height,
                                    const int* parent_mvs, int refine, int lambda, int max_sad, int* mvs, int* sad, void* stream) {
  const char* who = "lsfa_mv_refine_chain";
  LSFA_REQUIRE(luma && parent_mvs && mvs, "%s: NULL argument", who);
  LSFA_REQUIRE(refine >= 1 && refine <= kMaxRefine, "%s: refine %d is outside 1..%d", who, refine, kMaxRefine);
  RefineArgs a;
  long pairs;
  if (const int rc = me_stack_args(who, luma, plane_stride, n_chains, n_frames, width, height, lambda, max_sad, &a.blocks, &pairs)) return rc;
  // the kernel's own index arithmetic: a wave's pair index times the parent grid's blocks
  LSFA_REQUIRE(pairs < (1L << 24), "%s: %ld pairs of %d macroblocks exceed one grid", who, pairs, a.blocks);
  a.total = (long)width * height;
  a.W = width; a.H = height;
  a.mbw = ceil_div(width, 16);
  a.pmbw = ceil_div(ceil_div(width, 2), 16);
  a.pblocks = a.pmbw * ceil_div(ceil_div(height, 2), 16);
  a.r = refine; a.lambda = lambda; a.max_sad = max_sad; a.n_frames = n_frames;
  a.stride = plane_stride;
  a.waves = pairs * a.blocks;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_MV_ESTIMATE, s);
  hipLaunchKernelGGL(refine_chain_kernel, dim3((unsigned)((a.waves + kWaves - 1) / kWaves)), dim3(kThreads), 0, s, luma, parent_mvs, a, mvs, sad);
  LSFA_LAUNCH_CHECK(who);
  return LSFA_OK;
}
