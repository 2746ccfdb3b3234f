// Scene cuts from the motion search's own SADs: a macroblock whose best inter prediction (the `sad` a search wrote) costs more than coding
// it against its own mean is "unmatched", and a frame most of whose blocks are unmatched starts a new scene.  The textbook encoder rule
// (inter cost against intra cost per macroblock), NOT ffmpeg's scene detection; like the searches it is comparable with nothing in the
// reference and is defined by its own specification ("Scene cuts"; tests/ref_me_cut.py states it in numpy), integer arithmetic,
// one answer per input.  For pair (c, f), f = 1..F, and macroblock b of the level-0 grid with n_b covered pixels (256, fewer for a block cut
// by the right or bottom edge):
//   inter_b = sad[c][f - 1][b], as the search wrote it (the full search's or the pyramid's level-0 winner; max_sad does not change it);
//   m_b = (sum p + n_b / 2) / n_b in integers, over the covered pixels of the CURRENT plane f;   intra_b = sum |p - m_b|;
//   b is unmatched iff inter_b > intra_b + bias * n_b (bias 0..255 grey levels per pixel);
//   unmatched[c][f - 1] = the number of unmatched blocks.  (The frame decision, unmatched * 100 > percent * blocks, is the caller's.)
//
// cut_intra_kernel: refine_chain_kernel's grid - pairs x blocks in one launch, 256-lane workgroups - without its LDS, and SIXTEEN lanes per
// macroblock instead of a wave: a lane owns one row of the block, four dwords (plane_dword, so rows that are not dword aligned and the
// frame's edges read as the searches read them; four independent loads in flight), uncovered bytes masked to 0 (the byte masks of blocks
// cut by the right edge; a zero mask for the rows below the bottom edge).  Byte sum with v_sad_u8 against 0, a reduction over the sixteen
// lanes (__shfl_xor 8, 4, 2, 1), the mean, v_sad_u8 against the mean replicated into the covered bytes, a second reduction; the first lane
// of the sixteen stores.  No barrier.  (A wave per block, a dword per lane, took twice this kernel's time - 9.7 against 4.9 us under a
// kernel trace: 21,546 waves per 1000 x 600 segment that each wait for one load and then reduce over six steps twice;
// profiles/r10/me_cut.txt.)
//
// cut_count_kernel: one 1,024-lane workgroup per pair adds up sad > intra + bias * n_b over the grid in integers (three blocks a lane at
// 1000 x 600); the sixteen waves' counts meet in 64 bytes of LDS.  No memset, no atomics, no workspace: both outputs are written in full by plain stores.
#include "common.h"
#include "me_common.h"

using namespace lsfa;

namespace {

constexpr int kThreads = 256;
constexpr int kCountThreads = 1024;
constexpr int kCountWaves = kCountThreads / 64;
constexpr int kMaxBias = 255;

struct CutArgs {
  int W, H, mbw, blocks, n_frames, bias;
  long total;                   // W * H: a plane's size in bytes
  long long stride;             // bytes from plane to plane; negative for a stack stored in reverse
  long groups;                  // pairs * blocks: sixteen lanes each
};

__global__ __launch_bounds__(kThreads) void cut_intra_kernel(const unsigned char* __restrict__ luma, CutArgs a, int* __restrict__ intra) {
  long g = ((long)blockIdx.x * kThreads + threadIdx.x) >> 4;       // sixteen lanes per macroblock
  const bool live = g < a.groups;
  if (!live) g = a.groups - 1;       // lanes past the end do the last block again and store nothing: every lane reaches the shuffles
  const int pair = (int)(g / a.blocks), blk = (int)(g - (long)pair * a.blocks);
  const unsigned char *cur, *ref;
  pair_planes(luma, a.stride, a.n_frames, pair, cur, ref);
  const int by = blk / a.mbw, bx = blk - by * a.mbw;
  const int x0 = 16 * bx, y0 = 16 * by;
  const int bw = min(16, a.W - x0), bh = min(16, a.H - y0);
  const int r = (int)threadIdx.x & 15;
  uint32_t mask[4], d[4];
  covered_masks(bw, mask);
  uint32_t sum = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (r >= bh) mask[k] = 0u;
    // a dword with no covered byte is not read at all
    d[k] = mask[k] ? plane_dword(cur, a.W, a.H, a.total, x0 + 4 * k, y0 + r) & mask[k] : 0u;
    sum = __builtin_amdgcn_sad_u8(d[k], 0u, sum);
  }
  const int n = bw * bh;
  const uint32_t mean = (uint32_t)((lanes_sum<16>((int)sum) + n / 2) / n);       // <= 255
  uint32_t dev = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) dev = __builtin_amdgcn_sad_u8(d[k], (mean * 0x01010101u) & mask[k], dev);
  const int total = lanes_sum<16>((int)dev);
  if (r == 0 && live) intra[g] = total;
}

__global__ __launch_bounds__(kCountThreads) void cut_count_kernel(const int* __restrict__ sad, const int* __restrict__ intra, CutArgs a,
                                                             int* __restrict__ unmatched) {
  __shared__ int s_count[kCountWaves];
  const int pair = (int)blockIdx.x;
  const int* s = sad + (size_t)pair * a.blocks;
  const int* c = intra + (size_t)pair * a.blocks;
  int count = 0;
  for (int b = threadIdx.x; b < a.blocks; b += kCountThreads) {
    const int by = b / a.mbw, bx = b - by * a.mbw;
    const int n = min(16, a.W - 16 * bx) * min(16, a.H - 16 * by);
    // intra + bias * n <= 2 * 65,280; a sad that is not a search's own may be anything an int holds
    count += s[b] > c[b] + a.bias * n ? 1 : 0;
  }
  count = lanes_sum<64>(count);
  if ((threadIdx.x & 63) == 0) s_count[threadIdx.x >> 6] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int wv = 1; wv < kCountWaves; ++wv) count += s_count[wv];
    unmatched[pair] = count;
  }
}

}  // namespace

extern "C" int lsfa_mv_cut_score(const unsigned char* luma, long long plane_stride, int n_chains, int n_frames, int width, int height, const int* sad,
                                 int bias, int* intra, int* unmatched, void* stream) {
  const char* who = "lsfa_mv_cut_score";
  LSFA_REQUIRE(luma && sad && intra && unmatched, "%s: NULL argument", who);
  LSFA_REQUIRE(bias >= 0 && bias <= kMaxBias, "%s: bias %d is outside 0..%d", who, bias, kMaxBias);
  CutArgs a;
  long pairs;
  if (const int rc = me_stack_args(who, luma, plane_stride, n_chains, n_frames, width, height, 0, 0, &a.blocks, &pairs)) return rc;
  a.W = width; a.H = height;
  a.mbw = ceil_div(width, 16);
  a.n_frames = n_frames; a.bias = bias;
  a.total = (long)width * height;
  a.stride = plane_stride;
  a.groups = pairs * a.blocks;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_MV_ESTIMATE, s);
  hipLaunchKernelGGL(cut_intra_kernel, dim3((unsigned)((a.groups + kThreads / 16 - 1) / (kThreads / 16))), dim3(kThreads), 0, s, luma, a, intra);
  hipLaunchKernelGGL(cut_count_kernel, dim3((unsigned)pairs), dim3(kCountThreads), 0, s, sad, (const int*)intra, a, unmatched);
  LSFA_LAUNCH_CHECK(who);
  return LSFA_OK;
}
