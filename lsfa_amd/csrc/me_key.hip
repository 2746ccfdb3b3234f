// Stale key frames: the SAD of every macroblock of frame f against the KEY frame of its chain, compensated with the accumulated vectors -
// the residual the network is fed (`res_diff` before its resize), per block.  It stands in for an encoder's decision to spend an I-frame
// where the reference picture has stopped predicting (a dissolve, content that pans in, occlusion, the drift of chained vectors): cases the
// pair rule of me_cut.hip cannot see, because no single pair of consecutive frames crosses its threshold.  Like the searches and the pair
// rule it is comparable with nothing in the reference and is defined by its own specification ("Stale key frames";
// tests/ref_me_stale.py states it in numpy), integer arithmetic, one answer per input.  For chain c, frame f = 1..F and macroblock b of the
// level-0 grid:
//   q_f(p) = the walk back of lsfa_mv_segment_inputs from pixel p of frame f through the rows of frames f .. 1 (walk_move below: a step
//            that would leave the frame is not taken, so q_f(p) is always inside the frame);
//   keysad[c][f - 1][b] = sum over the covered pixels p of b of |P_f[p] - P_0[q_f(p)]|        (<= 65,280)
// The decision is lsfa_mv_cut_score's with keysad in the place of the search's sad (intra cost of plane f, bias, count of unmatched blocks).
//
// key_sad_kernel: refine_chain_kernel's grid - one wave per (pair, macroblock), four per 256-lane workgroup - without LDS.  A lane owns one
// dword of the block, four pixels of one row (plane_dword, so rows that are not dword aligned and the frame's edges read as the searches read
// them), and walks its four pixels back as four independent chains of at most f dependent loads - sixteen loads in flight per step -; the row
// table is read through the cache (the walks wander: a block's pixels end in up to four blocks per step).  The first step's row is the
// block's own, the same for the whole wave, and is read with scalar loads (the wave's index goes through readfirstlane, so pair and block
// are scalars).  Pixels outside the frame (edge blocks) start at the frame's last column / row and are masked out of the SAD: every walk,
// covered or not, stays inside the frame and the table.  The lane gathers its four key-frame bytes, packs them, masks uncovered bytes
// (covered_masks; a zero mask below the bottom edge) and issues one v_sad_u8 against its own dword; the wave sum is six __shfl_xor steps,
// lane 0 stores.  No barrier, no atomics, no memset, no workspace.
//
// key_sad_accu_kernel: the same lanes and the same sum for ONE frame whose source map exists already (MotionVectorAccumulator's accu, the
// frame-by-frame path): the walk is replaced by one 8-byte load per pixel.  A source position outside the plane reads as 0 (the
// accumulator never produces one).
#include "common.h"
#include "me_common.h"

using namespace lsfa;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct KeyArgs {
  int W, H, mbw, blocks, n_frames;
  long total;                   // W * H: a plane's size in bytes
  long long stride;             // bytes from plane to plane; negative for a stack stored in reverse
  long groups;                  // pairs * blocks (the per-frame form: blocks): one wave each
};

// One step of the walk back: the pixel (x, y) inside the frame moves by the vector (vx, vy) = (row[3] - row[5], row[4] - row[6]) of frame k's
// row of the block that contains it; a step that would leave the frame is not taken.  STATED A SECOND TIME: the rule is me_segment.hip's
// walk_step.  Shared from a header, segment_inputs_kernel's compiled code did not stay the same (other registers throughout), and that
// kernel is on every segment's path.  A change of the rule has to be made in both places (tests/ref_me_segment.py is the one statement
// both are tested against).  The test is written without && on purpose: with it the compiler loads row[4] and row[6] only behind a branch
// on the x test, and the four pixels of a lane ran one after the other, eight dependent round trips per step (51 us per 1000 x 600
// segment; profiles/r11/me_stale.txt).
__device__ __forceinline__ void walk_move(long long vx, long long vy, int W, int H, int& x, int& y) {
  const long long nx = (long long)x + vx, ny = (long long)y + vy;
  const bool inside = (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H);
  x = inside ? (int)nx : x;
  y = inside ? (int)ny : y;
}

// ... for the four pixels of a lane: the sixteen loads first (independent; a row of the table whatever the vectors say), then the moves
__device__ __forceinline__ void walk_step4(const int* __restrict__ rows_k, int mbw, int W, int H, int (&x)[4], int (&y)[4]) {
  int v[4][4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int* row = rows_k + (size_t)((y[s] >> 4) * mbw + (x[s] >> 4)) * 7;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[s][j] = row[3 + j];
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) walk_move((long long)v[s][0] - (long long)v[s][2], (long long)v[s][1] - (long long)v[s][3], W, H, x[s], y[s]);
}

// what both kernels share: this wave's macroblock and this lane's dword of it
struct KeyLane {
  long g;                       // the wave's (pair, block), scalar
  bool live;                    // false: a wave past the end, which does the last block again and stores nothing
  int blk, x0, y, px[4], py;    // the block; the lane's dword (x0 .. x0 + 3, y); the same positions clamped into the frame
  uint32_t mask;                // the dword's covered bytes; 0: nothing of it is inside the frame
};

__device__ __forceinline__ KeyLane key_lane(const KeyArgs& a) {
  KeyLane l;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  l.g = (long)blockIdx.x * kWaves + wave;
  l.live = l.g < a.groups;
  if (!l.live) l.g = a.groups - 1;
  l.blk = (int)(l.g % a.blocks);
  const int by = l.blk / a.mbw, bx = l.blk - by * a.mbw;
  const int lane = (int)threadIdx.x & 63, k = lane & 3, r = lane >> 2;
  uint32_t mask[4];
  covered_masks(min(16, a.W - 16 * bx), mask);
  l.x0 = 16 * bx + 4 * k; l.y = 16 * by + r;
  l.mask = l.y < a.H ? (k == 0 ? mask[0] : k == 1 ? mask[1] : k == 2 ? mask[2] : mask[3]) : 0u;
  l.py = min(l.y, a.H - 1);
#pragma unroll
  for (int s = 0; s < 4; ++s) l.px[s] = min(l.x0 + s, a.W - 1);
  return l;
}

// the lane's SAD of its own dword of `cur` against the four gathered key bytes, summed over the wave; lane 0 of a live wave stores
__device__ __forceinline__ void key_store(const unsigned char* __restrict__ cur, const KeyArgs& a, const KeyLane& l, const uint32_t (&kb)[4],
                                          int* __restrict__ keysad) {
  uint32_t sad = 0u;
  if (l.mask) {       // a dword with no covered byte is not read at all
    const uint32_t d = plane_dword(cur, a.W, a.H, a.total, l.x0, l.y) & l.mask;
    sad = __builtin_amdgcn_sad_u8(d, (kb[0] | (kb[1] << 8) | (kb[2] << 16) | (kb[3] << 24)) & l.mask, 0u);
  }
  const int total = lanes_sum<64>((int)sad);
  if (((int)threadIdx.x & 63) == 0 && l.live) keysad[l.g] = total;
}

__global__ __launch_bounds__(kThreads) void key_sad_kernel(const unsigned char* __restrict__ luma, const int* __restrict__ rows, KeyArgs a,
                                                           int* __restrict__ keysad) {
  const KeyLane l = key_lane(a);
  const int pair = (int)(l.g / a.blocks);
  const int c = pair / a.n_frames, f = pair - c * a.n_frames + 1;
  const unsigned char *cur, *ref;
  pair_planes(luma, a.stride, a.n_frames, pair, cur, ref);
  const unsigned char* key = luma + (long long)c * (a.n_frames + 1) * a.stride;
  const int* rows_c = rows + (size_t)c * a.n_frames * a.blocks * 7;
  int qx[4], qy[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) { qx[s] = l.px[s]; qy[s] = l.py; }
  // the first step's row is the block's own, the same for the wave: scalar loads (the clamped positions of an edge block lie in it too)
  const int* own = rows_c + ((size_t)(f - 1) * a.blocks + l.blk) * 7;
  const long long vx = (long long)own[3] - (long long)own[5], vy = (long long)own[4] - (long long)own[6];
#pragma unroll
  for (int s = 0; s < 4; ++s) walk_move(vx, vy, a.W, a.H, qx[s], qy[s]);
  for (int k = f - 1; k >= 1; --k) walk_step4(rows_c + (size_t)(k - 1) * a.blocks * 7, a.mbw, a.W, a.H, qx, qy);
  uint32_t kb[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) kb[s] = key[(size_t)qy[s] * a.W + qx[s]];
  key_store(cur, a, l, kb, keysad);
}

__global__ __launch_bounds__(kThreads) void key_sad_accu_kernel(const unsigned char* __restrict__ cur, const unsigned char* __restrict__ key,
                                                                const int2* __restrict__ accu, KeyArgs a, int* __restrict__ keysad) {
  const KeyLane l = key_lane(a);
  int2 q[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) q[s] = accu[(size_t)l.py * a.W + l.px[s]];
  uint32_t kb[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) kb[s] = plane_byte(key, a.W, a.H, q[s].x, q[s].y);
  key_store(cur, a, l, kb, keysad);
}

}  // namespace

extern "C" int lsfa_mv_key_sad(const unsigned char* luma, long long plane_stride, int n_chains, int n_frames, int width, int height, const int* rows,
                               int* keysad, void* stream) {
  const char* who = "lsfa_mv_key_sad";
  LSFA_REQUIRE(luma && rows && keysad, "%s: NULL argument", who);
  KeyArgs a;
  long pairs;
  if (const int rc = me_stack_args(who, luma, plane_stride, n_chains, n_frames, width, height, 0, 0, &a.blocks, &pairs)) return rc;
  a.W = width; a.H = height;
  a.mbw = ceil_div(width, 16);
  a.n_frames = n_frames;
  a.total = (long)width * height;
  a.stride = plane_stride;
  a.groups = pairs * a.blocks;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_MV_ESTIMATE, s);
  hipLaunchKernelGGL(key_sad_kernel, dim3((unsigned)((a.groups + kWaves - 1) / kWaves)), dim3(kThreads), 0, s, luma, rows, a, keysad);
  LSFA_LAUNCH_CHECK(who);
  return LSFA_OK;
}

extern "C" int lsfa_mv_key_sad_accu(const unsigned char* luma_cur, const unsigned char* luma_key, const int* accu, int width, int height, int* keysad,
                                    void* stream) {
  const char* who = "lsfa_mv_key_sad_accu";
  LSFA_REQUIRE(luma_cur && luma_key && accu && keysad, "%s: NULL argument", who);
  if (const int rc = me_frame_args(who, width, height, 0, 0)) return rc;
  LSFA_REQUIRE((reinterpret_cast<uintptr_t>(luma_cur) & 3u) == 0 && (reinterpret_cast<uintptr_t>(accu) & 7u) == 0,
               "%s: luma_cur must be 4-byte and accu 8-byte aligned", who);
  KeyArgs a;
  a.W = width; a.H = height;
  a.mbw = ceil_div(width, 16);
  a.blocks = a.mbw * ceil_div(height, 16);
  a.n_frames = 1;
  a.total = (long)width * height;
  a.stride = 0;
  a.groups = a.blocks;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof(LSFA_OP_MV_ESTIMATE, s);
  hipLaunchKernelGGL(key_sad_accu_kernel, dim3((unsigned)((a.groups + kWaves - 1) / kWaves)), dim3(kThreads), 0, s, luma_cur, luma_key,
                     reinterpret_cast<const int2*>(accu), a, keysad);
  LSFA_LAUNCH_CHECK(who);
  return LSFA_OK;
}
