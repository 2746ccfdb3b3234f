// Device kernels shared by nms.hip (lsfa_nms_sorted, _nms) and proposal.hip.
//
// Greedy NMS over score-sorted boxes, wave64-native (replaces nms_kernel + D2H of the 4.5 MB mask +
// serial host sweep + H2D of the keep list, lib/nms/nms_kernel.cu:40-150, multi_proposal.cu:262-357):
//
//   1. nms_mask_kernel — one 64-lane WAVE per 64x64 tile of the upper triangle (4 tiles per 256-thread
//      workgroup, tiles enumerated linearly so no workgroup is launched for the lower triangle).  A
//      lane owns one ROW box in registers; the 64 COLUMN boxes are staged in LDS and read back at
//      wave-uniform addresses.  Bit k of word (i, cb) is set iff IoU(box_i, box_{64cb+k})
//      > thresh and 64cb+k > i, as in the reference.  On diagonal tiles the same predicate, balloted
//      across the wave, is the TRANSPOSED word (the rows that suppress column k): it is written to
//      diagT so the sweep can resolve a block without a 64-step serial loop.
//      IoU > thresh is decided WITHOUT the division, bit for bit (iou_test.h).
//   2. nms_sweep_kernel — ONE wave walks the 64-box blocks in score order.  A block is resolved as a
//      fixpoint on ballots (G(k) = alive(k) && no earlier member of G suppresses k: a handful of
//      iterations, not 64 scalar steps); the survivors' mask rows are ORed into the removed-set in
//      LDS, 8 rows per batch of loads; it stops at `max_keep` survivors.  With `rois` set it also
//      writes the Proposal output (proposal_write_rows).
// proposal.hip alone has the mask-free nms_sweep_iou_kernel, nms.hip alone the float64 nms_mask_f64_kernel.
// devIoU arithmetic = oracle dev_iou (nms_kernel.cu:30-38), -ffp-contract=off.
#pragma once
#include <math.h>

#include "common.h"
#include "iou_test.h"
#include "nms_block.h"
#include "order_key.h"

namespace lsfa {

// number of upper-triangle tiles (diagonal included) of a col_blocks x col_blocks tile grid
__host__ __device__ static inline int nms_tile_count(int col_blocks) { return col_blocks * (col_blocks + 1) / 2; }

// tile -> its column block cb; tiles are enumerated column by column, so nms_tile_count(cb) tiles come before column cb and
// the row block is rb = tile - nms_tile_count(cb) <= cb.  The float seed is off by at most a step either way; the two loops
// settle it exactly.
__host__ __device__ static inline int nms_tile_column(int tile) {
  int cb = (int)((sqrtf(8.0f * (float)tile + 1.0f) - 1.0f) * 0.5f);
  while ((cb + 1) * (cb + 2) / 2 <= tile) ++cb;
  while (cb * (cb + 1) / 2 > tile) --cb;
  return cb;
}

// grid (ceil(tiles / 4), 1, images); block 256 = 4 waves = 4 tiles.
// boxes: (images, n_total, box_dim) floats; `order` (images, n) int32 or NULL: row p of the sorted list is
// boxes[order[p]] (Proposal: candidates stay where the decode kernel put them).  mask: (images, n, col_blocks);
// diagT: (images, n).
// PACKED4: boxes are a plain float4 array (Proposal's sorted boxes) and are loaded as one 16-byte access.
// The 64 column boxes of a tile are staged once in LDS (one per lane) and read back at wave-uniform addresses
// (a broadcast read per column, issued ahead by the unrolled loop); the loop body is the IoU test and a bit
// insert only — row / column validity and the j > i rule of diagonal tiles are applied to the finished words,
// and the transposed diagonal words come from 64 ballots over the finished rows (diagonal tiles only).
template <bool PACKED4>
static __global__ __launch_bounds__(256) void nms_mask_kernel(const float* __restrict__ boxes_all, long boxes_img_stride,
                                                              int box_dim, const int* __restrict__ order_all, int n,
                                                              IouTest t, uint64_t* __restrict__ mask_all,
                                                              uint64_t* __restrict__ diagT_all, int col_blocks, int diag_only) {
  __shared__ float4 cbox[4][64];
  __shared__ float carea[4][64];
  const int lane = threadIdx.x & 63;
  // wave-uniform, and the compiler is told so: the tile indices and the `diag` branch stay scalar
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int tile = blockIdx.x * 4 + wv;
  const bool tile_ok = tile < (diag_only ? col_blocks : nms_tile_count(col_blocks));
  // diag_only: the col_blocks diagonal tiles only (the Proposal's box sweep decides everything off the diagonal from the boxes
  // themselves: nms_sweep_iou_kernel in proposal.hip)
  const int cb = diag_only ? tile : nms_tile_column(tile);
  const int rb = diag_only ? tile : tile - nms_tile_count(cb);
  const int img = blockIdx.z;
  const float* boxes = boxes_all + (size_t)img * boxes_img_stride;
  const int* order = order_all ? order_all + (size_t)img * n : nullptr;
  uint64_t* mask = mask_all + (size_t)img * n * col_blocks;

  const int row = rb * 64 + lane, col = cb * 64 + lane;
  const bool row_ok = tile_ok && row < n, col_ok = tile_ok && col < n;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c = make_float4(0.f, 0.f, 0.f, 0.f);
  if (row_ok) {
    if (PACKED4) a = reinterpret_cast<const float4*>(boxes)[row];
    else { const float* p = boxes + (size_t)(order ? order[row] : row) * box_dim; a = make_float4(p[0], p[1], p[2], p[3]); }
  }
  if (col_ok) {
    if (PACKED4) c = reinterpret_cast<const float4*>(boxes)[col];
    else { const float* p = boxes + (size_t)(order ? order[col] : col) * box_dim; c = make_float4(p[0], p[1], p[2], p[3]); }
  }
  const float Sa = box_area(a);
  cbox[wv][lane] = c;
  carea[wv][lane] = box_area(c);
  __syncthreads();
  if (!tile_ok) return;
  const int ncol = min(64, n - cb * 64);
  const bool diag = rb == cb;
  uint32_t word[2] = {0, 0};
  bool unsure = !t.fast;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    uint32_t w = 0;
#pragma unroll 8
    for (int jj = 0; jj < 32; ++jj) {
      const int j = half * 32 + jj;
      const bool p = iou_exceeds_fast(a, Sa, cbox[wv][j], carea[wv][j], t, unsure);
      w |= (uint32_t)p << jj;
    }
    word[half] = w;
  }
  if (__builtin_expect(__any(unsure), 0)) {   // wave-uniform and rare: redo the tile with the real division
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      uint32_t w = 0;
      for (int jj = 0; jj < 32; ++jj) {
        const int j = half * 32 + jj;
        w |= (uint32_t)iou_exceeds_div(a, Sa, cbox[wv][j], carea[wv][j], t) << jj;
      }
      word[half] = w;
    }
  }
  uint64_t bits = ((uint64_t)word[1] << 32) | word[0];
  if (ncol < 64) bits &= (1ULL << ncol) - 1ULL;                       // columns past the last box
  if (diag) bits &= lane == 63 ? 0ULL : ~((2ULL << lane) - 1ULL);      // in a diagonal tile only j > i counts
  if (!row_ok) bits = 0;
  if (row_ok) mask[(size_t)row * col_blocks + cb] = bits;
  if (diag) {
    // transpose the finished 64 x 64 bit block: word of column k = the rows that suppress k
    uint32_t tlo = 0, thi = 0;
#pragma unroll 8
    for (int k = 0; k < 64; ++k) {
      const unsigned long long colword = __ballot((bits >> k) & 1ULL);
      if (lane == k) { tlo = (uint32_t)colword; thi = (uint32_t)(colword >> 32); }
    }
    if (row_ok) diagT_all[(size_t)img * n + row] = ((uint64_t)thi << 32) | tlo;
  }
}

constexpr int kSweepMaxBlocks = 512;   // n <= 32768
constexpr int kSweepMaxOut = 1024;     // Proposal output rows
constexpr int kSweepLazyMax = 4096;    // survivors whose positions fit the LDS list of the lazy sweep
constexpr int kSweepPairMax = 320;     // survivors the two-blocks-per-trip sweep gathers with five loads per lane

// OR over the wave, returned as a wave-uniform value, on the DPP cross-lane paths: quad swaps, half-row and row
// mirrors (every lane of a 16-lane row then holds the row's OR), row_bcast15 into rows 1 and 3, row_bcast31 into
// rows 2 and 3, read lane 63.  About 25 VALU instructions and no LDS traffic (a __shfl_xor butterfly
// is 12 dependent LDS-crossbar round trips).
__device__ __forceinline__ uint32_t wave_or32_dpp(uint32_t x) {
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, false);    // quad_perm [1,0,3,2]
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xF, 0xF, false);    // quad_perm [2,3,0,1]
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x141, 0xF, 0xF, false);   // row_half_mirror
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x140, 0xF, 0xF, false);   // row_mirror
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);   // row_bcast15 -> rows 1, 3
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);   // row_bcast31 -> rows 2, 3
  return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}
__device__ __forceinline__ uint64_t wave_or64_uniform(uint64_t v) {
  return ((uint64_t)wave_or32_dpp((uint32_t)(v >> 32)) << 32) | wave_or32_dpp((uint32_t)v);
}

// Proposal's output (PrepareOutput, multi_proposal.cu:363-388): rows index0, index0 + stride, ... < post_n of image `img` =
// [img, x1, y1, x2, y2] of the first post_n survivors, cyclic pad when only `num` < post_n survived, and their scores
// when asked for.  box(k) / key(k): the box and the order key of survivor k.
template <class Box, class Key>
__device__ __forceinline__ void proposal_write_rows(int img, int index0, int stride, int post_n, int num, float* __restrict__ rois,
                                                    float* __restrict__ scores, Box box, Key key) {
  for (int index = index0; index < post_n; index += stride) {
    const int k = index < num ? index : index % num;
    const float4 bx = box(k);
    float* o = rois + ((size_t)img * post_n + index) * 5;
    o[0] = (float)img;
    o[1] = bx.x; o[2] = bx.y; o[3] = bx.z; o[4] = bx.w;
    if (scores) scores[(size_t)img * post_n + index] = key_score(key(k));
  }
}

// grid (images); block 64 (one wave).  keep: (images, n) positions in the sorted list, or NULL; num_keep:
// (images) or NULL.  Proposal epilogue when rois != NULL: sorted_box (images, n) float4, sorted_key (images, n)
// order keys (for `scores`), rois (images*post_n, 5), scores (images*post_n) or NULL; max_keep = post_n.
//
// Which candidates of block b are already suppressed is found LAZILY when max_keep <= kSweepLazyMax: the
// survivors so far sit in an LDS list, each lane gathers one word of a survivor's mask row and the lanes OR
// them into the next block's removed-set word (nothing is ever loaded for blocks the sweep does not reach —
// Proposal stops after 300 survivors, usually within a few blocks — and the loads for block b+1 are in
// flight while block b is resolved).
// Larger keep budgets use the eager form: every survivor's whole row is ORed into a removed-set in LDS.
static __global__ __launch_bounds__(64) void nms_sweep_kernel(const uint64_t* __restrict__ mask_all,
                                                              const uint64_t* __restrict__ diagT_all, int n, int col_blocks,
                                                              int max_keep, int* __restrict__ keep_all,
                                                              int* __restrict__ num_keep_all,
                                                              const float4* __restrict__ sorted_box_all,
                                                              const uint32_t* __restrict__ sorted_key_all,
                                                              float* __restrict__ rois, float* __restrict__ scores) {
  __shared__ uint64_t remv[kSweepMaxBlocks];
  __shared__ int kept_pos[kSweepLazyMax];
#ifdef LSFA_SWEEP_PRIO      // lab (tools/lab/build_variant.sh): the one wave of a sweep is a latency chain; under the pipeline's contention it takes 67 us for 12 us of work
  __builtin_amdgcn_s_setprio(LSFA_SWEEP_PRIO);
#endif
  const int img = blockIdx.x;
  const uint64_t* mask = mask_all + (size_t)img * n * col_blocks;
  const uint64_t* diagT = diagT_all + (size_t)img * n;
  int* keep = keep_all ? keep_all + (size_t)img * n : nullptr;
  const int lane = threadIdx.x;
  const bool lazy = max_keep <= kSweepLazyMax;
  if (!lazy) {
    for (int i = lane; i < col_blocks; i += 64) remv[i] = 0;
  }
  __syncthreads();  // single-wave workgroup: orders the LDS accesses of different lanes
  int num = 0;
  if (lazy && max_keep <= kSweepPairMax) {
    // Two blocks per trip to memory (Proposal: 300 survivors).  For a pair (b, b+1) everything that does not depend on
    // the pair's own survivors was put together one iteration earlier: cur0 = removed(b), and cur1 = removed(b+1)
    // WITHOUT block b's contribution, which is added after block b is resolved from `intra` = word b+1 of block b's
    // rows (state-independent, loaded an iteration ahead).  While the pair is resolved, the loads for the NEXT pair are
    // in flight: word b+2 / b+3 of the rows that survived before b (gathered through kept_pos), of block b's and
    // block b+1's own rows (all 64 each, the survivors' words selected afterwards), the next pair's diagonal words and
    // its `intra`.  On heavy-overlap inputs (3-5 survivors per block, 70-90 blocks to reach 300) a block's resolution is
    // far shorter than a trip to L2/MALL, so halving the trips nearly halves the sweep.
    uint64_t colw0 = lane < n ? diagT[lane] : 0ULL, rowd0 = lane < n ? mask[(size_t)lane * col_blocks] : 0ULL;
    uint64_t colw1 = 0, rowd1 = 0, intra = 0;
    if (col_blocks > 1) {
      const int r1 = min(64 + lane, n - 1);
      const uint64_t cw = diagT[r1], rd = mask[(size_t)r1 * col_blocks + 1], it = mask[(size_t)min(lane, n - 1) * col_blocks + 1];
      colw1 = 64 + lane < n ? cw : 0ULL;
      rowd1 = 64 + lane < n ? rd : 0ULL;
      intra = lane < n ? it : 0ULL;
    }
    uint64_t cur0 = 0, cur1 = 0;
    for (int b = 0; b < col_blocks && num < max_keep; b += 2) {
      const bool more = b + 2 < col_blocks, more3 = b + 3 < col_blocks;
      // ---- requests for the next pair (t2 = b + 2, t3 = b + 3); unconditional loads on clamped indices ----
      const int t2 = more ? b + 2 : b, t3 = more3 ? b + 3 : t2;
      const uint64_t* m2 = mask + t2;
      const uint64_t* m3 = mask + t3;
      const int k0 = lane < num ? kept_pos[lane] : 0, k1 = lane + 64 < num ? kept_pos[lane + 64] : 0;
      const int k2 = lane + 128 < num ? kept_pos[lane + 128] : 0, k3 = lane + 192 < num ? kept_pos[lane + 192] : 0;
      const int k4 = lane + 256 < num ? kept_pos[lane + 256] : 0;
      const int ra = min(b * 64 + lane, n - 1), rb = min(b * 64 + 64 + lane, n - 1);
      const int rc = min(t2 * 64 + lane, n - 1), rd_ = min(t3 * 64 + lane, n - 1);
      const uint64_t g20 = m2[(size_t)k0 * col_blocks], g21 = m2[(size_t)k1 * col_blocks], g22 = m2[(size_t)k2 * col_blocks];
      const uint64_t g23 = m2[(size_t)k3 * col_blocks], g24 = m2[(size_t)k4 * col_blocks];
      const uint64_t g30 = m3[(size_t)k0 * col_blocks], g31 = m3[(size_t)k1 * col_blocks], g32 = m3[(size_t)k2 * col_blocks];
      const uint64_t g33 = m3[(size_t)k3 * col_blocks], g34 = m3[(size_t)k4 * col_blocks];
      const uint64_t sa2 = m2[(size_t)ra * col_blocks], sa3 = m3[(size_t)ra * col_blocks];      // block b's rows
      // block b+1's rows.  When there is no next pair (t2 / t3 clamped to b) word b of those rows lies LEFT of the diagonal,
      // which nms_mask_kernel never writes: the value would be discarded below (cur0 / cur1 are forced to 0), but read a
      // word that exists instead (their own diagonal word, or the last row's) so that nothing uninitialised is ever loaded
      const int tb2 = min(max(t2, b + 1), col_blocks - 1), tb3 = min(max(t3, b + 1), col_blocks - 1);
      const uint64_t sb2 = mask[(size_t)rb * col_blocks + tb2], sb3 = mask[(size_t)rb * col_blocks + tb3];
      const uint64_t n_colw0 = diagT[rc], n_rowd0 = m2[(size_t)rc * col_blocks], n_intra = m3[(size_t)rc * col_blocks];
      const uint64_t n_colw1 = diagT[rd_], n_rowd1 = m3[(size_t)rd_ * col_blocks];
      const bool h0 = lane < num, h1 = lane + 64 < num, h2 = lane + 128 < num, h3 = lane + 192 < num, h4 = lane + 256 < num;
      // ---- block b ----
      const int nb0 = min(64, n - b * 64);
      const bool alive0 = lane < nb0 && !((cur0 >> lane) & 1ULL);
      const uint64_t kept0 = resolve_block(__ballot(alive0), alive0, colw0, rowd0, max_keep - num);
      const bool mine0 = (kept0 >> lane) & 1ULL;
      if (mine0) {
        const int pos = num + lane_rank(kept0, lane);
        if (keep) keep[pos] = b * 64 + lane;
        kept_pos[pos] = b * 64 + lane;
      }
      num += __popcll(kept0);
      // ---- block b + 1 ----
      uint64_t kept1 = 0;
      bool mine1 = false;
      if (b + 1 < col_blocks && num < max_keep) {
        const uint64_t c1 = cur1 | wave_or64_uniform(mine0 ? intra : 0ULL);
        const int nb1 = min(64, n - (b + 1) * 64);
        const bool alive1 = lane < nb1 && !((c1 >> lane) & 1ULL);
        kept1 = resolve_block(__ballot(alive1), alive1, colw1, rowd1, max_keep - num);
        mine1 = (kept1 >> lane) & 1ULL;
        if (mine1) {
          const int pos = num + lane_rank(kept1, lane);
          if (keep) keep[pos] = (b + 1) * 64 + lane;
          kept_pos[pos] = (b + 1) * 64 + lane;
        }
        num += __popcll(kept1);
      }
      // ---- the next pair's state ----
      const bool va = b * 64 + lane < n, vb = b * 64 + 64 + lane < n;
      const uint64_t x2 = (h0 ? g20 : 0ULL) | (h1 ? g21 : 0ULL) | (h2 ? g22 : 0ULL) | (h3 ? g23 : 0ULL) | (h4 ? g24 : 0ULL) |
                          ((mine0 && va) ? sa2 : 0ULL) | ((mine1 && vb) ? sb2 : 0ULL);
      const uint64_t x3 = (h0 ? g30 : 0ULL) | (h1 ? g31 : 0ULL) | (h2 ? g32 : 0ULL) | (h3 ? g33 : 0ULL) | (h4 ? g34 : 0ULL) |
                          ((mine0 && va) ? sa3 : 0ULL) | ((mine1 && vb) ? sb3 : 0ULL);
      cur0 = more ? wave_or64_uniform(x2) : 0ULL;
      cur1 = more3 ? wave_or64_uniform(x3) : 0ULL;
      const bool vc = more && t2 * 64 + lane < n, vd = more3 && t3 * 64 + lane < n;
      colw0 = vc ? n_colw0 : 0ULL; rowd0 = vc ? n_rowd0 : 0ULL;
      intra = (vc && more3) ? n_intra : 0ULL;
      colw1 = vd ? n_colw1 : 0ULL; rowd1 = vd ? n_rowd1 : 0ULL;
      __syncthreads();
    }
  } else if (lazy) {
    // Software-pipelined: everything block b+1 needs from memory is requested before block b is resolved.
    //   removed(b+1) = OR of word b+1 of the rows kept in blocks < b   (gathered through kept_pos: known now)
    //                | OR of word b+1 of the rows block b keeps         (all 64 rows of block b are loaded
    //                                                                    speculatively, the kept lanes contribute)
    // so one block costs a ballot fixpoint and one cross-lane OR, not a dependent trip to memory.
    uint64_t colw = lane < n ? diagT[lane] : 0ULL;
    uint64_t rowd = lane < n ? mask[(size_t)lane * col_blocks] : 0ULL;
    // vmcnt(0) here, so that inside the loop the compiler knows colw / rowd have landed and their uses do not
    // wait for the loads the same iteration has just issued (the counter retires in order)
    __builtin_amdgcn_s_waitcnt(0x0F70);
    uint64_t cur = 0;     // removed-set word of the block being resolved (wave-uniform)
    for (int b = 0; b < col_blocks && num < max_keep; ++b) {
      const int base = b * 64;
      const int nb = min(64, n - base);
      const bool more = b + 1 < col_blocks;
      uint64_t col_n = 0, rowd_n = 0, spec = 0, v0 = 0, v1 = 0, v2 = 0, v3 = 0, v4 = 0, vrest = 0;
      if (more) {
        const int nxt = base + 64 + lane;
        if (nxt < n) { col_n = diagT[nxt]; rowd_n = mask[(size_t)nxt * col_blocks + b + 1]; }
        if (lane < nb) spec = mask[(size_t)(base + lane) * col_blocks + b + 1];
        const uint64_t* mcol = mask + b + 1;
        if (lane < num) v0 = mcol[(size_t)kept_pos[lane] * col_blocks];
        if (lane + 64 < num) v1 = mcol[(size_t)kept_pos[lane + 64] * col_blocks];
        if (lane + 128 < num) v2 = mcol[(size_t)kept_pos[lane + 128] * col_blocks];
        if (lane + 192 < num) v3 = mcol[(size_t)kept_pos[lane + 192] * col_blocks];
        if (lane + 256 < num) v4 = mcol[(size_t)kept_pos[lane + 256] * col_blocks];
        for (int k = lane + 320; k < num; k += 64) vrest |= mcol[(size_t)kept_pos[k] * col_blocks];
      }
      const bool alive = lane < nb && !((cur >> lane) & 1ULL);
      const uint64_t kept = resolve_block(__ballot(alive), alive, colw, rowd, max_keep - num);
      const bool mine = (kept >> lane) & 1ULL;
      if (mine) {
        const int pos = num + lane_rank(kept, lane);
        if (keep) keep[pos] = base + lane;
        kept_pos[pos] = base + lane;
      }
      num += __popcll(kept);
      if (more) cur = wave_or64_uniform(v0 | v1 | v2 | v3 | v4 | vrest | (mine ? spec : 0ULL));
      colw = col_n;
      rowd = rowd_n;
      __syncthreads();
    }
  } else {
    uint64_t col_next = lane < n ? diagT[lane] : 0ULL;
    for (int b = 0; b < col_blocks && num < max_keep; ++b) {
      const int base = b * 64;
      const int nb = min(64, n - base);
      const uint64_t colw = col_next;
      const int nxt = base + 64 + lane;
      col_next = nxt < n ? diagT[nxt] : 0ULL;     // next block's transposed diagonal: independent of the sweep state
      const uint64_t cur = remv[b];
      const bool alive = lane < nb && !((cur >> lane) & 1ULL);
      const uint64_t rowd = lane < nb ? mask[(size_t)(base + lane) * col_blocks + b] : 0ULL;
      const uint64_t kept = resolve_block(__ballot(alive), alive, colw, rowd, max_keep - num);
      if (kept == 0) continue;
      if ((kept >> lane) & 1ULL) {
        const int pos = num + lane_rank(kept, lane);
        if (keep) keep[pos] = base + lane;
      }
      num += __popcll(kept);
      __syncthreads();
      if (num >= max_keep || b + 1 >= col_blocks) break;
      // eager: OR the survivors' rows into remv for the blocks to the right of b, 8 rows per batch of loads
      uint64_t rem = kept;
      while (rem) {
        int ks[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (rem) { ks[u] = __builtin_ctzll(rem); rem &= rem - 1; } else ks[u] = -1;
        }
        for (int w0 = b + 1; w0 < col_blocks; w0 += 64) {
          const int w = w0 + lane;
          uint64_t v[8];
#pragma unroll
          for (int u = 0; u < 8; ++u)
            v[u] = (ks[u] >= 0 && w < col_blocks) ? mask[(size_t)(base + ks[u]) * col_blocks + w] : 0ULL;
          uint64_t acc = 0;
#pragma unroll
          for (int u = 0; u < 8; ++u) acc |= v[u];
          if (w < col_blocks) remv[w] |= acc;
        }
      }
      __syncthreads();
    }
  }
  if (num_keep_all && lane == 0) num_keep_all[img] = num;
  if (rois) {      // Proposal: max_keep = post_n <= kSweepMaxOut <= kSweepLazyMax, so kept_pos holds the survivors
    __syncthreads();
    const float4* sbox = sorted_box_all + (size_t)img * n;
    const uint32_t* skey = sorted_key_all + (size_t)img * n;
    proposal_write_rows(img, lane, 64, max_keep, num, rois, scores, [&](int k) { return sbox[kept_pos[k]]; },
                        [&](int k) { return skey[kept_pos[k]]; });
  }
}

}  // namespace lsfa
