// A ResNet unit's expanding 1x1 `conv3` (+ shortcut add) and the NEXT unit's reducing 1x1 `conv1` (+ folded bn2 + relu2) in ONE launch
// (dff_rfcn/symbols/resnet.py:70-101), for the stages whose maps do not fit the Infinity Cache: the sum (P x C fp32) is written once and
// never read back - the workgroup that produced a 128-pixel tile of it holds everything a 1x1 convolution needs for those pixels.
//   Cm = 32 KM (64 | 128)   channels of c2, conv3's input;  C = 4 Cm, the sum;  Cn = 32 KN (64 | 128), conv1's output
// One workgroup = four mixed-role waves = 128 pixels, 32 per wave, in the ring kernel's geometry (conv_ring_kernel.h).  Per tile:
//   1. c2 (128 x Cm) arrives by LDS-DMA in the ring's A-stage layout and is cut ONCE with cut8<2> under the map scale (amax_in); the
//      pieces (16 KM registers) stay live for the whole tile.
//   2. per 128-channel block j of the sum (KM blocks): acc3[4] = pieces x W3[j] (conv3's products in conv3's order: bit-identical to
//      conv_ring_kernel<4, 2, 2, false, false, 4>), the row epilogue (out-scale, through LDS to float4 rows, + residual, store), then
//      a = max(sum * scale2 + shift2, 0) (two roundings, as affine_relu4), which goes back into the wave's staging area in the A-stage layout.
//   3. the wave's own 32 x 128 block of `a` gets its own power-of-two scale s_j (its maximum into [2^13, 2^14); the map-wide maximum
//      cannot be known inside the launch, and a block's maximum is no larger: no value loses bits it keeps under the map scale, and
//      nothing overflows), is cut with it and multiplied by W1[4j .. 4j+3] into acc1[KN]; then sum1 += acc1 * (2^-s_j * w_scale[co]):
//      chains of 24 adds, then KM block sums.
//   4. bias + ReLU on sum1, z (128 x Cn) through the row path, its maximum into amax_out_z.
// Weights stream through a two-stage LDS ring of 8 KB stages (two 32-column tiles of one chunk, the fragments lsfa_conv_weights_pc
// writes): 2 KM stages of W3 and 2 KN stages of W1 per block, one barrier per stage, each wave issuing a quarter of the next stage
// before it multiplies the current one.  With two stages the newest DMA a wave has issued is always the one it waits for next, so the
// counted wait of every step is `vmcnt(0)`.  64 KB of staging + 16 KB of ring = 80 KB: two workgroups per CU where the registers
// allow it - every instantiation but Cm = Cn = 128, whose 64 registers of pieces and 64 of block sums leave no room for the rest inside the
// 256 of two waves per SIMD (it runs one workgroup per CU).
#pragma once
#include "conv_ring_kernel.h"

namespace lsfa {
namespace convsplit {

struct PairArgs {
  const float* x; const float* amax;
  const uint4* w3; const float* w3scale; const float* res; float* y; const float* scale2; const float* shift2;
  const uint4* w1; const float* w1scale; const float* bias; float* z;
  unsigned* amax_sum; unsigned* amax_z; unsigned* status;
  int P;
};

constexpr int kPairStage = 512;        // uint4 of a weight stage: 2 column tiles x 2 k-steps x 2 pieces x 64 lanes

// A block's 128 sum channels are worked in one group of four column tiles or in two groups of two: matrix instructions, row epilogue and
// residual of a group before the next group's.  Two groups hold 32 accumulator and 32 residual registers at a time instead of 64 + 64, which
// is what lets every instantiation but Cm = Cn = 64 (which fits as one group) run two workgroups per CU.  Per accumulator the products come
// in the same order either way.
constexpr int pair_groups(int KM, int KN) { return (KM == 2 && KN == 2) ? 1 : 2; }

// this wave's quarter of weight stage i of block j into ring slot i & 1
template <int KM, int KN>
__device__ __forceinline__ void pair_issue(uint4* R0, uint4* R1, const PairArgs& a, int j, int i, int wave, int lane) {
  constexpr int kW3 = 2 * KM;
  const uint4* src;
  if (i < kW3) {
    // one group: a chunk's two pairs of column tiles, then the next chunk; two groups: a pair's chunks, then the other pair's
    const int c = pair_groups(KM, KN) == 1 ? i >> 1 : i % KM, h = pair_groups(KM, KN) == 1 ? i & 1 : i / KM;
    src = a.w3 + (size_t)(c * (4 * KM) + 4 * j + 2 * h) * 256;
  } else {
    const int h = (i - kW3) / 4, c = (i - kW3) % 4;      // a pair of column tiles over the block's four chunks, then the next pair
    src = a.w1 + (size_t)((4 * j + c) * KN + 2 * h) * 256;
  }
  src += wave * 128 + lane;
  uint4* dst = ((i & 1) ? R1 : R0) + wave * 128;
  __builtin_amdgcn_global_load_lds(src, dst, 16, 0, 0);
  __builtin_amdgcn_global_load_lds(src + 64, dst + 64, 16, 0, 0);
}

// acc[2h + tt] += P x B(column tile tt of the stage), k-step 0 of both tiles, then k-step 1 (per accumulator: k-step 0, then 1)
template <int NA>
__device__ __forceinline__ void pair_mma(const uint4* B, const Cut& p, f32x16 (&acc)[NA], int h) {
  uint4 b[2][2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int q = 0; q < 2; ++q) b[tt][q] = B[((tt * 2 + s) * 2 + q) * 64];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) acc[2 * h + tt] = mma_pc<2>(s ? p.s1 : p.s0, b[tt][0], b[tt][1], b[tt][1], acc[2 * h + tt]);
  }
}

// a chunk of the wave's A image (256 uint4: 32 pixels x 8 swizzled slots) -> the lane's pieces
__device__ __forceinline__ Cut pair_cut(const uint4* A, const int (&frag)[4], float s) {
  const uint4 r0 = A[frag[0]], r1 = A[frag[1]], r2 = A[frag[2]], r3 = A[frag[3]];
  return cut_rows<2, false>(r0, r1, r2, r3, s, nullptr, 0, 0);
}

// every copy this wave has issued has landed and its LDS accesses are done, then the workgroup meets.  The wait is the BUILTIN (gfx9's
// encoding: vmcnt(0) expcnt(7) lgkmcnt(0)), which the compiler's own wait-count bookkeeping sees - behind an inline-assembly wait it still
// believes the copies pending and puts a `vmcnt(0)` of its own in front of the first LDS read that follows the NEXT stage's copies.
__device__ __forceinline__ void pair_sync() {
  __builtin_amdgcn_s_waitcnt(0x0070);
  __builtin_amdgcn_s_barrier();
}

// grid ceil(P / 128), block 256
template <int KM, int KN>
static __global__ __launch_bounds__(kThreads, (KM == 4 && KN == 4) ? 1 : 2) void conv_pair_kernel(PairArgs a) {
  constexpr int Cm = 32 * KM, C = 4 * Cm, Cn = 32 * KN;
  constexpr int kW3 = 2 * KM, kSB = 2 * KM + 2 * KN;      // weight stages per block: W3's, all (even: a block starts in ring slot 0)
  constexpr int kGroups = pair_groups(KM, KN), kGroupTiles = 4 / kGroups, kGroupStages = kW3 / kGroups;
  static_assert((KM == 2 || KM == 4) && (KN == 2 || KN == 4), "Cm and Cn are 64 or 128");
  // The ring's two stages and the staging area are THREE __shared__ objects on purpose: the compiler waits, before every LDS read, for the
  // LDS-DMA copies it cannot tell apart from the read's object - with one array that is a `vmcnt(0)` between a stage's copies and the
  // reads of the OTHER stage, i.e. no copy in flight under the matrix instructions at all.
  __shared__ __attribute__((aligned(16))) uint4 R0[kPairStage];
  __shared__ __attribute__((aligned(16))) uint4 R1[kPairStage];
  __shared__ __attribute__((aligned(16))) uint4 S[4][1024];      // per wave: 4 chunks x 4 KB (c2's arrival, the sum's rows, `a` in the A-stage layout, z's rows)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int P = a.P;
  const int m0 = blockIdx.x * kWgPix + wave * kWavePix;
  uint4* Sw = &S[wave][0];
  float* Tf = reinterpret_cast<float*>(Sw);

  // the map scale of c2: the rule of scale_finish / amax_exponent_asm with its clamp, written out (see kScaleExpMax there)
  const uint32_t* am = reinterpret_cast<const uint32_t*>(a.amax);
  uint32_t mi = max(max(am[lane] & 0x7FFFFFFFu, am[lane + 64] & 0x7FFFFFFFu), max(am[lane + 128] & 0x7FFFFFFFu, am[lane + 192] & 0x7FFFFFFFu));
  // c2: DMA i of chunk c moves pixels 8i .. 8i+7 of the wave's rows, lane -> pixel 8i + (lane >> 3), slot lane & 7
#pragma unroll
  for (int c = 0; c < KM; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pix = m0 + 8 * i + (lane >> 3);
      const int piece = LSFA_DMA_SRC_PIECE(i, lane);
      const float* src = pix < P ? a.x + (pix * Cm + c * kChunk + 4 * piece) : g_zero_block;
      __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint4*>(src), Sw + c * 256 + i * 64, 16, 0, 0);
    }
  pair_issue<KM, KN>(R0, R1, a, 0, 0, wave, lane);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mi = max(mi, (uint32_t)__shfl_xor((int)mi, d, 64));
  const int ei = (int)((mi >> 23) & 255u);
  if (ei == 255 && a.status && lane == 0) atomicOr(a.status, 2u);      // the INPUT map already holds inf / NaN
  const int s_in = 13 - ((ei == 0 || ei == 255) ? 0 : max(__builtin_amdgcn_readfirstlane(ei - 127), 13 - kScaleExpMax));
  const float a_scale = ldexpf(1.f, s_in), inv_in = ldexpf(1.f, -s_in);

  int frag[4];
  LSFA_FRAG_SLOTS(lane, frag)
  // the row path's lane -> (row 8k + lane / 8, channels 4 (lane % 8) ..); in the staging area a row's eight float4 sit in swizzled slots
  const int c4 = (lane & 7) * 4;
  int base[4], rowf[4];
  bool ok[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int row = 8 * k + (lane >> 3), p = m0 + row;
    ok[k] = p < P;
    base[k] = ok[k] ? p : 0;                                     // row 0 for a pixel past the end: a valid address, not used
    rowf[k] = row * 32 + (((lane & 7) ^ ((row >> 1) & 7)) << 2);
  }
  // where accumulator register r of a column tile goes: pixel row acc_row(r, lane) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5), channel lane & 31, the channel's piece
  // in the row's swizzled slot.  The row's swizzle (row >> 1) & 7 is ((r & 3) >> 1) | (lane >> 5) << 1 | ((r >> 2) & 1) << 2: the lane's part sits
  // in accl, the register's part is one XOR with a constant (PAIR_ACCF)
  const int accl = 128 * (lane >> 5) + (((((lane & 31) >> 2) ^ ((lane >> 5) << 1)) << 2) | (lane & 3));
#define PAIR_ACCF(r) ((((r) & 3) + 8 * ((r) >> 2)) * 32 + (accl ^ (((((r) & 3) >> 1) | ((((r) >> 2) & 1) << 2)) << 2)))

  __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0): c2 has landed (the wave reads only the rows it copied itself)
  Cut pc[KM];
#pragma unroll
  for (int c = 0; c < KM; ++c) pc[c] = pair_cut(Sw + c * 256, frag, a_scale);

  f32x16 sum1[KN];
#pragma unroll
  for (int t = 0; t < KN; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) sum1[t][r] = 0.f;
  float mx_sum = 0.f, nf_sum = 0.f;

#pragma unroll 1
  for (int j = 0; j < KM; ++j) {
    float mx = 0.f;
#pragma unroll
    for (int gq = 0; gq < kGroups; ++gq) {
      f32x16 acc3[kGroupTiles];
      float os3[kGroupTiles];
#pragma unroll
      for (int t = 0; t < kGroupTiles; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc3[t][r] = 0.f;
#pragma unroll
      for (int q = 0; q < kGroupStages; ++q) {
        const int i = gq * kGroupStages + q;
        pair_sync();
        pair_issue<KM, KN>(R0, R1, a, j, i + 1, wave, lane);
        if (q == 0) {      // the group's column scales: behind the first copy, long landed when the epilogue wants them
#pragma unroll
          for (int tq = 0; tq < kGroupTiles; ++tq) os3[tq] = a.w3scale[(unsigned)(j * 128 + (gq * kGroupTiles + tq) * 32 + (lane & 31))] * inv_in;
        }
        pair_mma<kGroupTiles>(((i & 1) ? R1 : R0) + lane, pc[kGroups == 1 ? q >> 1 : q], acc3, kGroups == 1 ? q & 1 : 0);
      }
      // conv3's epilogue, tile_rows_out's arithmetic on the staging area's swizzled rows: (0 + acc) * out-scale through LDS, + residual, store; then the next unit's bn1 + relu1
#pragma unroll
      for (int tq = 0; tq < kGroupTiles; ++tq)
#pragma unroll
        for (int r = 0; r < 16; ++r) Tf[(gq * kGroupTiles + tq) * 1024 + PAIR_ACCF(r)] = (0.f + acc3[tq][r]) * os3[tq];
      // the group's residual rows: every load before the first store (the residual is usually y itself; a lane reads and writes the same
      // addresses, no other lane touches them)
      float4 rr[4][kGroupTiles];
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int tq = 0; tq < kGroupTiles; ++tq)
          rr[k][tq] = *reinterpret_cast<const float4*>(a.res + (unsigned)(base[k] * C + j * 128 + (gq * kGroupTiles + tq) * 32 + c4));
#pragma unroll
      for (int tq = 0; tq < kGroupTiles; ++tq) {
        const int t = gq * kGroupTiles + tq;
        const float4 s2 = *reinterpret_cast<const float4*>(a.scale2 + (unsigned)(j * 128 + t * 32 + c4));
        const float4 h2 = *reinterpret_cast<const float4*>(a.shift2 + (unsigned)(j * 128 + t * 32 + c4));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float4* slot = reinterpret_cast<float4*>(&Tf[t * 1024 + rowf[k]]);
          float4 o = *slot;
          float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
          if (ok[k]) {
            o.x = o.x + rr[k][tq].x; o.y = o.y + rr[k][tq].y; o.z = o.z + rr[k][tq].z; o.w = o.w + rr[k][tq].w;
            nf_sum = nf_sum + fabsf(o.x); nf_sum = nf_sum + fabsf(o.y); nf_sum = nf_sum + fabsf(o.z); nf_sum = nf_sum + fabsf(o.w);
            *reinterpret_cast<float4*>(a.y + (unsigned)(base[k] * C + j * 128 + t * 32 + c4)) = o;
            w.x = fmaxf(o.x * s2.x + h2.x, 0.f); w.y = fmaxf(o.y * s2.y + h2.y, 0.f);
            w.z = fmaxf(o.z * s2.z + h2.z, 0.f); w.w = fmaxf(o.w * s2.w + h2.w, 0.f);
            mx = fmaxf(fmaxf(mx, fmaxf(w.x, w.y)), fmaxf(w.z, w.w));
          }
          *slot = w;      // chunk t of the wave's A image: piece lane & 7 of the row in its swizzled slot
        }
      }
    }
    mx_sum = fmaxf(mx_sum, mx);
    // the block's own scale: its maximum into [2^13, 2^14); 1 for a block of zeros (or a non-finite one: the status word reports it)
    uint32_t mb = __float_as_uint(mx);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mb = max(mb, (uint32_t)__shfl_xor((int)mb, d, 64));
    const int eb = __builtin_amdgcn_readfirstlane((int)((mb >> 23) & 255u));
    const int s_b = (eb == 0 || eb == 255) ? 0 : min(13 - (eb - 127), kScaleExpMax);
    const float b_scale = ldexpf(1.f, s_b), inv_b = ldexpf(1.f, -s_b);

    // conv1: per pair of column tiles, the block's four chunks of `a` cut (again: 256 vector instructions against 48 matrix instructions,
    // and 32 accumulator registers instead of 16 KN) and multiplied, then the pair's flush
#pragma unroll
    for (int h = 0; h < KN / 2; ++h) {
      f32x16 acc1[2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc1[t][r] = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int i = kW3 + 4 * h + c;
        pair_sync();
        if (i + 1 < kSB) pair_issue<KM, KN>(R0, R1, a, j, i + 1, wave, lane);
        else if (j + 1 < KM) pair_issue<KM, KN>(R0, R1, a, j + 1, 0, wave, lane);
        const Cut ap = pair_cut(Sw + c * 256, frag, b_scale);
        pair_mma<2>(((i & 1) ? R1 : R0) + lane, ap, acc1, 0);
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float os1 = a.w1scale[(unsigned)((2 * h + t) * 32 + (lane & 31))] * inv_b;
#pragma unroll
        for (int r = 0; r < 16; ++r) sum1[2 * h + t][r] = sum1[2 * h + t][r] + acc1[t][r] * os1;
      }
    }
  }
  publish_amax(amax_word(mx_sum, nf_sum), a.amax_sum, a.status, blockIdx.x * 4 + wave);
  // z = max(sum1 + bias, 0) through the row path (the staging area is the wave's own: no barrier)
#pragma unroll
  for (int t = 0; t < KN; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) Tf[t * 1024 + PAIR_ACCF(r)] = sum1[t][r];
  float4 bb[KN];
#pragma unroll
  for (int t = 0; t < KN; ++t) bb[t] = a.bias ? *reinterpret_cast<const float4*>(a.bias + (unsigned)(t * 32 + c4)) : make_float4(0.f, 0.f, 0.f, 0.f);
  float mx = 0.f, nf = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int t = 0; t < KN; ++t) {
      float4 o = *reinterpret_cast<const float4*>(&Tf[t * 1024 + rowf[k]]);
      if (!ok[k]) continue;
      o.x = o.x + bb[t].x; o.y = o.y + bb[t].y; o.z = o.z + bb[t].z; o.w = o.w + bb[t].w;
      nf = nf + fabsf(o.x); nf = nf + fabsf(o.y); nf = nf + fabsf(o.z); nf = nf + fabsf(o.w);
      o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f);
      *reinterpret_cast<float4*>(a.z + (unsigned)(base[k] * Cn + t * 32 + c4)) = o;
      mx = fmaxf(fmaxf(mx, fmaxf(o.x, o.y)), fmaxf(o.z, o.w));
    }
  publish_amax(amax_word(mx, nf), a.amax_z, a.status, blockIdx.x * 4 + wave);
}

#undef PAIR_ACCF

}  // namespace convsplit
}  // namespace lsfa
