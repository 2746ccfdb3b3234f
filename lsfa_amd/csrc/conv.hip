// The split-operand convolution family (conv_split_kernel.h, conv_ring_kernel.h): every convolution of the frame path.
// fp32 in, fp32 accumulate, fp32 out; every fp32 product is formed on the bf16 / fp16 matrix pipe from `pieces` pieces per operand:
//   3  three bf16 pieces, six products (exact cut, no scale needed)
//   2  two fp16 pieces + a power-of-two scale per map (amax_in), three products: the default of the fp32 path since r4
//   1  one bf16 piece, one product: the bf16 mode (BASELINE configs[2])
// The host side is one path ("Convolution launch"): the lab switches are resolved into one Force per call (force_for),
// plan_of turns the shape and the Force into a SplitPlan (ring plan, then the direct kernel's decision, then the in_scale stage fix),
// and the plan names its kernel in one table (kRingKernels).  The launch, lsfa_conv_plan_query and the workspace queries all read that plan.
// (The exact-fp32 reference kernel, lsfa_conv_nhwc_fwd, lives in conv_exact.hip.)
#include "common.h"

#include <stdlib.h>

#include <mutex>
#include <utility>

#include "conv_ring_kernel.h"

using namespace lsfa;

namespace {
// the ring kernels that exist, keyed by (nt, pieces, st, sp, af, wv); `threads` is the workgroup each is launched with
struct RingKernel {
  int nt, pieces, st;
  bool sp, af;
  int wv;
  void (*fn)(convsplit::Args, int, int, int);
  int threads;
};

// the key space, densely numbered: 72 four-wave keys (nt 2/4 x pieces 1..3 x st 2..4 x sp x af), then 8 eight-wave ones (nt 4, mixed
// roles, pieces 1/2 x st 2/3 x af).  Not every key has a kernel: 128 x 128 tiles of three pieces at four stages are 160 KB of LDS (ring_ok),
// and the input's bn + ReLU at the cut (af) exists for pieces 1 and 2 only.
constexpr int kRingKeys = 80;
constexpr RingKernel ring_key(int i) {
  if (i >= 72) return {4, 1 + (i - 72) / 4, 2 + (i - 72) / 2 % 2, false, (i & 1) != 0, 8, nullptr, 512};
  return {2 + 2 * (i / 36), 1 + i / 12 % 3, 2 + i / 4 % 3, (i / 2 & 1) != 0, (i & 1) != 0, 4, nullptr, (i / 2 & 1) ? 512 : 256};
}
constexpr bool ring_key_exists(const RingKernel& k) { return !(k.nt == 4 && k.pieces == 3 && k.st == 4) && !(k.af && k.pieces == 3); }

struct RingTable { RingKernel e[kRingKeys]; int n; };
template <int I>
constexpr void ring_table_add(RingTable& t) {
  constexpr RingKernel k = ring_key(I);
  if constexpr (ring_key_exists(k)) {
    t.e[t.n] = k;
    t.e[t.n++].fn = convsplit::conv_ring_kernel<k.nt, k.pieces, k.st, k.sp, k.af, k.wv>;
  }
}
template <int... I>
constexpr RingTable ring_table(std::integer_sequence<int, I...>) {
  RingTable t = {};
  (ring_table_add<I>(t), ...);
  return t;
}
const RingTable kRingKernels = ring_table(std::make_integer_sequence<int, kRingKeys>());      // 66 kernels

const RingKernel* ring_kernel(int nt, int pieces, int st, bool sp, bool af, int wv) {
  for (int i = 0; i < kRingKernels.n; ++i) {
    const RingKernel& k = kRingKernels.e[i];
    if (k.nt == nt && k.pieces == pieces && k.st == st && k.sp == sp && k.af == af && k.wv == wv) return &k;
  }
  return nullptr;
}

void (*const kDirectKernels[3])(convsplit::Args) = {convsplit::conv_split_direct_kernel<1>, convsplit::conv_split_direct_kernel<2>,
                                                    convsplit::conv_split_direct_kernel<3>};

// how a convolution is launched: which kernel, the tile grid, how K is cut
struct SplitPlan {
  const RingKernel* ring;   // the ring kernel's table entry (nt, st, sp, wv below are its key); NULL: no such kernel, or the direct kernel
  int nt;               // ring kernel: 32-channel column tiles per wave (2: 128 x 64 workgroup tiles, 4: 128 x 128)
  int st;               // ring kernel: stages of the LDS ring
  bool sp;              // ring kernel: split roles (512-thread workgroups: four loader waves + four consumer waves)
  int wv;               // ring kernel: waves that multiply (4: 128-pixel tiles; 8: 256-pixel tiles, eight mixed-role waves)
  bool direct;          // conv_split_direct_kernel: operands straight into registers, a wave per 32 x 64 tile, no K slices
  int nx, ny, slices;   // tiles: nx pixel tiles x ny channel tiles x slices
  int per_slice;        // chunks (of taps * Cin / 32) per slice
  int ws_slices;        // the slices the workspace queries size for: the RING plan's, also where the direct kernel runs (see split_workspace)
};

// The lab switches of one call.  kernel / nt / st / slices: 0 = the plan decides (kernel 1: ring kernel with mixed-role waves, 2: with loader /
// consumer waves, 4: 256 x 128 tiles of eight mixed-role waves); tile_order / k_order: see xcd_tile and Walk (conv_split_kernel.h).
struct Force { int kernel, nt, st, slices, tile_order, k_order; };

// what lsfa_conv_plan_override / lsfa_conv_order_override set (orders: -1 = the environment's)
std::mutex g_api_mutex;
Force g_api_force = {0, 0, 0, 0, -1, -1};

// the environment's switches, parsed once per process:
//   LSFA_CONV_PLAN_AT="chunks,cout,kernel,nt,st,slices" forces that plan on the launches of exactly that K (in chunks of 32) and channel count
//     (an in-situ A/B of one layer inside a whole pass: the small net's fuse convolution is 72,1024; the R-FCN convolution 16,1920)
//   LSFA_CONV_TILE_ORDER: how workgroup ids map to (slice, channel tile, pixel tile), see xcd_tile
//   LSFA_CONV_K_ORDER: how the ring kernel walks K, see Walk (conv_split_kernel.h)
struct EnvForce { int at_chunks, at_cout; Force f; };
EnvForce force_from_env() {
  EnvForce e = {0, 0, {0, 0, 0, 0, 1, 0}};
  if (const char* s = getenv("LSFA_CONV_PLAN_AT")) sscanf(s, "%d,%d,%d,%d,%d,%d", &e.at_chunks, &e.at_cout, &e.f.kernel, &e.f.nt, &e.f.st, &e.f.slices);
  if (const char* s = getenv("LSFA_CONV_TILE_ORDER")) e.f.tile_order = atoi(s);
  if (const char* s = getenv("LSFA_CONV_K_ORDER")) e.f.k_order = atoi(s);
  return e;
}

// the one resolver: a LSFA_CONV_PLAN_AT hit for this launch's (chunks of K, Cout), else the API override, else "the plan decides"
Force force_for(const convsplit::Args& a) {
  static const EnvForce env = force_from_env();
  Force f;
  {
    std::lock_guard<std::mutex> lock(g_api_mutex);
    f = g_api_force;
  }
  if (env.at_chunks > 0 && env.at_chunks == a.kh * a.kw * (a.Cin / 32) && env.at_cout == a.Cout && (env.f.kernel || env.f.nt || env.f.st || env.f.slices)) {
    f.kernel = env.f.kernel; f.nt = env.f.nt; f.st = env.f.st; f.slices = env.f.slices;
  }
  if (f.tile_order < 0) f.tile_order = env.f.tile_order;
  if (f.k_order < 0) f.k_order = env.f.k_order;
  return f;
}

// the st [A | B] stages the plan reasons with (conv_ring_kernel<4, 2, 2, false, false, 4> keeps a third A stage of 16 KB behind them, out of the
// LDS its two workgroups per CU left unused: Ring::kDepthA - no plan, workspace or answer of these functions depends on it)
size_t ring_lds_bytes(int nt, int pieces, int st) { return (size_t)st * (16384 + (size_t)nt * pieces * 2048); }
bool ring_ok(int nt, int pieces, int st) {
  if (st < 2 || st > 4 || (nt != 2 && nt != 4) || pieces < 1 || pieces > 3) return false;
  if ((nt * pieces) % 2) return false;
  if (nt == 4 && pieces == 3 && st == 4) return false;       // 160 KB exactly: no room for anything else
  return ring_lds_bytes(nt, pieces, st) <= 160 * 1024 && (st - 1) * (4 + nt * pieces / 2) <= 63;
}

// The ring kernel's plan, from the sweeps of tools/lab/conv_ring_lab.py over the network's shapes (profiles/r4/conv_ring_lab.txt: every
// tile width x ring depth x K cut x wave roles, hipGraph-timed):
//   * wave roles: loader / consumer waves (512-thread workgroups) win wherever a workgroup has at least four chunks of K to walk
//     (res4 conv1 21.7 -> 19.9 us, res3 conv2 31.9 -> 26.4, the DCN contraction 59.8 -> 56.2); on the two-chunk launches (res2
//     conv3: 37,500 pixels, K = 64) the extra waves only add launch weight (38 vs 48 us): mixed-role, two-stage;
//   * ring depth 3 (two chunks in flight) everywhere else: depth 4 never measured better, depth 2 loses 5-10 % on one-workgroup-per-CU grids;
//   * 128 x 128 tiles when there are >= 512 output channels and >= 64 chunks of K (the A tile's cut and copies feed twice the MFMAs),
//     128 x 64 otherwise (more tiles for the small maps of this network);
//   * K slices: by a small cost model over rounds of resident workgroups (below).
// (r5's candidate rules - loader / consumer waves everywhere, 256 x 128 tiles for the wide short-K outputs - won their isolated-layer sweeps
// by 5-45 % per layer and LOST 2-4 % in the six-image backbone pass, twice: profiles/r5/plan_ab.txt, profiles/r6/plan_lab_g12.txt.  They are
// gone from the plan; LSFA_CONV_PLAN_AT or lsfa_conv_plan_override select the same kernels for an A/B.  The plan follows the in-situ numbers.)
SplitPlan ring_plan(long P, int chunk_total, int Cout, int pieces, const Force& f) {
  SplitPlan p = {};
  p.wv = 4;
  p.nx = (int)((P + convsplit::kWgPix - 1) / convsplit::kWgPix);
  // 128 x 128 tiles: long K with >= 512 output channels (r4, one image), or - maps of several images, the batched pipeline - wherever the
  // wider tiles alone still give the chip well over a wave of workgroups (profiles/r4/conv_ring_lab_batch3.txt: res4 conv3 44.1 -> 39.3 us,
  // res5 conv3 108 -> 97, res5 sc 153 -> 127, res3 conv2 40.9 -> 38.6 at three images); never on launches of a few chunks (res2 conv3: 144 ->
  // 168; res3 conv3 at six images: 158 -> 179)
  const long tiles4 = (long)p.nx * (Cout / 128);
  int nt = (Cout % 128 == 0 &&
            ((Cout >= 512 && chunk_total >= 64) || (tiles4 >= 400 && chunk_total >= 8) || (tiles4 >= 200 && chunk_total >= 32 && Cout <= 256))) ? 4 : 2;
  if (f.nt && Cout % (32 * f.nt) == 0) nt = f.nt;
  const long tiles = (long)p.nx * (Cout / (32 * nt));
  // K slices: rounds of resident workgroups x chunks per slice (~0.9 us per chunk and workgroup with two chunks in flight: feat_conv_3x3 as
  // 456 workgroups of 192 chunks = two rounds on 256 one-workgroup CUs = 329 us; as 304 of 288 it is also two rounds: 431 us) + ~3.5 us
  // per round for dispatch, first arrival and epilogue + the reduce pass (measured 5.5 us + 0.125 us per MB of partial sums:
  // L2 / Infinity-Cache resident); never fewer than four chunks per slice
  const double out_mb = (double)P * Cout * 4.0 / 1e6;
  int s = 1;
  double best = 1e30;
  for (int c = 1; c <= 16; ++c) {
    if (c > 1 && chunk_total / c < 4) break;
    const int per_c = (chunk_total + c - 1) / c;
    if ((chunk_total + per_c - 1) / per_c != c) continue;
    // a CU's chunk rate is shared by the workgroups resident on it (456 workgroups on two slots per CU measured like two rounds:
    // res4 conv1 cut six ways 22.9 us against 19.9 cut three ways): rounds are counted per CU
    const long rounds = (tiles * c + 255) / 256;
    const double t = rounds * (per_c * 0.9 + 3.5) + (c > 1 ? 5.5 + 0.125 * c * out_mb : 0.0);
    if (t < best * 0.97) { best = t; s = c; }      // a finer cut must pay for itself
  }
  if (f.slices) s = f.slices;
  int per = (chunk_total + s - 1) / s;
  s = (chunk_total + per - 1) / per;                    // every slice non-empty
  bool sp = per >= 4;
  // the expanding 1x1s (conv3 of a bottleneck: K = Cout / 4, at most 16 chunks, an epilogue of residual + two outputs per tile): the four
  // loader waves only add launch weight; mixed roles, two stages (res5 conv3 42.7 -> 40.4 us, res3 conv3 31.1 -> 24.9; at three images
  // res5 conv3 113 -> 97, res4 conv3 44.1 -> 39.3)
  if (s == 1 && per <= 16 && Cout >= 128 * chunk_total) sp = false;
  // 128 x 128 tiles with at least ~1.5 workgroups per CU: two 256-thread mixed-role workgroups share a CU (two stages: 64 KB of LDS each)
  // and overlap each other better than one 512-thread workgroup's loader and consumer waves do (six images, conv_ring_lab_batch6.txt:
  // res5 shortcut 275 -> 257 us, res3 conv2 75 -> 67, res3 conv1 51 -> 44, feat_conv_3x3 1852 -> 1783; the DCN contraction 265 -> 270)
  if (s == 1 && nt == 4 && tiles4 >= 400) sp = false;
  if (f.kernel == 1) sp = false;
  if (f.kernel == 2) sp = true;
  // 256 x 128 tiles, eight mixed-role waves (r5): only when forced
  const bool wv8 = f.kernel == 4 && nt == 4 && pieces < 3;
  int st = sp ? 3 : 2;
  // the one-piece (bf16) form's 128 x 128 stage is 24 KB: two mixed-role workgroups per CU fit THREE stages each (144 KB), and the second
  // chunk in flight is worth 10-28 % at six images (profiles/r4/conv_ring_lab_batch6_bf16.txt: res4 conv3 67.8 -> 48.9 us, res5 conv3
  // 189 -> 141, res5 conv1 92 -> 79, the DCN contraction 187 -> 164); the 128 x 64 tiles and the two-piece form measured no better with it
  if (!sp && pieces == 1 && nt == 4) st = 3;
  if (f.st) st = f.st;
  while (st > 2 && !ring_ok(nt, pieces, st)) --st;
  if (wv8) { p.wv = 8; sp = false; nt = 4; st = (f.st == 2) ? 2 : 3; p.nx = (int)((P + 255) / 256); }
  p.nt = nt; p.st = st; p.slices = s; p.per_slice = per; p.sp = sp;
  p.ny = Cout / (32 * nt);
  return p;
}

// (r2-r5 also had a 3x3 halo form - a workgroup staging a 4 x 32 output patch's input halo once per channel chunk; with loader / consumer
// waves the ring kernel passed it on its last shapes in r4 (res2 conv2 24.0 vs 27.1 us) and it was removed in r6; profiles/r4/conv_ring_lab.txt
// has its last numbers)

// small weights on a small map: the direct kernel (a 64-channel group's weights <= 256 KB at three pieces, re-read by every 32-pixel
// tile) while the weights' re-reads stay modest: (P / 32) tiles x all weights <= 48 MB through L2.  Never with a forced kernel or tile
// width, nor with the input's bn + ReLU at the cut (the ring kernel's)
bool direct_fits(const convsplit::Args& a, long P, int pieces, const Force& f) {
  const size_t wbytes = (size_t)a.kh * a.kw * a.Cin * 2 * pieces;      // per output channel
  // r6: a narrow exact-cut launch (the RPN head: 512 -> 64 channels, three bf16 pieces) stays on the direct kernel for a whole segment's maps
  // (21,546 pixels) too - what its K-major form did until r5 whatever the size: on the ring kernel it would be 169 workgroups of 128 x 64 tiles,
  // and its K would be summed in one chain per output instead of the direct kernel's three (the ROI coordinates' margin against float64: 1.25 / 2.0)
  const bool narrow = pieces == 3 && a.Cout <= 64;
  return a.nphase <= 1 && a.stride == 1 && wbytes * 64 <= (256u << 10) && P <= (narrow ? 32768 : 16384) &&
         (size_t)((P + 31) / 32) * wbytes * a.Cout <= ((narrow ? 160u : 48u) << 20) && f.kernel == 0 && f.nt == 0 && !a.in_scale;
}

// The plan of a launch of a.N x a.Ho x a.Wo output pixels (a.Ho / a.Wo filled in): the ring plan, then the direct kernel's decision, then
// the in_scale stage fix.  Host arithmetic on the shape alone: no pointer but in_scale's presence is looked at.
SplitPlan plan_of(const convsplit::Args& a, int pieces, const Force& f) {
  const long P = (long)a.N * a.Ho * a.Wo;
  SplitPlan p = ring_plan(P, a.kh * a.kw * (a.Cin / 32), a.Cout, pieces, f);
  p.ws_slices = p.slices;
  // (a K-major input exists in the direct kernel only: conv_split_prepare has checked that it fits)
  if (a.x_kmajor || direct_fits(a, P, pieces, f)) {
    SplitPlan d = {};
    d.direct = true;
    d.slices = 1;
    d.ws_slices = p.ws_slices;
    return d;
  }
  // with the input's activation table in LDS (16 KB more per workgroup) three stages would leave one workgroup per CU
  if (a.in_scale && !p.sp && p.wv == 4 && pieces == 1 && p.nt == 4 && p.st == 3 && f.st == 0) p.st = 2;
  p.ring = ring_kernel(p.nt, pieces, p.st, p.sp, a.in_scale != nullptr, p.wv);
  return p;
}

// What the workspace queries report and the launch asks for.  Where the direct kernel runs this is the RING plan's cut although the launch
// needs no workspace at all (the RPN head, 1 x 38 x 63, 512 -> 64, three pieces: 2,451,456 bytes): an over-report the callers' allocations
// have always had; the value is kept here, shrinking it is a change of its own.
size_t split_workspace(int slices, long P, int Cout) { return slices > 1 ? align_up((size_t)slices * P * Cout * sizeof(float), 256) : 256; }

// waves per tile of the direct kernel: at least two chunks per wave, at most kDirectMaxWaves waves
int direct_waves(const convsplit::Args& a) {
  const int nchunks = a.kh * a.kw * (a.Cin / 32);
  int nw = (nchunks + 1) / 2;
  if (nw > convsplit::kDirectMaxWaves) nw = convsplit::kDirectMaxWaves;
  return nw < 1 ? 1 : nw;
}

// every split-operand convolution goes through here; the public entry points fill in what they expose
// validation, the launch plan (plan_of), and every derived field of the argument block
int conv_split_prepare(convsplit::Args& a, int pieces, SplitPlan& p, long& P_out, const char* who) {
  const int N = a.N, H = a.H, W = a.W, Cin = a.Cin, Cout = a.Cout, kh = a.kh, kw = a.kw, stride = a.stride, dil = a.dil;
  LSFA_REQUIRE(a.x && a.wfrag && a.y, "%s: NULL argument", who);
  LSFA_REQUIRE(pieces >= 1 && pieces <= 3, "%s: pieces must be 1 (bf16), 2 (fp16 hi / lo) or 3 (bf16 x 3), not %d", who, pieces);
  LSFA_REQUIRE(pieces != 2 || a.amax, "%s: the fp16 two-piece form needs amax_in (lsfa_amax_partial of x, a producer's amax_out, or a bound)", who);
  LSFA_REQUIRE(N > 0 && H > 0 && W > 0 && kh > 0 && kw > 0 && stride > 0 && a.pad_h >= 0 && a.pad_w >= 0 && dil > 0, "%s: bad shape", who);
  LSFA_REQUIRE(!a.y2 || (a.scale2 && a.shift2), "%s: y2 given without scale2 / shift2", who);
  LSFA_REQUIRE((a.scale2 == nullptr) == (a.shift2 == nullptr), "%s: scale2 and shift2 go together", who);
  LSFA_REQUIRE(a.y2 || !a.scale2 || a.amax_out, "%s: scale2 / shift2 without y2 only publish the second output's maximum: amax_out is missing", who);
  LSFA_REQUIRE((a.in_scale == nullptr) == (a.in_shift == nullptr), "%s: in_scale and in_shift go together", who);
  if (a.in_scale && (a.kh != 1 || a.kw != 1 || a.pad_h || a.pad_w || a.Cin > convsplit::kAffineMaxCin || a.x_kmajor || a.nphase > 1 || pieces == 3)) {
    set_error("%s: in_scale / in_shift need a 1x1 convolution without padding on at most %d channels of a channels-last map, pieces 1 or 2", who,
              convsplit::kAffineMaxCin);
    return LSFA_ENOTSUP;
  }
  LSFA_REQUIRE(!a.y2 || a.y2 != a.y, "%s: y2 must not alias y", who);
  LSFA_REQUIRE(a.act >= 0 && a.act <= 2, "%s: act must be 0 (none), 1 (ReLU) or 2 (LeakyReLU 0.1)", who);
  if (Cin % 32 != 0 || Cout % convsplit::kWgCh != 0) {
    set_error("%s: Cin=%d must be a multiple of 32 and Cout=%d of %d", who, Cin, Cout, convsplit::kWgCh);
    return LSFA_ENOTSUP;
  }
  const int Ho = (H + 2 * a.pad_h - dil * (kh - 1) - 1) / stride + 1, Wo = (W + 2 * a.pad_w - dil * (kw - 1) - 1) / stride + 1;
  LSFA_REQUIRE(Ho > 0 && Wo > 0, "%s: empty output", who);
  if (a.Ho <= 0) a.Ho = Ho;        // a transposed convolution's phase passes its own (smaller) output grid
  if (a.Wo <= 0) a.Wo = Wo;
  // taps that fall outside the image read zeros wherever they are, so a grid may extend past the symmetric-padding output
  // (a transposed convolution's odd phase needs one more column on the right: padding 0 on the left, 1 on the right)
  LSFA_REQUIRE(a.Ho <= Ho + kh && a.Wo <= Wo + kw, "%s: output grid %dx%d far larger than the convolution's %dx%d", who, a.Ho, a.Wo, Ho, Wo);
  if (a.lda <= 0) a.lda = Cin;
  if (a.ldy <= 0) a.ldy = Cout;
  LSFA_REQUIRE(a.lda >= Cin && a.ldy >= Cout && a.lda % 4 == 0, "%s: lda %d / ldy %d smaller than the channel counts (or lda not a multiple of 4)", who, a.lda, a.ldy);
  LSFA_REQUIRE(!(a.y_nchw && (a.view || a.ldy != Cout)), "%s: an NCHW output cannot be a view", who);
  LSFA_REQUIRE(((uintptr_t)a.x & 15) == 0, "%s: x must be 16-byte aligned", who);
  if (!a.view) { a.out_H = a.Ho; a.out_W = a.Wo; a.out_sy = a.out_sx = 1; }
  const long P = (long)N * a.Ho * a.Wo;
  LSFA_REQUIRE(P + 256 < (1L << 24), "%s: more than 2^24 output pixels", who);      // fdiv's range (conv_split_kernel.h)
  LSFA_REQUIRE(((long)N * a.out_H * a.out_W + 1) * (long)(a.y_nchw ? Cout : a.ldy) < (1L << 31) && P * Cout < (1L << 31) &&
               ((long)N * H * W + (long)(a.pad_h + 1) * (W + 1)) * a.lda < (1L << 31), "%s: tensor too large", who);
  if (a.x_kmajor) {
    // a K-major (NCHW) input exists in the direct kernel only: 1x1, stride 1, no padding, plain output grid, small weights
    const size_t wbytes = (size_t)Cin * 2 * pieces * 64;
    if (kh != 1 || kw != 1 || stride != 1 || a.pad_h || a.pad_w || a.nphase > 1 || a.lda < Cin || wbytes > (256u << 10) || a.Ho != H || a.Wo != W) {
      set_error("%s: an NCHW input (x_nchw) needs a 1x1 / stride 1 / pad 0 convolution with at most 256 KB of weights per 64 output channels", who);
      return LSFA_ENOTSUP;
    }
    LSFA_REQUIRE((long)N * a.lda * H * W < (1L << 31), "%s: tensor too large", who);
  }
  const Force f = force_for(a);
  p = plan_of(a, pieces, f);
  LSFA_REQUIRE(p.direct || p.ring, "%s: no ring kernel for nt=%d st=%d pieces=%d", who, p.nt, p.st, pieces);
  a.tile_order = f.tile_order;
  a.k_order = f.k_order;
  a.part_stride = P * Cout;
  a.chunks_per_slice = p.per_slice;
  a.inv_wo = 1.0f / (float)a.Wo;
  a.inv_howo = 1.0f / (float)(a.Ho * a.Wo);
  a.inv_nx = 1.0f / (float)(p.nx > 0 ? p.nx : 1);
  a.inv_ny = 1.0f / (float)(p.ny > 0 ? p.ny : 1);
  a.inv_cpt = 1.0f / (float)(Cin / 32);
  a.inv_kw = 1.0f / (float)kw;
  P_out = P;
  return LSFA_OK;
}

int conv_split_launch(convsplit::Args a, int pieces, void* ws, size_t ws_bytes, void* stream, const char* who, int prof_op = LSFA_OP_CONV) {
  SplitPlan p;
  long P = 0;
  const int rc = conv_split_prepare(a, pieces, p, P, who);
  if (rc != LSFA_OK) return rc;
  const int Cout = a.Cout;
  const int nph = a.nphase > 1 ? a.nphase : 1;
  const size_t need = split_workspace(p.slices, P, Cout) * (size_t)nph;
  if (p.slices > 1 && (!ws || ws_bytes < need)) {
    set_error("%s: workspace %zu < %zu bytes", who, ws_bytes, need);
    return LSFA_EWORKSPACE;
  }
  LSFA_REQUIRE(nph == 1 || !p.direct, "%s: phases need the ring kernel", who);
  hipStream_t s = (hipStream_t)stream;
  a.part = p.slices > 1 ? (float*)ws : nullptr;
  ProfScope prof(prof_op, s);
  if (p.direct) {
    const int nw = direct_waves(a);
    hipLaunchKernelGGL(kDirectKernels[pieces - 1], dim3((unsigned)((P + 31) / 32), Cout / 64), dim3(64 * nw),
                       (size_t)(nw > 1 ? nw - 1 : 1) * 32 * 64 * sizeof(float), s, a);      // the waves' sums; at least the 8 KB the row epilogue uses
  } else {
    const int tiles = p.nx * p.ny * p.slices * nph;
    hipLaunchKernelGGL(p.ring->fn, dim3((unsigned)(8 * ((tiles + 7) / 8))), dim3(p.ring->threads), 0, s, a, p.nx, p.ny, p.slices * nph);
  }
  if (p.slices > 1 && a.y_nchw && !a.res && !a.scale2 && nph == 1 && Cout % 64 == 0) {
    hipLaunchKernelGGL(convsplit::split_reduce_nchw_kernel, dim3((unsigned)((P + 63) / 64), (unsigned)(Cout / 64)), dim3(convsplit::kThreads), 0,
                       s, a, p.slices);
  } else if (p.slices > 1) {
    const long n4 = P * Cout / 4;
    hipLaunchKernelGGL(convsplit::split_reduce_kernel, dim3((unsigned)((n4 + convsplit::kThreads - 1) / convsplit::kThreads), nph),
                       dim3(convsplit::kThreads), 0, s, a, n4, p.slices);
  }
  LSFA_LAUNCH_CHECK(who);
  return LSFA_OK;
}

convsplit::Args args_of(const lsfa_conv_desc& d) {
  convsplit::Args a = {};
  a.x = d.x; a.wfrag = (const uint4*)d.wfrag; a.bias = d.bias; a.y = d.y;
  a.N = d.N; a.H = d.H; a.W = d.W; a.Cin = d.Cin; a.Cout = d.Cout; a.kh = d.kh; a.kw = d.kw; a.stride = d.stride;
  a.pad_h = d.pad_h; a.pad_w = d.pad_w; a.dil = d.dil; a.act = d.act; a.y_nchw = d.y_nchw;
  a.res = d.residual; a.y2 = d.y2; a.scale2 = d.scale2; a.shift2 = d.shift2;
  a.lda = d.lda; a.ldy = d.ldy; a.Ho = d.Ho; a.Wo = d.Wo;
  if (d.out_H > 0) { a.view = 1; a.out_H = d.out_H; a.out_W = d.out_W; a.out_sy = d.out_sy; a.out_sx = d.out_sx; }
  a.amax = d.amax_in; a.w_exp = d.w_exp; a.amax_out = d.amax_out; a.status = d.status;
  a.wscale = d.w_scale;
  a.x_kmajor = d.x_nchw ? 1 : 0;
  a.in_scale = d.in_scale; a.in_shift = d.in_shift;
  return a;
}
}  // namespace

extern "C" int lsfa_conv_plan_override(int kernel, int nt, int st, int slices) {
  LSFA_REQUIRE(kernel >= 0 && kernel <= 4 && kernel != 3 && (nt == 0 || nt == 2 || nt == 4) && (st == 0 || (st >= 2 && st <= 4)) && slices >= 0 && slices <= 16,
               "lsfa_conv_plan_override: kernel 0, 1, 2 or 4 (3 was the halo form, removed in r6), nt 0/2/4, st 0/2..4, slices 0..16");
  std::lock_guard<std::mutex> lock(g_api_mutex);
  g_api_force.kernel = kernel; g_api_force.nt = nt; g_api_force.st = st; g_api_force.slices = slices;
  return LSFA_OK;
}

extern "C" int lsfa_conv_order_override(int tile_order, int k_order) {
  LSFA_REQUIRE(tile_order >= -1 && tile_order <= 1 && k_order >= -1 && k_order <= 1, "lsfa_conv_order_override: tile_order and k_order are -1 (default), 0 or 1");
  std::lock_guard<std::mutex> lock(g_api_mutex);
  g_api_force.tile_order = tile_order; g_api_force.k_order = k_order;
  return LSFA_OK;
}

extern "C" size_t lsfa_conv_weight_bytes(int Cout, int kh, int kw, int Cin, int pieces) {
  if (Cout <= 0 || kh <= 0 || kw <= 0 || Cin <= 0 || Cin % 32 != 0 || Cout % 64 != 0 || pieces < 1 || pieces > 3) return 0;
  return (size_t)Cout * kh * kw * Cin * 2 * pieces;
}

extern "C" int lsfa_conv_weights(const float* w, int Cout, int kh, int kw, int Cin, int pieces, int w_exp, void* wfrag, void* stream) {
  LSFA_REQUIRE(w && wfrag, "lsfa_conv_weights: NULL argument");
  if (lsfa_conv_weight_bytes(Cout, kh, kw, Cin, pieces) == 0) {
    set_error("lsfa_conv_weights: Cin=%d must be a multiple of 32, Cout=%d of 64, pieces=%d one of 1, 2, 3", Cin, Cout, pieces);
    return LSFA_ENOTSUP;
  }
  LSFA_REQUIRE(w_exp > -120 && w_exp < 120 && (pieces == 2 || w_exp == 0), "lsfa_conv_weights: w_exp %d out of range (it is 0 unless pieces == 2)", w_exp);
  const long total = (long)kh * kw * (Cin / 32) * (Cout / 32) * 2 * 64;
  const dim3 grid((unsigned)((total + 255) / 256));
  hipStream_t s = (hipStream_t)stream;
  if (pieces == 3) hipLaunchKernelGGL(convsplit::pack_weights_kernel<3>, grid, dim3(256), 0, s, w, (uint4*)wfrag, Cout, kh * kw, Cin, 0);
  else if (pieces == 2) hipLaunchKernelGGL(convsplit::pack_weights_kernel<2>, grid, dim3(256), 0, s, w, (uint4*)wfrag, Cout, kh * kw, Cin, w_exp);
  else hipLaunchKernelGGL(convsplit::pack_weights_kernel<1>, grid, dim3(256), 0, s, w, (uint4*)wfrag, Cout, kh * kw, Cin, 0);
  LSFA_LAUNCH_CHECK("lsfa_conv_weights");
  return LSFA_OK;
}

// r5: the two-piece form with one power-of-two scale per OUTPUT channel: w_exp_pc[co] (device, Cout ints) scales channel co's weights where
// they are cut; the caller passes wscale[co] = 2^-w_exp_pc[co] (floats, device) as lsfa_conv_desc::w_scale.
extern "C" int lsfa_conv_weights_pc(const float* w, int Cout, int kh, int kw, int Cin, const int* w_exp_pc, void* wfrag, void* stream) {
  LSFA_REQUIRE(w && wfrag && w_exp_pc, "lsfa_conv_weights_pc: NULL argument");
  if (lsfa_conv_weight_bytes(Cout, kh, kw, Cin, 2) == 0) {
    set_error("lsfa_conv_weights_pc: Cin=%d must be a multiple of 32, Cout=%d of 64", Cin, Cout);
    return LSFA_ENOTSUP;
  }
  const long total = (long)kh * kw * (Cin / 32) * (Cout / 32) * 2 * 64;
  hipLaunchKernelGGL(convsplit::pack_weights_kernel<2>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, (uint4*)wfrag, Cout,
                     kh * kw, Cin, 0, w_exp_pc);
  LSFA_LAUNCH_CHECK("lsfa_conv_weights_pc");
  return LSFA_OK;
}

extern "C" size_t lsfa_conv_workspace_bytes(const lsfa_conv_desc* d) {
  if (!d || d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Cout <= 0 || d->Cin <= 0 || d->stride <= 0 || d->kh <= 0 || d->kw <= 0 || d->dil <= 0 ||
      d->pad_h < 0 || d->pad_w < 0 || d->pieces < 1 || d->pieces > 3 || d->Cin % 32 || d->Cout % 64)
    return 0;
  const int Hn = (d->H + 2 * d->pad_h - d->dil * (d->kh - 1) - 1) / d->stride + 1, Wn = (d->W + 2 * d->pad_w - d->dil * (d->kw - 1) - 1) / d->stride + 1;
  const int Ho = d->Ho > 0 ? d->Ho : Hn, Wo = d->Wo > 0 ? d->Wo : Wn;
  if (Ho <= 0 || Wo <= 0) return 0;
  convsplit::Args a = args_of(*d);
  a.Ho = Ho; a.Wo = Wo;
  return split_workspace(plan_of(a, d->pieces, force_for(a)).ws_slices, (long)d->N * Ho * Wo, d->Cout);
}

extern "C" int lsfa_conv_fwd(const lsfa_conv_desc* d, void* ws, size_t ws_bytes, void* stream) {
  LSFA_REQUIRE(d, "lsfa_conv_fwd: NULL descriptor");
  return conv_split_launch(args_of(*d), d->pieces, ws, ws_bytes, stream, "lsfa_conv_fwd", LSFA_OP_CONV);
}

extern "C" int lsfa_conv_plan_query(const lsfa_conv_desc* d, int* out8) {
  LSFA_REQUIRE(d && out8, "lsfa_conv_plan_query: NULL argument");
  convsplit::Args a = args_of(*d);
  SplitPlan p;
  long P = 0;
  const int rc = conv_split_prepare(a, d->pieces, p, P, "lsfa_conv_plan_query");
  if (rc != LSFA_OK) return rc;
  // the words name the kernel the launch would run: the direct kernel, or the table entry of the ring kernel
  const RingKernel direct = {2, d->pieces, 0, false, false, 4, nullptr, 0};
  const RingKernel& k = p.direct ? direct : *p.ring;
  out8[0] = p.direct ? 2 : 1;
  out8[1] = k.nt; out8[2] = k.st; out8[3] = k.sp ? 1 : 0; out8[4] = k.wv; out8[5] = p.slices;
  out8[6] = k.af ? 1 : 0; out8[7] = k.pieces;
  return LSFA_OK;
}

extern "C" int lsfa_amax_partial(const float* x, long long n, float* out, void* stream) {
  LSFA_REQUIRE(x && out && n > 0 && n % 4 == 0 && ((uintptr_t)x & 15) == 0, "lsfa_amax_partial: x must be 16-byte aligned, n a positive multiple of 4");
  hipLaunchKernelGGL(convsplit::amax_partial_kernel, dim3(convsplit::kAmaxSlots), dim3(256), 0, (hipStream_t)stream, (const float4*)x,
                     (long)(n / 4), out);
  LSFA_LAUNCH_CHECK("lsfa_amax_partial");
  return LSFA_OK;
}

// The device's status word (bit 0: a convolution wrote a non-finite value - with the fp16 form that is what an under-estimated amax
// produces; bit 1: a convolution's INPUT maximum was already inf / NaN): read it (synchronising `stream`), clear it, and turn a set bit
// into an error.
extern "C" int lsfa_status_check(unsigned* status_dev, void* stream) {
  LSFA_REQUIRE(status_dev, "lsfa_status_check: NULL status word");
  unsigned h = 0;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(&h, status_dev, sizeof(h), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(e, "lsfa_status_check");
  if (h == 0) return LSFA_OK;
  e = hipMemsetAsync(status_dev, 0, sizeof(unsigned), s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(e, "lsfa_status_check");
  set_error("lsfa_status_check: status 0x%x:%s%s", h,
            (h & 1u) ? " a convolution produced a non-finite output (fp16 two-piece form: amax_in under-estimates max|x|, or the input held inf / NaN)" : "",
            (h & 2u) ? " a convolution's input maximum was inf / NaN" : "");
  return LSFA_EOVERFLOW;
}

// Deconvolution(kernel 4, stride 2, pad 0) + Crop(offset (1,1)) to Hc x Wc as ONE launch of four 2x2-tap phase convolutions.
// Output row 2m + py of the cropped map reads input rows (m - 1, m) through taps ky = (3, 1) when py = 0 and rows (m, m + 1)
// through ky = (2, 0) when py = 1 (columns alike): phase (py, px) is an ordinary 2x2 convolution with padding (1 - py, 1 - px)
// whose weights wfrag[py * 2 + px] the caller cut with lsfa_conv_weights from w[:, :, kys, kxs] (Cout, 2, 2, Cin).
extern "C" size_t lsfa_deconv4x4s2_crop_workspace_bytes(int N, int Hi, int Wi, int Cin, int Cout, int Hc, int Wc, int pieces) {
  if (N <= 0 || Hi <= 0 || Wi <= 0 || Cin <= 0 || Cout <= 0 || Hc <= 0 || Wc <= 0 || pieces < 1 || pieces > 3) return 0;
  const int gh = (Hc + 1) / 2, gw = (Wc + 1) / 2;
  convsplit::Args a = {};
  a.N = N; a.Ho = gh; a.Wo = gw; a.Cin = Cin; a.Cout = Cout; a.kh = a.kw = 2; a.stride = 1; a.nphase = 4;      // as lsfa_deconv4x4s2_crop_fwd sizes its launch
  return split_workspace(plan_of(a, pieces, force_for(a)).ws_slices, (long)N * gh * gw, Cout) * 4;
}

extern "C" int lsfa_deconv4x4s2_crop_fwd(const float* x, int lda, int N, int Hi, int Wi, int Cin, const void* wfrag4, int pieces, int w_exp,
                                         const float* amax_in, const float* bias, int Cout, int act, float* y, int ldy, int Hc, int Wc,
                                         unsigned* amax_out, unsigned* status, void* ws, size_t ws_bytes, void* stream) {
  LSFA_REQUIRE(x && wfrag4 && y, "lsfa_deconv4x4s2_crop_fwd: NULL argument");
  LSFA_REQUIRE(act >= 0 && act <= 2 && Hc > 0 && Wc > 0 && Hc <= 2 * Hi + 1 && Wc <= 2 * Wi + 1, "lsfa_deconv4x4s2_crop_fwd: bad shape");
  convsplit::Args a = {};
  a.x = x; a.bias = bias; a.wfrag = (const uint4*)wfrag4; a.y = y;
  a.N = N; a.H = Hi; a.W = Wi; a.Cin = Cin; a.Cout = Cout; a.kh = a.kw = 2; a.stride = 1; a.dil = 1;
  a.act = act; a.lda = lda; a.ldy = ldy;
  a.view = 1; a.out_H = Hc; a.out_W = Wc; a.out_sy = a.out_sx = 2;
  a.nphase = 4;
  a.ph_wstride = (long)(lsfa_conv_weight_bytes(Cout, 2, 2, Cin, pieces) / 16);
  a.amax = amax_in; a.w_exp = w_exp; a.amax_out = amax_out; a.status = status;
  // the launch is sized for phase (0, 0), the largest grid
  a.pad_h = a.pad_w = 1; a.Ho = (Hc + 1) / 2; a.Wo = (Wc + 1) / 2;
  return conv_split_launch(a, pieces, ws, ws_bytes, stream, "lsfa_deconv4x4s2_crop_fwd", LSFA_OP_CONV);
}
