// Tracks: which detection of frame f is the same object as which detection of frame f - 1, decided on the device from the dets / counts
// lsfa_det_postprocess(_batch) left there and, optionally, from the block rows lsfa_mv_estimate(_chain) wrote: a row says where the content
// of a block came from, so the rows that start inside last frame's box say where the box went.  One launch advances S independent streams
// by F frames; the track table is the caller's and nothing is read back.
//
// NOT a port of anything in the reference, which has no tracker, and not SORT, Seq-NMS or a Kalman filter: the float64 / integer
// specification of include/lsfa_hip.h, "Tracks" (DESIGN.md "Tracks"; tests/ref_tracks.py states it in numpy), matched bit for bit.
//
// track_steps_kernel: one 1024-lane workgroup per stream, the table (four coordinates and four ints a slot) in LDS for all F frames; a
// slot's score is only ever stored, so it goes straight to the caller's tbox.  A frame is five phases between barriers:
//   mark      every (class, row) cell of ids takes -1, or kPending for an eligible row; the eligible rows are counted
//   predict   a wave per active track, the lanes over the rows: three integer sums (their order is free), one division per axis
//   associate the classes are dealt to the sixteen waves - a class's match touches that class's slots only.  A wave loads 64 rows of its class
//             at a time and walks the eligible ones in order; slot t belongs to lane t % 64 in every pass, so one lane alone ever reads or
//             writes a slot in this phase and no lane depends on another's LDS store.  Only the 64-slot groups that hold a track of the class
//             are visited.  The arg-max is a __shfl_xor reduction on (IoU descending, slot ascending)
//   age       a lane per slot; the free slots, ascending, go into an LDS list by a prefix
//   birth     the cells still kPending, in draw order, by a prefix again: the k-th of them takes the k-th free slot and id issued + k + 1,
//             so the counter needs no atomic.  Skipped when every eligible row was matched, ended when the last pending one is placed
#include <cmath>

#include "common.h"
#include "prefix256.h"

using namespace lsfa;

namespace {

constexpr int kThreads = 1024, kWaves = kThreads / 64;          // sixteen waves: the classes and the tracks are dealt to them
constexpr int kMaxT = LSFA_TRACK_MAX_TRACKS;
constexpr int kPending = -2;          // in ids between mark and birth: eligible and not matched yet
constexpr int kNoSlot = 0x7fffffff;
static_assert(kMaxT % 64 == 0 && kMaxT / 64 <= 32, "the groups of 64 slots are the bits of one word");

__device__ __forceinline__ bool finite_f64(double v) { return fabs(v) <= 1.7976931348623157e308; }          // false for NaN
__device__ __forceinline__ bool eligible(double x1, double y1, double x2, double y2, double score, double thresh) {
  return finite_f64(x1) && finite_f64(y1) && finite_f64(x2) && finite_f64(y2) && finite_f64(score) && score >= thresh && x2 >= x1 && y2 >= y1;
}
__device__ __forceinline__ int wrap_inc(int v) { return (int)((unsigned)v + 1u); }
// comparisons, not fmin / fmax: with a NaN (a slot the caller filled with garbage) they give what the same comparisons give in numpy
__device__ __forceinline__ double lesser(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double greater(double a, double b) { return b > a ? b : a; }

struct TrackArgs {
  const double* dets;
  const int* counts;
  const int* rows;
  const int* row_n;
  double* tbox;
  int* tint;
  int* issued;
  int* ids;
  int* n;
  long long rows_stream_stride, rows_frame_stride;
  double score_thresh, iou_thresh;
  int F, ncls, R, n_max, max_age, min_hits, T;
};

__global__ __launch_bounds__(kThreads) void track_steps_kernel(TrackArgs a) {
  __shared__ double s_box[kMaxT][4];
  __shared__ int s_int[kMaxT][4];          // id, class, hits, misses
  __shared__ unsigned short s_free[kMaxT];
  __shared__ unsigned char s_taken[kMaxT];
  __shared__ int s_wave[kWaves];
  __shared__ int s_sum[2][kWaves];         // eligible and matched, a wave each
  __shared__ int s_cell[kMaxT];            // per slot: the cell (less R) whose FINAL id reads kPending - a matched track whose id is -2 - else -1
  __shared__ int s_collide;                // any such cell in this frame: only a wrapped counter or a caller's garbage gives a track that id
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = a.T, R = a.R, ncls = a.ncls, F = a.F;
  double* tbox = a.tbox + (size_t)s * T * 5;
  int* tint = a.tint + (size_t)s * T * 4;
  for (int t = tid; t < T; t += kThreads) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s_box[t][k] = tbox[(size_t)t * 5 + k];
      s_int[t][k] = tint[(size_t)t * 4 + k];
    }
    s_taken[t] = 0;
  }
  int issued = a.issued[s];
  __syncthreads();
  const long long cells = (long long)ncls * R;          // (ncls - 1) * R < 2^31
  const int groups = (T + 63) >> 6;
  const int step_j = kThreads / R, step_r = kThreads % R;

  for (int f = 0; f < F; ++f) {
    const size_t sf = (size_t)s * F + f;
    const double* __restrict__ dets = a.dets + sf * (size_t)cells * 5;
    const int* __restrict__ counts = a.counts + sf * ncls;
    int* ids = a.ids + sf * (size_t)cells;

    // ---- mark -------------------------------------------------------------------------------------------------------------------------
    int mine = 0;
    for (int t = tid; t < T; t += kThreads) s_cell[t] = -1;
    if (tid == 0) s_collide = 0;
    int j = tid / R, r = tid % R;          // of cell i, kept in step: no 64-bit division a cell
    for (long long i = tid; i < cells; i += kThreads, j += step_j, r += step_r) {
      if (r >= R) {
        r -= R;
        ++j;
      }
      bool e = false;
      if (j >= 1 && r < min(max(counts[j], 0), R)) {
        const double* d = dets + (size_t)i * 5;
        e = eligible(d[0], d[1], d[2], d[3], d[4], a.score_thresh);
      }
      ids[i] = e ? kPending : -1;
      mine += e ? 1 : 0;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if (lane == 0) s_sum[0][wave] = mine;

    // ---- predict ----------------------------------------------------------------------------------------------------------------------
    int nrow = 0;
    if (a.rows != nullptr && a.row_n != nullptr) nrow = min(max(a.row_n[sf], 0), a.n_max);
    if (nrow > 0) {
      const int* __restrict__ rows = a.rows + (size_t)s * a.rows_stream_stride + (size_t)f * a.rows_frame_stride;
      for (int t = wave; t < T; t += kWaves) {
        if (s_int[t][0] == 0) continue;          // the whole wave
        const double x1 = s_box[t][0], y1 = s_box[t][1], x2 = s_box[t][2], y2 = s_box[t][3];
        long long sx = 0, sy = 0;
        int c = 0;
        for (long long k0 = lane; k0 < nrow; k0 += 4 * 64) {          // four rows a lane in flight; a row past the end reads row 0 and is not counted
          int v[4][4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const long long k = k0 + 64 * u;
            const int* row = rows + (size_t)(k < nrow ? k : 0) * 7;
#pragma unroll
            for (int q = 0; q < 4; ++q) v[u][q] = row[3 + q];
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int srcx = v[u][0], srcy = v[u][1], dstx = v[u][2], dsty = v[u][3];
            const double px = (double)srcx, py = (double)srcy;
            if (k0 + 64 * u < nrow && x1 <= px && px <= x2 && y1 <= py && py <= y2) {
              ++c;
              sx += (long long)dstx - (long long)srcx;
              sy += (long long)dsty - (long long)srcy;
            }
          }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
          c += __shfl_xor(c, d, 64);
          sx += __shfl_xor(sx, d, 64);
          sy += __shfl_xor(sy, d, 64);
        }
        if (lane == 0 && c > 0) {
          if (sx != 0) {
            const double dx = (double)sx / (double)c;
            s_box[t][0] = x1 + dx;
            s_box[t][2] = x2 + dx;
          }
          if (sy != 0) {
            const double dy = (double)sy / (double)c;
            s_box[t][1] = y1 + dy;
            s_box[t][3] = y2 + dy;
          }
        }
      }
    }
    __syncthreads();

    // ---- associate --------------------------------------------------------------------------------------------------------------------
    int matched = 0;
    for (int j = 1 + wave; j < ncls; j += kWaves) {
      const int cnt = min(max(counts[j], 0), R);
      if (cnt == 0) continue;
      unsigned mask = 0;          // the groups of 64 slots that hold a track of class j
      for (int p = 0; p < groups; ++p) {
        const int t = p * 64 + lane;
        const bool here = t < T && s_int[t][0] != 0 && s_int[t][1] == j;
        if (__any(here)) mask |= 1u << p;
      }
      if (mask == 0) continue;    // every eligible row of the class stays kPending
      for (int r0 = 0; r0 < cnt; r0 += 64) {
        const int r = r0 + lane;
        double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0, v4 = 0.0;
        bool e = false;
        if (r < cnt) {
          const double* d = dets + ((size_t)j * R + r) * 5;
          v0 = d[0]; v1 = d[1]; v2 = d[2]; v3 = d[3]; v4 = d[4];
          e = eligible(v0, v1, v2, v3, v4, a.score_thresh);
        }
        for (unsigned long long em = __ballot(e); em != 0; em &= em - 1) {
          const int k = __ffsll((long long)em) - 1;
          const double dx1 = __shfl(v0, k, 64), dy1 = __shfl(v1, k, 64), dx2 = __shfl(v2, k, 64), dy2 = __shfl(v3, k, 64), dscore = __shfl(v4, k, 64);
          const double area_d = (dx2 - dx1 + 1.0) * (dy2 - dy1 + 1.0);
          double best = -INFINITY;
          int slot = kNoSlot;
          for (unsigned q = mask; q != 0; q &= q - 1) {
            const int t = (__ffs((int)q) - 1) * 64 + lane;
            if (t < T && s_int[t][0] != 0 && s_int[t][1] == j && !s_taken[t]) {
              const double tx1 = s_box[t][0], ty1 = s_box[t][1], tx2 = s_box[t][2], ty2 = s_box[t][3];
              const double area_t = (tx2 - tx1 + 1.0) * (ty2 - ty1 + 1.0);
              const double ww = lesser(dx2, tx2) - greater(dx1, tx1) + 1.0, hh = lesser(dy2, ty2) - greater(dy1, ty1) + 1.0;
              const double w = ww > 0.0 ? ww : 0.0, h = hh > 0.0 ? hh : 0.0;
              const double inter = w * h;
              const double iou = inter / (area_d + area_t - inter);
              if (iou >= a.iou_thresh && iou > best) { best = iou; slot = t; }          // ascending t: the lowest slot keeps a tie
            }
          }
#pragma unroll
          for (int d = 32; d > 0; d >>= 1) {
            const double o_best = __shfl_xor(best, d, 64);
            const int o_slot = __shfl_xor(slot, d, 64);
            if (o_best > best || (o_best == best && o_slot < slot)) { best = o_best; slot = o_slot; }
          }
          if (slot != kNoSlot) {
            ++matched;
            if (lane == (slot & 63)) {          // the slot's own lane
              s_box[slot][0] = dx1; s_box[slot][1] = dy1; s_box[slot][2] = dx2; s_box[slot][3] = dy2;
              tbox[(size_t)slot * 5 + 4] = dscore;
              const int hits = wrap_inc(s_int[slot][2]);
              s_int[slot][2] = hits;
              s_int[slot][3] = 0;
              s_taken[slot] = 1;
              const int out = hits >= a.min_hits ? s_int[slot][0] : 0;
              ids[(size_t)j * R + r0 + k] = out;
              if (out == kPending) {
                s_cell[slot] = (j - 1) * R + r0 + k;
                s_collide = 1;
              }
            }
          }
        }
      }
    }
    if (lane == 0) s_sum[1][wave] = matched;
    __syncthreads();
    int eligible_n = 0, matched_n = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      eligible_n += s_sum[0][w];
      matched_n += s_sum[1][w];
    }

    // ---- age --------------------------------------------------------------------------------------------------------------------------
    int nfree = 0;
    for (int t0 = 0; t0 < T; t0 += kThreads) {
      const int t = t0 + tid;
      bool is_free = false;
      if (t < T) {
        int id = s_int[t][0];
        if (id != 0 && !s_taken[t]) {
          const int misses = wrap_inc(s_int[t][3]);
          if (misses > a.max_age) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              s_box[t][k] = 0.0;
              s_int[t][k] = 0;
            }
            tbox[(size_t)t * 5 + 4] = 0.0;
            id = 0;
          } else {
            s_int[t][3] = misses;
          }
        }
        s_taken[t] = 0;
        is_free = id == 0;
      }
      int round;
      const int pos = nfree + prefix_block<kWaves>(is_free, s_wave, &round);
      if (is_free) s_free[pos] = (unsigned short)t;
      nfree += round;
    }
    __syncthreads();

    // ---- birth ------------------------------------------------------------------------------------------------------------------------
    const int unmatched = eligible_n - matched_n;
    const int born = min(unmatched, nfree);
    int base = 0;               // pending rows in front of this round
    for (long long i0 = R; i0 < cells && base < unmatched; i0 += kThreads) {
      const long long i = i0 + tid;
      bool pending = i < cells && ids[i] == kPending;
      if (pending && s_collide) {          // never, but for ids of -2: is the -2 a matched track's id?
        for (int t = 0; t < T; ++t) pending = pending && s_cell[t] != (int)(i - R);
      }
      int round;
      const int pos = base + prefix_block<kWaves>(pending, s_wave, &round);
      base += round;
      if (pending) {
        int out = 0;
        if (pos < nfree) {
          const int slot = s_free[pos];
          const int id = (int)((unsigned)issued + (unsigned)pos + 1u);
          const double* d = dets + (size_t)i * 5;
#pragma unroll
          for (int k = 0; k < 4; ++k) s_box[slot][k] = d[k];
          tbox[(size_t)slot * 5 + 4] = d[4];
          s_int[slot][0] = id;
          s_int[slot][1] = (int)((unsigned)i / (unsigned)R);          // i < ncls * R < 2^32
          s_int[slot][2] = 1;
          s_int[slot][3] = 0;
          out = 1 >= a.min_hits ? id : 0;
        }
        ids[i] = out;
      }
    }
    issued = (int)((unsigned)issued + (unsigned)born);
    if (tid == 0) {
      int* n = a.n + sf * 4;
      n[0] = eligible_n; n[1] = matched_n; n[2] = born; n[3] = unmatched - born;
    }
    __syncthreads();
  }

  for (int t = tid; t < T; t += kThreads) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      tbox[(size_t)t * 5 + k] = s_box[t][k];
      tint[(size_t)t * 4 + k] = s_int[t][k];
    }
  }
  if (tid == 0) a.issued[s] = issued;
}

}  // namespace

extern "C" int lsfa_track_steps(const double* dets, const int* counts, int S, int F, int ncls, int R, const int* rows, const int* row_n, int n_max,
                                long long rows_stream_stride, long long rows_frame_stride, double score_thresh, double iou_thresh, int max_age,
                                int min_hits, int T, double* tbox, int* tint, int* issued, int* ids, int* n, void* stream) {
  LSFA_REQUIRE(dets && counts && tbox && tint && issued && ids && n, "lsfa_track_steps: NULL argument");
  LSFA_REQUIRE(S > 0 && S <= 65535 && F > 0 && F <= 4096, "lsfa_track_steps: bad shape: %d streams (1..65535) of %d frames (1..4096)", S, F);
  LSFA_REQUIRE(ncls > 0 && ncls <= LSFA_OVERLAY_MAX_CLASSES && R > 0 && (long long)(ncls - 1) * R < (1LL << 31),
               "lsfa_track_steps: bad shape: %d classes (at most %d) x %d rows", ncls, LSFA_OVERLAY_MAX_CLASSES, R);
  LSFA_REQUIRE(T > 0 && T <= LSFA_TRACK_MAX_TRACKS, "lsfa_track_steps: max_tracks %d is outside 1..%d", T, LSFA_TRACK_MAX_TRACKS);
  LSFA_REQUIRE(n_max >= 0 && rows_stream_stride >= 0 && rows_frame_stride >= 0, "lsfa_track_steps: n_max %d, row strides %lld / %lld: negative", n_max,
               rows_stream_stride, rows_frame_stride);
  LSFA_REQUIRE(max_age >= 0 && min_hits >= 1, "lsfa_track_steps: max_age %d must be at least 0 and min_hits %d at least 1", max_age, min_hits);
  LSFA_REQUIRE(std::isfinite(score_thresh) && std::isfinite(iou_thresh), "lsfa_track_steps: thresholds %g / %g: not finite", score_thresh, iou_thresh);
  TrackArgs a;
  a.dets = dets; a.counts = counts; a.rows = rows; a.row_n = row_n;
  a.tbox = tbox; a.tint = tint; a.issued = issued; a.ids = ids; a.n = n;
  a.rows_stream_stride = rows_stream_stride; a.rows_frame_stride = rows_frame_stride;
  a.score_thresh = score_thresh; a.iou_thresh = iou_thresh;
  a.F = F; a.ncls = ncls; a.R = R; a.n_max = n_max; a.max_age = max_age; a.min_hits = min_hits; a.T = T;
  hipLaunchKernelGGL(track_steps_kernel, dim3((unsigned)S), dim3(kThreads), 0, (hipStream_t)stream, a);
  LSFA_LAUNCH_CHECK("lsfa_track_steps");
  return LSFA_OK;
}
