// Detection overlay: the detections lsfa_det_postprocess(_batch) left on the device, burnt into the frame that is already on the device - a
// packed BGR frame or the planes of any of the 29 formats the YUV intake reads (yuvfmt.hip: 4:2:0, 4:2:2 and 4:4:4; planar, interleaved U, V
// or V, U, packed YUYV / UYVY; bytes or ten-bit words) - in two launches: a plan kernel that turns dets / counts into an ordered list of
// records, and a paint kernel per surface form.  Nothing is read back; both can sit inside a captured graph.
//
// NOT a port of anything in the reference: demo.py:150-157 ends with draw_boxes and cv2.imwrite, and cv2's rasteriser (Hershey fonts,
// anti-aliasing, its line joins) is not part of this project; draw_boxes picks random colours besides.  What is drawn is the integer
// specification of include/lsfa_hip.h, "Detection overlay" (DESIGN.md "Detection overlay"; tests/ref_overlay.py states it in numpy), matched
// bit for bit.  Out of scope: blending, anti-aliasing, packed 10-bit, 12-bit and RGB surfaces, masks.
//
// overlay_plan_kernel: one workgroup per image.  A prefix of the clamped counts over the classes says where each class's rows start, so only
// the rows under counts are walked, in draw order, 256 at a time (a frame without detections walks none); the position of a kept row is a
// prefix again - ballot and popcount inside a wave of 64, four wave counts through LDS - so the order of the records is the draw order by
// construction and no atomic's arrival order can show.  With ids (lsfa_overlay_plan_ids; the header's "Tracks") a row also needs a track id
// above 0, its colour is the track's and its label carries "-id" between the name and the score; ids == NULL is lsfa_overlay_plan.
// overlay_paint_kernel: one 256-lane workgroup per 64 x 16 tile of one frame, a lane owns four adjacent pixels of one row (the tile is
// even-sized and starts on an even pixel: its chroma samples are its own).  The workgroup first sifts the image's records, with the same
// prefix, into an LDS list of those that can touch the tile (the first 128 of them with their 16 ints, which the sift has in registers
// anyway); an empty list - most tiles of most frames - ends it before it touches the frame.  Otherwise each pixel walks the list from the
// back to its first hit.  Covered pixels are stored, whole dwords where a lane's four
// pixels are all covered and the address is aligned, bytes otherwise; an uncovered byte is never stored.
// Surfaces: BgrSurface and Yuv420Surface (lsfa_overlay_paint_bgr, lsfa_overlay_paint_yuv420) and, for lsfa_overlay_paint_yuv, PlanesSurface<SX,
// SEMI, WORDS> - compiled per horizontal chroma shift, two chroma planes or one interleaved, bytes or words; the vertical shift, V before U
// and the word's shift (c << 2 or c << 8, the whole word stored) are run-time values - and PackedSurface for YUYV / UYVY: nine
// instantiations.  The chroma sample (cx, cy) takes pixel (cx << sx, cy << sy): of a lane's four pixels all four or pixels 0 and 2, on every
// row or the even ones.  A wide store (4 to 16 bytes) is taken only where every sample of it is covered and its address is a multiple of
// its size; otherwise each covered sample is stored alone, so an uncovered sample - its ignored bits included - is never written.
#include "common.h"
#include "prefix256.h"

using namespace lsfa;

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 64, kTileH = 16;
constexpr int kRec = LSFA_OVERLAY_REC_INTS;
constexpr int kMaxChars = LSFA_OVERLAY_NAME_LEN + 6 + 6;      // a name, "-ddddd" of a track (lsfa_overlay_plan_ids only) and " d.ddd"
static_assert(10 + (kMaxChars + 3) / 4 <= kRec, "a record holds its characters");
static_assert(kTileW * kTileH == 4 * kThreads && kTileW % 2 == 0 && kTileH % 2 == 0, "four pixels per lane, even tiles");
constexpr int kStaged = 128;          // records of a tile's list kept in LDS (8 KiB); a longer list reads the rest from global memory
constexpr int kGlyphSpace = 0, kGlyphZero = 1, kGlyphDash = 38, kGlyphDot = 39, kGlyphUnknown = 41;

__device__ __forceinline__ bool finite_f64(double v) { return fabs(v) <= 1.7976931348623157e308; }          // false for NaN
__device__ __forceinline__ int corner(double v) { return (int)fmin(fmax(v, -1073741824.0), 1073741824.0); }  // the cast truncates

__global__ __launch_bounds__(kThreads) void overlay_plan_kernel(const double* __restrict__ dets, const int* __restrict__ counts,
                                                                const int* __restrict__ ids /* (N, ncls, R) or NULL */, int ncls, int R,
                                                                double thresh, int H, int W, int o, int in, int z, int with_score,
                                                                const unsigned char* __restrict__ names, int max_boxes,
                                                                int* __restrict__ records, int* __restrict__ n) {
  __shared__ int s_wave[kThreads / 64];
  __shared__ int s_first[LSFA_OVERLAY_MAX_CLASSES + 1];          // s_first[j]: the rows to draw of the classes 1 .. j-1; [ncls]: of all
  const int img = blockIdx.x;
  dets += (size_t)img * ncls * R * 5;
  counts += (size_t)img * ncls;
  if (ids) ids += (size_t)img * ncls * R;
  records += (size_t)img * max_boxes * kRec;
  // the rows to draw, class by class: an exclusive prefix of min(max(counts[j], 0), R) over j = 1 .. ncls-1, 256 classes a round, so that
  // the walk below touches those rows only - a frame without detections has none
  int carry = 0;
  for (int j0 = 1; j0 < ncls; j0 += kThreads) {
    const int j = j0 + (int)threadIdx.x;
    const int c = j < ncls ? min(max(counts[j], 0), R) : 0;
    int incl = c;               // inclusive prefix inside the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d, 64);
      if ((int)(threadIdx.x & 63) >= d) incl += up;
    }
    if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
    __syncthreads();
    int before = carry, all = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
      const int t = s_wave[w];
      before += w < (int)(threadIdx.x >> 6) ? t : 0;
      all += t;
    }
    if (j < ncls) s_first[j] = before + incl - c;
    carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) { s_first[0] = 0; s_first[ncls] = carry; }
  __syncthreads();
  const int total = carry;      // at most (ncls - 1) * R < 2^31
  int base = 0;                 // kept rows in front of this round
  for (int f0 = 0; f0 < total; f0 += kThreads) {
    const int f = f0 + (int)threadIdx.x;
    bool keep = false;
    int x1 = 0, y1 = 0, x2 = 0, y2 = 0, j = 0, id = 0;
    double score = 0.0;
    if (f < total) {
      // the class of row f: the last j in 1 .. ncls-1 with s_first[j] <= f (classes without rows share their successor's value)
      int lo = 1, hi = ncls - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_first[mid] <= f) lo = mid; else hi = mid - 1;
      }
      j = lo;
      const int r = f - s_first[j];
      {
        const double* d = dets + ((size_t)j * R + r) * 5;
        const double a = d[0], b = d[1], c = d[2], e = d[3];
        score = d[4];
        if (finite_f64(a) && finite_f64(b) && finite_f64(c) && finite_f64(e) && finite_f64(score) && score >= thresh) {
          x1 = corner(a); y1 = corner(b); x2 = corner(c); y2 = corner(e);
          keep = !(x2 < x1 || y2 < y1 || x2 < 0 || y2 < 0 || x1 > W - 1 || y1 > H - 1);
          if (ids) {
            id = ids[(size_t)j * R + r];
            keep = keep && id > 0;
          }
        }
      }
    }
    int round;
    const int pos = base + prefix_256(keep, s_wave, &round);
    base += round;
    if (keep && pos < max_boxes) {
      int* rec = records + (size_t)pos * kRec;
#pragma unroll
      for (int k = 10; k < kRec; ++k) rec[k] = 0;
      // the characters as bytes of ints 10..: this lane's own record, stored after its zeros
      unsigned char* ch = reinterpret_cast<unsigned char*>(rec + 10);
      int L = 0;
      if (z > 0) {
        if (names) {
          const unsigned char* nm = names + (size_t)j * LSFA_OVERLAY_NAME_LEN;
          for (int k = 0; k < LSFA_OVERLAY_NAME_LEN; ++k) {
            const int g = nm[k];
            if (g == 0xFF) break;
            ch[L++] = (unsigned char)(g < LSFA_OVERLAY_GLYPHS ? g : kGlyphUnknown);
          }
        } else {
          int p = 1;
          while (j / p >= 10) p *= 10;
          for (; p > 0; p /= 10) ch[L++] = (unsigned char)(kGlyphZero + (j / p) % 10);
        }
        if (ids) {
          const int m = id % 100000;
          ch[L++] = (unsigned char)kGlyphDash;
          int p = 1;
          while (m / p >= 10) p *= 10;
          for (; p > 0; p /= 10) ch[L++] = (unsigned char)(kGlyphZero + (m / p) % 10);
        }
        if (with_score) {
          const double prod = score * 1000.0;           // rounded to float64 here: the build contracts nothing (-ffp-contract=off)
          const int m = (int)fmin(fmax(floor(prod + 0.5), 0.0), 9999.0);
          ch[L++] = (unsigned char)kGlyphSpace;
          ch[L++] = (unsigned char)(kGlyphZero + m / 1000);
          ch[L++] = (unsigned char)kGlyphDot;
          ch[L++] = (unsigned char)(kGlyphZero + (m / 100) % 10);
          ch[L++] = (unsigned char)(kGlyphZero + (m / 10) % 10);
          ch[L++] = (unsigned char)(kGlyphZero + m % 10);
        }
      }
      int lx = 0, ly = 0, w = 0, h = 0;
      if (L > 0) {
        w = z * (6 * L + 1); h = 9 * z;
        lx = x1 - o; ly = y1 - o - h;
        if (ly < 0) ly = y1 + in;
        if (lx + w > W) lx = W - w;
        if (lx < 0) lx = 0;
      }
      rec[0] = x1; rec[1] = y1; rec[2] = x2; rec[3] = y2;
      rec[4] = lx; rec[5] = ly; rec[6] = w; rec[7] = h;
      rec[8] = ids ? 1 + (id - 1) % (ncls - 1) : j;
      rec[9] = L;
    }
  }
  if (threadIdx.x == 0) {
    n[2 * img] = min(base, max_boxes);
    n[2 * img + 1] = base;
  }
}

struct Paint {
  const int* records;
  const int* n;
  const unsigned char* font;
  const unsigned char* colors;
  int max_boxes, o, in, z, ncls;
  int H, W;
};

// packed BGR: three bytes a pixel
struct BgrSurface {
  unsigned char* p;
  long long pitch, stride;

  __device__ __forceinline__ void store(int img, int y, int x0, const int (&res)[4], const unsigned char* __restrict__ colors) const {
    unsigned char* row = p + (long long)img * stride + (long long)y * pitch + 3LL * x0;
    const bool all = (res[0] | res[1] | res[2] | res[3]) >= 0;
    if (all && (reinterpret_cast<uintptr_t>(row) & 3u) == 0) {
      uint32_t b[12];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) b[3 * k + c] = colors[3 * res[k] + c];
      }
      uint32_t* d = reinterpret_cast<uint32_t*>(row);
#pragma unroll
      for (int q = 0; q < 3; ++q) d[q] = b[4 * q] | b[4 * q + 1] << 8 | b[4 * q + 2] << 16 | b[4 * q + 3] << 24;
      return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (res[k] >= 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) row[3 * k + c] = colors[3 * res[k] + c];
      }
    }
  }
};

// 8-bit 4:2:0: Y[y][x] takes component 0; the chroma sample (cx, cy) components 1 and 2 of pixel (2cx, 2cy) - this lane's pixels 0 and 2 of
// an even row.  v == NULL: c is the interleaved U, V plane
struct Yuv420Surface {
  unsigned char* y;
  unsigned char* c;
  unsigned char* v;
  long long y_pitch, y_stride, c_pitch, c_stride;

  __device__ __forceinline__ void store(int img, int yy, int x0, const int (&res)[4], const unsigned char* __restrict__ colors) const {
    unsigned char* row = y + (long long)img * y_stride + (long long)yy * y_pitch + x0;
    const bool all = (res[0] | res[1] | res[2] | res[3]) >= 0;
    if (all && (reinterpret_cast<uintptr_t>(row) & 3u) == 0) {
      uint32_t dw = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) dw |= (uint32_t)colors[3 * res[k]] << (8 * k);
      *reinterpret_cast<uint32_t*>(row) = dw;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (res[k] >= 0) row[k] = colors[3 * res[k]];
      }
    }
    if (yy & 1) return;
    const long long co = (long long)img * c_stride + (long long)(yy >> 1) * c_pitch;
    const int cx = x0 >> 1;
    if (v == nullptr) {
      unsigned char* uv = c + co + 2LL * cx;
      if ((res[0] | res[2]) >= 0 && (reinterpret_cast<uintptr_t>(uv) & 3u) == 0) {
        *reinterpret_cast<uint32_t*>(uv) = (uint32_t)colors[3 * res[0] + 1] | (uint32_t)colors[3 * res[0] + 2] << 8 |
                                           (uint32_t)colors[3 * res[2] + 1] << 16 | (uint32_t)colors[3 * res[2] + 2] << 24;
        return;
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (res[2 * k] >= 0) {
          uv[2 * k] = colors[3 * res[2 * k] + 1];
          uv[2 * k + 1] = colors[3 * res[2 * k] + 2];
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (res[2 * k] >= 0) {
          c[co + cx + k] = colors[3 * res[2 * k] + 1];
          v[co + cx + k] = colors[3 * res[2 * k] + 2];
        }
      }
    }
  }
};

// ---- every YUV surface of the intake (lsfa_overlay_paint_yuv) ---------------------------------------------------------------------------
// BYTES (2, 4, 8 or 16, the address a multiple of it) as one store of the dwords r
template <int BYTES>
__device__ __forceinline__ void store_raw(unsigned char* a, const uint32_t (&r)[4]) {
  if constexpr (BYTES == 2) {
    *reinterpret_cast<uint16_t*>(a) = (uint16_t)r[0];
  } else if constexpr (BYTES == 4) {
    *reinterpret_cast<uint32_t*>(a) = r[0];
  } else if constexpr (BYTES == 8) {
    *reinterpret_cast<uint2*>(a) = make_uint2(r[0], r[1]);
  } else {
    static_assert(BYTES == 16, "a store of 2, 4, 8 or 16 bytes");
    *reinterpret_cast<uint4*>(a) = make_uint4(r[0], r[1], r[2], r[3]);
  }
}

// one sample: the byte c, or the whole 16-bit word c << shl (shl 2: the low ten bits, 8: the high ten; the ignored bits are written as 0)
template <bool WORDS>
__device__ __forceinline__ void store_sample(unsigned char* a, uint32_t c, int shl) {
  if constexpr (WORDS) *reinterpret_cast<uint16_t*>(a) = (uint16_t)(c << shl);
  else *a = (unsigned char)c;
}

// sample k (a constant under the unrolled loops) of a wide store's dwords
template <bool WORDS>
__device__ __forceinline__ void put_sample(uint32_t (&r)[4], int k, uint32_t c, int shl) {
  if constexpr (WORDS) r[k >> 1] |= (c << shl) << (16 * (k & 1));
  else r[k >> 2] |= c << (8 * (k & 3));
}

// Planes of bytes or words, chroma in two planes (SEMI false: c the U plane, v the V plane) or one interleaved plane (SEMI true: c; vu: V
// first), subsampled by (SX, sy).  The chroma sample (cx, cy) takes pixel (cx << SX, cy << sy): of this lane's four pixels every one
// (SX 0) or pixels 0 and 2 (SX 1), on the rows sy allows.  A wide store only where every sample of it is covered and it is aligned.
template <int SX, bool SEMI, bool WORDS>
struct PlanesSurface {
  unsigned char* y;
  unsigned char* c;
  unsigned char* v;
  long long y_pitch, y_stride, c_pitch, c_stride;
  int sy, vu, shl;

  __device__ __forceinline__ void store(int img, int yy, int x0, const int (&res)[4], const unsigned char* __restrict__ colors) const {
    constexpr int B = WORDS ? 2 : 1;
    unsigned char* row = y + (long long)img * y_stride + (long long)yy * y_pitch + (long long)B * x0;
    const bool all = (res[0] | res[1] | res[2] | res[3]) >= 0;
    if (all && (reinterpret_cast<uintptr_t>(row) & (uintptr_t)(4 * B - 1)) == 0) {
      uint32_t r[4] = {0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < 4; ++k) put_sample<WORDS>(r, k, colors[3 * res[k]], shl);
      store_raw<4 * B>(row, r);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (res[k] >= 0) store_sample<WORDS>(row + B * k, colors[3 * res[k]], shl);
      }
    }
    if (yy & sy) return;
    constexpr int NC = 4 >> SX;          // this lane's chroma samples of a row
    bool call = true;
#pragma unroll
    for (int k = 0; k < NC; ++k) call = call && res[k << SX] >= 0;
    const long long co = (long long)img * c_stride + (long long)(yy >> sy) * c_pitch;
    const int cx = x0 >> SX;
    if constexpr (SEMI) {
      constexpr int PAIR = 2 * B;
      unsigned char* uv = c + co + (long long)PAIR * cx;
      const int first = 1 + vu, second = 2 - vu;
      if (call && (reinterpret_cast<uintptr_t>(uv) & (uintptr_t)(NC * PAIR - 1)) == 0) {
        uint32_t r[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          put_sample<WORDS>(r, 2 * k, colors[3 * res[k << SX] + first], shl);
          put_sample<WORDS>(r, 2 * k + 1, colors[3 * res[k << SX] + second], shl);
        }
        store_raw<NC * PAIR>(uv, r);
        return;
      }
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        if (res[k << SX] >= 0) {
          store_sample<WORDS>(uv + PAIR * k, colors[3 * res[k << SX] + first], shl);
          store_sample<WORDS>(uv + PAIR * k + B, colors[3 * res[k << SX] + second], shl);
        }
      }
    } else {
      unsigned char* up = c + co + (long long)B * cx;
      unsigned char* vp = v + co + (long long)B * cx;
      if (call && ((reinterpret_cast<uintptr_t>(up) | reinterpret_cast<uintptr_t>(vp)) & (uintptr_t)(NC * B - 1)) == 0) {
        uint32_t ru[4] = {0, 0, 0, 0}, rv[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          put_sample<WORDS>(ru, k, colors[3 * res[k << SX] + 1], shl);
          put_sample<WORDS>(rv, k, colors[3 * res[k << SX] + 2], shl);
        }
        store_raw<NC * B>(up, ru);
        store_raw<NC * B>(vp, rv);
        return;
      }
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        if (res[k << SX] >= 0) {
          store_sample<WORDS>(up + B * k, colors[3 * res[k << SX] + 1], shl);
          store_sample<WORDS>(vp + B * k, colors[3 * res[k << SX] + 2], shl);
        }
      }
    }
  }
};

// packed 4:2:2 of bytes: a row is four-byte groups Y0 U Y1 V (uyvy 0) or U Y0 V Y1 (uyvy 1); group g takes U and V from pixel 2g and its Y
// bytes from pixels 2g and 2g + 1.  This lane's four pixels are two whole groups: one 8-byte store where all four are covered
struct PackedSurface {
  unsigned char* p;
  long long pitch, stride;
  int uyvy;

  __device__ __forceinline__ void store(int img, int yy, int x0, const int (&res)[4], const unsigned char* __restrict__ colors) const {
    unsigned char* row = p + (long long)img * stride + (long long)yy * pitch + 2LL * x0;
    const bool all = (res[0] | res[1] | res[2] | res[3]) >= 0;
    if (all && (reinterpret_cast<uintptr_t>(row) & 7u) == 0) {
      uint32_t r[4] = {0, 0, 0, 0};
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const uint32_t y0 = colors[3 * res[2 * g]], y1 = colors[3 * res[2 * g + 1]], u = colors[3 * res[2 * g] + 1], vv = colors[3 * res[2 * g] + 2];
        r[g] = uyvy ? (u | y0 << 8 | vv << 16 | y1 << 24) : (y0 | u << 8 | y1 << 16 | vv << 24);
      }
      store_raw<8>(row, r);
      return;
    }
    const int yo = uyvy ? 1 : 0, uo = 1 - yo;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (res[k] >= 0) {
        unsigned char* g = row + 4 * (k >> 1);
        g[yo + 2 * (k & 1)] = colors[3 * res[k]];
        if ((k & 1) == 0) {
          g[uo] = colors[3 * res[k] + 1];
          g[uo + 2] = colors[3 * res[k] + 2];
        }
      }
    }
  }
};

template <class Surface>
__global__ __launch_bounds__(kThreads) void overlay_paint_kernel(Paint a, Surface s) {
  __shared__ unsigned short s_list[LSFA_OVERLAY_MAX_BOXES];
  __shared__ int s_rec[kStaged][kRec];          // the first kStaged records of the list themselves: the walk reads them at LDS latency
  __shared__ unsigned char s_font[LSFA_OVERLAY_GLYPH_BYTES];
  __shared__ int s_wave[kThreads / 64];
  const int img = blockIdx.z;
  const int nrec = min(max(a.n[2 * img], 0), a.max_boxes);
  if (nrec == 0) return;
  const int* __restrict__ records = a.records + (size_t)img * a.max_boxes * kRec;
  // the tile, clipped to the frame
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
  const int tx1 = min(tx0 + kTileW, a.W) - 1, ty1 = min(ty0 + kTileH, a.H) - 1;
  const int o = a.o, in = a.in, z = a.z;

  // sift: the records that can touch the tile, in their order
  int cnt = 0;
  for (int b0 = 0; b0 < nrec; b0 += kThreads) {
    const int k = b0 + (int)threadIdx.x;
    bool touch = false;
    int rec[kRec];
    if (k < nrec) {
      const int* r = records + (size_t)k * kRec;
#pragma unroll
      for (int q = 0; q < kRec; ++q) rec[q] = r[q];
      const int x1 = rec[0], y1 = rec[1], x2 = rec[2], y2 = rec[3], lx = rec[4], ly = rec[5], w = rec[6], h = rec[7];
      const bool outer = x1 - o <= tx1 && x2 + o >= tx0 && y1 - o <= ty1 && y2 + o >= ty0;
      const bool inner = tx0 >= x1 + in && tx1 <= x2 - in && ty0 >= y1 + in && ty1 <= y2 - in;       // the tile is wholly inside the ring
      const bool label = z > 0 && w > 0 && h > 0 && lx <= tx1 && lx + (w - 1) >= tx0 && ly <= ty1 && ly + (h - 1) >= ty0;
      touch = (outer && !inner) || label;
    }
    int round;
    const int pos = cnt + prefix_256(touch, s_wave, &round);
    if (touch) {
      s_list[pos] = (unsigned short)k;
      if (pos < kStaged) {
#pragma unroll
        for (int q = 0; q < kRec; ++q) s_rec[pos][q] = rec[q];
      }
    }
    cnt += round;
  }
  if (cnt == 0) return;
  for (int i = threadIdx.x; i < LSFA_OVERLAY_GLYPH_BYTES; i += kThreads) s_font[i] = a.font[i];
  __syncthreads();

  // resolve: each pixel takes the last record of the list that covers it
  const int y = ty0 + ((int)threadIdx.x >> 4), x0 = tx0 + ((int)threadIdx.x & 15) * 4;
  int res[4] = {-1, -1, -1, -1};
  int pending = 0;
  if (y < a.H) {
#pragma unroll
    for (int k = 0; k < 4; ++k) pending |= x0 + k < a.W ? 1 << k : 0;
  }
  auto resolve = [&](const int* r) {
    const int x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3], lx = r[4], ly = r[5], w = r[6], h = r[7];
    const int j = min(max(r[8], 0), a.ncls), L = min(max(r[9], 0), kMaxChars);
    const bool row_label = z > 0 && w > 0 && y >= ly && y - ly < h;
    const bool row_outer = y >= y1 - o && y <= y2 + o;
    const bool row_inner = y >= y1 + in && y <= y2 - in;
    if (!row_label && !row_outer) return;
    const int dy = y - ly - z;
    const int v = row_label && dy >= 0 ? dy / z : 7;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!(pending >> k & 1)) continue;
      const int x = x0 + k;
      int c = -1;
      if (row_label && x >= lx && x - lx < w) {
        c = j;
        const int dx = x - lx - z;
        if (dx >= 0 && v < 7) {
          const int u = dx / z;
          if (u < 6 * L) {
            const int g = u / 6, col = u - 6 * g;
            if (col < 5) {
              const int idx = min((r[10 + (g >> 2)] >> (8 * (g & 3))) & 255, LSFA_OVERLAY_GLYPHS - 1);
              if (s_font[8 * idx + v] >> (4 - col) & 1) c = a.ncls;
            }
          }
        }
      } else if (row_outer && x >= x1 - o && x <= x2 + o && !(row_inner && x >= x1 + in && x <= x2 - in)) {
        c = j;
      }
      if (c >= 0) {
        res[k] = c;
        pending &= ~(1 << k);
      }
    }
  };
  for (int q = cnt - 1; q >= 0 && pending; --q) {
    if (q < kStaged) resolve(s_rec[q]);
    else resolve(records + (size_t)s_list[q] * kRec);
  }
  if ((res[0] & res[1] & res[2] & res[3]) < 0) return;          // every one of the four is -1: nothing of this lane's is covered
  s.store(img, y, x0, res, a.colors);
}

int fill_paint(const char* who, Paint& a, int N, int H, int W, const int* records, const int* n, int max_boxes, int thickness, int label_scale,
               const unsigned char* font, const unsigned char* colors, int ncls) {
  LSFA_REQUIRE(records && n && font && colors, "%s: NULL argument", who);
  LSFA_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && H <= (1 << 16) && W <= (1 << 16), "%s: bad shape: %d frames of %d x %d", who, N, W, H);
  LSFA_REQUIRE(max_boxes > 0 && max_boxes <= LSFA_OVERLAY_MAX_BOXES, "%s: max_boxes %d is outside 1..%d", who, max_boxes, LSFA_OVERLAY_MAX_BOXES);
  LSFA_REQUIRE(thickness >= 1 && thickness <= 8, "%s: thickness %d is outside 1..8", who, thickness);
  LSFA_REQUIRE(label_scale >= 0 && label_scale <= 4, "%s: label_scale %d is outside 0..4", who, label_scale);
  LSFA_REQUIRE(ncls > 0 && ncls <= LSFA_OVERLAY_MAX_CLASSES, "%s: ncls %d is outside 1..%d", who, ncls, LSFA_OVERLAY_MAX_CLASSES);
  a.records = records; a.n = n; a.font = font; a.colors = colors;
  a.max_boxes = max_boxes; a.o = (thickness - 1) / 2; a.in = thickness - a.o; a.z = label_scale; a.ncls = ncls;
  a.H = H; a.W = W;
  return LSFA_OK;
}

template <class Surface>
void launch_paint(const Paint& a, const Surface& s, int N, hipStream_t stream) {
  auto kernel = overlay_paint_kernel<Surface>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div(a.W, kTileW), (unsigned)ceil_div(a.H, kTileH), (unsigned)N), dim3(kThreads), 0, stream, a, s);
}

}  // namespace

// lsfa_overlay_plan (ids == NULL) and lsfa_overlay_plan_ids
static int plan(const char* who, const double* dets, const int* counts, const int* ids, int N, int ncls, int R, double thresh, int H, int W, int thickness,
                int label_scale, int with_score, const unsigned char* names, int max_boxes, int* records, int* n, void* stream) {
  LSFA_REQUIRE(dets && counts && records && n, "%s: NULL argument", who);
  LSFA_REQUIRE(N > 0 && N <= 65535 && ncls > 0 && ncls <= LSFA_OVERLAY_MAX_CLASSES && R > 0 && (long long)(ncls - 1) * R < (1LL << 31),
               "%s: bad shape: %d images of %d classes (at most %d) x %d rows", who, N, ncls, LSFA_OVERLAY_MAX_CLASSES, R);
  LSFA_REQUIRE(H > 0 && W > 0 && H <= (1 << 16) && W <= (1 << 16), "%s: bad frame: %d x %d", who, W, H);
  LSFA_REQUIRE(max_boxes > 0 && max_boxes <= LSFA_OVERLAY_MAX_BOXES, "%s: max_boxes %d is outside 1..%d", who, max_boxes, LSFA_OVERLAY_MAX_BOXES);
  LSFA_REQUIRE(thickness >= 1 && thickness <= 8, "%s: thickness %d is outside 1..8", who, thickness);
  LSFA_REQUIRE(label_scale >= 0 && label_scale <= 4, "%s: label_scale %d is outside 0..4", who, label_scale);
  const int o = (thickness - 1) / 2;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(overlay_plan_kernel, dim3((unsigned)N), dim3(kThreads), 0, s, dets, counts, ids, ncls, R, thresh, H, W, o, thickness - o, label_scale,
                     with_score ? 1 : 0, names, max_boxes, records, n);
  LSFA_LAUNCH_CHECK(who);
  return LSFA_OK;
}

extern "C" int lsfa_overlay_plan(const double* dets, const int* counts, int N, int ncls, int R, double thresh, int H, int W, int thickness,
                                 int label_scale, int with_score, const unsigned char* names, int max_boxes, int* records, int* n, void* stream) {
  return plan("lsfa_overlay_plan", dets, counts, nullptr, N, ncls, R, thresh, H, W, thickness, label_scale, with_score, names, max_boxes, records, n, stream);
}

extern "C" int lsfa_overlay_plan_ids(const double* dets, const int* counts, const int* ids, int N, int ncls, int R, double thresh, int H, int W,
                                     int thickness, int label_scale, int with_score, const unsigned char* names, int max_boxes, int* records, int* n,
                                     void* stream) {
  LSFA_REQUIRE(ids, "lsfa_overlay_plan_ids: NULL ids");
  LSFA_REQUIRE(ncls >= 2, "lsfa_overlay_plan_ids: ncls %d: a track's colour is one of the classes 1..ncls-1", ncls);
  return plan("lsfa_overlay_plan_ids", dets, counts, ids, N, ncls, R, thresh, H, W, thickness, label_scale, with_score, names, max_boxes, records, n, stream);
}

extern "C" int lsfa_overlay_paint_bgr(unsigned char* bgr, long long pitch, long long frame_stride, int N, int H, int W, const int* records, const int* n,
                                      int max_boxes, int thickness, int label_scale, const unsigned char* font, const unsigned char* colors, int ncls,
                                      void* stream) {
  Paint a;
  if (int rc = fill_paint("lsfa_overlay_paint_bgr", a, N, H, W, records, n, max_boxes, thickness, label_scale, font, colors, ncls)) return rc;
  LSFA_REQUIRE(bgr, "lsfa_overlay_paint_bgr: NULL frame");
  LSFA_REQUIRE(pitch >= 3LL * W, "lsfa_overlay_paint_bgr: pitch %lld is below the row's %lld bytes", pitch, 3LL * W);
  LSFA_REQUIRE(frame_stride >= 0, "lsfa_overlay_paint_bgr: frame stride %lld is negative", frame_stride);
  BgrSurface s;
  s.p = bgr; s.pitch = pitch; s.stride = frame_stride;
  launch_paint(a, s, N, (hipStream_t)stream);
  LSFA_LAUNCH_CHECK("lsfa_overlay_paint_bgr");
  return LSFA_OK;
}

extern "C" int lsfa_overlay_paint_yuv420(unsigned char* y, long long y_pitch, long long y_frame_stride, unsigned char* u_or_uv, unsigned char* v,
                                         long long c_pitch, long long c_frame_stride, int N, int H, int W, const int* records, const int* n,
                                         int max_boxes, int thickness, int label_scale, const unsigned char* font, const unsigned char* colors,
                                         int ncls, void* stream) {
  Paint a;
  if (int rc = fill_paint("lsfa_overlay_paint_yuv420", a, N, H, W, records, n, max_boxes, thickness, label_scale, font, colors, ncls)) return rc;
  LSFA_REQUIRE(y && u_or_uv, "lsfa_overlay_paint_yuv420: NULL plane");
  const long long c_row = (v ? 1LL : 2LL) * ((W + 1) / 2);
  LSFA_REQUIRE(y_pitch >= W, "lsfa_overlay_paint_yuv420: Y pitch %lld is below the row's %d bytes", y_pitch, W);
  LSFA_REQUIRE(c_pitch >= c_row, "lsfa_overlay_paint_yuv420: chroma pitch %lld is below the %s row's %lld bytes", c_pitch, v ? "I420" : "NV12", c_row);
  LSFA_REQUIRE(y_frame_stride >= 0 && c_frame_stride >= 0, "lsfa_overlay_paint_yuv420: frame strides %lld / %lld: negative", y_frame_stride,
               c_frame_stride);
  Yuv420Surface s;
  s.y = y; s.c = u_or_uv; s.v = v;
  s.y_pitch = y_pitch; s.y_stride = y_frame_stride; s.c_pitch = c_pitch; s.c_stride = c_frame_stride;
  launch_paint(a, s, N, (hipStream_t)stream);
  LSFA_LAUNCH_CHECK("lsfa_overlay_paint_yuv420");
  return LSFA_OK;
}

namespace {

template <int SX, bool SEMI, bool WORDS>
void launch_planes(const Paint& a, unsigned char* y, unsigned char* c, unsigned char* v, long long y_pitch, long long y_stride, long long c_pitch,
                   long long c_stride, int sy, int vu, int shl, int N, hipStream_t stream) {
  PlanesSurface<SX, SEMI, WORDS> s;
  s.y = y; s.c = c; s.v = v;
  s.y_pitch = y_pitch; s.y_stride = y_stride; s.c_pitch = c_pitch; s.c_stride = c_stride;
  s.sy = sy; s.vu = vu; s.shl = shl;
  launch_paint(a, s, N, stream);
}

}  // namespace

// the intake's refusals of planes (yuvfmt.hip fill_planes) and the overlay's own of everything else; nine instantiations of the paint kernel:
// (4:4:4 | 4:2:0 and 4:2:2) x (two chroma planes | one interleaved) x (bytes | words), and the packed rows
extern "C" int lsfa_overlay_paint_yuv(void* y, long long y_pitch, long long y_frame_stride, void* u_or_uv, void* v, long long c_pitch,
                                      long long c_frame_stride, int N, int H, int W, int format, const int* records, const int* n, int max_boxes,
                                      int thickness, int label_scale, const unsigned char* font, const unsigned char* colors, int ncls, void* stream) {
  const char* who = "lsfa_overlay_paint_yuv";
  Paint a;
  if (int rc = fill_paint(who, a, N, H, W, records, n, max_boxes, thickness, label_scale, font, colors, ncls)) return rc;
  const int sub = format & 15, layout = (format >> 4) & 15, sample = (format >> 8) & 15;
  LSFA_REQUIRE(format >= 0 && format < (1 << 12) && sub <= LSFA_YUV_444 && layout <= LSFA_YUV_UYVY && sample <= LSFA_YUV_HI10,
               "%s: format 0x%x is not sub (0..2) | layout (0..4) << 4 | sample (0..2) << 8", who, (unsigned)format);
  const bool packed = layout >= LSFA_YUV_YUYV, words = sample != LSFA_YUV_U8, planar = layout == LSFA_YUV_PLANAR;
  LSFA_REQUIRE(!packed || (sub == LSFA_YUV_422 && !words), "%s: format 0x%x: the packed layouts exist only as 4:2:2 of bytes", who, (unsigned)format);
  LSFA_REQUIRE(y, "%s: NULL plane", who);
  if (packed) {
    LSFA_REQUIRE(!u_or_uv && !v && c_pitch == 0 && c_frame_stride == 0,
                 "%s: a packed frame is one plane: both chroma pointers must be NULL and the chroma pitch %lld and frame stride %lld zero", who, c_pitch,
                 c_frame_stride);
  } else {
    LSFA_REQUIRE(u_or_uv, "%s: NULL plane", who);
    LSFA_REQUIRE(planar == (v != nullptr), "%s: layout %d goes with %s", who, layout,
                 planar ? "two chroma planes: v is NULL" : "one chroma plane: v must be NULL");
  }
  const int B = words ? 2 : 1;
  if (words) {
    LSFA_REQUIRE(((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(u_or_uv) | reinterpret_cast<uintptr_t>(v)) & 1u) == 0,
                 "%s: a plane of 16-bit words starts at an odd address", who);
    LSFA_REQUIRE((((unsigned long long)y_pitch | (unsigned long long)y_frame_stride | (unsigned long long)c_pitch | (unsigned long long)c_frame_stride) & 1u) == 0,
                 "%s: pitches and frame strides are bytes between 16-bit words and must be even: Y %lld / %lld, chroma %lld / %lld", who, y_pitch,
                 y_frame_stride, c_pitch, c_frame_stride);
  }
  const int sx = sub == LSFA_YUV_444 ? 0 : 1, sy = sub == LSFA_YUV_420 ? 1 : 0;
  const int cw = (W + (1 << sx) - 1) >> sx;
  const long long y_row = packed ? 4LL * cw : (long long)B * W;
  LSFA_REQUIRE(y_pitch >= y_row, "%s: %s pitch %lld is below the row's %lld bytes", who, packed ? "packed" : "Y", y_pitch, y_row);
  const long long c_row = packed ? 0 : (long long)(planar ? 1 : 2) * B * cw;
  LSFA_REQUIRE(c_pitch >= c_row, "%s: chroma pitch %lld is below the row's %lld bytes", who, c_pitch, c_row);
  LSFA_REQUIRE(y_frame_stride >= 0 && c_frame_stride >= 0, "%s: frame strides %lld / %lld: negative", who, y_frame_stride, c_frame_stride);
  hipStream_t st = (hipStream_t)stream;
  unsigned char* yb = static_cast<unsigned char*>(y);
  unsigned char* cb = static_cast<unsigned char*>(u_or_uv);
  unsigned char* vb = static_cast<unsigned char*>(v);
  if (packed) {
    PackedSurface s;
    s.p = yb; s.pitch = y_pitch; s.stride = y_frame_stride; s.uyvy = layout == LSFA_YUV_UYVY ? 1 : 0;
    launch_paint(a, s, N, st);
  } else {
    const int vu = layout == LSFA_YUV_VU ? 1 : 0, shl = sample == LSFA_YUV_U8 ? 0 : sample == LSFA_YUV_LO10 ? 2 : 8;
    switch (sx | (planar ? 0 : 2) | (words ? 4 : 0)) {
#define LSFA_SURF(SX, SEMI, WORDS)                                                                                                       \
  case SX | (SEMI ? 2 : 0) | (WORDS ? 4 : 0):                                                                                            \
    launch_planes<SX, SEMI, WORDS>(a, yb, cb, vb, y_pitch, y_frame_stride, c_pitch, c_frame_stride, sy, vu, shl, N, st);                 \
    break;
      LSFA_SURF(0, false, false) LSFA_SURF(1, false, false) LSFA_SURF(0, true, false) LSFA_SURF(1, true, false)
      LSFA_SURF(0, false, true) LSFA_SURF(1, false, true) LSFA_SURF(0, true, true) LSFA_SURF(1, true, true)
#undef LSFA_SURF
    }
  }
  LSFA_LAUNCH_CHECK(who);
  return LSFA_OK;
}
