// NMS on score-sorted boxes: device-resident entry point and the reference's
// host-pointer `_nms` (lib/nms/gpu_nms.hpp:14-15).  Kernels: nms_kernels.h, and the float64 mask kernel here.
#include <mutex>
#include <string>
#include <vector>

#include "nms_kernels.h"

using namespace lsfa;

extern "C" size_t lsfa_nms_workspace_bytes(int n) {
  if (n <= 0) return 256;
  const size_t col_blocks = (size_t)ceil_div(n, 64);
  // mask (n, col_blocks) + transposed diagonal words (n)
  return align_up((size_t)n * col_blocks * sizeof(uint64_t), 256) + align_up((size_t)n * sizeof(uint64_t), 256);
}

namespace {

// ---- float64 boxes: lib/nms/nms.py:37-74 run on float64 dets (pred_eval's py_nms_wrapper) --------
// Same tiling as nms_mask_kernel; the column boxes are read at wave-uniform addresses (scalar loads).
// numpy keeps `ovr <= thresh`, so a pair suppresses when NOT (ovr <= thresh): iou_test.h's float64 pair,
// decided per column (the division for the columns that need it, not a second pass over the tile).
__global__ __launch_bounds__(256) void nms_mask_f64_kernel(const double* __restrict__ boxes, int box_dim, int n, IouTest64 t,
                                                           uint64_t* __restrict__ mask, uint64_t* __restrict__ diagT,
                                                           int col_blocks) {
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (tile >= nms_tile_count(col_blocks)) return;
  const int cb = nms_tile_column(tile), rb = tile - nms_tile_count(cb);
  const int row = rb * 64 + lane;
  const bool row_ok = row < n;
  Box64 a = {0, 0, 0, 0};
  if (row_ok) {
    const double* p = boxes + (size_t)row * box_dim;
    a = {p[0], p[1], p[2], p[3]};
  }
  const double Sa = box_area(a);
  const int ncol = min(64, n - cb * 64);
  const bool diag = rb == cb;
  uint64_t bits = 0, tbits = 0;
  for (int j = 0; j < ncol; ++j) {
    const double* q = boxes + (size_t)(cb * 64 + j) * box_dim;     // wave-uniform
    const Box64 b = {q[0], q[1], q[2], q[3]};
    const double Sb = box_area(b);
    bool unsure = !t.fast;
    bool p = iou_exceeds_fast(a, Sa, b, Sb, t, unsure);
    if (__builtin_expect(__any(unsure), 0)) {
      if (unsure) p = iou_exceeds_div(a, Sa, b, Sb, t);
    }
    p = p && row_ok && (!diag || j > lane);
    bits |= (uint64_t)p << j;
    if (diag) {
      const unsigned long long colword = __ballot(p);
      if (lane == j) tbits = colword;
    }
  }
  if (row_ok) mask[(size_t)row * col_blocks + cb] = bits;
  if (diag && row_ok) diagT[row] = tbits;
}

// The body of lsfa_nms_sorted and lsfa_nms_sorted_f64.  `who` is the export that was called: every message names it;
// launch_mask(mask, diagT, col_blocks, stream) launches its precision's mask kernel.
template <class LaunchMask>
int nms_sorted(const char* who, const void* boxes, int n, int box_dim, int* keep, int* num_keep, void* ws, size_t ws_bytes,
               void* stream, LaunchMask launch_mask) {
  LSFA_REQUIRE(n >= 0 && box_dim >= 4, "%s: bad shape n=%d box_dim=%d", who, n, box_dim);
  LSFA_REQUIRE(keep && num_keep, "%s: keep/num_keep must be non-NULL", who);
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    hipError_t e = hipMemsetAsync(num_keep, 0, sizeof(int), s);
    if (e != hipSuccess) return hip_fail(e, (std::string(who) + ": hipMemsetAsync").c_str());
    return LSFA_OK;
  }
  LSFA_REQUIRE(boxes && ws, "%s: boxes/ws must be non-NULL", who);
  const int col_blocks = ceil_div(n, 64);
  if (col_blocks > kSweepMaxBlocks) {
    set_error("%s: n=%d exceeds the supported %d boxes", who, n, kSweepMaxBlocks * 64);
    return LSFA_ENOTSUP;
  }
  if (ws_bytes < lsfa_nms_workspace_bytes(n)) {
    set_error("%s: workspace %zu < %zu bytes", who, ws_bytes, lsfa_nms_workspace_bytes(n));
    return LSFA_EWORKSPACE;
  }
  uint64_t* mask = (uint64_t*)ws;
  uint64_t* diagT = (uint64_t*)((unsigned char*)ws + align_up((size_t)n * col_blocks * sizeof(uint64_t), 256));
  ProfScope prof(LSFA_OP_NMS, s);
  launch_mask(mask, diagT, col_blocks, s);
  hipLaunchKernelGGL(nms_sweep_kernel, dim3(1), dim3(64), 0, s, (const uint64_t*)mask, (const uint64_t*)diagT, n,
                     col_blocks, n, keep, num_keep, (const float4*)nullptr, (const uint32_t*)nullptr, (float*)nullptr,
                     (float*)nullptr);
  LSFA_LAUNCH_CHECK(who);
  return LSFA_OK;
}

}  // namespace

extern "C" int lsfa_nms_sorted(const float* boxes, int n, int box_dim, float thresh, int* keep, int* num_keep,
                               void* ws, size_t ws_bytes, void* stream) {
  return nms_sorted("lsfa_nms_sorted", boxes, n, box_dim, keep, num_keep, ws, ws_bytes, stream,
                    [&](uint64_t* mask, uint64_t* diagT, int col_blocks, hipStream_t s) {
                      hipLaunchKernelGGL(nms_mask_kernel<false>, dim3(ceil_div(nms_tile_count(col_blocks), 4), 1, 1), dim3(256), 0, s,
                                         boxes, (long)n * box_dim, box_dim, (const int*)nullptr, n, make_iou_test(thresh), mask, diagT,
                                         col_blocks, 0);
                    });
}

extern "C" int lsfa_nms_sorted_f64(const double* boxes, int n, int box_dim, double thresh, int* keep, int* num_keep,
                                   void* ws, size_t ws_bytes, void* stream) {
  return nms_sorted("lsfa_nms_sorted_f64", boxes, n, box_dim, keep, num_keep, ws, ws_bytes, stream,
                    [&](uint64_t* mask, uint64_t* diagT, int col_blocks, hipStream_t s) {
                      hipLaunchKernelGGL(nms_mask_f64_kernel, dim3(ceil_div(nms_tile_count(col_blocks), 4)), dim3(256), 0, s, boxes,
                                         box_dim, n, make_iou_test64(thresh), mask, diagT, col_blocks);
                    });
}

namespace {
// `_nms` keeps the reference's host-pointer, synchronous contract, but not its three cudaMalloc/cudaFree
// per call (nms_kernel.cu:113-146): one scratch block per device, grown on demand, reused under a lock.
struct HostNmsScratch { void* p = nullptr; size_t cap = 0; };
std::mutex g_host_nms_mu;
HostNmsScratch g_host_nms[64];
}  // namespace

// lib/nms/nms_kernel.cu:97-150: host pointers in and out, synchronous, device selected by id.
// The reference prints CUDA errors and carries on (CUDA_CHECK :18-25); here an error leaves
// *num_out = 0 and the message in lsfa_last_error().  If the caller was on another device it stays
// switched to `device_id`, like after the reference's cudaSetDevice (:106-111).
extern "C" void _nms(int* keep_out, int* num_out, const float* boxes_host, int boxes_num, int boxes_dim,
                     float nms_overlap_thresh, int device_id) {
  *num_out = 0;
  if (boxes_num <= 0) return;
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess) { set_error("_nms: hipGetDevice failed"); return; }
  if (cur != device_id && hipSetDevice(device_id) != hipSuccess) { set_error("_nms: hipSetDevice(%d) failed", device_id); return; }
  if (device_id < 0 || device_id >= 64) { set_error("_nms: device_id %d out of range", device_id); return; }
  const size_t ws_bytes = lsfa_nms_workspace_bytes(boxes_num);
  const size_t bbytes = align_up((size_t)boxes_num * boxes_dim * sizeof(float), 256);
  const size_t kbytes = align_up(sizeof(int) * ((size_t)boxes_num + 1), 256);
  std::lock_guard<std::mutex> lk(g_host_nms_mu);
  HostNmsScratch& sc = g_host_nms[device_id];
  hipError_t e = hipSuccess;
  if (sc.cap < bbytes + ws_bytes + kbytes) {
    if (sc.p) (void)hipFree(sc.p);
    sc.p = nullptr; sc.cap = 0;
    const size_t want = (bbytes + ws_bytes + kbytes) * 2;      // headroom: the next, slightly larger call reuses it
    e = hipMalloc(&sc.p, want);
    if (e == hipSuccess) sc.cap = want;
  }
  if (e == hipSuccess) {
    float* boxes_dev = (float*)sc.p;
    void* ws = (unsigned char*)sc.p + bbytes;
    int* keep_dev = (int*)((unsigned char*)sc.p + bbytes + ws_bytes);
    e = hipMemcpy(boxes_dev, boxes_host, (size_t)boxes_num * boxes_dim * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
      int rc = lsfa_nms_sorted(boxes_dev, boxes_num, boxes_dim, nms_overlap_thresh, keep_dev, keep_dev + boxes_num, ws,
                               ws_bytes, nullptr);
      if (rc == LSFA_OK) {
        std::vector<int> host((size_t)boxes_num + 1);
        e = hipMemcpy(host.data(), keep_dev, sizeof(int) * host.size(), hipMemcpyDeviceToHost);
        if (e == hipSuccess) {
          const int k = host[boxes_num];
          for (int i = 0; i < k; ++i) keep_out[i] = host[i];
          *num_out = k;
        }
      }
    }
  }
  if (e != hipSuccess) hip_fail(e, "_nms");
}
