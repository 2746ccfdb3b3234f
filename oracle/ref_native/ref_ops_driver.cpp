/* Host driver of the reference's own PSROI pooling and MultiProposal kernels.
 *
 * The arithmetic is NOT in this file: it is in _ref/psroi.inc, _ref/proposal.inc and _ref/anchors.inc, which
 * the build cuts out of the reference tree (oracle/ref_native/slice.py) and which are never committed.  This
 * file holds the launch geometry and the host code that cannot be sliced because it is tangled with MXNet,
 * thrust and cudaMalloc; each such piece names the lines of the reference it follows.
 *
 * Built three times from the same text, with -ffp-contract=on (one expression `a*b + c` fuses: the rule
 * claimed for nvcc's -fmad=true, the authoritative build), =off and =fast.
 */
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "cuda_host_shim.h"

namespace ref {
#include "psroi.inc"
#include "proposal.inc"
#include "anchors.inc"

/* MXNet's launch constants: mshadow/cuda/tensor_gpu-inl.cuh (kMaxThreadsPerBlock, kBaseThreadNum, kMaxGridNum)
 * and mxnet_op.h's cuda_get_num_blocks. */
static const int kMaxThreadsPerBlock = 1024;
static const int kBaseThreadNum = 256;
static const int kMaxGridNum = 65535;
static int cuda_get_num_blocks(int n) { return std::min(kMaxGridNum, (n + kBaseThreadNum - 1) / kBaseThreadNum); }
}  // namespace ref

extern "C" {

/* PSROIPoolForward's launch, psroi_pooling.cu:116-126.  The kernel advances its bottom_rois and bottom_data
 * PARAMETERS inside its grid-stride loop, so it is only right when every thread's loop body runs once; the
 * reference's geometry gives that for count <= 65535 * 256, which is checked here.  Each emulated thread is a
 * fresh call, so the parameters start from the caller's pointers every time.  Returns 0, or -1 if the
 * geometry would make a thread loop twice. */
int ref_psroi_pool(const float* data, const float* rois, int channels, int height, int width, int num_rois,
                   float spatial_scale, int output_dim, int pooled_size, int group_size, float* out, float* mapping) {
  const int count = num_rois * output_dim * pooled_size * pooled_size;
  const int blocks = ref::cuda_get_num_blocks(count);
  if ((long long)blocks * ref::kBaseThreadNum < count) return -1;
  ref::launch_1d(blocks, ref::kBaseThreadNum, [&] {
    ref::PSROIPoolForwardKernel<float>(count, data, spatial_scale, channels, height, width, pooled_size, pooled_size,
                                       rois, output_dim, group_size, out, mapping);
  });
  return 0;
}

/* utils::GenerateAnchors as MultiProposalGPUOp::Forward calls it, multi_proposal.cu:440-450.  anchors (n, 5). */
int ref_generate_anchors(int feature_stride, const float* ratios, int nr, const float* scales, int ns, float* anchors) {
  const float far_corner = feature_stride - 1.0;             /* double arithmetic, then float, as :443-444 */
  const std::vector<float> base = {0.0f, 0.0f, far_corner, far_corner};
  std::vector<float> out;
  ref::GenerateAnchors(base, std::vector<float>(ratios, ratios + nr), std::vector<float>(scales, scales + ns), &out);
  std::memcpy(anchors, out.data(), sizeof(float) * out.size());
  return (int)out.size() / 5;
}

/* MultiProposalGPUOp::Forward, multi_proposal.cu:428-551, restated: the call order and launch geometry of the
 * sliced kernels; thrust::stable_sort_by_key(greater) (:517-521) as std::stable_sort; _nms (:309-357) as its
 * kernel launch plus the host's mask sweep (:338-354).  cudaMalloc / cudaMemcpy become host vectors.
 * Outputs: rois (B*post_n, 5), scores (B*post_n); debug (each may be null): decoded (B, count_anchors, 5) = the
 * workspace after FilterBoxKernel, order (B, pre_n), keep (B, pre_n) filled up to nkeep[b]. */
void ref_multi_proposal(const float* scores_in, const float* bbox_deltas, const float* im_info, int num_images, int num_anchors,
                        int height, int width, int feature_stride, const float* scales, int n_scales, const float* ratios,
                        int n_ratios, int param_pre_nms_top_n, int param_post_nms_top_n, float threshold, int rpn_min_size,
                        float* out, float* out_score, float* decoded, int* order_out, int* keep_out, int* nkeep_out) {
  using namespace ref;
  const int count_anchors = num_anchors * height * width;
  const int count = num_images * count_anchors;
  const int pre_n = std::min(param_pre_nms_top_n > 0 ? param_pre_nms_top_n : count_anchors, count_anchors);   /* :435-437 */
  const int post_n = std::min(param_post_nms_top_n, pre_n);

  std::vector<float> workspace_proposals((size_t)count * 5, 0.f);                               /* :440-458 */
  ref_generate_anchors(feature_stride, ratios, n_ratios, scales, n_scales, workspace_proposals.data());
  float* wp = workspace_proposals.data();

  unsigned grid = (count + kMaxThreadsPerBlock - 1) / kMaxThreadsPerBlock;                      /* :461-486 */
  launch_1d(grid, kMaxThreadsPerBlock, [&] {
    ProposalGridKernel<float>(count, num_anchors, height, width, feature_stride, scores_in, wp);
  });
  launch_1d(grid, kMaxThreadsPerBlock, [&] {
    BBoxPredKernel<float>(count, num_anchors, height, width, feature_stride, im_info, wp, bbox_deltas, wp);
  });
  launch_1d(grid, kMaxThreadsPerBlock, [&] {
    FilterBoxKernel<float>(count, count_anchors, (float)rpn_min_size, im_info, wp);
  });
  if (decoded) std::memcpy(decoded, wp, sizeof(float) * (size_t)count * 5);

  std::vector<float> score(count_anchors);                                                      /* :490-507 */
  std::vector<int> order(count_anchors);
  std::vector<float> ordered((size_t)pre_n * 5);
  std::vector<int> keep(pre_n);
  const int mask_bits = 64;              /* threads per nms_kernel block = bits of one mask word */
  for (int b = 0; b < num_images; ++b) {                                                        /* :509-551 */
    const float* wpb = wp + (size_t)b * count_anchors * 5;
    grid = (count_anchors + kMaxThreadsPerBlock - 1) / kMaxThreadsPerBlock;
    launch_1d(grid, kMaxThreadsPerBlock, [&] { CopyScoreKernel<float>(count_anchors, wpb, score.data(), order.data()); });

    std::stable_sort(order.begin(), order.end(), [&](int i, int j) { return score[i] > score[j]; });   /* :517-521 */

    grid = (pre_n + kMaxThreadsPerBlock - 1) / kMaxThreadsPerBlock;
    launch_1d(grid, kMaxThreadsPerBlock, [&] {
      ReorderProposalsKernel<float>(pre_n, wpb, order.data(), ordered.data());
    });

    /* _nms, :313-354 */
    const int boxes_num = pre_n;
    const int col_blocks = (boxes_num + mask_bits - 1) / mask_bits;
    std::vector<uint64_t> mask_host((size_t)boxes_num * col_blocks, 0);
    launch_blocks(dim3(col_blocks, col_blocks), mask_bits, [&] {
      nms_kernel(boxes_num, threshold, ordered.data(), mask_host.data());
    });
    std::vector<uint64_t> removed(col_blocks, 0);           /* the sweep: a box not yet removed survives and */
    int out_size = 0;                                       /* removes what its mask row names, :338-354 */
    for (int box = 0; box < boxes_num; ++box) {
      const int word = box / mask_bits, bit = box % mask_bits;
      if (removed[word] >> bit & 1) continue;
      keep[out_size++] = box;
      const uint64_t* row = mask_host.data() + (size_t)box * col_blocks;
      for (int w = word; w < col_blocks; ++w) removed[w] |= row[w];
    }

    grid = (post_n + kMaxThreadsPerBlock - 1) / kMaxThreadsPerBlock;                 /* :545-549 */
    launch_1d(grid, kMaxThreadsPerBlock, [&] {
      PrepareOutput<float>(post_n, ordered.data(), keep.data(), out_size, b,
                           out + (size_t)b * post_n * 5, out_score + (size_t)b * post_n);
    });
    if (order_out) std::memcpy(order_out + (size_t)b * pre_n, order.data(), sizeof(int) * pre_n);
    if (keep_out) std::memcpy(keep_out + (size_t)b * pre_n, keep.data(), sizeof(int) * out_size);
    if (nkeep_out) nkeep_out[b] = out_size;
  }
}

}  // extern "C"
