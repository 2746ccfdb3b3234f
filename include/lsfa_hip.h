/*
 * lsfa_hip.h — C ABI of liblsfa_hip.so, the MI355X (gfx950) implementation of
 * LSFA's per-frame inference hot path.
 *
 * Conventions (all entry points):
 *   - plain C ABI: pointers + sizes, no C++/torch types.  Pointers are DEVICE
 *     pointers unless the parameter name ends in `_host`.
 *   - tensors are contiguous fp32 NCHW exactly as the reference operators
 *     receive them from MXNet (psroi_pooling-inl.h:73-76 CheckContiguous).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  No
 *     entry point allocates, frees or synchronises unless documented; scratch
 *     memory comes from the caller (`ws`, sized by lsfa_*_workspace_bytes), so
 *     every launch sequence can be captured in a hipGraph.
 *   - return value: 0 on success, a negative LSFA_E* code for argument errors,
 *     or a positive hipError_t.  Nothing throws.  lsfa_last_error() returns a
 *     thread-local message (the counterpart of MXGetLastError, which is how
 *     the reference's CHECK_xx / LOG(FATAL) reach Python as MXNetError).
 *
 * Each declaration cites the reference interface it replaces
 * (paths relative to the hustvl/LSFA tree).
 */
#ifndef LSFA_HIP_H_
#define LSFA_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSFA_OK 0
#define LSFA_EINVAL (-1)    /* bad argument (the reference's CHECK_EQ / CHECK_GT) */
#define LSFA_EWORKSPACE (-2) /* workspace too small */
#define LSFA_ENOTSUP (-3)   /* shape outside what the kernels support */

const char* lsfa_last_error(void);
/* ABI version of this header; bumped on any signature change. */
int lsfa_abi_version(void);

/* ------------------------------------------------------------------------ *
 * Position-sensitive ROI pooling.
 * Replaces: PSROIPoolingOp<gpu>::Forward   dff_rfcn/operator_cxx/psroi_pooling-inl.h:55-80
 *           PSROIPoolForward / PSROIPoolForwardKernel  psroi_pooling.cu:32-128
 *           params (spatial_scale, output_dim, pooled_size, group_size)  psroi_pooling-inl.h:33-47
 * data  (N, output_dim*group*group, H, W);  rois (R,5) = [batch_idx,x1,y1,x2,y2]
 * out   (R, output_dim, pooled, pooled)
 * mapping_channel (R, output_dim, pooled, pooled) or NULL (the reference's
 *       second, invisible output "maxidx"; written as float like the reference).
 * ------------------------------------------------------------------------ */
int lsfa_psroi_pool_fwd(const float* data, const float* rois,
                        int N, int C, int H, int W, int R,
                        float spatial_scale, int output_dim, int pooled_size, int group_size,
                        float* out, float* mapping_channel, void* stream);

/* Fused R-FCN head tail: PSROI pooling of the class map and of the box map,
 * the global 7x7 average (Pooling global_pool avg) and the class softmax, in
 * one launch, without materialising the (R,dim,7,7) tensors.
 * Replaces: psroipooled_cls_rois / psroipooled_loc_rois / ave_cls_scors_rois /
 *           ave_bbox_pred_rois / cls_prob   dff_rfcn/symbols/resnet_v1_101_flownet_rfcn.py:520-540 (key), :628-648 (cur)
 * cls_map (N, ncls*g*g, H, W), box_map (N, nbox*g*g, H, W), rois (R,5)
 * cls_prob (R, ncls)  softmax over classes;  cls_score (R,ncls) pre-softmax average or NULL
 * bbox_pred (R, nbox)
 * ------------------------------------------------------------------------ */
int lsfa_rfcn_head_fwd(const float* cls_map, const float* box_map, const float* rois,
                       int N, int H, int W, int R, int ncls, int nbox,
                       float spatial_scale, int pooled_size, int group_size,
                       float* cls_prob, float* cls_score, float* bbox_pred, void* stream);

/* The same head on a position-sensitive layout: ps_map (N, H, W, group*group, ncls+nbox), i.e. for
 * every cell and bin the ncls class scores then the nbox box values are contiguous.  That is what
 * rfcn_cls and rfcn_bbox (resnet_v1_101_flownet_rfcn.py:517-518) produce when both 1x1 convolutions
 * run as ONE GEMM [H*W,512] x [512, group^2*(ncls+nbox)] with the weight rows permuted
 * (row (gh*G+gw)*(ncls+nbox)+d  <-  rfcn_cls row (d*G+gh)*G+gw, or rfcn_bbox row ((d-ncls)*G+gh)*G+gw).
 * Results are bit-identical to lsfa_rfcn_head_fwd on the equivalent NCHW maps. */
int lsfa_rfcn_head_ps_fwd(const float* ps_map, const float* rois,
                          int N, int H, int W, int R, int ncls, int nbox,
                          float spatial_scale, int pooled_size, int group_size,
                          float* cls_prob, float* cls_score, float* bbox_pred, void* stream);
/* ... with `cell_ld` floats between consecutive cells of ps_map (>= group*group*(ncls+nbox)): the map as lsfa_conv_split_fwd
 * writes it, its 1911 columns padded to 1920 = 30 x 64 output channels. */
int lsfa_rfcn_head_ps_ld_fwd(const float* ps_map, int cell_ld, const float* rois, int N, int H, int W, int R, int ncls,
                             int nbox, float spatial_scale, int pooled_size, int group_size, float* cls_prob,
                             float* cls_score, float* bbox_pred, void* stream);

/* ------------------------------------------------------------------------ *
 * Motion-vector / flow guided bilinear feature warp with fused epilogue.
 * Replaces: mx.sym.GridGenerator(transform_type='warp') + mx.sym.BilinearSampler
 *           at resnet_v1_101_flownet_rfcn.py:468-469 (key), :571-572 (cur), :678-679 (batch)
 *           `* scale_map` :470 ; res_diff_ada (rnet_conv0 1x1 3->C, +bias) :57-67 and
 *           `conv_feat + res_diff` :576 ; `cur_feat + warp_conv_feat` :236.
 * out[n,c,y,x] = bilerp(feat[n,c], x+flow[n,0,y,x], y+flow[n,1,y,x])   (taps outside the map are 0)
 *                [* mul[n,c,y,x]]                                         if mul  != NULL
 *                [+ (res_w[c,:] . res[n,:,y,x] + res_b[c])]               if res  != NULL (res has res_c channels)
 *                [+ add[n,c,y,x]]                                         if add  != NULL
 * feat may have a smaller batch than flow (feat_n divides N): map n samples feature n mod feat_n.  feat_n = 1 broadcasts the
 * key-frame feature as tile_as does (operator_py/tile_as.py:16-19); feat_n = B < N serves the F frames of a segment of B lock-step
 * clips laid out frame-major (map f*B + b reads clip b's key feature).
 * ------------------------------------------------------------------------ */
int lsfa_warp_bilinear(const float* feat, int feat_n, const float* flow,
                       int N, int C, int H, int W,
                       const float* mul, const float* add,
                       const float* res, int res_c, const float* res_w, const float* res_b,
                       float* out, void* stream);
/* r6: the same operator on CHANNELS-LAST maps - feat_cl (feat_n, H, W, C), add_cl / out_cl (N, H, W, C), C a multiple of 4, 16-byte aligned;
 * flow (N, 2, H, W) and res (N, res_c, H, W) as above; no `mul` (the non-key path's epilogue: + rnet_conv0(res) + add).  Same arithmetic,
 * same bits as lsfa_warp_bilinear on the transposed maps.  amax_out (or NULL): 256 zeroed slots that receive max|out| over channels
 * [amax_c0, C) (a multiple of 4) - the scale of the convolution that reads them: the R-FCN score maps take channels [512, 1024), the RPN head
 * [0, 512) with an exact three-piece cut; both are GEMMs over the channel axis, so with this layout the non-key path needs no
 * lsfa_nchw_to_nhwc in front of them. */
int lsfa_warp_bilinear_cl(const float* feat_cl, int feat_n, const float* flow, int N, int C, int H, int W, const float* add_cl,
                          const float* res, int res_c, const float* res_w, const float* res_b, float* out_cl, unsigned* amax_out,
                          int amax_c0, void* stream);
/* The small net's `bn_before_fuse` (resnet_v1_101_flownet_rfcn.py:231-235 `add`, :243-246 `addv2`): warp_conv_feat_bn on the warped feature
 * before `cur_feat + warp_conv_feat` (:236).  The BatchNorm's shift does not commute with the warp's zero padding, so it is an epilogue step:
 *   r = bilerp(...) [+ rnet_conv0(res)];  r = r * bn_scale[c];  r = r + bn_shift[c];  [r = r + add]        (each step rounded on its own)
 * bn_scale = gamma / sqrt(moving_var + eps), bn_shift = beta - moving_mean * bn_scale (folded on the host).  NCHW (lsfa_warp_bilinear's
 * arguments without `mul`; the gather kernel) and channels-last (lsfa_warp_bilinear_cl's, amax_out included). */
int lsfa_warp_bilinear_bn(const float* feat, int feat_n, const float* flow, int N, int C, int H, int W, const float* add, const float* res,
                          int res_c, const float* res_w, const float* res_b, const float* bn_scale, const float* bn_shift, float* out,
                          void* stream);
int lsfa_warp_bilinear_bn_cl(const float* feat_cl, int feat_n, const float* flow, int N, int C, int H, int W, const float* add_cl,
                             const float* res, int res_c, const float* res_w, const float* res_b, const float* bn_scale, const float* bn_shift,
                             float* out_cl, unsigned* amax_out, int amax_c0, void* stream);
/* Kernel choice (process-wide; results are identical bit for bit): 0 = by shape (default), 1 = the gather kernel only (rounds 1-2),
 * 2 = the LDS-staged kernel (round 3: whole planes copied into LDS by DMA, taps read from LDS) or LSFA_ENOTSUP when the shape or
 * alignment does not allow it (H*W even and <= 4096, 16-byte aligned maps, (C*H*W) % 4 == 0). */
int lsfa_warp_set_variant(int variant);

/* ------------------------------------------------------------------------ *
 * Short-term aggregation, channel attention (small_net_fuse_type `concatv1` / `concatv2`).
 * Replaces: Pooling(global_pool=True, pool_type='avg') "global_pool", s_feat_conv1 (1x1) + relu, s_feat_conv2 (1x1) + sigmoid,
 *           broadcast_mul + add; resnet_v1_101_flownet_rfcn.py:251-259 (concatv1), :261-271 (concatv2).
 * Maps are channels-last (N, HW, C), 16-byte aligned, channel counts multiples of 4.  Deterministic: no float atomics, and an image's
 * result does not depend on the other images of the batch.
 *
 * lsfa_channel_mean: mean[n, c] over the HW pixels of image n of the concatenation [x1 | x2] (channel c < C1 reads x1[.., c], else
 *   x2[.., c - C1]; C2 = 0 / x2 = NULL: x1 alone).  Order: partial[n, k, c] = ((0 + x[16k]) + x[16k + 1]) + ... over the k-th run of 16
 *   pixels, ascending; mean = ((partial[0] + partial[1]) + ... + partial[last]) / HW.  ws: lsfa_channel_mean_workspace_bytes(N, C1 + C2, HW).
 * lsfa_channel_gate: gate[n, o] = sigmoid(w2[o, :] . relu(w1[:, :] . m[n, :] + b1) + b2[o]) for N images; w1 (M, K), w2 (O, M) fp32 row-major,
 *   hidden (N, M) scratch.  Each dot product: lane l of a wave accumulates elements 4(l + 64j) .. +3, j ascending, with fmaf from 0, then the
 *   64 lane sums meet in a butterfly (distance 32, 16, .., 1), then + bias; sigmoid(v) = 1 / (1 + exp(-v)), exp correctly rounded.  A weight
 *   row is read once per 8 images.  (No matrix instructions: a GEMV.)
 * lsfa_gate_apply: out = x * gate[n, c] + y (two roundings); `concatv1` passes x = y.  amax_out (or NULL): 256 zeroed slots that receive
 *   max|out| over channels [amax_c0, C) (the R-FCN convolution's scale, as lsfa_warp_bilinear_cl leaves it).
 * ------------------------------------------------------------------------ */
size_t lsfa_channel_mean_workspace_bytes(int N, int C, int HW);
int lsfa_channel_mean(const float* x1, int C1, const float* x2, int C2, int N, int HW, float* mean, void* ws, size_t ws_bytes, void* stream);
int lsfa_channel_gate(const float* m, int N, int K, const float* w1, const float* b1, int M, const float* w2, const float* b2, int O,
                      float* hidden, float* gate, void* stream);
int lsfa_gate_apply(const float* x, const float* gate, const float* y, int N, int HW, int C, float* out, unsigned* amax_out, int amax_c0,
                    void* stream);

/* ------------------------------------------------------------------------ *
 * Long-term aggregation combine (Nq_net tail).
 * Replaces: softmax(axis=0) + SliceChannel + tile x2 + mul x2 + add
 *           resnet_v1_101_flownet_rfcn.py:104-108
 * logits (2,1,H,W): index 0 weights `a` (warped old key feature), 1 weights `b`.
 * out = w0*a + w1*b,  (w0,w1) = softmax(logits[:, 0, y, x]).
 * ------------------------------------------------------------------------ */
int lsfa_aggregate_softmax2(const float* a, const float* b, const float* logits,
                            int C, int H, int W, float* out, void* stream);

/* N maps per launch: a, b, out (N, C, H, W); logits (2, N, H, W) = the Nq convolutions' output for
 * Concat(warp x N, cur x N) on the batch axis (:95), row n weighting a[n], row N+n weighting b[n].
 * N = 1 is lsfa_aggregate_softmax2.  Used when several clips advance together (BASELINE configs[2]) and for
 * the HBM-resident roofline measurement (configs[4]). */
int lsfa_aggregate_softmax2_batched(const float* a, const float* b, const float* logits,
                                    int N, int C, int H, int W, float* out, void* stream);
/* r5: the same with the 2N logit rows `logit_row_stride` floats apart (>= H*W): channel 0 of the Nq net's last convolution
 * written NCHW with its output channels padded to 64 is read in place (row stride 64*H*W) instead of through a strided copy */
int lsfa_aggregate_softmax2_rows(const float* a, const float* b, const float* logits, long logit_row_stride,
                                 int N, int C, int H, int W, float* out, void* stream);

/* Fgfa variant: weights from cosine similarity of 2 embeddings
 * Replaces: compute_weight + softmax + tile/mul/add  resnet_v1_101_flownet_rfcn.py:111-116, :136-147
 * emb_cur, emb_warp (1,E,H,W); a = warped feature, b = current feature (1,C,H,W).
 * w_a = <norm(emb_warp), norm(emb_cur)>, w_b = <norm(emb_cur), norm(emb_cur)>, softmax over the two. */
int lsfa_aggregate_cosine(const float* a, const float* b, const float* emb_warp, const float* emb_cur,
                          int C, int E, int H, int W, float* out, void* stream);

/* ------------------------------------------------------------------------ *
 * RPN proposal generation (anchors -> decode -> clip -> filter -> stable sort
 * -> top pre_n -> NMS -> first post_n, cyclic pad).
 * Replaces: MultiProposalGPUOp::Forward  dff_rfcn/operator_cxx/multi_proposal.cu:403-558
 *           (+ kernels :47-388, anchors multi_proposal-inl.h:256-295, params :124-159);
 *           this is also the in-repo specification of mx.contrib.sym.Proposal as called at
 *           resnet_v1_101_flownet_rfcn.py:501, :609.
 * cls_prob (B, 2A, H, W), bbox_pred (B, 4A, H, W), im_info (B,3) = [im_h, im_w, im_scale]
 * rois (B*post_n, 5), scores (B*post_n, 1) or NULL.
 * `ws` must hold lsfa_proposal_workspace_bytes(...) bytes.
 * ------------------------------------------------------------------------ */
size_t lsfa_proposal_workspace_bytes(int B, int A, int H, int W, int pre_nms_top_n);
/* Launch plan (process-wide; results are identical bit for bit).  AUTO picks the chip-wide plan (six short kernels spread over the CUs)
 * for count <= 32768 anchors and pre_nms_top_n <= 8192, else the single-workgroup plan (one 16-wave workgroup per image, everything in
 * its CU's LDS).  Inside the chip-wide plan AUTO builds the full suppression mask for ONE image (lowest latency: 18 + 12 us against the
 * box sweep's 160) and takes the mask-free box sweep for B >= 2, a batched pass of the frame pipeline: one workgroup per image instead
 * of every CU, +2.2 ... +4.2 % frames/s (profiles/r6/proposal_plan_ab.txt, proposal_plan_ab2.txt).  The workspace size is the same. */
enum { LSFA_PROPOSAL_PLAN_AUTO = 0, LSFA_PROPOSAL_PLAN_SINGLE_WORKGROUP = 1, LSFA_PROPOSAL_PLAN_CHIP_WIDE = 2 /* full mask for any B */,
       /* the chip-wide plan with the mask-free NMS stage for any B: what AUTO takes for B >= 2.  Only the diagonal tiles of the suppression
        * mask are built and one 16-wave workgroup per image decides everything across blocks from the survivors' boxes in LDS.  No
        * dependent trips to L2, but 64 x (survivors so far) IoU tests per block on ONE CU's four SIMDs: slower alone, cheaper for the
        * pipeline, whose other streams keep the rest of the chip */
       LSFA_PROPOSAL_PLAN_CHIP_WIDE_BOX_SWEEP = 3,
       /* r6, ABLATION ONLY (tools/lab/tail_ablation.sh, LSFA_LAB_SKIP_TAIL=1): the chip-wide plan WITHOUT its suppression stage - rois and
        * scores are not written.  What the NMS launches cost the frame pipeline is the difference to a normal run; never a product setting. */
       LSFA_PROPOSAL_PLAN_LAB_NO_NMS = 99 };
int lsfa_proposal_set_plan(int plan);
int lsfa_proposal(const float* cls_prob, const float* bbox_pred, const float* im_info,
                  int B, int A, int H, int W, int feature_stride,
                  const float* scales_host, int n_scales, const float* ratios_host, int n_ratios,
                  int rpn_pre_nms_top_n, int rpn_post_nms_top_n, float threshold, int rpn_min_size,
                  float* rois, float* scores, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------ *
 * NMS on score-sorted boxes, device resident.
 * Replaces: nms_kernel + the host sweep of _nms   lib/nms/nms_kernel.cu:40-84, :97-150
 *           and multi_proposal.cu:262-357.
 * boxes (n, box_dim>=4) sorted by score descending; keep (n) int32 indices into
 * boxes, num_keep (1) int32; both device.  keep[num_keep:] is not written (undefined).  ws >= lsfa_nms_workspace_bytes(n).
 * ------------------------------------------------------------------------ */
size_t lsfa_nms_workspace_bytes(int n);
int lsfa_nms_sorted(const float* boxes, int n, int box_dim, float thresh,
                    int* keep, int* num_keep, void* ws, size_t ws_bytes, void* stream);

/* The same sweep on float64 boxes with numpy's arithmetic and keep rule (`ovr <= thresh` survives).
 * Replaces: the loop of nms()   lib/nms/nms.py:47-72   after its `scores.argsort()[::-1]` (:45), which the
 * caller does (the host side mirrors the reference: lsfa_amd/nms/nms.py).  pred_eval's per-class NMS runs on
 * float64 dets (dff_rfcn/core/tester.py:270-271); this is that path for callers of py_nms_wrapper. */
int lsfa_nms_sorted_f64(const double* boxes, int n, int box_dim, double thresh,
                        int* keep, int* num_keep, void* ws, size_t ws_bytes, void* stream);

/* The reference's exact host-pointer entry point (lib/nms/gpu_nms.hpp:14-15):
 * boxes_host (boxes_num, boxes_dim) already sorted by score; keep_out has room
 * for boxes_num ints.  Allocates, copies and synchronises like the original. */
void _nms(int* keep_out, int* num_out, const float* boxes_host, int boxes_num,
          int boxes_dim, float nms_overlap_thresh, int device_id);

/* ------------------------------------------------------------------------ *
 * Per-frame detection post-processing, all classes in one launch.
 * Replaces: bbox_pred (nonlinear_pred) lib/bbox/bbox_transform.py:103-140, clip_boxes :45-60,
 *           `/ scale` dff_rfcn/core/tester.py:148-152, and the per-class threshold + NMS +
 *           max_per_image loop tester.py:265-281 (py_nms_wrapper -> lib/nms/nms.py:37-74).
 * rois (R,5) [batch,x1,y1,x2,y2]; deltas (R, 4*nreg); probs (R, ncls).
 * class_agnostic != 0: every class uses delta columns 4:8 (tester.py:269).
 * Arithmetic is float64 like the numpy reference (nonlinear_pred upcasts, :114).
 * Outputs: dets (ncls, R, 5) float64 rows [x1,y1,x2,y2,score] for the survivors of
 * class j in NMS (score-descending) order, counts (ncls) int32 (class 0 = background: count 0),
 * keep_idx (ncls, R) int32 = roi index of each survivor (may be NULL).
 * max_per_image <= 0 disables the cap.
 * ------------------------------------------------------------------------ */
size_t lsfa_det_workspace_bytes(int R, int ncls);
int lsfa_det_postprocess(const float* rois, const float* deltas, const float* probs,
                         int R, int ncls, int nreg, int class_agnostic,
                         double im_h, double im_w, double scale,
                         double score_thresh, double nms_thresh, int max_per_image,
                         double* dets, int* counts, int* keep_idx,
                         void* ws, size_t ws_bytes, void* stream);

/* The same for the B images of a batch in one launch pair (the non-key frames of a segment, the clips of a lock-step batch): image b's rois /
 * deltas / probs are rows [b*R, (b+1)*R) (MultiProposal's layout, multi_proposal.cu:560-575), its outputs dets[b] (ncls, R, 5), counts[b] (ncls),
 * keep_idx[b] (ncls, R); one image size and scale for all (frames of one clip). */
int lsfa_det_postprocess_batch(const float* rois, const float* deltas, const float* probs,
                               int B, int R, int ncls, int nreg, int class_agnostic,
                               double im_h, double im_w, double scale,
                               double score_thresh, double nms_thresh, int max_per_image,
                               double* dets, int* counts, int* keep_idx,
                               void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------ *
 * RPN head.  rpn_cls_score + rpn_bbox_pred (1x1 convolutions of channels [0, 512) of the NCHW feature, both as ONE convolution: lsfa_conv_fwd
 * with x_nchw = 1, output channel o < 2A = score channel o, 2A <= o < 6A = box delta o - 2A, padded to 64) leave `logits` (N, H*W, ld)
 * channels-last; lsfa_rpn_softmax_split applies the per-anchor two-way softmax (Reshape (2, A*H, W) -> SoftmaxActivation(channel) ->
 * Reshape) and splits them into the NCHW maps MultiProposal takes.
 * Replaces: dff_rfcn/symbols/resnet_v1_101_flownet_rfcn.py:479-494 (and the rpn_inv_normalize the caller folds into the weights).
 * cls_prob (N, 2A, H, W): channel a = background, A + a = foreground of anchor a; bbox_pred (N, 4A, H, W).
 * ------------------------------------------------------------------------ */
int lsfa_rpn_softmax_split(const float* logits, int N, int H, int W, int ld, int A, float* cls_prob, float* bbox_pred, void* stream);

/* Box decode + clip + rescale only (float64 out), for callers that keep the
 * reference's im_detect() signature:  tester.py:143-152. pred_boxes (R, 4*nreg) */
int lsfa_bbox_pred_clip(const float* rois, const float* deltas, int R, int nreg,
                        double im_h, double im_w, double scale, double* pred_boxes, void* stream);

/* ------------------------------------------------------------------------ *
 * Deformable convolution support: bilinear im2col of the DCN units
 * (mx.contrib.symbol.DeformableConvolution, dff_rfcn/symbols/sym_common.py:138-157).
 * data (N,C,H,W), offset (N, 2*kh*kw*dg, Ho, Wo) -> col (N, C*kh*kw, Ho*Wo);
 * the GEMM with the (Cout, C*kh*kw) weight is the caller's (MFMA library GEMM).
 * ------------------------------------------------------------------------ */
int lsfa_deform_im2col(const float* data, const float* offset,
                       int N, int C, int H, int W, int kh, int kw,
                       int pad, int stride, int dilate, int deform_groups,
                       int Ho, int Wo, float* col, void* stream);

/* The same sampling for channels-last tensors: data (N,H,W,C), offset (N,Ho,Wo,2*kh*kw*dg),
 * col (N, Ho*Wo, kh*kw, C) — a row of col is one output pixel, ordered (tap, channel), so the
 * contraction is rows x (kh*kw*C, Cout).  C/deform_groups must be a multiple of 4. */
int lsfa_deform_im2col_cl(const float* data, const float* offset,
                          int N, int C, int H, int W, int kh, int kw,
                          int pad, int stride, int dilate, int deform_groups,
                          int Ho, int Wo, float* col, void* stream);
/* ... with the offsets of a pixel offset_ld floats apart (>= 2*kh*kw*dg): the offset branch of a DCN unit
 * (sym_common.py:249-257, 72 channels) computed by lsfa_conv_split_fwd with its output channels padded to 128. */
int lsfa_deform_im2col_cl_ld(const float* data, const float* offset, int offset_ld,
                             int N, int C, int H, int W, int kh, int kw,
                             int pad, int stride, int dilate, int deform_groups,
                             int Ho, int Wo, float* col, void* stream);

/* ------------------------------------------------------------------------ *
 * Convolution + bias + ReLU on channels-last maps with the fp32 matrix cores (implicit GEMM).
 * Replaces: mx.sym.Convolution (no_bias) + the BatchNorm folded into it + Activation('relu') of the
 *           pre-activation ResNet units' conv2   dff_rfcn/symbols/resnet.py:84-93, sym_common.py:92-135
 *           (any kh x kw, stride, dilation; zero padding `pad` on every side).
 * x (N, H, W, Cin), y (N, Ho, Wo, Cout) channels-last; w (Cout, kh*kw, Cin): K contiguous per output channel
 * (the reference's (Cout, Cin, kh, kw) weight permuted once at bind time); bias (Cout) or NULL.
 * Cin % 32 == 0, Cout % 64 == 0.  Small tile grids split the taps over workgroups and need
 * lsfa_conv_nhwc_workspace_bytes(...) of workspace (partial tiles, added in a fixed order: deterministic).
 * ------------------------------------------------------------------------ */
size_t lsfa_conv_nhwc_workspace_bytes(int N, int H, int W, int Cout, int kh, int kw, int stride, int pad, int dil);
int lsfa_conv_nhwc_fwd(const float* x, int N, int H, int W, int Cin, const float* w, const float* bias, int Cout,
                       int kh, int kw, int stride, int pad, int dil, int relu, float* y,
                       void* ws, size_t ws_bytes, void* stream);

/* The same convolution with the tail of a pre-activation unit fused in (resnet.py:93-101 + the next unit's :78-80):
 * y = conv(x) [+ bias] + residual (residual may be y itself: in place), and, when y2 != NULL, the NEXT unit's
 * BatchNorm + ReLU of that sum as a second output, y2 = max(y*scale2[c] + shift2[c], 0) — so conv3 + the shortcut add
 * + bn1/relu1 of the following unit are one launch. */
int lsfa_conv_nhwc_fused_fwd(const float* x, int N, int H, int W, int Cin, const float* w, const float* bias, int Cout,
                             int kh, int kw, int stride, int pad, int dil, int relu, const float* residual, float* y,
                             float* y2, const float* scale2, const float* shift2,
                             void* ws, size_t ws_bytes, void* stream);

/* The convolutions of the frame path (and, with kh = kw = 1, the 1x1 convolutions = plain GEMMs of the channels-last units):
 * fp32 in, fp32 accumulate, fp32 out, with every fp32 product formed on the bf16 / fp16 matrix pipe from `pieces` pieces per operand
 * (gfx950 has no xf32 MFMA and its fp32 MFMA runs at 1/16 of the bf16 / fp16 rate):
 *   pieces = 3  three bf16 pieces (8 + 8 + 8 mantissa bits, an exact cut) and the six partial products of weight >= 2^-16;
 *   pieces = 2  two fp16 pieces of x * s and w * 2^w_exp (hi = fp16(v), lo = fp16(v - hi)) and the three products hi hi + hi lo + lo hi:
 *               half the matrix-pipe cycles of the six-product form and at least as close to a float64 convolution (tests/test_hip_ops.py).
 *               fp16's exponent range makes it need the map's scale: `amax_in` = 256 floats whose maximum is >= max|x| (lsfa_amax_partial
 *               of x, a producing convolution's `amax_out`, or of a map that bounds x); s is the power of two that puts that maximum
 *               into [2^13, 2^14).  An UNDER-estimate makes fp16(x s) overflow: the output turns non-finite and bit 0 of *status is
 *               raised - lsfa_status_check() turns it into an error instead of a silently wrong feature map.
 *               The exponent rule, for maps and weights alike: e = 13 - floor(log2 max), clamped at 100 (weights: +-100), so that 2^e and
 *               2^-e are finite normal floats.  A map whose maximum is below 2^-87 is scaled by 2^100 and sits lower in fp16's range: the
 *               result stays finite with a clear status word, each activation carrying an absolute error of up to 2^-125 (fp16's
 *               subnormal spacing under that scale) next to the usual relative one.  A zero or subnormal maximum takes e = 13: every
 *               piece is zero and the output is the bias.  A weight (channel) whose maximum is 2^114 or more is refused where the weights
 *               are bound (hip.SplitWeight).  The accumulator columns are multiplied back by the single float 2^-(e_map + e_weight): from
 *               e_map + e_weight = 150 on that float is zero and the channel's output is the bias (tests/test_conv_scale_range_gpu.py).
 *   pieces = 1  one bf16 piece (round to nearest even), one product: the bf16 mode (BASELINE configs[2]).
 * Replaces mx.sym.Convolution (+ the BatchNorm / ReLU / residual add around it) of dff_rfcn/symbols/resnet.py:70-101,
 * sym_common.py:92-135, resnet_v1_101_flownet_rfcn.py:44-55 (feat_conv_3x3), :150-207 (FlowNet), :94-109 (Nq), :209-236 (small net),
 * :479-546 (RPN / R-FCN score maps).
 * Weights are cut and laid out once at bind time: lsfa_conv_weights writes lsfa_conv_weight_bytes(...) bytes (2 * pieces per weight, in
 * MFMA fragment order) from w (Cout, kh, kw, Cin); Cin % 32 == 0, Cout % 64 == 0; w_exp (pieces == 2 only) = 13 - floor(log2 max|w|).
 * Operands may be VIEWS of wider channels-last maps (FlowNet's Concat / Crop / Deconvolution nodes then need no copies):
 *   x   (N, H, W, lda) with the Cin input channels first in each pixel's row (lda = 0: Cin; a multiple of 4);
 *   y   points at the first output element; ldy floats between output pixels (0: Cout); out_H > 0 places output pixel (oy, ox) of
 *       image n at y + (((n*out_H + oy*out_sy)*out_W + ox*out_sx) * ldy) - a channel slice of a concatenated map, or every other pixel
 *       of it (one parity of a stride-2 transposed convolution); Ho, Wo > 0: the output grid of this launch when it is not the
 *       convolution's own;
 *   y_nchw != 0: y, y2 and residual are (N, Cout, Ho, Wo) - the layout the reference's operators take - instead of channels-last.
 * Epilogue: + bias[c], + residual (may alias y), act (0 none, 1 ReLU, 2 LeakyReLU 0.1), and optionally a second output
 * y2 = max(y * scale2[c] + shift2[c], 0) - the NEXT pre-activation unit's bn1 + relu1 (resnet.py:77-79) - and `amax_out`: 256 unsigned
 * slots that receive (atomicMax on the bit pattern; the caller zeroes them once per frame) max|y2| if scale2 / shift2 are given (with
 * y2 == NULL that maximum is all the second output leaves behind), else max|y|.
 * K may be cut into slices whose partial sums go through `ws` and are added in a fixed order (bit-reproducible). */
typedef struct lsfa_conv_desc {
  const float* x; int lda; int N, H, W, Cin;
  const void* wfrag; int pieces; int w_exp; const float* amax_in;
  const float* bias; int Cout, kh, kw, stride, pad_h, pad_w, dil;
  int act; int y_nchw; const float* residual; float* y; int ldy;
  float* y2; const float* scale2; const float* shift2;
  unsigned* amax_out; unsigned* status;
  int Ho, Wo, out_H, out_W, out_sy, out_sx;
  int prof_tag;          /* lsfa_prof_*: r5: ignored - every call of the family is timed as "conv" (FLOPs and time over the same calls) */
  int x_nchw;            /* != 0: x is an NCHW map (N, lda, H, W) whose channels [0, Cin) are the input (K-major for the contraction): 1x1 /
                          * stride 1 / no padding and small weights only (Cout * Cin * 2 * pieces <= 256 KB per 64 output channels) -
                          * the RPN's 1x1 convolutions on the feature map the reference's operators exchange; else LSFA_ENOTSUP */
  const float* in_scale; /* with in_shift (Cin floats each, or both NULL): the convolution's input is max(x * in_scale[k] + in_shift[k], 0), */
  const float* in_shift; /* k the input channel, applied where the operand is cut - a pre-activation ResNet unit's bn1 + relu1
                          * (dff_rfcn/symbols/resnet.py:78-80) on the previous unit's sum without that map ever being stored: the
                          * previous conv3 is given scale2 / shift2 but y2 = NULL and only publishes the activated map's maximum in its
                          * amax_out, which is this call's amax_in.  1x1, no padding, Cin <= 2048, pieces 1 or 2; else LSFA_ENOTSUP.  The
                          * values multiplied are bit for bit the ones y2 would have held. */
  const float* w_scale;  /* r5, pieces == 2: Cout floats 2^-w_exp[co] for weights cut by lsfa_conv_weights_pc (one power-of-two scale per
                          * OUTPUT channel: a BatchNorm folded into trained weights spreads the channels' magnitudes over many octaves, and
                          * every channel keeps its 22 bits); NULL: one scale 2^w_exp for the whole tensor (lsfa_conv_weights) */
} lsfa_conv_desc;
size_t lsfa_conv_weight_bytes(int Cout, int kh, int kw, int Cin, int pieces);
int lsfa_conv_weights(const float* w, int Cout, int kh, int kw, int Cin, int pieces, int w_exp, void* wfrag, void* stream);
/* r5: the two-piece cut with w_exp_pc[co] (device, Cout ints) per output channel; pass 2^-w_exp_pc[co] as lsfa_conv_desc::w_scale */
int lsfa_conv_weights_pc(const float* w, int Cout, int kh, int kw, int Cin, const int* w_exp_pc, void* wfrag, void* stream);
size_t lsfa_conv_workspace_bytes(const lsfa_conv_desc* d);
int lsfa_conv_fwd(const lsfa_conv_desc* d, void* ws, size_t ws_bytes, void* stream);
/* r8: a pre-activation unit's conv3 + shortcut add and the NEXT unit's conv1 in one launch (dff_rfcn/symbols/resnet.py:70-101: conv3 :93-95,
 * `sum = conv3 + shortcut` :101, then the next unit's bn1 :78, relu1 :79, conv1 :80 with bn2 folded in and relu2 :82), for the stages whose sum
 * is too large to stay in cache between two launches: it is written once and not read back.
 *   x (N,H,W,Cm) channels-last = c2, amax_in its 256 maxima;  y (N,H,W,C) = conv3(x) + residual (residual may BE y), C = 4 Cm;
 *   z (N,H,W,Cn) = max(conv1(max(y * scale2[c] + shift2[c], 0)) + bias, 0)   (scale2 / shift2: C floats, bias: Cn floats or NULL).
 * w3frag / w1frag: lsfa_conv_weights_pc fragments of the (C,1,1,Cm) and (Cn,1,1,C) weights, w3_scale / w1_scale their 2^-w_exp[co].
 * conv3's arithmetic is lsfa_conv_fwd's (same products, same order: y is bit-identical to the two-launch form).  conv1's operand is cut
 * with one power-of-two scale per 32-pixel x 128-channel block of the activated sum (the block's own maximum into [2^13, 2^14)) instead of
 * one per map, and accumulated per block.  amax_out_sum: 256 slots that receive the maximum of the activated sum (what a strided shortcut
 * that reads y through in_scale / in_shift needs as its amax_in); amax_out_z: those of z.  Either may be NULL.
 * LSFA_ENOTSUP for: pieces3 / pieces1 other than 2 (two fp16 pieces), C != 4 Cm, Cm or Cn outside {64, 128}, views (ldx != Cm, ldy != C,
 * ldz != Cn), y_nchw != 0, stride != 1.  No workspace, no allocation, no synchronisation. */
int lsfa_conv_pair_fwd(const float* x, int ldx, int N, int H, int W, int Cm, const float* amax_in, const void* w3frag,
                       const float* w3_scale, int pieces3, int C, const float* residual, float* y, int ldy, const float* scale2,
                       const float* shift2, const void* w1frag, const float* w1_scale, int pieces1, int Cn, const float* bias,
                       float* z, int ldz, int stride, int y_nchw, unsigned* amax_out_sum, unsigned* amax_out_z, unsigned* status,
                       void* stream);
/* 256 partial maxima of |x| (n floats, n % 4 == 0, 16-byte aligned): an `amax_in` for maps no convolution of this library produced */
int lsfa_amax_partial(const float* x, long long n, float* out256, void* stream);
/* Reads and clears the status word the convolutions raise (synchronises `stream`): LSFA_OK, or LSFA_EOVERFLOW with lsfa_last_error()
 * saying which bit was set.  The frame loop calls it where it synchronises anyway (end of a video, after a benchmark region). */
#define LSFA_EOVERFLOW (-4)
int lsfa_status_check(unsigned* status_dev, void* stream);
/* measurement hook (tools/lab/conv_ring_lab.py): force the kernel (1: the ring kernel, mixed-role waves; 2: the ring kernel with
 * loader / consumer waves; never the direct form then; 3 was the 3x3 halo form, removed in r6: refused), the tile width nt (2 | 4), the
 * ring depth st (2..4) and the number of K slices; 0 = the launch plan decides.  Process-wide; results stay bit-reproducible per setting. */
int lsfa_conv_plan_override(int kernel, int nt, int st, int slices);
/* r6, measurement / test hook: the two orders the ring kernel's launch can be laid out in, process-wide like the override above; -1 = back to
 * the default (or the LSFA_CONV_TILE_ORDER / LSFA_CONV_K_ORDER environment variables).  tile_order: 0 = workgroups numbered with the pixel tile
 * fastest, 1 = the channel tile fastest (all channel tiles of a pixel tile on one XCD); results do not depend on it.  k_order: 0 = K walked tap by
 * tap (a tap's channel chunks, then the next tap), 1 = channel chunk by channel chunk (a chunk's taps, then the next chunk: a tap's rows are the
 * previous tap's rows shifted, served from the CU's L1); the summation order differs between the two, within a setting every plan agrees. */
int lsfa_conv_order_override(int tile_order, int k_order);
/* r5: 4 = the ring kernel on 256-pixel tiles (eight mixed-role waves; nt 4, pieces 1 | 2).
 * measurement hook (bench.py's per-instantiation roofline table): which kernel lsfa_conv_fwd would launch for `d` -
 * out[0] kernel (1 ring, 2 direct), out[1] nt, out[2] st, out[3] loader / consumer waves, out[4] waves that multiply (4 | 8),
 * out[5] K slices, out[6] the input's activation applied at the cut, out[7] pieces.  Launches nothing. */
int lsfa_conv_plan_query(const lsfa_conv_desc* d, int* out8);
/* Deconvolution(kernel 4, stride 2) + Crop(offset (1,1)) to Hc x Wc (+ bias + activation) as ONE launch of four 2x2-tap phase
 * convolutions (resnet_v1_101_flownet_rfcn.py:170-176 `deconv5` ... `deconv2`): x (N, Hi, Wi, lda) with Cin channels used,
 * wfrag4 = four consecutive blocks of lsfa_conv_weight_bytes(Cout, 2, 2, Cin, pieces) bytes, block py*2 + px =
 * lsfa_conv_weights of the (Cout, 2, 2, Cin) weight w[:, :, kys, kxs] transposed to (out, in, ky, kx), kys = (3, 1) for py = 0
 * and (2, 0) for py = 1 (kxs alike); y points at channel c0 of pixel (0, 0) of the (N, Hc, Wc, ldy) map. */
size_t lsfa_deconv4x4s2_crop_workspace_bytes(int N, int Hi, int Wi, int Cin, int Cout, int Hc, int Wc, int pieces);
int lsfa_deconv4x4s2_crop_fwd(const float* x, int lda, int N, int Hi, int Wi, int Cin, const void* wfrag4, int pieces, int w_exp,
                              const float* amax_in, const float* bias, int Cout, int act, float* y, int ldy, int Hc, int Wc,
                              unsigned* amax_out, unsigned* status, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * The stem of the ResNets and the frame shrink in front of the small net, three launches instead of six library ones.
 *   lsfa_avgpool_nchw      mx.symbol.Pooling(kernel=(k,k), stride=(k,k), pool_type='avg', pooling_convention='full')
 *                          (dff_rfcn/symbols/resnet_v1_101_flownet_rfcn.py:216 `resize_data`, k = 4): x (N,C,H,W) -> y (N,C,ceil(H/k),
 *                          ceil(W/k)); edge windows are clipped to the image and averaged over what they hold.
 *   lsfa_stem_weights      conv0's weight as w_l (3,7,7,64) floats = [ci][ky][kx][co] with bn0's scale folded in -> wfrag, the
 *                          lsfa_stem_weight_bytes() (16-byte aligned) bytes lsfa_stem_conv7x7s2 reads: the matrix-instruction
 *                          fragments of the weights as two fp16 pieces with a power-of-two scale per output channel.  Once per
 *                          weight load.
 *   lsfa_stem_conv7x7s2    bn_data + conv0 + bn0 + relu0 (dff_rfcn/symbols/resnet.py:151, :162): x (N,3,H,W) NCHW; in_scale/in_shift (3)
 *                          = bn_data as a per-channel affine (NULL: none), applied before the zero padding; wfrag from
 *                          lsfa_stem_weights; bias (64) = bn0's shift; y (N,Ho,Wo,64) channels-last, Ho = (H-1)/2+1.  fp32 operands
 *                          as two fp16 pieces on the matrix pipe (three products, fp32 accumulation: fp32 accuracy, like
 *                          lsfa_conv_fwd's pieces = 2); the input's scale is taken per 4 x 32 output tile from the tile's own
 *                          patch, so an image's result does not depend on what else is in the batch.
 *   lsfa_maxpool3x3s2_nhwc pool0 (resnet.py:163: 3x3, stride 2, pad 1, max): x (N,H,W,C) -> y (N,(H-1)/2+1,(W-1)/2+1,C), C % 4 == 0;
 *                          y2 != NULL: also max(y*scale2[c] + shift2[c], 0), the first unit's bn1 + relu1 (resnet.py:78-80).
 *                          amax_out != NULL: 256 slots (zeroed by the caller) that receive max|y2| (max|y| without y2) the way
 *                          lsfa_conv_fwd's amax_out does, for the next convolution's amax_in.
 * ------------------------------------------------------------------------ */
int lsfa_avgpool_nchw(const float* x, int N, int C, int H, int W, int k, float* y, void* stream);
/* r6: the same with the N images given by a DEVICE table of N base pointers (image n = C x H x W floats at x_table[n]): frames that arrive as
 * separate tensors (dff_rfcn/core/loader.py:131-141 hands one array per frame) go through a batched pass without a staging copy into one
 * (N, C, H, W) buffer.  The table's address is what a captured graph bakes in; lsfa_ptr_table_set rewrites its entries before a replay. */
int lsfa_avgpool_nchw_tbl(const float* const* x_table, int N, int C, int H, int W, int k, float* y, void* stream);
/* r5: transform (lib/utils/image.py:296-308), the last host-side step of a frame moved behind its upload: decoded frames
 * (N, H, W, 3) uint8 BGR on the device -> `data` (N, 3, H, W) float32, channel i = (im[..., 2 - i] - pixel_means[2 - i]) * pixel_scale.
 * computed in float64 like the reference's numpy statements and rounded to float32 once.
 * pixel_means_bgr_host: three doubles in host memory, B, G, R order (config.network.PIXEL_MEANS); H*W % 4 == 0. */
int lsfa_image_transform_u8(const unsigned char* im_hwc_bgr, int N, int H, int W, const double* pixel_means_bgr_host, double pixel_scale,
                            float* data_nchw, void* stream);
size_t lsfa_stem_weight_bytes(void);
int lsfa_stem_weights(const float* w_l, void* wfrag, void* stream);
int lsfa_stem_conv7x7s2(const float* x, int N, int H, int W, const float* in_scale, const float* in_shift,
                        const void* wfrag, const float* bias, float* y, void* stream);
int lsfa_maxpool3x3s2_nhwc(const float* x, int N, int H, int W, int C, float* y, float* y2, const float* scale2,
                           const float* shift2, unsigned* amax_out, void* stream);
/* lsfa_stem_conv7x7s2 with an accumulation input and a choice of activation: y = act(conv(x) + bias + accum), accum (N,Ho,Wo,64)
 * or NULL (may be y itself), act 0 none / 1 ReLU / 2 LeakyReLU(0.1).  FlowNet's flow_conv1 (7x7 / 2, 6 -> 64 channels,
 * resnet_v1_101_flownet_rfcn.py:153) is two such passes, one per image of the pair, with the weight's input channels 0-2 / 3-5.
 * amax_out (or NULL): 256 zeroed slots that receive max|y|, like lsfa_conv_fwd's. */
int lsfa_stem_conv7x7s2_ex(const float* x, int N, int H, int W, const float* in_scale, const float* in_shift,
                           const void* wfrag, const float* bias, const float* accum, int act, float* y, unsigned* amax_out,
                           void* stream);
/* r6: lsfa_stem_conv7x7s2_ex with the N images given by a device table of base pointers (3 x H x W floats each): see lsfa_avgpool_nchw_tbl. */
int lsfa_stem_conv7x7s2_tbl(const float* const* x_table, int N, int H, int W, const float* in_scale, const float* in_shift,
                            const void* wfrag, const float* bias, const float* accum, int act, float* y, unsigned* amax_out, void* stream);

/* ---------------------------------------------------------------------------
 * FlowNet-S pieces that are not MFMA-sized (lsfa_amd/csrc/flownet.hip); with lsfa_conv_split_view_fwd and the two-pass stem
 * convolution they make get_flownet (resnet_v1_101_flownet_rfcn.py:150-207) free of library calls.
 *   lsfa_head_conv3x3    Convolution1..5 (:178-203): 3x3, pad 1, stride 1, Cin -> Cout <= 4 channels.  x (N,H,W,lda) channels-last
 *                        (the first Cin channels of each pixel), w (Cout,3,3,Cin), y = (conv + bias) * mul either NCHW
 *                        (N,Cout,H,W) (out_nchw != 0: the `flow` output, mul = 2.5, :204) or channels [c0, c0+Cout) of (N,H,W,ldy).
 *   lsfa_upsample_flow   upsample_flow*to* (:180, :185, :190, :195): Deconvolution(kernel 4, stride 2, C -> C, C <= 8) + Crop(offset 1)
 *                        to Hc x Wc; in (N,Hi,Wi,C), w (C,C,4,4) (MXNet's (in, out, kh, kw)), out channels [c0, c0+C) of (N,Hc,Wc,ldy);
 *                        amax_out (or NULL): the 256 slots of the destination map that receive max|result| (see lsfa_conv_fwd).
 *   lsfa_avgpool2_nhwc   Pooling(kernel 2, stride 2, avg, 'full') on (N,H,W,C), C % 4 == 0 -> (N,ceil(H/2),ceil(W/2),C), edge
 *                        windows clipped (:201).
 * ------------------------------------------------------------------------ */
int lsfa_head_conv3x3(const float* x, int lda, int N, int H, int W, int Cin, const float* w, const float* bias, int Cout,
                      float mul, float* y, int out_nchw, int ldy, int c0, void* stream);
int lsfa_upsample_flow(const float* in, int N, int Hi, int Wi, int C, const float* w, const float* bias, int Hc, int Wc,
                       float* out, int ldy, int c0, unsigned* amax_out, void* stream);
int lsfa_avgpool2_nhwc(const float* x, int N, int H, int W, int C, float* y, void* stream);
/* channels [c0, c0 + C) of an (N, Ctot, HW) map as (N, HW, C) rows: the NCHW feature the reference's operators exchange
 * (`conv_feat`, resnet_v1_101_flownet_rfcn.py:479-481 SliceChannel; Concat(warp, feat), :94-133) in the channels-last form lsfa_conv_fwd
 * reads (the R-FCN score maps, the Nq / embedding nets).  amax_out (or NULL): 256 zeroed slots that receive max|x| of the copied values
 * (lsfa_conv_fwd's amax_in). */
int lsfa_nchw_to_nhwc(const float* x, int N, int Ctot, int HW, int c0, int C, float* y, unsigned* amax_out, void* stream);

/* Inference BatchNorm (use_global_stats) + ReLU as one pass: y = max(x*scale[c]+shift[c], 0)
 * (sym_common.py:92-102 bn + relu of every pre-activation unit, resnet.py:70-101).
 * relu != 0 applies the ReLU.  In-place (y == x) allowed. */
int lsfa_scale_shift_relu(const float* x, const float* scale, const float* shift,
                          int N, int C, int HW, int relu, float* y, void* stream);

/* y = leaky(x*scale[c]+shift[c]) with leaky(v) = v > 0 ? v : v*slope — a convolution's bias and the
 * LeakyReLU(0.1) that follows it in FlowNet (resnet_v1_101_flownet_rfcn.py:153-176) as one pass. */
int lsfa_scale_shift_leaky(const float* x, const float* scale, const float* shift,
                           int N, int C, int HW, float slope, float* y, void* stream);

/* The same pass for a channels-last map: x, y are (rows, C) with the channel the fastest axis
 * (rows = N*H*W), C a multiple of 4, all pointers 16-byte aligned.  In-place allowed. */
int lsfa_scale_shift_relu_cl(const float* x, const float* scale, const float* shift,
                             long long rows, int C, int relu, float* y, void* stream);

/* ------------------------------------------------------------------------ *
 * Compressed-domain motion vectors: accumulation back to the key frame, the accumulated field and
 * the residual.
 * Replaces: create_and_load_mv_residual (accumulate = 1)   external/data_loader_py2/coviar_data_loader.c:71-177
 *           and the identity initialisation of accu_src    :316-323.
 * mvs (n_mvs, 7) int32 DEVICE rows = AVMotionVector's {source, w, h, src_x, src_y, dst_x, dst_y} in decoder
 * order (later blocks overwrite earlier ones, as the reference's serial loop does); max_block_area >= w*h of
 * every block.  accu_* (H, W, 2) int32 = per pixel the (x, y) it came from in the GOP's first frame
 * (row-major here; the reference's buffer is x-major).  lsfa_mv_accumulate writes EVERY pixel of accu_new
 * (accu_new != accu_old): ping-pong the two buffers from frame to frame.
 * mv (H, W, 2) int32 = (x, y) - accu  (:131-141);  res (H, W, 3) int32 = cur - ref[accu]  (:144-171),
 * bgr_* (H, W, 3) uint8.  Outputs feed transform_mv_res (lib/utils/image.py:202-263).
 * ------------------------------------------------------------------------ */
size_t lsfa_mv_workspace_bytes(int width, int height);
int lsfa_mv_identity(int* accu, int width, int height, void* stream);
int lsfa_mv_accumulate(const int* mvs, int n_mvs, int max_block_area, const int* accu_old, int* accu_new,
                       int width, int height, void* ws, size_t ws_bytes, void* stream);
int lsfa_mv_field(const int* accu, int width, int height, int* mv, void* stream);
int lsfa_mv_residual(const unsigned char* bgr_cur, const unsigned char* bgr_ref, const int* accu,
                     int width, int height, int* res, void* stream);
/* r5: transform_mv_res (lib/utils/image.py:202-228) on the device: the decoded frame's motion vectors (H, W, 2) and residual (H, W, 3) -
 * int32 as lsfa_mv_field / lsfa_mv_residual leave them (flags bit 0) or float32 - to the network's `motion_vector` (1, 2, h, w) and `res_diff`
 * (1, 3, h, w): cv2.resize by im_scale (INTER_LINEAR, float32 work type), zero padding to rcnn_stride, the residual's in-place channel loop
 * (BGR -> RGB, minus pixel_means, times pixel_scale, channel 2 from the rewritten channel 0 as in the reference), cv2.resize by 1 / rcnn_stride
 * in float64, motion vectors times im_scale / rcnn_stride; rounded to float32 once, where the reference hands its float64 arrays to the
 * executor.  One launch, nothing materialised at full resolution.  h1, w1 = cvRound(H * im_scale), cvRound(W * im_scale) (the caller rounds as
 * numpy does); out_h, out_w = ceil(h1 / stride), ceil(w1 / stride) - checked.  pixel_means_bgr_host: three doubles in host memory.
 * flags bit 1: the motion vectors are negated first, the `motion_vector = - motion_vector` of get_image (lib/utils/image.py:54).
 * OpenCV is not in the reference tree: the interpolation arithmetic follows OpenCV 3.2's resize.cpp as restated in oracle/np_ref.py
 * (parity unpinned for that part; everything around it is pinned by golden G6).  One case of resize() is NOT restated: at a scale of
 * exactly 1/2 in both directions OpenCV turns INTER_LINEAR into INTER_AREA (resizeAreaFast: the mean of the 2 x 2 block as (a + b + c + d) * 0.25f,
 * in an order its SIMD and scalar paths do not share).  The two-tap form used here weighs the same four pixels by 0.25 each: identical for
 * integer-valued sources (decoder frames, motion vectors, residuals: every partial sum is exact), up to an ulp apart for fractional float32
 * maps.  The second resize (1 / rcnn_stride = 1/16) never takes that switch. */
int lsfa_transform_mv_res(const void* motion_vector, const void* res_diff, int flags, int H, int W, double im_scale, int h1, int w1,
                          int rcnn_stride, const double* pixel_means_bgr_host, double pixel_scale, float* out_mv, float* out_res,
                          int out_h, int out_w, void* stream);
/* r5: resize + transform (lib/utils/image.py:266-308) of decoded frames in one launch: N frames (H, W, 3) BGR, uint8 (is_u8) or float32, on the
 * device -> `data` (N, 3, out_h, out_w) float32: cv2.resize by im_scale on the float image (get_image's .astype(np.float32), :52; INTER_LINEAR,
 * float32 work type), zero padding to `stride` (config.network.IMAGE_STRIDE; 0: none), channel i = (im[..., 2 - i] - pixel_means[2 - i]) *
 * pixel_scale: the subtraction in float32 when stride == 0 (a float32 image minus a Python float) and in float64 when stride > 0 (the padded copy is
 * np.zeros(...), a float64 image: image.py:288-293), the product in float64, rounded to float32 once.  h1, w1 = cvRound(H * im_scale), cvRound(W * im_scale); out_h, out_w = h1, w1 rounded up to
 * the stride - checked.  (lsfa_image_transform_u8 is the uint8-image form of `transform`: float64 subtraction; the two agree for zero means.)
 * is_u8: 0 = float32 frames; 1 = uint8 frames converted to float and interpolated in float (a decoder's frame after get_image's .astype); 2 (r6) = a
 * uint8 frame as cv2.imread hands it over - the LAST frame of a video, :45 - interpolated on OpenCV's fixed-point uint8 path (2048-scaled short
 * coefficients, int32 horizontal pass, `(((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2` vertically: OpenCV 3.2 imgwarp.cpp, restated as
 * oracle/np_ref.py::cv2_resize_linear_u8 - parity unpinned like the float path), then transformed with a float64 subtraction (a uint8 image's rule).
 * The result is about one intensity level from the float interpolation at most (measured <= 0.81).  NOT restated (either path): OpenCV's switch to INTER_AREA at im_scale 0.5. */
int lsfa_image_resize_transform(const void* im_hwc_bgr, int is_u8, int N, int H, int W, double im_scale, int h1, int w1, int stride,
                                const double* pixel_means_bgr_host, double pixel_scale, float* data_nchw, int out_h, int out_w, void* stream);

/* ------------------------------------------------------------------------ *
 * Block-matching motion estimation on decoded frames: the (n, 7) rows lsfa_mv_accumulate takes, computed from two uint8 frames.
 * Replaces (in function, NOT in arithmetic): the vectors the reference reads out of an MPEG-4 stream - ffmpeg's encoder
 * (data/reencode_vid.sh) and libav's AVMotionVector side data (external/data_loader_py2/coviar_data_loader.c:88-103).  Neither is part of
 * this project and no output of them exists to compare with, so these two exports are defined by the specification in
 * lsfa_amd/csrc/me.hip / DESIGN.md "Motion estimation" (restated in numpy as tests/ref_me.py) and are bit-exact with THAT; parity with an
 * encoder's search (EPZS, half-pel, 4MV) is unpinned and not claimed.  Out of scope: half-pel refinement, 8x8 partitions, B-frames, reading
 * a real bitstream.
 * lsfa_luma_u8: bgr (H, W, 3) uint8, the layout lsfa_mv_residual takes -> luma (H, W) uint8, Y = (29 B + 150 G + 77 R + 128) >> 8.
 * lsfa_mv_estimate: luma_cur, luma_ref (H, W) uint8, 4-byte aligned; 16 x 16 macroblocks on a ceil(W / 16) x ceil(H / 16) grid, edge blocks
 * cover what is left of the frame; full search over (dx, dy) in [-search, search]^2 (search 1..32) of the candidates whose shifted covered
 * rectangle lies inside the frame; cost = SAD + lambda (|dx| + |dy|) (lambda 0..2^24), ties by (|dx| + |dy|, dy, dx); max_sad > 0 turns a
 * winner whose SAD exceeds it into a zero vector (0: off).  mvs (mbh * mbw, 7) int32 rows {-1, 16, 16, 16 bx + 8 + dx, 16 by + 8 + dy,
 * 16 bx + 8, 16 by + 8} - EVERY block, zero vectors included (lsfa_mv_accumulate skips those itself), so the row count depends on the frame
 * size alone and nothing is compacted or read back; sad (mbh, mbw) int32, the winner's SAD, may be NULL.  One launch, no workspace.
 * ------------------------------------------------------------------------ */
int lsfa_luma_u8(const unsigned char* bgr, int width, int height, unsigned char* luma, void* stream);
int lsfa_mv_estimate(const unsigned char* luma_cur, const unsigned char* luma_ref, int width, int height,
                     int search, int lambda, int max_sad, int* mvs /* (mbh*mbw, 7) */, int* sad /* may be NULL */,
                     void* stream);
/* A segment at a time: the inputs of every non-key frame behind a key frame in two launches, from frames alone.
 * lsfa_mv_estimate_chain: luma holds n_chains * (n_frames + 1) planes (H, W) uint8, plane_stride bytes apart; plane 0 of a chain is its key
 *   frame.  A stack of planes is one thing for this export and lsfa_mv_refine_chain: luma, 4-byte aligned, points at plane 0; |plane_stride|
 *   is a multiple of 4 that holds a plane and lies below 2^36; a NEGATIVE plane_stride is a stack stored in reverse (plane 0 at the highest
 *   address; with n_chains = n_frames = 1 the reference plane followed by the current one behind it: a ping-pong pair).  A stride of
 *   2^36 or more, in either direction, is refused by both.  Pair (c, f), f = 1..n_frames, is
 *   lsfa_mv_estimate(plane f, plane f - 1) of chain c, bit for bit: mvs (n_chains, n_frames, mbh * mbw, 7), sad (n_chains, n_frames, mbh,
 *   mbw) or NULL.  One launch (the one-workgroup-per-macroblock grid times pairs), no workspace.
 * lsfa_mv_segment_inputs: mvs as lsfa_mv_estimate_chain wrote them; bgr holds n_chains * (n_frames + 1) packed (H, W, 3) uint8 frames,
 *   frame_stride bytes apart, frame 0 of a chain its key frame.  out_mv (n_frames, n_chains, 2, out_h, out_w) and out_res (n_frames,
 *   n_chains, 3, out_h, out_w) float32, frame-major: out_*[f - 1][c] equals lsfa_mv_identity, lsfa_mv_accumulate of chain c's frames 1..f
 *   (max_block_area 256), lsfa_mv_field, lsfa_mv_residual(cur = frame f, ref = frame 0) and lsfa_transform_mv_res(flags = 1 | 2, ...) bit
 *   for bit; im_scale .. pixel_scale, out_h, out_w as lsfa_transform_mv_res takes and checks them.  One launch, no workspace, no
 *   full-resolution map, no atomics: the source pixel of p in frame f is found by walking back, q = p; for k = f .. 1: q' = q + (row[3] -
 *   row[5], row[4] - row[6]) with row = mvs[c][k - 1][(q.y >> 4) * mbw + (q.x >> 4)], the step not taken where q' lies outside the frame
 *   (the accumulation's own rule); then mv = p - q, res = cur[p] - key[q], and transform_mv_res_kernel's arithmetic on the (at most 16)
 *   source pixels an output element reads.
 *   CONTRACT of mvs: the full-grid rows of lsfa_mv_estimate[_chain] - one row per macroblock in grid order, destination centres at
 *   16 b + 8, so that the destination blocks partition the frame and the block that contains a pixel IS its last writer.  Other rows
 *   (a decoder's block lists: use lsfa_mv_accumulate) give the result of the walk as stated, defined and memory-safe, but not the
 *   accumulation's. */
int lsfa_mv_estimate_chain(const unsigned char* luma, long long plane_stride, int n_chains, int n_frames, int width, int height,
                           int search, int lambda, int max_sad, int* mvs /* (n_chains, n_frames, mbh*mbw, 7) */,
                           int* sad /* (n_chains, n_frames, mbh, mbw) or NULL */, void* stream);
int lsfa_mv_segment_inputs(const int* mvs, const unsigned char* bgr, long long frame_stride, int n_chains, int n_frames, int width, int height,
                           double im_scale, int h1, int w1, int rcnn_stride, const double* pixel_means_bgr_host, double pixel_scale,
                           float* out_mv /* (n_frames, n_chains, 2, oh, ow) */, float* out_res /* (n_frames, n_chains, 3, oh, ow) */,
                           int out_h, int out_w, void* stream);
/* Pyramid (coarse-to-fine) search (lsfa_amd/csrc/me_pyramid.hip): vectors of up to R 2^L + r (2^L - 1) <= 137 pixels per axis, a second
 * mode beside the full search and NOT equal to the full search with a larger range (a coarse level can lock onto the wrong minimum; a
 * block whose true source is valid can have an ancestor whose shifted rectangle is not).  Defined by its own specification, restated in
 * numpy as tests/ref_me_pyramid.py, and bit-exact with that:
 *   P_0 is the plane lsfa_mv_estimate reads; P_{k+1} is ceil(w_k / 2) x ceil(h_k / 2), P_{k+1}[y][x] = (a + b + c + d + 2) >> 2 over P_k
 *   at (2x, 2y), (2x + 1, 2y), (2x, 2y + 1), (2x + 1, 2y + 1) with coordinates clamped to P_k - each level from the level below, so both
 *   roundings of P_2 are specified.  The top level L (1 or 2) is lsfa_mv_estimate[_chain](P_L, search = R, lambda, max_sad = 0) on P_L's
 *   own macroblock grid.  Levels k = L - 1 .. 0 refine: block (bx, by) of P_k has the parent (bx >> 1, by >> 1) on level k + 1, winner
 *   (pdx, pdy); candidates (2 pdx + ex, 2 pdy + ey), (ex, ey) in [-r, r]^2, plus (0, 0); valid iff the covered rectangle shifted by the
 *   candidate lies inside P_k; cost = SAD + lambda (|dx| + |dy|) on the absolute vector, the same lambda on every level; winner smallest
 *   under (cost, |dx| + |dy|, dy, dx); max_sad on level 0 only; rows {-1, 16, 16, 16 bx + 8 + dx, 16 by + 8 + dy, 16 bx + 8, 16 by + 8}
 *   for every block.  The level-0 rows keep the CONTRACT of lsfa_mv_segment_inputs above.
 * lsfa_luma_pyramid: luma holds n_planes (1..65535) planes (H, W) uint8, plane_stride bytes apart; level1 receives n_planes planes
 *   ceil(H / 2) x ceil(W / 2), stride1 bytes apart, and with levels = 2 level2 the planes of P_2, stride2 apart (levels = 1: level2 and
 *   stride2 are not read).  Output strides are multiples of 4 that hold a plane and the output bases 4-byte aligned (what the searches
 *   want).  One launch for all planes and both levels; P_2 is formed from the workgroup's P_1 tile.
 * lsfa_mv_refine_chain: one refinement step on level k for every pair of a segment.  luma holds the n_chains * (n_frames + 1) planes
 *   (height, width) of level k as lsfa_mv_estimate_chain takes them, forwards or in reverse.  parent_mvs (n_chains, n_frames,
 *   mbh_{k+1} * mbw_{k+1}, 7) are the
 *   rows of level k + 1 (mb*_{k+1} from ceil(width / 2) x ceil(height / 2)); refine r = 1..3; lambda, max_sad as lsfa_mv_estimate.  mvs
 *   (n_chains, n_frames, mbh * mbw, 7), sad (n_chains, n_frames, mbh, mbw) or NULL.  One launch, one wave per macroblock, no workspace.
 *   Parent rows that are not the mode's own: candidates with a component beyond +-255 are dropped like invalid ones (memory-safe, defined). */
int lsfa_luma_pyramid(const unsigned char* luma, long long plane_stride, int n_planes, int width, int height, int levels,
                      unsigned char* level1, long long stride1, unsigned char* level2 /* NULL with levels = 1 */, long long stride2,
                      void* stream);
int lsfa_mv_refine_chain(const unsigned char* luma, long long plane_stride, int n_chains, int n_frames, int width, int height,
                         const int* parent_mvs /* (n_chains, n_frames, mbh1*mbw1, 7) */, int refine, int lambda, int max_sad,
                         int* mvs /* (n_chains, n_frames, mbh*mbw, 7) */, int* sad /* (n_chains, n_frames, mbh, mbw) or NULL */, void* stream);
/* Scene cuts from the searches' own SADs (lsfa_amd/csrc/me_cut.hip): a third, opt-in mode of the front end.  The textbook encoder rule -
 * a macroblock's inter cost against its intra cost - NOT ffmpeg's scene detection; like the two searches it replaces nothing of the
 * reference (ImageNet-VID snippets have no cuts; the reference's key frames are every TEST.KEY_FRAME_INTERVAL-th) and is comparable with
 * nothing in it.  Defined by its own specification (DESIGN.md "Scene cuts", restated in numpy as tests/ref_me_cut.py) and bit-exact with
 * that.  For pair (c, f), f = 1..n_frames (plane f against plane f - 1 of chain c) and macroblock b of the level-0 grid, n_b its covered
 * pixels (256, fewer for a block cut by the right or bottom edge):
 *   inter_b = sad[c][f - 1][b] as a search wrote it (the full search's or the pyramid's level-0 winner; max_sad does not change it);
 *   m_b = (sum p + n_b / 2) / n_b, integer division, over the covered pixels of the CURRENT plane f;  intra_b = sum |p - m_b|;
 *   b is unmatched iff inter_b > intra_b + bias * n_b, bias 0..255 grey levels per pixel (two frames of one flat, noisy area differ by
 *   about sqrt(2) times the noise, a block from its own mean by the noise only: without a bias every flat block would vote "cut");
 *   unmatched[c][f - 1] = the number of unmatched blocks.  The frame decision is the caller's: a cut iff unmatched * 100 > percent * mbh * mbw.
 * lsfa_mv_cut_score: luma is the stack lsfa_mv_estimate_chain takes, addressed and refused as there (a negative plane_stride is a stack
 *   stored in reverse; plane 0 of a chain is read by no pair's intra cost).  intra (n_chains, n_frames, mbh, mbw) and unmatched (n_chains,
 *   n_frames) int32 are both written in full.  Two launches (sixteen lanes per macroblock; one workgroup per pair), no workspace, no memset, no
 *   atomics, nothing read back. */
int lsfa_mv_cut_score(const unsigned char* luma, long long plane_stride, int n_chains, int n_frames, int width, int height,
                      const int* sad /* (n_chains, n_frames, mbh, mbw) */, int bias, int* intra /* (n_chains, n_frames, mbh, mbw) */,
                      int* unmatched /* (n_chains, n_frames) */, void* stream);
/* Stale key frames (lsfa_amd/csrc/me_key.hip): a fourth, opt-in mode of the front end.  It stands in for an encoder's decision to spend an
 * I-frame where the reference picture has stopped predicting - a fade or dissolve, content that pans in, occlusion that builds up, the
 * drift of chained vectors: all invisible to the pair rule above, which no single pair of consecutive frames crosses.  Like the other three
 * modes it replaces nothing of the reference (its key frames are a property of its dataset) and is comparable with nothing in it; no parity
 * with any encoder's I-frame decision is claimed.  Defined by its own specification (DESIGN.md "Stale key frames", restated in numpy as
 * tests/ref_me_stale.py) and bit-exact with that.  For chain c with planes P_0 (its key frame) .. P_F and the level-0 rows of frames 1..F as
 * any of the searches wrote them:
 *   q_f(p) = the walk back of lsfa_mv_segment_inputs above for pixel p of frame f through the rows of frames f .. 1, a step that would
 *            leave the frame not taken: always inside the frame;
 *   keysad[c][f - 1][b] = sum over the covered pixels p of macroblock b of |P_f[p] - P_0[q_f(p)]|  (<= 65,280): `res_diff` before its resize,
 *            per block;
 *   the decision is lsfa_mv_cut_score's, unchanged, with keysad as its `sad`: intra_b over the CURRENT plane f; b is unmatched against the key
 *   iff keysad_b > intra_b + bias * n_b; frame f is stale iff unmatched * 100 > percent * mbh * mbw (the caller's).  bias (0..255) and percent
 *   (1..100) are the mode's own, independent of the pair rule's.
 * lsfa_mv_key_sad: the segment form.  luma is the stack lsfa_mv_estimate_chain takes, addressed and refused as there (negative plane_stride
 *   included); rows (n_chains, n_frames, mbh * mbw, 7) under the CONTRACT of lsfa_mv_segment_inputs (other rows: the walk as stated, defined
 *   and memory-safe); keysad (n_chains, n_frames, mbh, mbw) int32, written in full.  One launch (a wave per macroblock of every pair), no
 *   workspace, no memset, no atomics, nothing read back.
 * lsfa_mv_key_sad_accu: the per-frame form, for a frame whose source map exists: luma_cur (4-byte aligned) and luma_key (height, width)
 *   uint8, accu (height, width, 2) int32 = the (x, y) in the key frame every pixel comes from, as lsfa_mv_accumulate leaves it (8-byte
 *   aligned); keysad (mbh, mbw).  A source position outside the plane reads as 0 (lsfa_mv_accumulate never produces one).  On the map
 *   accumulated from the rows of frames 1..f it equals lsfa_mv_key_sad's frame f bit for bit (the walk-back identity).  One launch. */
int lsfa_mv_key_sad(const unsigned char* luma, long long plane_stride, int n_chains, int n_frames, int width, int height,
                    const int* rows /* (n_chains, n_frames, mbh*mbw, 7) */, int* keysad /* (n_chains, n_frames, mbh, mbw) */, void* stream);
int lsfa_mv_key_sad_accu(const unsigned char* luma_cur, const unsigned char* luma_key, const int* accu /* (height, width, 2) */, int width,
                         int height, int* keysad /* (mbh, mbw) */, void* stream);

/* ------------------------------------------------------------------------ *
 * YUV 4:2:0 intake (lsfa_amd/csrc/yuvfmt.hip, the one intake source): the planes a decoder hands over - libav, the VCN decode engines, a raw .yuv dump - straight to
 * the packed BGR frame lsfa_mv_residual / lsfa_luma_u8 / lsfa_image_transform_u8 take, to the luma plane lsfa_mv_estimate searches and to the
 * network's `data`.  Replaces (in function, NOT in arithmetic): the swscale conversion inside the reference's coviar loader
 * (external/data_loader_py2/coviar_data_loader.c), which runs on the CPU.  Neither swscale nor OpenCV is part of this project, and both carry
 * options (chroma siting, bilinear chroma) that change the result, so the conversion is defined by the specification below (DESIGN.md "YUV
 * intake", restated in numpy as tests/ref_yuv.py) and is bit-exact with THAT; parity with swscale or OpenCV is unpinned and not claimed.
 *   Pixel (x, y) takes Y[y][x] and the chroma sample (x >> 1, y >> 1): nearest-neighbour chroma, no interpolation.  Chroma planes are
 *   ceil(W / 2) x ceil(H / 2); odd W and H are allowed.  C = Y - o, D = U - 128, E = V - 128, all int; >> is arithmetic (it floors); clip
 *   clamps to 0..255.
 *     matrix 0, BT.601 limited range (what MPEG-4 streams carry), o = 16:
 *        R = clip((298 C + 409 E + 128) >> 8)   G = clip((298 C - 100 D - 208 E + 128) >> 8)   B = clip((298 C + 516 D + 128) >> 8)
 *     matrix 1, BT.709 limited range, o = 16:
 *        R = clip((298 C + 459 E + 128) >> 8)   G = clip((298 C -  55 D - 136 E + 128) >> 8)   B = clip((298 C + 541 D + 128) >> 8)
 *     matrix 2, BT.601 full range (JFIF), o = 0:
 *        R = clip((256 C + 359 E + 128) >> 8)   G = clip((256 C -  88 D - 183 E + 128) >> 8)   B = clip((256 C + 454 D + 128) >> 8)
 * Out of scope: interpolated chroma; any binding to rocDecode (a decoded surface's base, pitch and height ARE the arguments:
 * INTEGRATION.md).  10-bit samples (P010, yuv420p10le) and the other chroma formats (NV21, 4:2:2, 4:4:4, packed YUYV / UYVY) have entry
 * points of their own at the end of this header.
 * Planes: a base pointer, a row pitch in bytes and, for N frames, a frame stride in bytes each; a pitch wider than the row is normal
 * (y_pitch >= W; c_pitch >= 2 ceil(W / 2) for NV12, >= ceil(W / 2) for I420), a frame stride may be anything that does not overlap.
 * v == NULL: u_or_uv is the interleaved U, V plane (NV12); otherwise u_or_uv and v are I420's two chroma planes, with one pitch and stride.
 * One launch each, no workspace.  Dword-aligned planes (half-word aligned I420 chroma) of W % 4 == 0, H % 2 == 0 take the kernel that reads
 * four pixels of two rows per thread; anything else takes a byte-wise kernel, picked per launch.
 * lsfa_yuv420_to_bgr_u8: bgr (N, H, W, 3) uint8, packed; y_packed (N, H, W) or NULL: the Y plane with the pitch removed - the contiguous plane
 *   lsfa_mv_estimate wants, without a copy of its own (limited-range Y is NOT lsfa_luma_u8 of the converted frame: different numbers).
 * lsfa_image_transform_yuv420: `data` (N, 3, H, W) float32, channel i = (bgr[2 - i] - pixel_means[2 - i]) * pixel_scale, subtraction and product
 *   in float64, rounded to float32 once: bit-identical to lsfa_image_transform_u8 of lsfa_yuv420_to_bgr_u8's frame, which is never stored.
 *   No H*W % 4 condition.
 * lsfa_image_resize_transform_yuv420: lsfa_image_resize_transform with is_u8 = 1 reading its taps from the planes (the converted frame as
 *   float, interpolated in float, padded to `stride`, the float32 / float64 subtraction rule by `stride` stated there); bit-identical to it
 *   on lsfa_yuv420_to_bgr_u8's frame.  h1, w1, out_h, out_w as there - checked.  The fixed-point is_u8 = 2 form is not offered for YUV.
 * Each of the three equals lsfa_yuv_to_bgr_u8 / lsfa_image_transform_yuv / lsfa_image_resize_transform_yuv ("YUV intake, other chroma
 * formats" below) with format LSFA_YUV_FORMAT(LSFA_YUV_420, v ? LSFA_YUV_PLANAR : LSFA_YUV_UV, LSFA_YUV_U8): a forward to the same code.
 * ------------------------------------------------------------------------ */
int lsfa_yuv420_to_bgr_u8(const unsigned char* y, long long y_pitch, long long y_frame_stride, const unsigned char* u_or_uv,
                          const unsigned char* v /* NULL: NV12 */, long long c_pitch, long long c_frame_stride, int N, int H, int W, int matrix,
                          unsigned char* bgr, unsigned char* y_packed /* may be NULL */, void* stream);
int lsfa_image_transform_yuv420(const unsigned char* y, long long y_pitch, long long y_frame_stride, const unsigned char* u_or_uv,
                                const unsigned char* v /* NULL: NV12 */, long long c_pitch, long long c_frame_stride, int N, int H, int W, int matrix,
                                const double* pixel_means_bgr_host, double pixel_scale, float* data_nchw, void* stream);
int lsfa_image_resize_transform_yuv420(const unsigned char* y, long long y_pitch, long long y_frame_stride, const unsigned char* u_or_uv,
                                       const unsigned char* v /* NULL: NV12 */, long long c_pitch, long long c_frame_stride, int N, int H, int W,
                                       int matrix, double im_scale, int h1, int w1, int stride, const double* pixel_means_bgr_host,
                                       double pixel_scale, float* data_nchw, int out_h, int out_w, void* stream);

/* ------------------------------------------------------------------------ *
 * Plumbing without a reference counterpart: a hipStream_t that is nobody else's (non-blocking; PyTorch's
 * streams come from a small round-robin pool, and two graphs captured on pool twins share one BLAS
 * workspace — lsfa_amd/core/streams.py wraps these in torch.cuda.ExternalStream for capture and replay).
 * ------------------------------------------------------------------------ */
int lsfa_stream_create(void** stream_out, int high_priority);
int lsfa_stream_destroy(void* stream);
/* up to 32 device-to-device copies of 4-byte elements (elems4[k] of them, dst[k] <- src[k]) as one launch: a frame's - or a whole
 * segment's - images, motion vectors and residuals into the static buffers a captured graph reads.  r5: src[k] == NULL zero-fills
 * dst[k] (amax slots, the padding channels of a Concat map): the frame path issues no PyTorch fill or copy kernel */
int lsfa_copy_many(int njobs, void* const* dst, const void* const* src, const long* elems4, void* stream);
/* r6: table_dev[i] = ptrs_host[i] for i < n, as one tiny launch per 64 entries on `stream` (the values travel as kernel arguments): how the
 * per-image pointer tables of the *_tbl entry points are rewritten between replays of a captured graph. */
int lsfa_ptr_table_set(void** table_dev, int n, const void* const* ptrs_host, void* stream);

/* ------------------------------------------------------------------------ *
 * Live per-op timing with HIP events on the launch stream (bench.py's roofline leg).
 * lsfa_prof_enable(mask) makes the entry points whose op id bit is set in `mask`
 * (-1 = all, 0 = off) bracket their launches with hipEventRecord on `stream`;
 * lsfa_prof_read synchronises the events and returns accumulated milliseconds and
 * launch counts per op id, then clears them.  Do not enable during graph capture.
 * ------------------------------------------------------------------------ */
enum {
  LSFA_OP_PSROI = 0, LSFA_OP_RFCN_HEAD = 1, LSFA_OP_WARP = 2, LSFA_OP_AGG = 3,
  LSFA_OP_PROPOSAL = 4, LSFA_OP_NMS = 5, LSFA_OP_DET = 6, LSFA_OP_DCN_IM2COL = 7,
  LSFA_OP_BNRELU = 8, LSFA_OP_CONV = 9, LSFA_OP_STEM = 10, LSFA_OP_FLOWNET = 11,
  LSFA_OP_MV_ESTIMATE = 12, LSFA_OP_COUNT = 13
};
int lsfa_prof_enable(int mask);
int lsfa_prof_read(double* ms_host /*LSFA_OP_COUNT*/, int* launches_host /*LSFA_OP_COUNT*/);
const char* lsfa_op_name(int op_id);

/* ------------------------------------------------------------------------ *
 * 10-bit YUV 4:2:0 intake (lsfa_amd/csrc/yuvfmt.hip): what HEVC Main10, VP9 profile 2 and AV1 10-bit decode to - the VCN engines' P010 /
 * P016 surfaces, libav's yuv420p10le - to the same three outputs as the 8-bit intake above, which it mirrors argument for argument with
 * `shift` behind `matrix`.  Everything behind the intake stays 8-bit.  Defined by the specification below (DESIGN.md "YUV intake", "10-bit
 * planes"; restated in numpy as tests/ref_yuv10.py) and bit-exact with THAT; parity with swscale is unpinned and not claimed.
 *   A sample is a 16-bit little-endian word w, and s = (w >> shift) & 1023.  shift = 6 is P010: the value sits in the high ten bits and the
 *   low six are ignored whatever they hold (so a P016 surface is read as its high ten bits).  shift = 0 is yuv420p10le / I010: the value
 *   sits in the low ten bits and the high six are masked.  Any word is defined input.
 *   Geometry as above: pixel (x, y) takes Y[y][x] and the chroma sample (x >> 1, y >> 1); chroma planes are ceil(W / 2) x ceil(H / 2); odd
 *   W and H are allowed.  v == NULL: u_or_uv holds interleaved U, V words (P010's layout); otherwise u_or_uv and v are two planes with one
 *   pitch and one frame stride.  Either layout goes with either shift.
 *   C = Y - 4 o, D = U - 512, E = V - 512 with o and the coefficients of the 8-bit table above (o = 64, 64, 0 for matrices 0, 1, 2):
 *     matrix 0:  R = clip((298 C + 409 E + 512) >> 10)   G = clip((298 C - 100 D - 208 E + 512) >> 10)   B = clip((298 C + 516 D + 512) >> 10)
 *   and likewise for matrices 1 and 2: the 8-bit formulas with rounding constant 512 and shift 10, so the conversion is done in ten bits and
 *   rounded once; clip clamps to 0..255; every intermediate stays below 2^20 in magnitude.  Planes that are exactly 4 x an 8-bit plane give
 *   the 8-bit specification's BGR bit for bit.
 *   y_packed (uint8, what lsfa_mv_estimate searches) = min(255, (Y + 2) >> 2); on 4 x an 8-bit plane it gives that plane back.
 * Planes are const void*: bases of 16-bit words.  Pitches and frame strides are in BYTES.  LSFA_EINVAL, before anything is launched, for a NULL
 * plane or output, N, H or W below 1, a matrix outside 0..2, a shift other than 0 or 6, an odd base, pitch or frame stride, and a pitch below
 * its row (2 W for Y; 4 ceil(W / 2) for interleaved, 2 ceil(W / 2) for planar chroma).
 * One launch each, on `stream`, no workspace, nothing allocated; reported under LSFA_OP_STEM.  8-byte aligned planes (4-byte aligned planar
 * chroma) of W % 4 == 0, H % 2 == 0 take the kernel that reads four pixels of two rows per thread; anything else takes an element-wise
 * kernel, picked per launch.
 * lsfa_yuv420p10_to_bgr_u8: bgr (N, H, W, 3) uint8, packed; y_packed (N, H, W) uint8 or NULL.
 * lsfa_image_transform_yuv420p10: `data` (N, 3, H, W) float32: lsfa_image_transform_u8 of lsfa_yuv420p10_to_bgr_u8's frame, bit for bit
 *   (subtraction and product in float64, rounded once), without storing the frame.
 * lsfa_image_resize_transform_yuv420p10: lsfa_image_resize_transform with is_u8 = 1 of that frame, bit for bit, reading its taps from the
 *   planes; h1, w1, stride, out_h, out_w as there - checked.
 * Each of the three, once `shift` is 0 or 6, equals lsfa_yuv_to_bgr_u8 / lsfa_image_transform_yuv / lsfa_image_resize_transform_yuv below with
 * format LSFA_YUV_FORMAT(LSFA_YUV_420, v ? LSFA_YUV_PLANAR : LSFA_YUV_UV, shift ? LSFA_YUV_HI10 : LSFA_YUV_LO10): a forward to the same code.
 * ------------------------------------------------------------------------ */
int lsfa_yuv420p10_to_bgr_u8(const void* y, long long y_pitch, long long y_frame_stride, const void* u_or_uv, const void* v /* NULL: interleaved */,
                             long long c_pitch, long long c_frame_stride, int N, int H, int W, int matrix, int shift, unsigned char* bgr,
                             unsigned char* y_packed /* may be NULL */, void* stream);
int lsfa_image_transform_yuv420p10(const void* y, long long y_pitch, long long y_frame_stride, const void* u_or_uv, const void* v /* NULL: interleaved */,
                                   long long c_pitch, long long c_frame_stride, int N, int H, int W, int matrix, int shift,
                                   const double* pixel_means_bgr_host, double pixel_scale, float* data_nchw, void* stream);
int lsfa_image_resize_transform_yuv420p10(const void* y, long long y_pitch, long long y_frame_stride, const void* u_or_uv,
                                          const void* v /* NULL: interleaved */, long long c_pitch, long long c_frame_stride, int N, int H, int W,
                                          int matrix, int shift, double im_scale, int h1, int w1, int stride, const double* pixel_means_bgr_host,
                                          double pixel_scale, float* data_nchw, int out_h, int out_w, void* stream);

/* ------------------------------------------------------------------------ *
 * YUV intake, other chroma formats (lsfa_amd/csrc/yuvfmt.hip): 4:2:2 and 4:4:4, chroma interleaved V, U, packed YUYV / UYVY - what capture
 * cards and webcams (YUYV / YUY2, UYVY), MJPEG cameras (yuvj422p, yuvj444p: matrix 2), contribution codecs (yuv422p10le, P210), screen
 * content (4:4:4) and Android cameras (NV21) hand over - to the same three outputs as the two intakes above.  The three exports mirror the
 * 10-bit prototypes argument for argument with `format` where those have `shift`.  The specification is the shipped one with the chroma
 * address generalised (DESIGN.md "YUV intake", "Other chroma formats"; restated in numpy as tests/ref_yuvfmt.py on tests/ref_yuv.py's and
 * tests/ref_yuv10.py's conversions) and is bit-exact with THAT.  format = sub | layout << 4 | sample << 8, three independent choices:
 *   sub: pixel (x, y) takes Y[y][x] and the chroma sample (x >> sx, y >> sy), nearest neighbour; chroma planes are
 *     ceil(W / 2^sx) x ceil(H / 2^sy); any W, H >= 1.   0: 4:2:0 (sx, sy) = (1, 1)   1: 4:2:2 (1, 0)   2: 4:4:4 (0, 0)
 *   layout: 0: two planes U (u_or_uv) and V (v) with one pitch and one frame stride   1: one interleaved plane U, V (v == NULL)
 *     2: one interleaved plane V, U (v == NULL: NV21 / NV61 / NV42)   3: packed Y0 U Y1 V (YUYV / YUY2)   4: packed U Y0 V Y1 (UYVY).
 *     Packed (3, 4): a row is ceil(W / 2) four-byte groups; `y` is the packed plane and y_pitch its pitch, at least 4 ceil(W / 2); both
 *     chroma pointers are NULL and both chroma pitches and strides 0; with odd W the last group's second Y is never part of the result.
 *   sample: 0: bytes, converted by the 8-bit table ("YUV 4:2:0 intake" above), y_packed = Y   1: 16-bit words with the value in the low ten
 *     bits: the 10-bit specification's conversion, rounding and y_packed rule with shift = 0   2: in the high ten bits: shift = 6.
 *   Packed layouts exist only with sub = 1 and sample = 0; every other combination is valid: 27 + 2 formats.  Matrices 0..2 as above.
 *   The 4:2:0 formats of the two intakes above (layouts 0 and 1) are formats like any other: those six exports forward here.
 * Out of scope: interpolated or sited chroma; packed 10-bit (v210, Y210, Y410); 12-bit; 4:1:1 / 4:1:0; YVYU; alpha; BT.2020 / HDR transfer; RGB
 * surfaces.
 * Pitches and frame strides are in BYTES.  LSFA_EINVAL, before anything is launched, for: a format outside the above; a NULL plane or output;
 * v given with layouts 1 and 2 or missing with layout 0; a chroma pointer, pitch or stride with a packed layout; N, H or W below 1; a matrix
 * outside 0..2; for words an odd base, pitch or frame stride; a pitch below its row (Y: W samples; planar chroma ceil(W / 2^sx) samples,
 * interleaved twice that; packed 4 ceil(W / 2) bytes).
 * One launch each, on `stream`, no workspace, nothing allocated; reported under LSFA_OP_STEM.  W % 4 == 0 (and for 4:2:0 an even H) with
 * every base, pitch and frame stride a multiple of the load it feeds takes the four-pixel kernel compiled for the format; anything else -
 * odd bases, pitches or strides, any other W, an odd H of 4:2:0 - the element-wise kernel, which takes layout and subsampling at run time
 * (compiled for bytes and for words), as the resize kernel does.  The loads, in bytes (words: twice): Y 4; packed 8; planar chroma 2 (4:4:4: 4) per plane; interleaved chroma 4 (4:4:4: 8).
 * The outputs as above: bgr and y_packed dword aligned, `data` 16-byte aligned for the four-pixel kernel.
 * lsfa_yuv_to_bgr_u8: bgr (N, H, W, 3) uint8, packed; y_packed (N, H, W) uint8 or NULL.
 * lsfa_image_transform_yuv: `data` (N, 3, H, W) float32: DEFINED as lsfa_image_transform_u8 of lsfa_yuv_to_bgr_u8's frame, bit for bit.
 * lsfa_image_resize_transform_yuv: DEFINED as lsfa_image_resize_transform with is_u8 = 1 of that frame, bit for bit, reading its taps from the
 *   planes; h1, w1, stride, out_h, out_w as there - checked.
 * ------------------------------------------------------------------------ */
#define LSFA_YUV_420 0
#define LSFA_YUV_422 1
#define LSFA_YUV_444 2
#define LSFA_YUV_PLANAR 0
#define LSFA_YUV_UV 1
#define LSFA_YUV_VU 2
#define LSFA_YUV_YUYV 3
#define LSFA_YUV_UYVY 4
#define LSFA_YUV_U8 0
#define LSFA_YUV_LO10 1
#define LSFA_YUV_HI10 2
#define LSFA_YUV_FORMAT(sub, layout, sample) ((sub) | (layout) << 4 | (sample) << 8)
int lsfa_yuv_to_bgr_u8(const void* y, long long y_pitch, long long y_frame_stride, const void* u_or_uv, const void* v, long long c_pitch,
                       long long c_frame_stride, int N, int H, int W, int matrix, int format, unsigned char* bgr,
                       unsigned char* y_packed /* may be NULL */, void* stream);
int lsfa_image_transform_yuv(const void* y, long long y_pitch, long long y_frame_stride, const void* u_or_uv, const void* v, long long c_pitch,
                             long long c_frame_stride, int N, int H, int W, int matrix, int format, const double* pixel_means_bgr_host,
                             double pixel_scale, float* data_nchw, void* stream);
int lsfa_image_resize_transform_yuv(const void* y, long long y_pitch, long long y_frame_stride, const void* u_or_uv, const void* v,
                                    long long c_pitch, long long c_frame_stride, int N, int H, int W, int matrix, int format, double im_scale,
                                    int h1, int w1, int stride, const double* pixel_means_bgr_host, double pixel_scale, float* data_nchw,
                                    int out_h, int out_w, void* stream);

/* ------------------------------------------------------------------------ *
 * Detection overlay (lsfa_amd/csrc/overlay.hip): the detections lsfa_det_postprocess(_batch) left on the device, burnt into the frame that is
 * already on the device - a packed BGR frame, or the planes of any format the YUV intake reads (NV12 / I420 by lsfa_overlay_paint_yuv420,
 * all 29 by lsfa_overlay_paint_yuv), e.g. the surface a hardware encoder takes next.  Nothing is read back and every call can sit inside a captured graph.
 * Replaces (in function, NOT in pixels): draw_boxes + cv2.imwrite at the end of the reference's demo.py:150-157.  cv2's rasteriser is not
 * part of this project - no Hershey fonts, no anti-aliasing, none of cv2's line joins - and draw_boxes picks random colours.  The overlay
 * is defined by the integer specification below (DESIGN.md "Detection overlay"; restated in numpy as tests/ref_overlay.py) and is bit-exact
 * with THAT; parity with cv2 is not claimed.
 *   Input per image: dets (ncls, R, 5) float64 rows [x1, y1, x2, y2, score] in pixels of the frame that is drawn into; counts (ncls) int32.
 *   Draw order: classes j = 1 .. ncls-1 ascending (class 0 is never drawn), rows 0 .. min(max(counts[j], 0), R) - 1 ascending inside a class.
 *   A row is eligible when all five values are finite and score >= thresh.  Its corners are trunc() of the coordinates (`map(int, bbox)`),
 *   each double clamped to [-2^30, 2^30] first and NOT clamped to the frame.  An eligible row is skipped when x2 < x1 or y2 < y1, or when the
 *   box lies wholly outside [0, W-1] x [0, H-1] (x2 < 0, y2 < 0, x1 > W-1 or y1 > H-1).  The first max_boxes eligible rows that are not
 *   skipped become records, in draw order; n = {records written, eligible rows that are not skipped} goes to the device.
 *   Outline, thickness t in 1..8 (the reference: 3), centred on the edge: o = (t - 1) / 2, i = t - o; the pixels inside
 *   [x1-o, x2+o] x [y1-o, y2+o] and not inside [x1+i, x2-i] x [y1+i, y2-i]; an empty inner rectangle fills the outer one.
 *   Label, scale z in 0..4 (0: none): the characters are the class's name - at most LSFA_OVERLAY_NAME_LEN glyph indices of row j of `names`,
 *   0xFF ends a name, an index above 41 reads as '?'; names == NULL: the decimal digits of j - then, if with_score, " d.ddd" (a space first)
 *   from m = clamp(floor(score * 1000 + 0.5), 0, 9999), the product rounded to float64 before the addition (no fused multiply-add).
 *   L characters (L = 0: no label) give the rectangle w = z (6L + 1), h = 9z at lx = x1 - o, ly = y1 - o - h; if ly < 0 then ly = y1 + i
 *   (inside the box, under its top edge); if lx + w > W then lx = W - w; then if lx < 0 then lx = 0.
 *   Glyphs are 5 x 7 in a 6 x 8 cell, this project's own drawings (lsfa_amd/overlay.py): index 0 space, 1..10 '0'..'9', 11..36 'a'..'z',
 *   37 '_', 38 '-', 39 '.', 40 '%', 41 '?'.  `font` is LSFA_OVERLAY_GLYPH_BYTES bytes: glyph g, row v at byte 8 g + v, bit 4 its left column.
 *   A pixel (x, y) of the label rectangle is a TEXT pixel when, with dx = x - lx - z, dy = y - ly - z, u = dx / z, v = dy / z: dx >= 0,
 *   dy >= 0, u < 6L, u % 6 < 5, v < 7 and bit 4 - u % 6 of row v of glyph u / 6 is set; every other pixel of it is background.
 *   A pixel's result comes from the LAST record in draw order whose outline or label rectangle contains it: colors[ncls] (the text colour)
 *   for a text pixel, else colors[j].  Opaque, clipped to the frame pixel by pixel.  A pixel no record covers is never written.
 *   colors: (ncls + 1, 3) uint8 in the component order of the surface: B, G, R or Y, U, V (made on the host, lsfa_amd/overlay.py bgr_to_yuv).
 *   4:2:0 surfaces: Y[y][x] takes component 0 of pixel (x, y)'s result; chroma sample (cx, cy) takes components 1 and 2 of the result of
 *   pixel (2cx, 2cy) and is untouched when that pixel is uncovered - the intake's nearest-neighbour rule.  Odd W, H: chroma is ceil / 2.
 *   Every YUV surface of the intake (lsfa_overlay_paint_yuv; format = sub | layout << 4 | sample << 8, LSFA_YUV_FORMAT of "YUV intake, other
 *   chroma formats", the same 27 + 2 codes).  Everything up to a pixel's result is as above; only the samples that take it are new:
 *     colors: the (ncls + 1, 3) uint8 Y, U, V table of the 4:2:0 surfaces, whatever the sample width: no colour arithmetic on the device.
 *     Sample value of a colour component c: sample 0: the byte c; 1 (low ten bits): the 16-bit word c << 2; 2 (high ten bits): the word
 *     c << 8.  The whole word is stored: the bits the intake ignores are written as 0.  (The intake converts planes that are exactly 4 x an
 *     8-bit plane to the 8-bit BGR bit for bit, so a colour drawn into a 10-bit surface reads back as the same BGR as in 8 bits.)
 *     Luma: Y[y][x] takes component 0 of pixel (x, y)'s result when the pixel is covered.
 *     Chroma: with the format's shifts (sx, sy) - 4:2:0 (1, 1), 4:2:2 (1, 0), 4:4:4 (0, 0) - the chroma sample (cx, cy) takes components 1
 *     and 2 of the result of pixel (cx << sx, cy << sy), the first pixel the intake's nearest-neighbour rule maps to it, which always lies
 *     inside the frame; the sample is untouched when that pixel is uncovered.  sub = 0 is the (2cx, 2cy) rule above.
 *     Layouts: 0: two planes U, V; 1: interleaved U, V; 2: interleaved V, U; 3: packed groups Y0 U Y1 V; 4: packed groups U Y0 V Y1.  In
 *     a packed row group g takes its U and V from pixel 2g and its two Y bytes from pixels 2g and 2g + 1; with odd W the last group's second
 *     Y byte is never written.
 *     A sample whose pixel is uncovered is never stored: not rewritten with its own value and not as part of a wider store; for words
 *     this includes their ignored bits.
 * Out of scope: blending, transparency, anti-aliasing; packed 10-bit, 12-bit and RGB surfaces (draw on the converted BGR frame); masks
 * and tracks.  (Tracks are drawn by lsfa_overlay_plan_ids, declared under "Tracks" below, from the ids lsfa_track_steps assigns.)
 * A record is LSFA_OVERLAY_REC_INTS ints: x1, y1, x2, y2, lx, ly, w, h, j, L, then the L glyph indices four to an int (character k in bits
 * 8 (k % 4) of int 10 + k / 4), unused bits 0.  The caller sizes the buffers: records (N, max_boxes, LSFA_OVERLAY_REC_INTS) int32 and
 * n (N, 2) int32, max_boxes in 1..LSFA_OVERLAY_MAX_BOXES.  The paint calls read only the first min(n[0], max_boxes) records of an image and
 * are memory-safe whatever those hold.
 * lsfa_overlay_plan: one workgroup per image; compaction on the device as a prefix over (class, row) - only the rows under counts are
 *   walked, so a frame without detections costs the launch - no atomics.  One launch.
 * lsfa_overlay_paint_bgr: bgr (N, H, W, 3) uint8 with a row pitch and a frame stride in BYTES, in place.  One launch for the N frames.
 * lsfa_overlay_paint_yuv420: the planes, pitches and strides of lsfa_yuv420_to_bgr_u8 (v == NULL: NV12), in place.  One launch.
 * lsfa_overlay_paint_yuv: the planes, pitches and strides of lsfa_yuv_to_bgr_u8 up to W, then `format`, in place.  One launch.  The
 *   4:2:0 codes of layouts 0 and 1 of bytes leave the bytes lsfa_overlay_paint_yuv420 leaves.
 *   One 256-lane workgroup per 64 x 16 tile; a tile no record can touch leaves before it touches the frame.  thickness and label_scale
 *   must be the plan's.
 * LSFA_EINVAL, before anything is launched, for: a NULL pointer (but names, and v for NV12); N, H, W, R or max_boxes below 1; ncls below 1 or
 * above LSFA_OVERLAY_MAX_CLASSES; H or W above 65536, N above 65535, max_boxes above LSFA_OVERLAY_MAX_BOXES, (ncls - 1) * R at or above 2^31; thickness outside 1..8;
 * label_scale outside 0..4; a pitch below its row (3 W; Y: W; chroma 2 ceil(W / 2) interleaved, ceil(W / 2) planar); a negative frame stride.
 * lsfa_overlay_paint_yuv refuses besides what the intake refuses of planes: a format outside the 27 + 2; v given with layouts 1 and 2 or
 * missing with layout 0; a chroma pointer, pitch or stride with a packed layout; for words an odd base, pitch or frame stride; a pitch below
 * its row (Y: W samples; planar chroma ceil(W / 2^sx) samples, interleaved twice that; packed 4 ceil(W / 2) bytes).
 * On `stream`, no workspace, nothing allocated; not reported under a profiling id.
 * ------------------------------------------------------------------------ */
#define LSFA_OVERLAY_REC_INTS 16
#define LSFA_OVERLAY_NAME_LEN 12
#define LSFA_OVERLAY_GLYPHS 42
#define LSFA_OVERLAY_GLYPH_BYTES 336
#define LSFA_OVERLAY_MAX_BOXES 4096
#define LSFA_OVERLAY_MAX_CLASSES 4096
int lsfa_overlay_plan(const double* dets, const int* counts, int N, int ncls, int R, double thresh, int H, int W, int thickness, int label_scale,
                      int with_score, const unsigned char* names /* (ncls, LSFA_OVERLAY_NAME_LEN) or NULL */, int max_boxes, int* records, int* n,
                      void* stream);
int lsfa_overlay_paint_bgr(unsigned char* bgr, long long pitch, long long frame_stride, int N, int H, int W, const int* records, const int* n,
                           int max_boxes, int thickness, int label_scale, const unsigned char* font, const unsigned char* colors, int ncls,
                           void* stream);
int lsfa_overlay_paint_yuv420(unsigned char* y, long long y_pitch, long long y_frame_stride, unsigned char* u_or_uv,
                              unsigned char* v /* NULL: NV12 */, long long c_pitch, long long c_frame_stride, int N, int H, int W,
                              const int* records, const int* n, int max_boxes, int thickness, int label_scale, const unsigned char* font,
                              const unsigned char* colors, int ncls, void* stream);
int lsfa_overlay_paint_yuv(void* y, long long y_pitch, long long y_frame_stride, void* u_or_uv, void* v /* layout 0 only */, long long c_pitch,
                           long long c_frame_stride, int N, int H, int W, int format, const int* records, const int* n, int max_boxes,
                           int thickness, int label_scale, const unsigned char* font, const unsigned char* colors, int ncls, void* stream);

/* ------------------------------------------------------------------------ *
 * Tracks (lsfa_amd/csrc/tracks.hip): which detection of frame f is the same object as which detection of frame f - 1, decided on the device
 * from what lsfa_det_postprocess(_batch) left there and, optionally, from the block rows lsfa_mv_estimate / lsfa_mv_estimate_chain wrote, which
 * are in the same pixel coordinates: a row says "the block now at dst came from src", a forward prediction of where last frame's boxes went.
 * Replaces nothing in the reference, which has no tracker, and is comparable with nothing there.  It is not SORT, not Seq-NMS and not a
 * Kalman filter; it does not rescore or remove detections: dets and counts are read-only.  It is defined by the float64 / integer
 * specification below (DESIGN.md "Tracks"; restated in numpy as tests/ref_tracks.py) and is bit-exact with THAT.
 *   One call advances S independent streams (the clips of a lock-step batch) by F consecutive frames each (1 frame by frame, or e.g. the 9
 *   non-key frames of a segment).  Streams never interact; the frames of a stream are processed in order f = 0 .. F-1.
 *   State per stream, the caller's device tensors: tbox (S, T, 5) float64 [x1, y1, x2, y2, score]; tint (S, T, 4) int32 [id, class, hits,
 *   misses], id == 0: the slot is free; issued (S) int32, the number of ids handed out so far.  All zero is the empty tracker.  T = max_tracks
 *   in 1..LSFA_TRACK_MAX_TRACKS.
 *   Input for frame f of stream s: dets[s][f] (ncls, R, 5) float64 and counts[s][f] (ncls) int32 as lsfa_det_postprocess_batch leaves them,
 *   and optionally the first row_n[s][f] rows of rows + s * rows_stream_stride + f * rows_frame_stride (strides in ints), each 7 int32
 *   {.., .., .., srcx, srcy, dstx, dsty}: what lsfa_mv_estimate(_chain) writes and lsfa_mv_accumulate reads; columns 0..2 are not read.
 *   rows == NULL, row_n == NULL or row_n[s][f] <= 0: no prediction for that frame (a key frame that starts a new chain).  row_n is clamped to
 *   n_max.
 *   1. Eligible detections E, in draw order: classes j = 1 .. ncls-1 ascending (class 0 never), rows r = 0 .. min(max(counts[j], 0), R) - 1
 *      ascending; a row is eligible when all five values are finite, score >= score_thresh, x2 >= x1 and y2 >= y1 (the overlay's rule without
 *      its outside-the-frame skip).
 *   2. Predict, every active track independently: a row participates when x1 <= (double)srcx <= x2 and y1 <= (double)srcy <= y2 (content
 *      that was inside the box in the previous frame).  With c participating rows, sx = sum(dstx - srcx), sy = sum(dsty - srcy) in int64: if
 *      c > 0 and sx != 0 then dx = (double)sx / (double)c, x1 += dx, x2 += dx; likewise sy, dy, y1, y2.  Every operation is rounded once,
 *      nothing is contracted; a zero sum leaves the coordinates bit for bit; boxes are not clipped to the frame.
 *   3. Associate, each detection of E in draw order: the candidates are the active tracks of the same class that no earlier detection of
 *      this frame took, with IoU >= iou_thresh; the largest IoU wins, a tie goes to the lowest slot.  IoU is the reference's py_nms arithmetic
 *      in float64: areas (x2 - x1 + 1) * (y2 - y1 + 1), w = max(0, min(x2a, x2b) - max(x1a, x1b) + 1), h likewise, inter / (area_a + area_b
 *      - inter); min, max and >= are comparisons and a comparison with NaN is false: no match.  A matched track takes the detection's five
 *      values, hits += 1, misses = 0.
 *   4. Age: every active track that was not matched: misses += 1; if misses > max_age the slot is freed and its nine values are zeroed.
 *   5. Birth, every unmatched detection of E in draw order: it goes into the lowest free slot (slots freed in step 4 count) with
 *      id = ++issued[s], class j, the five values, hits = 1, misses = 0.  With no free slot it is dropped: counted, and no id is consumed.
 *      (hits, misses and issued are 32-bit and wrap.)
 *   6. Output: ids[s][f] (ncls, R) int32, all ncls * R entries written every frame: -1 for a row that is not eligible, the track's id when
 *      its hits >= min_hits, else 0 (tentative, or dropped); n[s][f] (4) int32 {eligible, matched, born, dropped}.
 * Out of scope: re-identification after a track died; matching across classes; appearance features; velocity models; clipping or killing
 * tracks that left the frame (ageing does that); rescoring or suppressing detections.
 * lsfa_track_steps: one launch, one workgroup per stream, the table in LDS for the F frames; no workspace, nothing allocated, no atomics,
 *   nothing read back; on `stream`, capturable; not reported under a profiling id.  Memory-safe whatever the state tensors and the rows hold:
 *   a class outside 1..ncls-1 in a slot never matches, and row values are only compared and summed.
 * LSFA_EINVAL, before anything is launched, for: a NULL pointer other than rows / row_n; S, F, R or T below 1; ncls below 1 or above 4096;
 *   T above LSFA_TRACK_MAX_TRACKS, S above 65535, F above 4096; (ncls - 1) * R at or above 2^31; n_max < 0; a negative stride; max_age < 0;
 *   min_hits < 1; a threshold that is not finite.
 * lsfa_overlay_plan_ids: lsfa_overlay_plan (the same body; that export is the ids == NULL case) for ids (N, ncls, R) int32: a row is
 *   eligible only if, in addition, ids[j][r] > 0; the record's colour field holds 1 + (id - 1) % (ncls - 1) instead of j - one stable colour per
 *   track from the same `colors` table; the label is the class name, then '-', then the decimal digits of id % 100000, then the score as before:
 *   at most 12 + 6 + 6 = 24 characters, which is what a record holds.  The paint calls are the overlay's.  LSFA_EINVAL as lsfa_overlay_plan,
 *   and for ids == NULL or ncls < 2.
 * ------------------------------------------------------------------------ */
#define LSFA_TRACK_MAX_TRACKS 1024
int lsfa_track_steps(const double* dets, const int* counts, int S, int F, int ncls, int R, const int* rows /* or NULL */,
                     const int* row_n /* (S, F) or NULL */, int n_max, long long rows_stream_stride, long long rows_frame_stride,
                     double score_thresh, double iou_thresh, int max_age, int min_hits, int T, double* tbox, int* tint, int* issued, int* ids,
                     int* n, void* stream);
int lsfa_overlay_plan_ids(const double* dets, const int* counts, const int* ids, int N, int ncls, int R, double thresh, int H, int W,
                          int thickness, int label_scale, int with_score, const unsigned char* names, int max_boxes, int* records, int* n,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* LSFA_HIP_H_ */
