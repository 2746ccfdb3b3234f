"""Every caller of iou_exceeds_fast (lsfa_amd/csrc/iou_test.h) on inputs that reach its division redo on purpose.

A pair whose d = fma(-thresh, uni, inter) falls into the sliver 0 < d < thresh * 2^-22 * uni (2^-51 in float64), a union
that is not positive, and a threshold outside the fast range make a caller redo its work with iou_exceeds_div.  The inputs
are built in tests/test_iou_sliver_cpu.py, which proves without a GPU that each holds such pairs at the stated positions,
that each pair decides a survivor, and that a sign-only fast test and a caller that never redoes compute other survivors.
Here the five call sites run them; every comparison is exact equality with the oracle.

  site                                         tests
  nms_mask_kernel<false> (whole tile redone)   test_nms_* with float32 (lsfa_nms_sorted and `_nms`)
  nms_mask_f64_kernel (per column)             test_nms_* with float64 (lsfa_nms_sorted_f64 and py_nms_wrapper)
  nms_mask_kernel<true>                        test_proposal_* under 'chip' (all tiles), 'chip-box-sweep' (diagonal tiles), 'auto'
  iou_exceeds / suppressed_by                  test_proposal_* under 'single'
  the box sweep                                test_proposal_* under 'chip-box-sweep', and 'auto' with two images
  det_class_kernel phase 3                     test_det_postprocess_*

Left uncovered, with the reason:
  * Proposal: suppressed_by's first use (a chunk of 1024 candidates against all survivors, stride 1) needs more than 1024
    candidates and is not reached; its second use (stride 16) is.  The only union that is not positive which the decode
    lets through is 0 (a negative area cannot be decoded), and float32 keeps such a pair with or without the redo.
  * det_class_kernel: a float64 suppress-side sliver from float32 rois exists at 0.7 (boxes 31000283 pixels wide, see
    tests/test_iou_sliver_cpu.py); at 0.3 two equal squares cannot give one below 4e7 pixels, and none was built.  There the
    redo's "suppress" outcome is the zero-area pair, and nms_sorted_f64 covers the sliver's.
"""
import numpy as np
import pytest
import torch

import oracle
import test_iou_sliver_cpu as sets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check_nms(hip, boxes, thresh):
    """float32: lsfa_nms_sorted and the host-pointer `_nms`; float64: lsfa_nms_sorted_f64 and py_nms_wrapper on float64 dets."""
    want = sets.oracle_keep(boxes, thresh)
    if boxes.dtype == np.float32:
        keep, num = hip.nms_sorted(t(boxes), thresh)
        np.testing.assert_array_equal(keep[:int(num.item())].cpu().numpy(), want)
        np.testing.assert_array_equal(hip.nms_host(boxes, thresh), want)
    else:
        from lsfa_amd.nms.nms import py_nms_wrapper
        keep, num = hip.nms_sorted_f64(t(boxes), thresh)
        np.testing.assert_array_equal(keep[:int(num.item())].cpu().numpy(), want)
        np.testing.assert_array_equal(np.asarray(py_nms_wrapper(thresh)(sets.with_scores(boxes)), np.int64), want)
    return want


@pytest.mark.parametrize("thresh", sets.FAST_THRESHOLDS)
@pytest.mark.parametrize("dtype", sets.DTYPES)
@pytest.mark.parametrize("n,layout", sets.NMS_SETS)
def test_nms_sliver_pairs_in_every_tile_position(hip, n, layout, dtype, thresh):
    """Sliver pairs of both outcomes in a diagonal tile, an off-diagonal tile and the partial last tile (as a column, and as
    the one pair of its own rows), among ordinary boxes that the redone tile must reproduce."""
    boxes, _ = sets.nms_set(n, layout, dtype, thresh)
    check_nms(hip, boxes, thresh)


@pytest.mark.parametrize("thresh", sets.FAST_THRESHOLDS)
@pytest.mark.parametrize("dtype", sets.DTYPES)
@pytest.mark.parametrize("kind", sorted(sets.DEGENERATE_BOX))
def test_nms_degenerate_unions(hip, kind, dtype, thresh):
    """Zero-area, negative-area and infinite boxes, two and more of each: float32 keeps the later ones (NaN > thresh is
    false; a negative quotient is not above the threshold), float64 suppresses them for a NaN quotient (numpy's rule)."""
    boxes, _ = sets.nms_degenerate_set(kind, dtype, thresh)
    want = check_nms(hip, boxes, thresh)
    assert (33 in want) == (129 in want) == (dtype == "float32" or kind == "negative")


@pytest.mark.parametrize("dtype", sets.DTYPES)
def test_nms_thresholds_outside_the_fast_range_divide_everywhere(hip, dtype):
    boxes = sets.nms_slow_set(dtype)
    for thresh in sets.SLOW_THRESHOLDS[dtype]:
        check_nms(hip, boxes, thresh)


@pytest.mark.parametrize("dtype", sets.DTYPES)
def test_nms_identical_boxes_at_thresh_one_are_all_kept(hip, dtype):
    """IoU = 1 and d == 0, which is not positive: nothing suppresses."""
    want = check_nms(hip, sets.identical_boxes(dtype), 1.0)
    assert len(want) == 130


# ---- Proposal ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cases", [("top",), ("boundary",), ("degenerate",), ("top", "boundary"), ("degenerate", "boundary")],
                         ids=lambda c: "+".join(c))
@pytest.mark.parametrize("side", sorted(sets.PROPOSAL_SIDES))
@pytest.mark.parametrize("plan", ["auto", "single", "chip", "chip-box-sweep"])
def test_proposal_sliver_pairs_under_every_plan(hip, plan, side, cases):
    """'keep': the float32 7/10 pair, decoded from a 272 x 272 anchor three cells apart.  'suppress': two 1376 x 1376 boxes
    offset by (183, 69), 1559251 / 2227501, found by a search on the CPU and confirmed through the oracle's decoded boxes
    (tests/test_iou_sliver_cpu.py).  Two pairs an image: ranked first and second; A below 64 other survivors and B a block
    further down (the box sweep's share of wave k % 16, suppressed_by's strided range); across the boundary of two
    64-candidate blocks; first block against last.  'degenerate' adds two zero-area boxes (dw = -20 with rpn_min_size = 0
    lets a zero-area decoded box through), whose union is 0 and whose quotient is NaN."""
    prob, deltas, im_info = sets.proposal_batch(side, cases)
    kw = sets.proposal_kwargs(side)
    want_rois, want_scores = oracle.proposal(prob, deltas, im_info, **kw)
    hip.proposal_set_plan(plan)
    try:
        op = hip.ProposalOp(feature_stride=kw["feature_stride"], scales=kw["scales"], ratios=kw["ratios"], threshold=kw["threshold"],
                            rpn_min_size=kw["rpn_min_size"], output_score=True)
        rois, scores = op(t(prob), t(deltas), t(im_info))
        rois, scores = rois.cpu().numpy(), scores.cpu().numpy()
    finally:
        hip.proposal_set_plan("auto")
    np.testing.assert_array_equal(rois, want_rois)
    np.testing.assert_array_equal(scores, want_scores)


# ---- detection post-processing ---------------------------------------------------------------------------------------------
def check_det(got, want):
    (dets, counts, keep_idx), (w_d, w_c, w_k) = got, want
    counts = counts.cpu().numpy()
    np.testing.assert_array_equal(counts, w_c)
    for j in range(len(w_c)):
        np.testing.assert_array_equal(keep_idx[j, :counts[j]].cpu().numpy(), w_k[j, :counts[j]])
        np.testing.assert_array_equal(dets[j, :counts[j]].cpu().numpy(), w_d[j, :counts[j]])      # zero deltas: exp(0) = 1 on both sides


@pytest.mark.parametrize("layout,thresh", sets.DET_CASES)
def test_det_postprocess_sliver_and_zero_area_pairs(hip, layout, thresh):
    """R = 70, three classes, zero deltas.  Class 1 ranks the rois in index order: the 3/10 resp. 7/10 float64 pair in the
    diagonal tile and in the off-diagonal tile (positions 0..63 against 64..69); in the 'zero_*' layouts a pair of
    zero-area rois (x2 = x1 - 1) whose second box numpy's rule suppresses; in 'suppress' (0.7 only) one 31000283-pixel box
    against two offset copies, a float64 suppress-side sliver from float32 rois.  Class 2 ranks the same boxes at random."""
    rois, deltas, probs, _ = sets.det_set(layout, thresh)
    im = sets.det_image(layout)
    want = oracle.det_postprocess(rois, deltas, probs, *im, nms_thresh=thresh, max_per_image=0)
    got = hip.det_postprocess(t(rois), t(deltas), t(probs), *im, nms_thresh=thresh, max_per_image=0)
    check_det(got, want)


@pytest.mark.parametrize("layouts,thresh", [(pair, th) for th in sets.FAST_THRESHOLDS for pair in (("sliver", "zero_off_diagonal"), ("zero_diagonal", "sliver"))]
                         + [(("suppress", "suppress"), 0.7)], ids=lambda v: "+".join(v) if isinstance(v, tuple) else str(v))
def test_det_postprocess_batch_sliver_and_zero_area_pairs(hip, layouts, thresh):
    """lsfa_det_postprocess_batch with B = 2 (one image size for both): each image equals the oracle on that image alone."""
    d = sets.DET
    R, ncls = d["R"], d["ncls"]
    im = sets.det_image(layouts[0])
    assert im == sets.det_image(layouts[1])
    imgs = [sets.det_set(layout, thresh)[:3] for layout in layouts]
    rois, deltas, probs = [np.concatenate([img[k] for img in imgs], 0) for k in range(3)]
    rois[R:, 0] = 1
    probs[R:, 1:] = probs[R:, :0:-1].copy()              # the second image ranks by the other class's scores
    out = (torch.full((2, ncls, R, 5), -7.0, dtype=torch.float64, device=DEV), torch.full((2, ncls), -7, dtype=torch.int32, device=DEV),
           torch.full((2, ncls, R), -7, dtype=torch.int32, device=DEV))
    dets, counts, keep_idx = hip.det_postprocess_batch(t(rois), t(deltas), t(probs), 2, *im, out, nms_thresh=thresh, max_per_image=0)
    for b in range(2):
        sl = slice(b * R, (b + 1) * R)
        want = oracle.det_postprocess(rois[sl], deltas[sl], probs[sl], *im, nms_thresh=thresh, max_per_image=0)
        check_det((dets[b], counts[b], keep_idx[b]), want)
