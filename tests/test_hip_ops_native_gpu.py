"""The HIP kernels of the detection tail and the motion-vector accumulator against the reference's own native code.

tests/golden/ref_native.npz holds what the reference's PSROIPoolForwardKernel, MultiProposal kernels and
create_and_load_mv_residual compute when compiled for the host from the reference tree itself
(oracle/ref_native, tests/golden/make_native_golden.py).  Each HIP path is compared with those numbers directly,
not through the oracle, and every comparison is exact equality.  The reference tree is not needed here.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PSROI_SETS = ["net", "g3", "p6g3"]
PROPOSAL_CASES = [("a", "a"), ("b", "b"), ("c07", "c"), ("c03", "c")]       # outputs, inputs
PLANS = ["single", "chip", "chip-box-sweep"]
MV_SIZES = ["37x23", "96x64"]


@pytest.fixture(scope="module")
def native():
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_native.npz"))


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("name", PSROI_SETS)
def test_psroi_pool_is_the_references(hip, native, name):
    scale, D, P, G = native["psroi_%s_params" % name]
    data, rois = native["psroi_%s_data" % name].astype(np.float32), native["psroi_%s_rois" % name]
    got, got_mc = hip.psroi_pool(t(data), t(rois), float(scale), int(D), int(P), int(G), with_mapping=True)
    np.testing.assert_array_equal(got.cpu().numpy(), native["psroi_%s_out" % name])
    np.testing.assert_array_equal(got_mc.cpu().numpy(), native["psroi_%s_map" % name].astype(np.float32))


def bin_mean(bins):
    """(R, D, P, P) float32 -> (R, D): the bins summed in (ph, pw) order in float32, then divided by P*P
    (Pooling global_pool avg, resnet_v1_101_flownet_rfcn.py:535-536)."""
    R, D, P, _ = bins.shape
    flat = bins.reshape(R, D, P * P)
    total = np.zeros((R, D), np.float32)
    for k in range(P * P):
        total = total + flat[:, :, k]
    assert total.dtype == np.float32
    return total / np.float32(P * P)


@pytest.mark.parametrize("layout", ["nchw", "position-sensitive"])
def test_fused_heads_are_the_mean_of_the_references_bins(hip, native, layout):
    """lsfa_rfcn_head_fwd / lsfa_rfcn_head_ps_fwd on the network's parameter set: the map's 5 output channels are
    3 classes + 2 box dims (contiguous in ctop); cls_score and bbox_pred are the mean of the reference's bins."""
    scale, D, P, G = native["psroi_net_params"]
    assert (scale, D, P, G) == (0.0625, 5, 7, 7)
    ncls, nbox, gg = 3, 2, 49
    data, rois = native["psroi_net_data"].astype(np.float32), native["psroi_net_rois"]
    want = bin_mean(native["psroi_net_out"])
    if layout == "nchw":
        cls_map, box_map = data[:, :ncls * gg], data[:, ncls * gg:]
        _, score, box = hip.rfcn_head(t(cls_map), t(box_map), t(rois), want_score=True)
    else:
        N, _, H, W = data.shape
        ps = data.reshape(N, ncls + nbox, gg, H, W).transpose(0, 3, 4, 2, 1)          # (N, H, W, 49, D)
        _, score, box = hip.rfcn_head_ps(t(ps), t(rois), ncls, nbox, want_score=True)
    np.testing.assert_array_equal(score.cpu().numpy(), want[:, :ncls])
    np.testing.assert_array_equal(box.cpu().numpy(), want[:, ncls:])


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("name,inputs", PROPOSAL_CASES)
def test_proposal_is_the_references(hip, native, name, inputs, plan):
    min_size, pre, post, threshold = native["prop_%s_params" % name]
    prob, deltas, im_info = [native["prop_%s_%s" % (inputs, k)] for k in ("prob", "deltas", "im_info")]
    op = hip.ProposalOp(rpn_pre_nms_top_n=int(pre), rpn_post_nms_top_n=int(post), threshold=float(threshold),
                        rpn_min_size=int(min_size), output_score=True)
    hip.proposal_set_plan(plan)
    try:
        rois, scores = op(t(prob), t(deltas), t(im_info))
        rois, scores = rois.cpu().numpy(), scores.cpu().numpy()
    finally:
        hip.proposal_set_plan('auto')
    np.testing.assert_array_equal(rois, native["prop_%s_rois" % name])
    np.testing.assert_array_equal(scores, native["prop_%s_scores" % name])


@pytest.mark.parametrize("area", ["given", "from-rows"])
@pytest.mark.parametrize("size", MV_SIZES)
def test_mv_accumulation_is_the_references(hip, native, size, area):
    width, height = [int(v) for v in size.split("x")]
    rows, counts = native["mv_%s_rows" % size], native["mv_%s_counts" % size]
    max_area = int((rows[:, 1].astype(np.int64) * rows[:, 2]).max()) if area == "given" else None
    acc = hip.MotionVectorAccumulator(width, height, DEV)
    end = 0
    for f, n in enumerate(counts):
        frame, end = rows[end:end + n], end + n
        acc.add_frame(torch.from_numpy(np.ascontiguousarray(frame)), max_block_area=max_area)
        np.testing.assert_array_equal(acc.accu.cpu().numpy(), native["mv_%s_accu" % size][f], err_msg="frame %d" % f)
    np.testing.assert_array_equal(acc.motion_vectors().cpu().numpy(), native["mv_%s_mv" % size])
    bgr = native["mv_%s_bgr" % size]
    res = acc.residual(torch.from_numpy(bgr[1]), torch.from_numpy(bgr[0]))
    np.testing.assert_array_equal(res.cpu().numpy(), native["mv_%s_res" % size])
