"""Real launches of the well-formed calls of tests/binding_contract.py: unusual but LEGAL arguments still give the right bits.

  * a caller's `out` comes back as that object and holds what the call that allocates its own returns;
  * an input the wrapper may copy, passed as a non-contiguous view of the same values, gives torch.equal results;
  * one anchor per operator family against the reference that family's own test uses (the CPU oracle bit for bit; float64 torch with
    that test's tolerance for the gate, the pools and the convolutions), so that the small shapes are checked against something other
    than themselves.

Every argument here is legal and 16-byte aligned; the refusals live in test_binding_contract_gpu.py, which launches nothing."""
import numpy as np
import pytest
import torch

import binding_contract as bc
import oracle
import ref64

pytestmark = pytest.mark.gpu

ROWS = {r.id: r for r in bc.ROWS}
# results that depend on what an object has seen before: a second call is not a repeat of the first
STATEFUL = ("MotionEstimator.", "MotionVectorAccumulator.add_frame")
ALLOCATED = ("out", "out_z", "sad_out")          # the buffers a wrapper allocates itself where the caller gives none
# inputs that are NOT copied: the wrapper takes them as they lie (with a rule of its own for pitched planes), or refuses a view
AS_THEY_LIE = {
    "aggregate_softmax2[_rows]": {"logits": "read in place: rows of a wider buffer, described by logit_row_stride"},
    "copy_many": {("pairs", 0, 1): "a plain copy of dense memory"},
    "transform_mv_res": {"motion_vector": "dense maps only", "res_diff": "dense maps only"},
    "image_resize_transform": {"im": "dense frames only"},
    "image_transform_u8": {"im": "dense frames only"},
    "ImageTable.set": {("images", 0): "the table holds the images' own addresses", ("images", 1): "the table holds the images' own addresses"},
    "stem_conv": {"w_l": "fragments from stem_weight_layout"},
    "stem_conv[table]": {"w_l": "fragments from stem_weight_layout"},
    "conv_pair": {"x": "a view goes to the library as a pixel pitch, which refuses it", "scale2": "dense", "shift2": "dense", "bias": "dense"},
    "luma_u8": {"bgr": "dense frames only"},
    "mv_estimate": {"luma_cur": "dense planes only", "luma_ref": "dense planes only"},
    "mv_estimate_chain": {"luma_stack": "dense frames, one stride from frame to frame"},
    "luma_pyramid": {"luma": "dense planes"},
    "mv_refine_chain": {"luma_stack": "dense frames", "parent_rows": "dense rows"},
    "mv_cut_score": {"luma_stack": "dense frames", "sad": "dense"},
    "mv_segment_inputs": {"rows": "dense rows", "bgr_stack": "dense frames"},
    "SegmentMotionEstimator.segment": {"bgr_stack": "dense frames"},
    "SegmentMotionEstimator.segment_yuv": {"y": "the estimator's own plane rule", "uv": "the estimator's own plane rule"},
}
for _v in ("nv12", "i420"):
    for _w in ("yuv420_to_bgr_u8", "image_transform_yuv420", "image_resize_transform_yuv420"):
        if _v == "i420":
            AS_THEY_LIE["%s[%s]" % (_w, _v)] = {"u": "u and v must share one pitch", "v": "u and v must share one pitch"}


def legal_rows():
    return [r for r in bc.ROWS if r.legal]


def tensors(ret):
    if isinstance(ret, torch.Tensor):
        return [ret]
    if isinstance(ret, (tuple, list)):
        return [t for e in ret for t in tensors(e)]
    return []


def n(t):
    return t.detach().cpu().numpy()


def results(r, ret):
    """the tensors a call returned, as far as they are defined: of nms_sorted's (keep, num_keep) the first num_keep entries of keep"""
    if r.name.startswith("nms_sorted"):
        keep, num = ret
        return [keep[:int(num.item())], num]
    return tensors(ret)


@pytest.fixture()
def env(hip):
    return bc.Env(fake=False)


def run(env, rid, **override):
    fn, kw = ROWS[rid].make(env)
    kw.update(override)
    return kw, fn(**kw)


@pytest.mark.parametrize("r", [r for r in legal_rows() if any(k in r.args and r.args[k].optional or (k, 0) in r.args for k in ALLOCATED)
                               and not r.name.startswith(STATEFUL)], ids=lambda r: r.id)
def test_a_given_out_is_returned_and_holds_what_the_allocating_call_returns(env, r):
    fn, kw = r.make(env)
    given = [t for k in ALLOCATED if k in kw for t in tensors(kw[k])]
    ret = tensors(fn(**kw))
    assert given and all(any(g is t for t in ret) for g in given), "%s: the caller's buffers are not what comes back" % r.id
    if r.id == "det_postprocess_batch" or not all(r.args[k].optional for k in ALLOCATED if k in r.args):
        return                                      # `out` is required: nothing allocates in its place
    drop = ALLOCATED + (("c0",) if r.id == "head_conv3x3[slice]" else ())          # (a fresh map has the head's channels alone)
    own = tensors(fn(**{k: v for k, v in kw.items() if k not in drop}))
    assert len(own) == len(ret)
    for got, want in zip(ret, own):
        if r.id == "head_conv3x3[slice]":           # channels [c0, c0 + Cout) of the caller's wider map against a fresh Cout-channel map
            got = got[..., kw["c0"]:kw["c0"] + want.shape[3]]
        assert got.dtype == want.dtype and torch.equal(got, want), r.id


def copied_inputs(r):
    lie = AS_THEY_LIE.get(r.id, {})
    return [p for p, a in r.args.items() if a.role in ("in", "vec") and p not in lie]


@pytest.mark.parametrize("r", [r for r in legal_rows() if copied_inputs(r) and not r.name.startswith(STATEFUL)], ids=lambda r: r.id)
def test_a_non_contiguous_view_of_an_input_gives_the_same_bits(env, r):
    fn, kw = r.make(env)
    base = [t.clone() for t in results(r, fn(**kw))]
    assert base or r.name in ("copy_many",)
    for path in copied_inputs(r):
        view = env.view_of_larger(bc.get(kw, path))
        assert torch.equal(view, bc.get(kw, path)) and view.data_ptr() % 16 == 0
        got = results(r, fn(**bc.put(kw, path, view)))
        assert len(got) == len(base)
        for g, b in zip(got, base):
            assert torch.equal(g, b), "%s: %s as a view of a larger buffer changes the result" % (r.id, path)


def test_every_legal_row_is_in_one_of_the_two_sweeps_or_says_why_not():
    swept = set(r.id for r in legal_rows() if not r.name.startswith(STATEFUL))
    assert len(swept) > 55
    stale = sorted(k for k in AS_THEY_LIE if k not in ROWS) + sorted("%s:%s" % (k, p) for k, v in AS_THEY_LIE.items() if k in ROWS for p in v
                                                                     if p not in ROWS[k].args)
    assert not stale, stale


# ---- anchors: the small shapes against the references of the families' own tests ---------------------------------------------------------
def test_anchor_rfcn_head_family_against_the_oracle(env):
    kw, got = run(env, "psroi_pool")
    np.testing.assert_array_equal(n(got), oracle.psroi_pool(n(kw["data"]), n(kw["rois"]), 0.0625, 2, 3, 3))
    kw, (prob, box) = run(env, "rfcn_head")
    want_prob, _, want_box = oracle.rfcn_head(n(kw["cls_map"]), n(kw["box_map"]), n(kw["rois"]), 0.0625, 3, 3)
    np.testing.assert_array_equal(n(prob), want_prob)
    np.testing.assert_array_equal(n(box), want_box)
    # the same maps as position-sensitive cells, dense and 56 floats apart with NaN in the padding
    N, H, W = 2, 5, 7
    nchw = np.concatenate([n(kw["cls_map"]).reshape(N, 2, 9, H * W), n(kw["box_map"]).reshape(N, 4, 9, H * W)], 1)
    ps = env.dev(torch.from_numpy(np.ascontiguousarray(nchw.transpose(0, 3, 2, 1)).reshape(N, H, W, 9, 6)))
    prob, box = bc.hip.rfcn_head_ps(ps, kw["rois"], 2, 4, pooled_size=3, group_size=3)
    np.testing.assert_array_equal(n(prob), want_prob)
    np.testing.assert_array_equal(n(box), want_box)
    padded = torch.full((N, H, W, 56), float("nan"), device=bc.CUDA0)
    padded[..., :54] = ps.view(N, H, W, 54)
    prob, box = bc.hip.rfcn_head_ps_ld(padded, 56, kw["rois"], H, W, 2, 4, pooled_size=3, group_size=3)
    np.testing.assert_array_equal(n(prob), want_prob)
    np.testing.assert_array_equal(n(box), want_box)


def test_anchor_warp_family_against_the_oracle(env):
    cl = lambda a: np.ascontiguousarray(a.transpose(0, 3, 1, 2))
    kw, got = run(env, "warp_bilinear")
    want = oracle.warp_bilinear(n(kw["feat"]), n(kw["flow"]), mul=n(kw["mul"]), add=n(kw["add"]), res=n(kw["res"]), res_w=n(kw["res_w"]), res_b=n(kw["res_b"]))
    np.testing.assert_array_equal(n(got), want)
    kw, got = run(env, "warp_bilinear_cl")
    want = oracle.warp_bilinear(cl(n(kw["feat_cl"])), n(kw["flow"]), add=cl(n(kw["add_cl"])), res=n(kw["res"]), res_w=n(kw["res_w"]), res_b=n(kw["res_b"]))
    np.testing.assert_array_equal(cl(n(got)), want)
    assert float(kw["amax_out"].view(torch.float32).max()) == float(np.abs(want[:, 4:]).max())
    # warp (+ res), then * scale and + shift as two float32 roundings, then + add
    for rid, feat, add, back in (("warp_bilinear[bn]", "feat", "add", lambda a: a), ("warp_bilinear_cl[bn]", "feat_cl", "add_cl", cl)):
        kw, got = run(env, rid)
        w = oracle.warp_bilinear(back(n(kw[feat])), n(kw["flow"]), res=n(kw["res"]), res_w=n(kw["res_w"]), res_b=n(kw["res_b"]))
        s, t = n(kw["bn"][0])[None, :, None, None], n(kw["bn"][1])[None, :, None, None]
        want = (((w * s).astype(np.float32) + t).astype(np.float32) + back(n(kw[add]))).astype(np.float32)
        np.testing.assert_array_equal(back(n(got)), want)


def test_anchor_gate_family_against_float64(env):
    kw, got = run(env, "channel_mean")
    x = torch.cat([kw["x1"], kw["x2"]], 3).double()
    want = x.mean((1, 2))
    # the kernel adds 12 pixels in a fixed order in float32 and divides once: (12 - 1) additions + 1 division, each within half an ulp of a
    # partial sum no larger than the sum of magnitudes
    bound = 12 * 2.0 ** -24 * x.abs().sum((1, 2)) / 12 + 1e-45
    assert bool(((got.double() - want).abs() <= bound).all())
    kw, got = run(env, "channel_gate")
    h = torch.relu(kw["m"].double() @ kw["w1"].double().T + kw["b1"].double())
    want = n(torch.sigmoid(h @ kw["w2"].double().T + kw["b2"].double()))
    ulp = np.spacing(want.astype(np.float32))
    assert (np.abs(n(got).astype(np.float64) - want) / ulp).max() <= 16                # test_gate_within_a_few_ulps_of_float64_and_batch_invariant's
    kw, got = run(env, "gate_apply")
    prod = (n(kw["x"]) * n(kw["gate"])[:, None, None, :]).astype(np.float32)
    want = (prod + n(kw["y"])).astype(np.float32)
    np.testing.assert_array_equal(n(got), want)
    assert float(kw["amax_out"].view(torch.float32).max()) == float(np.abs(want[..., 4:]).max())


def test_anchor_aggregation_family_against_the_oracle(env):
    for rid in ("aggregate_softmax2[one]", "aggregate_softmax2[_batched]"):
        kw, got = run(env, rid)
        np.testing.assert_array_equal(n(got), oracle.aggregate_softmax2(n(kw["a"]), n(kw["b"]), n(kw["logits"])))
    kw, got = run(env, "aggregate_softmax2[_rows]")
    np.testing.assert_array_equal(n(got), oracle.aggregate_softmax2(n(kw["a"]), n(kw["b"]), n(kw["logits"])[:, :35].reshape(4, 1, 5, 7)))
    kw, got = run(env, "aggregate_cosine")
    np.testing.assert_array_equal(n(got), oracle.aggregate_cosine(n(kw["a"]), n(kw["b"]), n(kw["emb_warp"]), n(kw["emb_cur"])))


def test_anchor_proposal_nms_and_detection_tail_against_the_oracle(env):
    kw, (rois, scores) = run(env, "ProposalOp.__call__")
    want_rois, want_scores = oracle.proposal(n(kw["cls_prob"]), n(kw["bbox_pred"]), n(kw["im_info"]), 16, (8,), (0.5, 1, 2), 50, 10, 0.7, 4)
    np.testing.assert_array_equal(n(rois), want_rois)
    np.testing.assert_array_equal(n(scores), want_scores)
    boxes = np.array([[0, 0, 10, 10, .9], [1, 1, 11, 11, .8], [20, 20, 30, 30, .7], [0, 0, 10, 10, .6], [21, 20, 30, 31, .5], [50, 50, 60, 60, .4]], np.float32)
    want = oracle.nms_sorted(boxes, 0.5)
    keep, num = bc.hip.nms_sorted(env.dev(torch.from_numpy(boxes)), 0.5)
    assert int(num.item()) == len(want) == 3
    np.testing.assert_array_equal(n(keep)[:len(want)], want)
    keep, num = bc.hip.nms_sorted_f64(env.dev(torch.from_numpy(boxes).double()), 0.5)
    np.testing.assert_array_equal(n(keep)[:int(num.item())], oracle.nms_f64(boxes.astype(np.float64), 0.5))
    kw, got = run(env, "bbox_pred_clip")
    # fp64 arithmetic in the same order on both sides; exp() of the two libms may differ by an ulp (test_det_postprocess_vs_oracle's tolerance)
    np.testing.assert_allclose(n(got), oracle.bbox_pred_clip(n(kw["rois"]), n(kw["deltas"]), 80, 112, 1.0), rtol=1e-12, atol=1e-9)
    kw, (dets, counts, keep_idx) = run(env, "det_postprocess")
    w_d, w_c, w_k = oracle.det_postprocess(n(kw["rois"]), n(kw["deltas"]), n(kw["probs"]), 80, 112, 1.0)
    np.testing.assert_array_equal(n(counts), w_c)
    assert w_c.sum() > 0
    for c in range(4):
        np.testing.assert_allclose(n(dets)[c, :w_c[c]], w_d[c, :w_c[c]], rtol=1e-12, atol=1e-9)
        np.testing.assert_array_equal(n(keep_idx)[c, :w_c[c]], w_k[c, :w_c[c]])
    kw, (dets, counts, keep_idx) = run(env, "det_postprocess_batch")
    for b in range(2):
        sl = slice(3 * b, 3 * b + 3)
        w_d, w_c, w_k = oracle.det_postprocess(n(kw["rois"])[sl], n(kw["deltas"])[sl], n(kw["probs"])[sl], 80, 112, 1.0)
        np.testing.assert_array_equal(n(counts)[b], w_c)
        for c in range(4):
            np.testing.assert_allclose(n(dets)[b, c, :w_c[c]], w_d[c, :w_c[c]], rtol=1e-12, atol=1e-9)
            np.testing.assert_array_equal(n(keep_idx)[b, c, :w_c[c]], w_k[c, :w_c[c]])


def test_anchor_deformable_im2col_and_affine_activations_against_the_oracle(env):
    kw, got = run(env, "deform_im2col")
    want = oracle.deform_im2col(n(kw["data"]), n(kw["offset"]), 3, 3, 1, 1, 1, 2)
    np.testing.assert_array_equal(n(got), want)
    kw, got = run(env, "deform_im2col_cl")
    want = oracle.deform_im2col(n(kw["data"]).transpose(0, 3, 1, 2), n(kw["offset"]).transpose(0, 3, 1, 2), 3, 3, 1, 1, 1, 2)
    np.testing.assert_array_equal(n(got), want.reshape(2, 8, 9, 42).transpose(0, 3, 2, 1).reshape(2, 42, 72))
    kw, got = run(env, "scale_shift_relu")
    np.testing.assert_array_equal(n(got), oracle.scale_shift_relu(n(kw["x"]), n(kw["scale"]), n(kw["shift"]), True))
    kw, got = run(env, "scale_shift_leaky")
    np.testing.assert_array_equal(n(got), oracle.scale_shift_leaky(n(kw["x"]), n(kw["scale"]), n(kw["shift"]), 0.1))
    kw, got = run(env, "scale_shift_relu_cl")
    np.testing.assert_array_equal(n(got), oracle.scale_shift_relu(n(kw["x"]).reshape(70, 8, 1), n(kw["scale"]), n(kw["shift"]), True).reshape(2, 5, 7, 8))


def test_anchor_pools_against_float64(env):
    import torch.nn.functional as F
    for rid in ("avgpool_nchw", "avgpool_nchw[table]"):
        kw, got = run(env, rid)
        x = kw["x"].materialize() if rid.endswith("[table]") else kw["x"]
        want = F.avg_pool2d(x.double(), 2, 2, ceil_mode=True)
        assert got.shape == want.shape and float((got.double() - want).abs().max()) < 1e-4     # test_avgpool_nchw_vs_torch_ceil_mode's
    kw, got = run(env, "avgpool2_nhwc")
    np.testing.assert_array_equal(n(got).view(np.uint32), ref64.avgpool2_full_f32_in_order(n(kw["x"])).view(np.uint32))
    kw, (p1, p2) = run(env, "maxpool3x3s2_nhwc")
    want = ref64.maxpool3x3s2_pad1_ref(n(kw["x"]))
    np.testing.assert_array_equal(n(p1).view(np.uint32), want.view(np.uint32))
    want2 = np.maximum(want * n(kw["scale2"]) + n(kw["shift2"]), np.float32(0))
    np.testing.assert_array_equal(n(p2), want2)
    assert float(kw["amax_out"].view(torch.float32).max()) == float(want2.max())
    kw, got = run(env, "nchw_to_nhwc")
    np.testing.assert_array_equal(n(got).view(np.uint32), ref64.nchw_slice_to_nhwc_ref(n(kw["x"]), 4, 4).view(np.uint32))


def test_anchor_convolutions_against_float64(env):
    """test_conv_nhwc_mfma_vs_torch's and test_conv_split_vs_float64_and_fp32_mfma's bound: 2e-6 * sqrt(K) of the output's scale"""
    import torch.nn.functional as F
    hip = bc.hip

    def conv64(x, w, b, pad):
        return F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), 1, pad, 1).permute(0, 2, 3, 1)

    def close(got, want, K):
        return float((got.double() - want).abs().max()) < 2e-6 * np.sqrt(K) * max(float(want.abs().max()), 1.0)
    x, w, b = env.f32(1, 5, 6, 32), env.f32(64, 32, 3, 3, lo=-0.1, hi=0.1), env.f32(64)
    res = env.f32(1, 5, 6, 64)
    want = torch.relu(conv64(x, w, b, 1) + res.double())
    got = hip.conv_nhwc(x, hip.conv_weight_kc(w), b, 3, 3, pad=1, relu=True, residual=res)
    assert close(got, want, 288)
    for pieces in (3, 2, 0):
        status = hip.new_status(bc.CUDA0)
        got = hip.conv_split(x, hip.SplitWeight(w, pieces=pieces), b, pad=1, relu=True, residual=res, amax_in=hip.amax_partial(x), status=status)
        hip.check_status(status)
        assert close(got, want, 288), pieces
    # between views of wider maps: channels [32, 64) of x2 into channels [64, 128) of a 128-channel map, LeakyReLU(0.1)
    x2 = torch.cat([env.f32(1, 5, 6, 32), x], 3).contiguous()
    wide = hip.zeros_f32((1, 5, 6, 128), bc.CUDA0)
    hip.conv_split_view(x2, hip.SplitWeight(w), b, wide, pad=(1, 1), act=2, c0=64, cin0=32)
    y = conv64(x, w, b, 1)
    assert close(wide[..., 64:], torch.where(y > 0, y, y * 0.1), 288) and not wide[..., :64].any()
    # conv3 + shortcut and the next conv1 in one launch against conv_split twice (test_conv_pair_gpu's reference: the same bits)
    kw, (yp, zp) = run(env, "conv_pair")
    y_ref = hip.conv_split(kw["x"], kw["sw3"], None, residual=kw["residual"], amax_in=kw["amax_in"])
    assert torch.equal(yp, y_ref)
