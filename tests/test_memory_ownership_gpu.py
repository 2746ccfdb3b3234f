"""No result may depend on memory a call does not own (tests/guarded_arena.py on the GPU).

Every legal row of tests/binding_contract.py, and every row of RAGGED below, is called three times: on ordinary tensors, and with every
tensor it is given and every tensor the wrapper allocates placed between bands of 0xFF, then of 0x7F.  Asserted: the bands are intact
after both guarded calls (no store outside a tensor), the defined results of the three calls are torch.equal with dtype and shape (no
read outside an input, no output element left unwritten, no dependence on what a workspace held), and a status word the call used
stays clear.  The tensors a call is GIVEN are part of its results: an input comes back as it went in, and the channels of a wide map
outside the call's slice stay as they were."""
import os

import numpy as np
import pytest
import torch

import binding_contract as bc
import guarded_arena as ga
import test_binding_legal_gpu as legal

pytestmark = pytest.mark.gpu

# ---- what the header leaves undefined -------------------------------------------------------------------------------------------------------
# (wrapper, region, where include/lsfa_hip.h says so, returned tensors -> the defined part of them).  No entry names a whole output.
UNDEFINED = [
    ("nms_sorted", "keep[num_keep:]", "include/lsfa_hip.h:220", lambda r, ret: legal.results(r, ret)),
    ("nms_sorted_f64", "keep[num_keep:]", "include/lsfa_hip.h:220 (the same sweep, :226)", lambda r, ret: legal.results(r, ret)),
]


def defined(r, kw, ret):
    for wrapper, _, _, part in UNDEFINED:
        if r.name == wrapper:
            ret = part(r, ret)
    return ga.everything(r, kw, ret)


def three_way(r):
    """the three calls of row r -> the number of result tensors compared"""
    plain = ga.run_plain(r, defined)
    assert plain, "%s: nothing to compare" % r.id
    for pattern in ga.PATTERNS:
        got = ga.run_guarded(r, pattern, defined)
        assert len(got) == len(plain), r.id
        for i, (g, p) in enumerate(zip(got, plain)):
            assert g.dtype == p.dtype and g.shape == p.shape, "%s: result %d is %s %s, unguarded %s %s" % (r.id, i, g.dtype, tuple(g.shape), p.dtype, tuple(p.shape))
            if not torch.equal(g, p):
                diff = (g != p).reshape(-1).nonzero().view(-1)
                raise AssertionError("%s: result %d %s %s differs from the unguarded call under pattern 0x%02X in %d element(s), the first at flat index %d "
                                     "(%r, unguarded %r)" % (r.id, i, tuple(g.shape), g.dtype, pattern, diff.numel(), int(diff[0]),
                                                             g.reshape(-1)[diff[0]].item(), p.reshape(-1)[diff[0]].item()))
    return len(plain)


@pytest.mark.parametrize("r", legal.legal_rows(), ids=lambda r: r.id)
def test_a_table_row_owns_its_memory(hip, r):
    three_way(r)


def test_the_table_has_its_75_legal_rows_and_the_exemptions_name_no_whole_output():
    assert len(legal.legal_rows()) == 75
    for wrapper, region, where, _ in UNDEFINED:
        assert wrapper in set(r.name for r in bc.ROWS) | set(r.name for r in RAGGED) and "[" in region and where.startswith("include/lsfa_hip.h:")


# ---- RAGGED: the smallest shapes that reach the paths the table's minimal shapes do not ------------------------------------------------------------
RAGGED = []
# Each row is table-shaped: make(env) -> (callable, kwargs); the values come from env.  A callable that needs a process-wide switch (a
# forced convolution plan, a warp variant, a Proposal plan) sets it and resets it in `finally`.
hip = bc.hip
_sw = bc._sw


class Ragged(object):
    def __init__(self, rid, name, make):
        self.id, self.name, self.make = rid, name, make


def ragged(rid, name=None):
    def deco(make):
        RAGGED.append(Ragged(rid, name or rid.split("[")[0], make))
        return make
    return deco


def under_plan(plan, fn):
    """fn under lsfa_conv_plan_override(*plan), the override reset whatever happens"""
    def call(**kw):
        hip.conv_plan_override(*plan)
        try:
            return fn(**kw)
        finally:
            hip.conv_plan_override()
    return call


# ---- ring convolution: 598 pixels, 128-pixel tiles that straddle the two images, a partial last tile ----------------------------------------------
def _ring_row(pieces, plan, nchw):
    def make(env):
        N, H, W, Cin, Cout = 2, 13, 23, 64, 256
        maps = (N, Cout, H, W) if nchw else (N, H, W, Cout)
        kw = dict(x=env.f32(N, H, W, Cin), sw=_sw(env, Cout, Cin, 3, pieces), bias=env.f32(Cout), pad=1, relu=True, out=env.zeros(*maps),
                  residual=env.f32(*maps), out2=env.zeros(*maps), scale2=env.f32(Cout, lo=0.5, hi=1.5), shift2=env.f32(Cout), nchw=nchw,
                  amax_in=env.amax_in(), amax_out=env.amax(), status=env.status())
        return under_plan(plan, hip.conv_split), kw
    RAGGED.append(Ragged("conv_split[ring-p%d-k%d-nt%d-s%d-%s]" % (pieces, plan[0], plan[1], plan[3], "nchw" if nchw else "cl"), "conv_split", make))


for _pieces in (1, 2, 3):
    for _plan in [(k, nt, 0, s) for k in (1, 2) for nt in (2, 4) for s in (1, 3)] + ([(4, 4, 0, 1), (4, 4, 0, 3)] if _pieces < 3 else []):
        for _nchw in (False, True):
            _ring_row(_pieces, _plan, _nchw)


# ---- the input's activation at the cut ------------------------------------------------------------------------------------------------------
def _cut_row(pieces, slices):
    def make(env):
        kw = dict(x=env.f32(2, 14, 22, 512), sw=_sw(env, 128, 512, 1, pieces), bias=env.f32(128), stride=2, relu=True, in_scale=env.f32(512, lo=0.5, hi=1.5),
                  in_shift=env.f32(512), amax_in=env.amax_in(), amax_out=env.amax(), status=env.status())
        return under_plan((0, 0, 0, slices), hip.conv_split), kw
    RAGGED.append(Ragged("conv_split[cut-p%d-s%d]" % (pieces, slices), "conv_split", make))


for _pieces in (1, 2):
    for _slices in (1, 3):
        _cut_row(_pieces, _slices)


# ---- the direct kernel: 35 pixels, a partial 32-pixel tile, 27 chunks of K -----------------------------------------------------------------------
def _small_map_row(pieces):
    """three bf16 pieces of 27 x 32 channels are more than the direct kernel's 256 KB per 64 output channels: that one takes the ring kernel"""
    def make(env):
        return hip.conv_split, dict(x=env.f32(1, 5, 7, 96), sw=_sw(env, 64, 96, 3, pieces), bias=env.f32(64), pad=1, act=2, out=env.zeros(1, 5, 7, 64),
                                    residual=env.f32(1, 5, 7, 64), amax_in=env.amax_in(), amax_out=env.amax(), status=env.status())
    RAGGED.append(Ragged("conv_split[%s-3x3-p%d]" % ("ring-35-pixels" if pieces == 3 else "direct", pieces), "conv_split", make))


for _pieces in (1, 2, 3):
    _small_map_row(_pieces)


@ragged("conv_split[direct-3x3-nchw-out2]")
def _(env):
    return hip.conv_split, dict(x=env.f32(1, 5, 7, 96), sw=_sw(env, 64, 96, 3, 2), bias=env.f32(64), pad=1, relu=True, nchw=True, residual=env.f32(1, 64, 5, 7),
                                out2=env.zeros(1, 64, 5, 7), scale2=env.f32(64, lo=0.5, hi=1.5), shift2=env.f32(64), amax_in=env.amax_in(),
                                amax_out=env.amax(), status=env.status())


@ragged("conv_split[direct-1x1-x_nchw]")
def _(env):
    return hip.conv_split, dict(x=env.f32(1, 100, 5, 7), sw=_sw(env, 64, 96, 1, 3), bias=env.f32(64), x_nchw=True, status=hip.new_status(bc.CUDA0))


# ---- views of wider maps and the four-phase transposed convolution -------------------------------------------------------------------------------
@ragged("conv_split_view[slice-of-416]")
def _(env):
    return hip.conv_split_view, dict(x=env.f32(1, 10, 16, 128), sw=_sw(env, 128, 96, 3, 3), bias=env.f32(128), out=env.f32(1, 10, 16, 416), pad=(1, 1), act=2,
                                     c0=256, cin0=32, amax_in=env.amax_in(), amax_out=env.amax(), status=env.status())


@ragged("conv_split_view[phase-placed]")
def _(env):
    return hip.conv_split_view, dict(x=env.f32(1, 10, 16, 96), sw=_sw(env, 128, 96, 2, 3), bias=env.f32(128), out=env.f32(1, 19, 32, 416), pad=(0, 0), act=2,
                                     c0=256, grid=(9, 15), place=(1, 1, 2, 2), amax_in=env.amax_in(), amax_out=env.amax(), status=env.status())


def _deconv_row(cin, cout, lout, c0, pieces):
    def make(env):
        sw4 = hip.deconv_phase_weights(env.f32(cin, cout, 4, 4, lo=-0.05, hi=0.05), pieces=pieces)
        return hip.deconv4x4s2_crop, dict(x=env.f32(1, 10, 16, cin), sw4=sw4, bias=env.f32(cout), out=env.f32(1, 19, 32, lout), c0=c0, act=2,
                                          amax_in=env.amax_in(), amax_out=env.amax(), status=env.status())
    RAGGED.append(Ragged("deconv4x4s2_crop[%d-%d-p%d]" % (cin, cout, pieces), "deconv4x4s2_crop", make))


for _pieces in (3, 2, 1):
    _deconv_row(96, 128, 416, 256, _pieces)
_deconv_row(1056, 256, 800, 512, 3)
_deconv_row(1056, 256, 800, 512, 1)


# ---- conv_pair: 198 pixels in 128-pixel tiles (the second partial, the first across two images), Cm = Cn = 64 the smallest it takes ----------------
@ragged("conv_pair[198-pixels]")
def _(env):
    return hip.conv_pair, dict(x=env.f32(2, 9, 11, 64), sw3=_sw(env, 256, 64, 1, 2), residual=env.f32(2, 9, 11, 256), scale2=env.f32(256, lo=0.5, hi=1.5),
                               shift2=env.f32(256), sw1=_sw(env, 64, 256, 1, 2), bias=env.f32(64), out=env.zeros(2, 9, 11, 256), out_z=env.zeros(2, 9, 11, 64),
                               amax_in=env.amax_in(), amax_out_sum=env.amax(), amax_out_z=env.amax(), status=env.status())


@ragged("conv_pair[198-pixels-own-outputs-128]")
def _(env):
    return hip.conv_pair, dict(x=env.f32(2, 9, 11, 128), sw3=_sw(env, 512, 128, 1, 2), residual=env.f32(2, 9, 11, 512), scale2=env.f32(512, lo=0.5, hi=1.5),
                               shift2=env.f32(512), sw1=_sw(env, 128, 512, 1, 2))


@ragged("conv_nhwc[19x11]")
def _(env):
    return hip.conv_nhwc, dict(x=env.f32(1, 19, 11, 64), w_kc=env.f32(64, 9, 64, lo=-0.1, hi=0.1), bias=env.f32(64), kh=3, kw=3, pad=1, relu=True,
                               residual=env.f32(1, 19, 11, 64), out2=env.zeros(1, 19, 11, 64), scale2=env.f32(64), shift2=env.f32(64))


# ---- stem and pools ---------------------------------------------------------------------------------------------------------------------------
def _stem_row(n, h, w, affine):
    def fn(x, w_l, bias, in_scale, in_shift, scale2, shift2):
        """the stem, its accumulate-in-place pass on the same map, then the pool with its second output"""
        amax = hip.amax_slots(3, x.device)
        y = hip.stem_conv(x, w_l, bias, in_scale=in_scale, in_shift=in_shift, act=0, amax_out=amax[0])
        first = y.clone()
        hip.stem_conv(x, w_l, None, in_scale=in_scale, in_shift=in_shift, out=y, accum=y, act=2, amax_out=amax[1])
        return first, y, hip.maxpool3x3s2_nhwc(y, scale2=scale2, shift2=shift2, amax_out=amax[2]), amax

    def make(env):
        w_l = hip.stem_weight_layout(env.f32(64, 3, 7, 7, lo=-0.1, hi=0.1))
        return fn, dict(x=env.f32(n, 3, h, w, lo=0, hi=255), w_l=w_l, bias=env.f32(64), in_scale=env.f32(3, lo=0.5, hi=1.5) if affine else None,
                        in_shift=env.f32(3) if affine else None, scale2=env.f32(64), shift2=env.f32(64))
    RAGGED.append(Ragged("stem_conv[%dx%dx%d%s]" % (n, h, w, "-in_scale" if affine else ""), "stem_conv", make))


for _shape in ((3, 71, 131), (1, 9, 8)):
    for _affine in (False, True):
        _stem_row(*_shape, _affine)


@ragged("avgpool_nchw[1x5x9x7]")
def _(env):
    return hip.avgpool_nchw, dict(x=env.f32(1, 5, 9, 7), k=2)


@ragged("avgpool2_nhwc[odd]")
def _(env):
    return hip.avgpool2_nhwc, dict(x=env.f32(2, 5, 7, 12))


# ---- deformable im2col: taps that leave the map on every side --------------------------------------------------------------------------------------
def _dcn_row(C, dg, cl):
    def make(env):
        N, H, W, Ho, Wo = 2, 9, 11, 5, 6
        off = bc.plain(env.f32(N, Ho, Wo, 18 * dg, lo=-2, hi=2)).clone()
        off[:, 2] *= 8
        data = env.f32(N, H, W, C)
        if cl:
            return hip.deform_im2col_cl, dict(data=data, offset=env.dev(off), kh=3, kw=3, pad=1, stride=2, dilate=1, deform_groups=dg)
        return hip.deform_im2col, dict(data=env.dev(bc.plain(data).permute(0, 3, 1, 2)), offset=env.dev(off.permute(0, 3, 1, 2)), kh=3, kw=3, pad=1, stride=2,
                                       dilate=1, deform_groups=dg)
    name = "deform_im2col_cl" if cl else "deform_im2col"
    RAGGED.append(Ragged("%s[C%d-dg%d]" % (name, C, dg), name, make))


for _c, _dg in ((12, 1), (32, 4)):
    for _cl in (True, False):
        _dcn_row(_c, _dg, _cl)


# ---- warp: the operand sets and shapes of test_hip_ops.py's staged / misaligned / large-flow tests ---------------------------------------------------
def with_warp_variant(variant, fn):
    def call(**kw):
        hip.warp_set_variant(variant)
        try:
            return fn(**kw)
        finally:
            hip.warp_set_variant("auto")
    return call


def _warp_row(case, variant):
    def make(env):
        H, W = {"45x80": (45, 80), "26x40": (26, 40)}.get(case, (38, 63))
        N, C = (3, 40) if case in ("broadcast", "45x80", "26x40") else (2, 24)
        flow = bc.plain(env.f32(N, 2, H, W, lo=-2.8, hi=2.8)).clone()
        if case == "border":
            flow = bc.plain(env.f32(N, 2, H, W, lo=-70, hi=70)).clone()
            flow[0, :, 0, :7], flow[1, :, -1, -7:] = 1e9, -1e9
            flow[0, 0, 5, :], flow[0, 1, :, 9] = -1.5, 1.25
        kw = dict(feat=env.f32(1 if case == "broadcast" else N, C, H, W), flow=env.dev(flow))
        if case in ("key", "mul+add+res4", "broadcast"):
            kw["mul"] = env.f32(N, C, H, W, lo=0.9, hi=1.1)
        if case in ("cur", "mul+add+res4", "border", "in-place", "45x80", "26x40"):
            kw["add"] = env.f32(N, C, H, W)
        if case in ("cur", "mul+add+res4", "border", "45x80"):
            rc = 4 if case == "mul+add+res4" else 3
            kw.update(res=env.f32(N, rc, H, W, lo=-4, hi=4), res_w=env.f32(C, rc, 1, 1, lo=-0.01, hi=0.01), res_b=env.f32(C, lo=-0.01, hi=0.01))
        if case == "in-place":
            kw["out"] = kw["add"]
        return with_warp_variant(variant, hip.warp_bilinear), kw
    RAGGED.append(Ragged("warp_bilinear[%s-%s]" % (case, variant), "warp_bilinear", make))


for _case in ("plain", "key", "cur", "mul+add+res4", "border", "broadcast", "in-place", "45x80", "26x40"):
    for _variant in ("staged", "gather"):
        _warp_row(_case, _variant)


@ragged("warp_bilinear[misaligned]")
def _(env):
    """6 x 8 planes ask for float4 accesses; `out` and `add` start 4 bytes past a 16-byte boundary"""
    N, C, H, W = 2, 8, 6, 8
    off4 = lambda t: t.reshape(-1)[1:].view(N, C, H, W)
    flow = bc.plain(env.f32(N, 2, H, W, lo=-2.5, hi=2.5)).clone()
    flow[:, 1, 0] = -4.0
    return with_warp_variant("gather", hip.warp_bilinear), dict(
        feat=env.f32(N, C, H, W), flow=env.dev(flow), add=off4(env.f32(N * C * H * W + 1)), out=off4(env.zeros(N * C * H * W + 1)),
        res=env.f32(N, 3, H, W), res_w=env.f32(C, 3, 1, 1), res_b=env.f32(C))


@ragged("warp_bilinear[large-flow]")
def _(env):
    flow = bc.plain(env.f32(1, 2, 38, 63, lo=-80, hi=80)).clone()
    flow[0, :, 0, :5], flow[0, :, 1, :5] = 1e9, -1e9
    return hip.warp_bilinear, dict(feat=env.f32(1, 8, 38, 63), flow=env.dev(flow))


@ragged("warp_bilinear[32-maps]")
def _(env):
    return hip.warp_bilinear, dict(feat=env.f32(32, 8, 5, 6), flow=env.f32(32, 2, 5, 6, lo=-4, hi=4), add=env.f32(32, 8, 5, 6))


@ragged("warp_bilinear_cl[32-maps]")
def _(env):
    return hip.warp_bilinear_cl, dict(feat_cl=env.f32(1, 5, 6, 8), flow=env.f32(32, 2, 5, 6, lo=-4, hi=4), add_cl=env.f32(32, 5, 6, 8), amax_out=env.amax(),
                                      amax_c0=4)


# ---- heads: the three PSROI parameter sets of tests/golden/ref_native.npz (ROIs outside the map, inverted, degenerate) -------------------------------
_native = {}


def native():
    if not _native:
        _native.update(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_native.npz")))
    return _native


def _head_rows(name):
    def operands(env):
        z = native()
        scale, D, P, G = z["psroi_%s_params" % name]
        data = torch.from_numpy(z["psroi_%s_data" % name].astype(np.float32))
        return float(scale), int(D), int(P), int(G), data, env.dev(torch.from_numpy(z["psroi_%s_rois" % name]))

    def pool(env):
        scale, D, P, G, data, rois = operands(env)
        return hip.psroi_pool, dict(data=env.dev(data), rois=rois, spatial_scale=scale, output_dim=D, pooled_size=P, group_size=G, with_mapping=True)

    def head(env):
        scale, D, P, G, data, rois = operands(env)
        return hip.rfcn_head, dict(cls_map=env.dev(data), box_map=env.f32(2, 4 * G * G, 10, 13), rois=rois, spatial_scale=scale, pooled_size=P, group_size=G,
                                   want_score=True)

    def head_ps(env):
        scale, D, P, G, data, rois = operands(env)
        maps = torch.cat([data.view(2, D, G * G, 10, 13), bc.plain(env.f32(2, 4, G * G, 10, 13)).cpu()], 1)          # (N, D + 4, G^2, H, W)
        return hip.rfcn_head_ps, dict(ps_map=env.dev(maps.permute(0, 3, 4, 2, 1)), rois=rois, ncls=D, nbox=4, spatial_scale=scale, pooled_size=P,
                                      group_size=G, want_score=True)
    for wrapper, make in (("psroi_pool", pool), ("rfcn_head", head), ("rfcn_head_ps", head_ps)):
        RAGGED.append(Ragged("%s[%s]" % (wrapper, name), wrapper, make))


for _name in ("net", "g3", "p6g3"):
    _head_rows(_name)


# ---- proposal, NMS, detection tail ---------------------------------------------------------------------------------------------------------------
def _sorted_boxes(env, n, dtype):
    b = bc.plain(env.f32(n, 5, lo=0, hi=40)).clone()
    b[:, 2:4] = b[:, :2] + b[:, 2:4] / 2 + 1
    b[:, 4] = torch.linspace(0.99, 0.01, n)
    return env.dev(b.to(dtype))


for _n in (1, 64, 65, 129):
    ragged("nms_sorted[%d]" % _n)(lambda env, n=_n: (hip.nms_sorted, dict(boxes=_sorted_boxes(env, n, torch.float32), thresh=0.5)))
    ragged("nms_sorted_f64[%d]" % _n)(lambda env, n=_n: (hip.nms_sorted_f64, dict(boxes=_sorted_boxes(env, n, torch.float64), thresh=0.5)))


def _proposal_row(plan):
    def make(env):
        # 105 anchors per image: pre_nms_top_n above them, post_nms_top_n above what survives the suppression (the rest is the cyclic pad)
        op = hip.ProposalOp(feature_stride=16, scales=(8,), ratios=(0.5, 1, 2), rpn_pre_nms_top_n=200, rpn_post_nms_top_n=150, rpn_min_size=4, output_score=True)

        def call(**kw):
            hip.proposal_set_plan(plan)
            try:
                return op(**kw)
            finally:
                hip.proposal_set_plan("auto")
        im_info = env.dev(torch.tensor([[80.0, 112.0, 1.0], [80.0, 112.0, 1.0]]))
        return call, dict(cls_prob=env.f32(2, 6, 5, 7, lo=0, hi=1), bbox_pred=env.f32(2, 12, 5, 7, lo=-0.2, hi=0.2), im_info=im_info)
    RAGGED.append(Ragged("ProposalOp.__call__[%s]" % plan, "ProposalOp.__call__", make))


for _plan in ("auto", "single", "chip", "chip-box-sweep"):
    _proposal_row(_plan)


@ragged("det_postprocess[70-rois-cap-10]")
def _(env):
    return hip.det_postprocess, dict(rois=env.rois(70, 1, 112, 80), deltas=env.f32(70, 8, lo=-0.2, hi=0.2), probs=env.f32(70, 4, lo=0, hi=1), im_h=80, im_w=112,
                                     scale=1.0, max_per_image=10)


@ragged("det_postprocess_batch[70-rois-cap-10]")
def _(env):
    return hip.det_postprocess_batch, dict(rois=env.rois(140, 1, 112, 80), deltas=env.f32(140, 8, lo=-0.2, hi=0.2), probs=env.f32(140, 4, lo=0, hi=1), B=2,
                                           im_h=80, im_w=112, scale=1.0, max_per_image=10,
                                           out=(env.zeros(2, 4, 70, 5, dtype=torch.float64), env.zeros(2, 4, dtype=torch.int32),
                                                env.dev(torch.full((2, 4, 70), -1, dtype=torch.int32))))


# ---- aggregation and gate ------------------------------------------------------------------------------------------------------------------------
@ragged("aggregate_softmax2[one-C12]")
def _(env):
    return hip.aggregate_softmax2, dict(a=env.f32(1, 12, 5, 7), b=env.f32(1, 12, 5, 7), logits=env.f32(2, 1, 5, 7, lo=-3, hi=3))


@ragged("aggregate_softmax2[batched-C12]")
def _(env):
    return hip.aggregate_softmax2, dict(a=env.f32(3, 12, 5, 7), b=env.f32(3, 12, 5, 7), logits=env.f32(6, 1, 5, 7, lo=-3, hi=3))


@ragged("aggregate_softmax2[rows-C12]")
def _(env):
    # rows of 35 logits 40 floats apart; the buffer ends with the last row
    return hip.aggregate_softmax2, dict(a=env.f32(3, 12, 5, 7), b=env.f32(3, 12, 5, 7), logits=env.f32(5 * 40 + 35, lo=-3, hi=3), logit_row_stride=40)


@ragged("aggregate_cosine[C12]")
def _(env):
    return hip.aggregate_cosine, dict(a=env.f32(1, 12, 5, 7), b=env.f32(1, 12, 5, 7), emb_warp=env.f32(1, 6, 5, 7), emb_cur=env.f32(1, 6, 5, 7))


@ragged("channel_mean[HW35]")
def _(env):
    return hip.channel_mean, dict(x1=env.f32(2, 5, 7, 8), x2=env.f32(2, 5, 7, 4))


@ragged("gate_apply[amax]")
def _(env):
    return hip.gate_apply, dict(x=env.f32(2, 5, 7, 12), gate=env.f32(2, 12, lo=0, hi=1), y=env.f32(2, 5, 7, 12), amax_out=env.amax(), amax_c0=4)


# ---- motion front end: 21 x 37 and 33 x 50 frames, blocks cut at the right and bottom edges ------------------------------------------------------------
def _luma_stack(env, C, F1, H, W):
    """(C, F1, H, W) planes a multiple of 4 bytes apart whose last plane ends exactly where its allocation ends"""
    ps = -(-H * W // 4) * 4
    flat = env.u8((C * F1 - 1) * ps + H * W)
    return flat.as_strided((C, F1, H, W), (F1 * ps, ps, W, 1))


@ragged("luma_u8[21x37]")
def _(env):
    return hip.luma_u8, dict(bgr=env.u8(21, 37, 3))


def _motion_rows(H, W):
    tag = "%dx%d" % (H, W)

    @ragged("mv_estimate[%s]" % tag)
    def _(env):
        return hip.mv_estimate, dict(luma_cur=env.u8(H, W), luma_ref=env.u8(H, W), search=8, return_sad=True)

    @ragged("mv_estimate_chain[%s]" % tag)
    def _(env):
        return hip.mv_estimate_chain, dict(luma_stack=_luma_stack(env, 2, 3, H, W), search=8, return_sad=True)

    @ragged("luma_pyramid[%s]" % tag)
    def _(env):
        return hip.luma_pyramid, dict(luma=_luma_stack(env, 1, 3, H, W)[0], levels=2)

    @ragged("mv_refine_chain[%s]" % tag, "mv_refine_chain")
    def _(env):
        def fn(luma_stack):
            """the pyramid's own sequence: level 1 of the stack, the full search there, one refinement at level 0; then the cut score"""
            C, F1 = luma_stack.shape[:2]
            p1 = hip.luma_pyramid(luma_stack.view(-1, H, W) if luma_stack.is_contiguous() else luma_stack[0], 1)[0]
            parent = hip.mv_estimate_chain(p1.unsqueeze(0), search=8)
            rows, sad = hip.mv_refine_chain(luma_stack, parent, return_sad=True)
            return p1, parent, rows, sad, hip.mv_cut_score(luma_stack, sad)
        return fn, dict(luma_stack=_luma_stack(env, 1, 3, H, W))

    @ragged("mv_segment_inputs[%s]" % tag, "mv_segment_inputs")
    def _(env):
        def fn(luma_stack, bgr_stack, im_scale):
            rows = hip.mv_estimate_chain(luma_stack, search=8)
            return rows, hip.mv_segment_inputs(rows, bgr_stack, im_scale, pixel_means=(1.0, 2.0, 3.0))
        return fn, dict(luma_stack=_luma_stack(env, 2, 3, H, W), bgr_stack=env.u8(2, 3, H, W, 3), im_scale=1.6)

    def estimator_row(levels):
        def make(env):
            me = hip.MotionEstimator(W, H, bc.CUDA0, search=8, levels=levels, cut=dict(bias=4, percent=50), stale=dict(bias=4, percent=50))

            def fn(frames):
                """a key frame and two frames behind it: the second pair's planes lie in reverse (the reference plane behind the current one)"""
                me.key_frame(frames[0])
                got = []
                for f in frames[1:]:
                    me.next_frame(f)
                    got += [me.rows.clone(), me.sad.clone(), me.unmatched.clone(), me.key_unmatched.clone(), me.keysad.clone()]
                    got += [t.clone() for t in me.network_inputs(f, frames[0], 1.0)]
                return got
            return fn, dict(frames=[env.u8(H, W, 3) for _ in range(3)])
        RAGGED.append(Ragged("MotionEstimator[%s-levels%d-cut-stale]" % (tag, levels), "MotionEstimator.next_frame", make))
    estimator_row(0)
    estimator_row(1)

    @ragged("SegmentMotionEstimator[%s-pyramid-cut-stale]" % tag, "SegmentMotionEstimator.segment")
    def _(env):
        sme = hip.SegmentMotionEstimator(W, H, frames=2, clips=2, device=bc.CUDA0, search=8, levels=2, cut=dict(bias=4, percent=50), stale=dict(bias=4, percent=50))

        def fn(bgr_stack):
            out = sme.segment(bgr_stack, 1.6)
            return out, sme.rows, sme.sad, sme.intra, sme.unmatched, sme.keysad, sme.key_unmatched
        return fn, dict(bgr_stack=env.u8(2, 3, H, W, 3))


for _h, _w in ((21, 37), (33, 50)):
    _motion_rows(_h, _w)


# ---- YUV and image intake -------------------------------------------------------------------------------------------------------------------------
def _yuv_rows(H, W, n, pitch):
    def planes(env, i420):
        ch, cw = -(-H // 2), -(-W // 2)

        def plane(rows, cols):
            lead = () if n is None else (n,)
            return env.u8(*(lead + (rows, cols))) if pitch is None else env.u8(*(lead + (rows, cols + pitch)))[..., :cols]
        return dict(y=plane(H, W), u=plane(ch, cw), v=plane(ch, cw)) if i420 else dict(y=plane(H, W), uv=plane(ch, 2 * cw))
    lead = () if n is None else (n,)
    tag = "%dx%d%s%s" % (H, W, "" if n is None else "x%d" % n, "" if pitch is None else "-pitched")
    for i420 in (False, True):
        fmt = "i420" if i420 else "nv12"
        ragged("yuv420_to_bgr_u8[%s-%s]" % (fmt, tag))(lambda env, i420=i420: (hip.yuv420_to_bgr_u8, dict(
            planes(env, i420), y_packed=env.zeros(*(lead + (H, W)), dtype=torch.uint8))))
        ragged("image_transform_yuv420[%s-%s]" % (fmt, tag))(lambda env, i420=i420: (hip.image_transform_yuv420, dict(
            planes(env, i420), pixel_means=(1.0, 2.0, 3.0), pixel_scale=0.0125)))
        ragged("image_resize_transform_yuv420[%s-%s]" % (fmt, tag))(lambda env, i420=i420: (hip.image_resize_transform_yuv420, dict(
            planes(env, i420), im_scale=1.6, pixel_means=(1.0, 2.0, 3.0), stride=16)))


for _geo in ((2, 2, None, None), (4, 6, None, None), (5, 7, None, None), (6, 8, 3, 4)):
    _yuv_rows(*_geo)


for _scale in (1.0, 1.6):
    ragged("image_resize_transform[f32-%s]" % _scale)(lambda env, s=_scale: (hip.image_resize_transform, dict(
        im=env.f32(2, 21, 37, 3, lo=0, hi=255), im_scale=s, pixel_means=(1.0, 2.0, 3.0), stride=16)))
    ragged("image_resize_transform[u8-%s]" % _scale)(lambda env, s=_scale: (hip.image_resize_transform, dict(
        im=env.u8(2, 21, 37, 3), im_scale=s, pixel_means=(1.0, 2.0, 3.0))))
    ragged("image_resize_transform[u8_fixed_point-%s]" % _scale)(lambda env, s=_scale: (hip.image_resize_transform, dict(
        im=env.u8(21, 37, 3), im_scale=s, pixel_means=(1.0, 2.0, 3.0), stride=16, u8_fixed_point=True)))
    ragged("transform_mv_res[21x37-%s]" % _scale)(lambda env, s=_scale: (hip.transform_mv_res, dict(
        motion_vector=env.i32(21, 37, 2, lo=-8, hi=8), res_diff=env.i32(21, 37, 3, lo=-20, hi=20), im_scale=s, pixel_means=(1.0, 2.0, 3.0), rcnn_stride=16)))


@ragged("image_transform_u8[12-pixels]")
def _(env):
    return hip.image_transform_u8, dict(im=env.u8(2, 2, 6, 3), pixel_means=(1.0, 2.0, 3.0))


# ---- wrappers whose table rows hand over every buffer: the same calls with the outputs the wrapper allocates itself --------------------------------
@ragged("channel_gate[own-out]")
def _(env):
    return hip.channel_gate, dict(m=env.f32(2, 8), w1=env.f32(12, 8), b1=env.f32(12), w2=env.f32(5, 12), b2=env.f32(5))


for _fn, _cl, _extra in ((hip.scale_shift_relu, False, dict(relu=True)), (hip.scale_shift_leaky, False, dict(slope=0.1)),
                         (hip.scale_shift_relu_cl, True, dict(relu=True))):
    ragged("%s[own-out]" % _fn.__name__)(lambda env, fn=_fn, cl=_cl, extra=_extra: (fn, dict(
        dict(x=env.f32(*((2, 5, 7, 12) if cl else (2, 12, 5, 7))), scale=env.f32(12), shift=env.f32(12)), **extra)))


for _nchw in (False, True):
    ragged("head_conv3x3[own-out-%s]" % ("nchw" if _nchw else "cl"))(lambda env, nchw=_nchw: (hip.head_conv3x3, dict(
        x=env.f32(2, 5, 7, 8), w=env.f32(2, 3, 3, 8), bias=env.f32(2), mul=2.5, nchw=nchw)))


@ragged("nchw_to_nhwc[own-out]")
def _(env):
    return hip.nchw_to_nhwc, dict(x=env.f32(2, 8, 5, 7), c0=4, c=4, amax_out=env.amax())


@ragged("MotionVectorAccumulator[own-maps-21x37]", "MotionVectorAccumulator.network_inputs")
def _(env):
    acc = hip.MotionVectorAccumulator(37, 21, bc.CUDA0)

    def fn(luma_cur, luma_ref, bgr_cur, bgr_ref):
        """the rows of a search on the frame (blocks cut at both edges), accumulated with the block area read from them"""
        acc.reset()
        acc.add_frame(hip.mv_estimate(luma_cur, luma_ref, search=8))
        return acc.motion_vectors(), acc.residual(bgr_cur, bgr_ref), acc.network_inputs(bgr_cur, bgr_ref, 1.6, pixel_means=(1.0, 2.0, 3.0))
    return fn, dict(luma_cur=env.u8(21, 37), luma_ref=env.u8(21, 37), bgr_cur=env.u8(21, 37, 3), bgr_ref=env.u8(21, 37, 3))


@pytest.mark.parametrize("r", RAGGED, ids=lambda r: r.id)
def test_a_ragged_call_owns_its_memory(hip, r):
    three_way(r)


# ---- the harness on the device: what tests/test_memory_ownership_cpu.py shows on the host ------------------------------------------------------------
def test_the_device_arena_reports_a_stray_store_and_an_unwritten_output(hip):
    """torch ops on views of the arena's own storage: a store one element past `out` and one before it, and an output whose last element
    stays unwritten"""
    def past(x, out, before, after):
        p = bc.plain(out)
        if p.storage_offset() < before or p.untyped_storage().nbytes() < 4 * (p.storage_offset() + p.numel() + after):
            before = after = 0              # the unguarded call: `out` fills its allocation, there is nothing of its own to stray into
        whole = torch.as_strided(p, (p.numel() + before + after,), (1,), p.storage_offset() - before)
        whole[before:before + p.numel()].copy_(x.reshape(-1))
        if before:
            whole[0] = 1.0
        if after:
            whole[-1] = 1.0
        return out

    def row(fn, **extra):
        return Ragged(fn.__name__, fn.__name__, lambda env: (fn, dict(dict(x=env.f32(2, 9), out=env.zeros(2, 9)), **extra)))
    assert three_way(row(past, before=0, after=0)) == 2
    for before, after, where in ((0, 1, "+0 bytes from its end"), (1, 0, "-4 bytes from its start")):
        with pytest.raises(AssertionError) as e:
            three_way(row(past, before=before, after=after))
        assert "out (2, 9) torch.float32" in str(e.value) and where in str(e.value), str(e.value)

    def unwritten(x, out):
        y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        y.view(-1)[:-1].copy_(x.view(-1)[:-1])
        return y
    with pytest.raises(AssertionError) as e:
        three_way(row(unwritten))
    assert "differs from the unguarded call under pattern 0xFF in 1 element(s), the first at flat index 17" in str(e.value), str(e.value)
