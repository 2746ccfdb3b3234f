"""lsfa_luma_pyramid / lsfa_mv_refine_chain (lsfa_amd/csrc/me_pyramid.hip), hip.SegmentMotionEstimator / hip.MotionEstimator with levels > 0 and
TestLoader(estimate_mv=dict(levels=...)) on the GPU: the two kernels against tests/ref_me_pyramid.py bit for bit, the segment's inputs against
the per-frame accumulation of the same rows, the known answer beyond the full search's reach, graph capture, the YUV path and the error
paths.  tests/test_me_pyramid_cpu.py pins the reference itself."""
import functools

import numpy as np
import pytest
import torch

import me_util
import ref_me
import ref_me_pyramid as rp
from me_util import plane_stack, t

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MEANS = (102.9801, 115.9465, 122.7717)
PIXEL_SCALE = 0.5

clip = functools.partial(me_util.clip, m=(7, -5))          # this file's clips move further than the segment tests': (7, -5) unless a test says otherwise


# ---- lsfa_luma_pyramid -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", [(5, 3), (37, 23), (250, 130), (64, 48)])
def test_luma_pyramid_equals_the_reference(hip, width, height):
    """both levels of three different planes in one launch, and level 1 alone, against ref_me_pyramid.pyramid bit for bit; the planes of the
    input lie 12 bytes further apart than they are large (0xA5 between them), those of the outputs a multiple of 4"""
    rs = np.random.RandomState(width)
    planes = [rs.randint(0, 256, (height, width)).astype(np.uint8) for _ in range(3)]
    stride = -(-height * width // 4) * 4 + 12
    stack = plane_stack(planes, [[0, 1, 2]], stride=stride)[0]
    assert stack.stride(0) == stride and tuple(stack.shape) == (3, height, width)
    want = [rp.pyramid(p, 2) for p in planes]
    for levels in (2, 1):
        got = hip.luma_pyramid(stack, levels)
        assert len(got) == levels
        for k in range(1, levels + 1):
            assert got[k - 1].dtype == torch.uint8 and tuple(got[k - 1].shape) == (3,) + want[0][k].shape and got[k - 1].stride(0) % 4 == 0
            for i in range(3):
                np.testing.assert_array_equal(got[k - 1][i].cpu().numpy(), want[i][k], err_msg="levels %d level %d plane %d" % (levels, k, i))
    # a single dense plane into the caller's buffers, which are written nowhere else
    h1, w1 = want[0][1].shape
    h2, w2 = want[0][2].shape
    s1, s2 = -(-h1 * w1 // 4) * 4 + 8, -(-h2 * w2 // 4) * 4 + 4
    b1 = torch.full((s1,), 0x5A, dtype=torch.uint8, device=DEV)
    b2 = torch.full((s2,), 0x5A, dtype=torch.uint8, device=DEV)
    hip.luma_pyramid(t(planes[1])[None], 2, out=[b1[:h1 * w1].view(1, h1, w1), b2[:h2 * w2].view(1, h2, w2)])
    np.testing.assert_array_equal(b1[:h1 * w1].view(h1, w1).cpu().numpy(), want[1][1])
    np.testing.assert_array_equal(b2[:h2 * w2].view(h2, w2).cpu().numpy(), want[1][2])
    assert (b1[h1 * w1:] == 0x5A).all() and (b2[h2 * w2:] == 0x5A).all()


# ---- lsfa_mv_refine_chain --------------------------------------------------------------------------------------------------------------------------
def random_parent_rows(rs, width, height, C, F, span):
    """rows of the level above a (height, width) plane for (C, F) pairs: every block a random vector within +-span, so that with small planes
    many candidates point outside and are dropped"""
    h1, w1 = -(-height // 2), -(-width // 2)
    z = np.zeros((h1, w1), np.uint8)
    base = ref_me.estimate(z, z, 1, 0)[0]
    rows = np.broadcast_to(base, (C, F) + base.shape).copy()
    rows[..., 3] += rs.randint(-span, span + 1, rows.shape[:3])
    rows[..., 4] += rs.randint(-span, span + 1, rows.shape[:3])
    return rows


@pytest.mark.parametrize("refine", [1, 2, 3])
@pytest.mark.parametrize("width,height", [(37, 23), (96, 64), (250, 130)])
def test_refine_chain_equals_the_reference(hip, width, height, refine):
    """two chains of three frames in one launch, and one pair alone, with lambda 0 / 4 and max_sad off / on == ref_me_pyramid.refine, rows and
    SAD, bit for bit.  Chain 0 is frames 0 .. 3, chain 1 frames 1 .. 4: different content at every (chain, frame) position."""
    rs = np.random.RandomState(width + refine)
    planes = [ref_me.luma(f) for f in clip(5, width, height, seed=width)]
    chains = [[0, 1, 2, 3], [1, 2, 3, 4]]
    stack = plane_stack(planes, chains)
    parents = random_parent_rows(rs, width, height, 2, 3, 12)
    mbh, mbw = -(-height // 16), -(-width // 16)
    dropped = 0
    for lam in (0, 4):
        for max_sad in (0, 1800):
            rows, sad = hip.mv_refine_chain(stack, t(parents), refine, lam, max_sad, return_sad=True)
            assert rows.dtype == torch.int32 and tuple(rows.shape) == (2, 3, mbh * mbw, 7) and tuple(sad.shape) == (2, 3, mbh, mbw)
            rows, sad = rows.cpu().numpy(), sad.cpu().numpy()
            for c in range(2):
                for f in range(1, 4):
                    w_rows, w_sad = rp.refine(planes[chains[c][f]], planes[chains[c][f - 1]], parents[c, f - 1], refine, lam, max_sad)
                    np.testing.assert_array_equal(rows[c, f - 1], w_rows, err_msg="rows lam %d max_sad %d pair (%d, %d)" % (lam, max_sad, c, f))
                    np.testing.assert_array_equal(sad[c, f - 1], w_sad, err_msg="SAD lam %d max_sad %d pair (%d, %d)" % (lam, max_sad, c, f))
                    if max_sad:
                        zeroed = (w_sad.reshape(-1) > max_sad)
                        dropped += int(zeroed.sum())
                        assert (w_rows[zeroed, 3:5] == w_rows[zeroed, 5:7]).all()
            # the single-pair form: n_chains = n_frames = 1, without the optional output
            one = hip.mv_refine_chain(stack[1:, 1:3], t(parents[1:, 1:2]), refine, lam, max_sad)
            np.testing.assert_array_equal(one.cpu().numpy()[0, 0], rows[1, 1])
    assert dropped > 0          # the threshold bites somewhere


# ---- the estimators --------------------------------------------------------------------------------------------------------------------------------
_SEGMENT = {}


def segment_case(levels):
    """four frames at 250 x 130 and the reference's rows / SAD of their three pairs, once per `levels`"""
    if levels not in _SEGMENT:
        frames = clip(4, 250, 130, seed=21 + levels)
        lum = [ref_me.luma(f) for f in frames]
        _SEGMENT[levels] = (frames, [rp.estimate(lum[f], lum[f - 1], levels, 4, 4, 0, 2) for f in range(1, 4)])
    return _SEGMENT[levels]


def accumulated_inputs(hip, frames, rows, scale):
    """the per-frame chain on given rows: lsfa_mv_identity, lsfa_mv_accumulate frame by frame, then lsfa_mv_field, lsfa_mv_residual and
    lsfa_transform_mv_res (hip.MotionVectorAccumulator) -> (mv (n, 2, h, w), res (n, 3, h, w))"""
    height, width = frames[0].shape[:2]
    acc = hip.MotionVectorAccumulator(width, height, DEV)
    dev = [t(f) for f in frames]
    mvs, ress = [], []
    for f in range(1, len(frames)):
        acc.add_frame(rows[f - 1], max_block_area=256)
        mv, res = acc.network_inputs(dev[f], dev[0], scale, MEANS, PIXEL_SCALE)
        mvs.append(mv[0].clone())
        ress.append(res[0].clone())
    return torch.stack(mvs), torch.stack(ress)


@pytest.mark.parametrize("levels", [1, 2])
def test_segment_estimator_equals_the_reference_and_the_per_frame_chain(hip, levels):
    frames, want = segment_case(levels)
    sme = hip.SegmentMotionEstimator(250, 130, frames=3, device=DEV, search=4, lam=4, levels=levels, refine=2)
    assert sme.reach == rp.reach(levels, 4, 2) == (10, 22)[levels - 1]
    stack = t(np.stack(frames)[None])
    for scale in (1.0, 0.6):
        mv, res = sme.segment(stack, scale, MEANS, PIXEL_SCALE)
        assert tuple(sme.rows.shape) == (1, 3, sme.mbh * sme.mbw, 7) and tuple(sme.sad.shape) == (1, 3, sme.mbh, sme.mbw)
        for f in range(3):
            np.testing.assert_array_equal(sme.rows[0, f].cpu().numpy(), want[f][0], err_msg="rows of frame %d" % (f + 1))
            np.testing.assert_array_equal(sme.sad[0, f].cpu().numpy(), want[f][1], err_msg="SAD of frame %d" % (f + 1))
        w_mv, w_res = accumulated_inputs(hip, frames, sme.rows[0], scale)
        assert torch.equal(mv[:, 0], w_mv) and torch.equal(res[:, 0], w_res), scale
        assert float(mv.abs().max()) > 0
    v = (sme.rows[0, :, :, 3:5] - sme.rows[0, :, :, 5:7]).abs().max()
    assert int(v) > 4          # beyond the top level's own range: the refinement doubled something


def test_levels_zero_is_bit_identical_to_the_estimator_without_the_argument(hip):
    frames = clip(4, 250, 130, seed=4)
    stack = t(np.stack(frames)[None])
    plain = hip.SegmentMotionEstimator(250, 130, frames=3, device=DEV, search=8, lam=4)
    zero = hip.SegmentMotionEstimator(250, 130, frames=3, device=DEV, search=8, lam=4, levels=0, refine=7)        # refine is ignored at levels = 0
    assert zero.reach == plain.reach == 8
    a_mv, a_res = plain.segment(stack, 1.25, MEANS, PIXEL_SCALE)
    b_mv, b_res = zero.segment(stack, 1.25, MEANS, PIXEL_SCALE)
    assert torch.equal(a_mv, b_mv) and torch.equal(a_res, b_res) and torch.equal(plain.rows, zero.rows) and torch.equal(plain.sad, zero.sad)
    lum = [ref_me.luma(f) for f in frames]
    np.testing.assert_array_equal(zero.rows[0, 2].cpu().numpy(), ref_me.estimate(lum[3], lum[2], 8, 4)[0])
    me0, me1 = hip.MotionEstimator(250, 130, DEV, search=8, lam=4), hip.MotionEstimator(250, 130, DEV, search=8, lam=4, levels=0)
    for me in (me0, me1):
        me.key_frame(stack[0, 0])
        me.next_frame(stack[0, 1])
    assert torch.equal(me0.rows, me1.rows) and torch.equal(me0.rows, plain.rows[0, 0])


def test_known_answer_beyond_the_old_reach_on_the_device(hip):
    """white noise translated by (44, -24) through segment(): every eligible block's row carries the translation (a grey BGR frame's luma is
    its grey value: (29 + 150 + 77) v + 128 >> 8 = v), which no parameter of the full search can express"""
    k = rp.KNOWN
    ref, cur, ok = rp.known_answer_case()
    stack = t(np.stack([np.repeat(p[:, :, None], 3, axis=2) for p in (ref, cur)])[None])
    np.testing.assert_array_equal(ref_me.luma(stack[0, 1].cpu().numpy()), cur)
    sme = hip.SegmentMotionEstimator(k['width'], k['height'], frames=1, device=DEV, search=k['search'], lam=k['lam'], levels=k['levels'], refine=k['refine'])
    assert sme.reach == 54
    sme.segment(stack, 1.0)
    rows = sme.rows[0, 0].cpu().numpy()
    v = ref_me.vectors(rows, 12, 16)
    hit = (v[..., 0] == k['m'][0]) & (v[..., 1] == k['m'][1])
    assert int(ok.sum()) * 3 > ok.size and hit[ok].all(), np.argwhere(ok & ~hit).tolist()
    assert (sme.sad[0, 0].cpu().numpy()[ok] == 0).all()
    np.testing.assert_array_equal(rows, rp.estimate(cur, ref, k['levels'], k['search'], k['lam'], 0, k['refine'])[0])
    full = hip.SegmentMotionEstimator(k['width'], k['height'], frames=1, device=DEV, search=32, lam=k['lam'])
    full.segment(stack, 1.0)
    fv = ref_me.vectors(full.rows[0, 0].cpu().numpy(), 12, 16)
    assert not ((fv[..., 0] == k['m'][0]) & (fv[..., 1] == k['m'][1])).any()


def test_motion_estimator_rows_equal_the_segment_form(hip):
    """MotionEstimator(levels=2).next_frame frame by frame (ping-pong planes, the pair handed to the refinement forwards and in reverse)
    == the segment form's rows on the same frames == the reference"""
    frames, want = segment_case(2)
    dev = [t(f) for f in frames]
    me = hip.MotionEstimator(250, 130, DEV, search=4, lam=4, levels=2, refine=2)
    assert me.reach == 22
    sme = hip.SegmentMotionEstimator(250, 130, frames=3, device=DEV, search=4, lam=4, levels=2, refine=2)
    mv, res = sme.segment(t(np.stack(frames)[None]), 1.0, MEANS, PIXEL_SCALE)
    me.key_frame(dev[0])
    for f in range(1, 4):
        rows = me.next_frame(dev[f])
        assert torch.equal(rows, sme.rows[0, f - 1]) and torch.equal(me.sad, sme.sad[0, f - 1]), f
        np.testing.assert_array_equal(rows.cpu().numpy(), want[f - 1][0])
        a_mv, a_res = me.network_inputs(dev[f], dev[0], 1.0, MEANS, PIXEL_SCALE)
        assert torch.equal(a_mv[0], mv[f - 1, 0]) and torch.equal(a_res[0], res[f - 1, 0]), f


def test_two_clips_in_lock_step(hip):
    width, height = 250, 130
    clips = [clip(4, width, height, seed=3), clip(4, width, height, seed=4, m=(-9, 6))]
    sme = hip.SegmentMotionEstimator(width, height, frames=3, clips=2, device=DEV, search=4, lam=4, levels=2)
    mv, res = sme.segment(t(np.stack([np.stack(c) for c in clips])), 0.6, MEANS, PIXEL_SCALE)
    one = hip.SegmentMotionEstimator(width, height, frames=3, device=DEV, search=4, lam=4, levels=2)
    for c in range(2):
        w_mv, w_res = [x.clone() for x in one.segment(t(np.stack(clips[c])[None]), 0.6, MEANS, PIXEL_SCALE)]
        assert torch.equal(sme.rows[c], one.rows[0]) and torch.equal(sme.sad[c], one.sad[0]), c
        assert torch.equal(mv[:, c], w_mv[:, 0]) and torch.equal(res[:, c], w_res[:, 0]), c
    assert not torch.equal(sme.rows[0], sme.rows[1])


def test_short_segment(hip):
    """n < frames through an estimator built for five: the planes of every level and the rows of every level are stacks of their own in
    front of the same memory"""
    width, height = 96, 64
    frames = clip(6, width, height, seed=12)
    stack = t(np.stack(frames)[None])
    sme = hip.SegmentMotionEstimator(width, height, frames=5, device=DEV, search=4, lam=4, levels=2)
    full_mv, full_res = [x.clone() for x in sme.segment(stack, 1.0, MEANS, PIXEL_SCALE)]
    full_rows = sme.rows.clone()
    for n in (1, 3):
        a_mv, a_res = sme.segment(stack, 1.0, MEANS, PIXEL_SCALE, n=n)
        assert tuple(a_mv.shape)[:2] == (n, 1) and torch.equal(a_mv, full_mv[:n]) and torch.equal(a_res, full_res[:n]), n
        assert torch.equal(sme.rows, full_rows[:, :n])


def test_segment_graph_capture(hip):
    """segment with levels = 2 captured on one stream (six launches, no parallel branches) and replayed on NEW frame contents == the eager call"""
    width, height = 250, 130
    clips = [clip(4, width, height, seed=1, sigma=0.0), clip(4, width, height, seed=2, m=(-9, 6))]
    buf = t(np.stack(clips[0])[None]).clone()
    sme = hip.SegmentMotionEstimator(width, height, frames=3, device=DEV, search=4, lam=4, levels=2)
    sme.segment(buf, 1.25, MEANS, PIXEL_SCALE)              # warm-up: the outputs are allocated at the first call for a scale and a length
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_mv, out_res = sme.segment(buf, 1.25, MEANS, PIXEL_SCALE)
    eager = hip.SegmentMotionEstimator(width, height, frames=3, device=DEV, search=4, lam=4, levels=2)
    seen = []
    for k, c in enumerate(clips[::-1] + clips):
        buf.copy_(t(np.stack(c)[None]))
        g.replay()
        torch.cuda.synchronize()
        e_mv, e_res = eager.segment(t(np.stack(c)[None]), 1.25, MEANS, PIXEL_SCALE)
        assert torch.equal(out_mv, e_mv) and torch.equal(out_res, e_res), k
        assert torch.equal(sme.rows, eager.rows) and torch.equal(sme.sad, eager.sad), k
        seen.append(sme.rows.clone())
    assert not torch.equal(seen[0], seen[1])


def test_launch_counts(hip):
    """a segment with levels = 2 is six launches (luma, pyramid, top search, two refinements, inputs), levels = 1 five, levels = 0 three"""
    stack = t(np.stack(clip(3, 96, 64, seed=2))[None])
    for levels, want in ((0, 3), (1, 5), (2, 6)):
        sme = hip.SegmentMotionEstimator(96, 64, frames=2, device=DEV, search=4, lam=4, levels=levels)
        sme.segment(stack, 1.0)
        hip.prof_enable(True, ops=["mv_estimate"])
        try:
            sme.segment(stack, 1.0)
            ms, n = hip.prof_read()["mv_estimate"]
        finally:
            hip.prof_enable(False)
        assert n == want and ms > 0.0, levels


def test_segment_yuv_from_the_decoders_y_planes(hip):
    """segment_yuv with luma_from='y' and levels = 1 == segment on the converted frames, with the Y planes searched"""
    width, height, C, n = 96, 64, 2, 3
    rs = np.random.RandomState(3)
    N = C * (n + 1)
    base = clip(N, width, height, seed=8)
    y = t(np.stack([ref_me.luma(f) for f in base]))
    uv = t(rs.randint(96, 160, (N, height // 2, width)).astype(np.uint8))
    bgr = hip.yuv420_to_bgr_u8(y, uv).view(C, n + 1, height, width, 3)
    from_y = hip.SegmentMotionEstimator(width, height, frames=n, clips=C, device=DEV, search=4, lam=4, luma_from='y', levels=1)
    mv, res = from_y.segment_yuv(y, uv, im_scale=1.0, pixel_means=MEANS, pixel_scale=PIXEL_SCALE)
    ys = y.view(C, n + 1, height, width)
    p1 = hip.luma_pyramid(y, 1)[0]
    top = hip.mv_estimate_chain(p1.view(C, n + 1, height // 2, width // 2), 4, 4, 0)
    want_rows, want_sad = hip.mv_refine_chain(ys, top, 2, 4, 0, return_sad=True)
    assert torch.equal(from_y.rows, want_rows) and torch.equal(from_y.sad, want_sad) and torch.equal(from_y.bgr, bgr)
    y_np = y.cpu().numpy()
    np.testing.assert_array_equal(from_y.rows[1, 0].cpu().numpy(), rp.estimate(y_np[n + 2], y_np[n + 1], 1, 4, 4, 0, 2)[0])
    w_mv, w_res = hip.mv_segment_inputs(want_rows, bgr, 1.0, MEANS, PIXEL_SCALE)
    assert torch.equal(mv, w_mv) and torch.equal(res, w_res)


def test_error_paths(hip):
    """the refusals of the two exports (an error code and its message, nothing launched) and of the wrappers and estimators"""
    L = hip.lib()
    W, H = 96, 64
    luma = torch.zeros((1, 3, H, W), dtype=torch.uint8, device=DEV)
    parent = torch.zeros((1, 2, 6, 7), dtype=torch.int32, device=DEV)
    rows = torch.full((1, 2, 24, 7), -7, dtype=torch.int32, device=DEV)
    p1 = torch.full((3, H // 2, W // 2), 0x5A, dtype=torch.uint8, device=DEV)
    p2 = torch.full((3, H // 4, W // 4), 0x5A, dtype=torch.uint8, device=DEV)

    def refine(**kw):
        a = dict(luma=luma.data_ptr(), stride=W * H, C=1, F=2, W=W, H=H, parent=parent.data_ptr(), r=2, lam=4, max_sad=0, mvs=rows.data_ptr(), sad=None)
        a.update(kw)
        return L.lsfa_mv_refine_chain(a['luma'], a['stride'], a['C'], a['F'], a['W'], a['H'], a['parent'], a['r'], a['lam'], a['max_sad'], a['mvs'], a['sad'], None)

    def pyramid(**kw):
        a = dict(luma=luma.data_ptr(), stride=W * H, N=3, W=W, H=H, levels=2, p1=p1.data_ptr(), s1=W * H // 4, p2=p2.data_ptr(), s2=W * H // 16)
        a.update(kw)
        return L.lsfa_luma_pyramid(a['luma'], a['stride'], a['N'], a['W'], a['H'], a['levels'], a['p1'], a['s1'], a['p2'], a['s2'], None)

    for call, kw, text in ((refine, dict(luma=None), b"NULL"), (refine, dict(parent=None), b"NULL"), (refine, dict(mvs=None), b"NULL"),
                           (refine, dict(W=0), b"bad frame size"), (refine, dict(r=0), b"refine 0"), (refine, dict(r=4), b"refine 4"),
                           (refine, dict(lam=-1), b"lambda -1"), (refine, dict(max_sad=-1), b"max_sad -1"), (refine, dict(C=0), b"at least 1"),
                           (refine, dict(F=0), b"at least 1"), (refine, dict(stride=W * H - 4), b"plane stride"),
                           (refine, dict(stride=W * H + 2), b"multiple of 4"), (refine, dict(stride=-(W * H) + 4), b"plane stride"),
                           (refine, dict(luma=luma.data_ptr() + 1), b"4-byte aligned"), (refine, dict(C=1 << 14, F=1 << 14), b"exceed one grid"),
                           (pyramid, dict(levels=0), b"levels 0"), (pyramid, dict(levels=3), b"levels 3"), (pyramid, dict(luma=None), b"NULL"),
                           (pyramid, dict(p1=None), b"NULL"), (pyramid, dict(p2=None), b"NULL"), (pyramid, dict(H=0), b"bad frame size"),
                           (pyramid, dict(N=0), b"planes"), (pyramid, dict(stride=W * H - 1), b"plane stride"),
                           (pyramid, dict(s1=W * H // 4 - 4), b"level 1 stride"), (pyramid, dict(s1=W * H // 4 + 2), b"multiple of 4"),
                           (pyramid, dict(s2=W * H // 16 + 1), b"level 2 stride"), (pyramid, dict(p1=p1.data_ptr() + 2), b"4-byte aligned")):
        assert call(**kw) != 0, kw
        msg = L.lsfa_last_error()
        assert text in msg and (b"lsfa_mv_refine_chain" if call is refine else b"lsfa_luma_pyramid") in msg, (kw, msg)
    torch.cuda.synchronize()
    assert (rows == -7).all() and (p1 == 0x5A).all() and (p2 == 0x5A).all()          # nothing was launched
    assert refine() == 0 and pyramid() == 0 and pyramid(levels=1, p2=None, s2=0) == 0
    torch.cuda.synchronize()
    assert (rows[..., 0] == -1).all() and (p1 == 0).all() and (p2 == 0).all()

    for bad, text in ((dict(levels=3), "levels 3"), (dict(levels=-1), "levels -1"), (dict(levels=1, refine=0), "refine 0"), (dict(levels=2, refine=4), "refine 4")):
        with pytest.raises(hip.LsfaError, match=text):
            hip.SegmentMotionEstimator(W, H, device=DEV, **bad)
        with pytest.raises(hip.LsfaError, match=text):
            hip.MotionEstimator(W, H, DEV, **bad)
    with pytest.raises(hip.LsfaError, match="levels 3"):
        hip.luma_pyramid(luma[0], 3)
    with pytest.raises(hip.LsfaError, match="uint8 CUDA stack"):
        hip.luma_pyramid(luma, 1)                              # four axes
    with pytest.raises(hip.LsfaError, match="dense"):
        hip.luma_pyramid(luma[0, :, :, ::2], 1)
    with pytest.raises(hip.LsfaError, match="multiple of 4"):     # a misaligned stride: planes 1,538 bytes apart
        hip.luma_pyramid(luma[0], 1, out=[torch.empty(3 * 1538, dtype=torch.uint8, device=DEV).as_strided((3, H // 2, W // 2), (1538, W // 2, 1))])
    with pytest.raises(hip.LsfaError, match="parent_rows"):       # the block count of another grid
        hip.mv_refine_chain(luma, torch.zeros((1, 2, 24, 7), dtype=torch.int32, device=DEV))
    with pytest.raises(hip.LsfaError, match="parent_rows"):
        hip.mv_refine_chain(luma, parent.float())
    with pytest.raises(hip.LsfaError, match="refine 5"):
        hip.mv_refine_chain(luma, parent, 5)
    with pytest.raises(hip.LsfaError, match="output buffer"):
        hip.mv_refine_chain(luma, parent, out=rows[:, :1])
    with pytest.raises(hip.LsfaError, match="dense frames"):
        hip.mv_refine_chain(luma[:, :, :, ::2], parent)
    torch.cuda.synchronize()


# ---- frames alone into the loader ------------------------------------------------------------------------------------------------------------------
def test_loader_hands_out_the_pyramid_estimators_slices(hip):
    """TestLoader(estimate_mv=dict(..., levels=1)) over the 24-frame clip of test_pipeline_from_frames_alone at key interval 10: every non-key
    frame receives the slice a SegmentMotionEstimator(levels=1) of its own produces for the segment's frames"""
    from lsfa_amd.config.config import lsfa_test_config
    from lsfa_amd.core.loader import TestLoader
    from lsfa_amd.utils.synthetic import synthetic_roidb
    H, W, K, n = 96, 160, 10, 24
    cfg = lsfa_test_config(key_frame_interval=K)
    roidb = synthetic_roidb(1, n, H, W, K)
    loader = TestLoader(roidb, cfg, device=DEV, estimate_mv=dict(search=4, lam=4, levels=1, refine=2))
    clip_ = roidb[0]['clip']
    sme = hip.SegmentMotionEstimator(W, H, frames=K - 1, device=DEV, search=4, lam=4, levels=1, refine=2)
    seen = 0
    for f, (im_info, flag, batch) in enumerate(loader):
        if flag != 2:
            continue
        d = dict(zip(loader.data_name, batch.data[0]))
        key_f = f // K * K
        m = min(key_f + K - 1, n - 2) - key_f
        stack = torch.stack([clip_.frame_u8(g) for g in range(key_f, key_f + m + 1)]).unsqueeze(0).to(DEV)
        mv, res = sme.segment(stack, float(clip_.im_info()[0, 2]), cfg.network.PIXEL_MEANS, cfg.network.PIXEL_SCALE)
        assert torch.equal(d['motion_vector'], mv[f - key_f - 1]) and torch.equal(d['res_diff'], res[f - key_f - 1]), f
        seen += 1
    assert seen == 9 + 9 + 2
    assert loader._estimators[(W, H)].levels == 1 and loader._estimators[(W, H)].reach == 10
