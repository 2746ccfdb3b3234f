"""lsfa_mv_estimate_chain / lsfa_mv_segment_inputs (lsfa_amd/csrc/me.hip, me_segment.hip), hip.SegmentMotionEstimator and
TestLoader(estimate_mv=...) on the GPU: the chained search against tests/ref_me.py and the per-pair kernel, the segment's inputs against
the per-frame MotionEstimator and the oracle's accumulation + np_ref.transform_mv_res, all bit for bit; graph capture, the error paths and
the batched pipeline fed from frames alone.  tests/test_me_segment_cpu.py pins the identity the inputs kernel rests on."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import oracle
import ref_me
import ref_me_segment
from me_util import clip, plane_stack, t
from oracle import np_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SMALL = [(96, 64), (37, 23), (250, 130)]                      # (width, height): whole blocks; one partial row and column; 10 columns / 2 rows
PARAMS = [(4, 0, 0), (16, 4, 0), (32, 4, 20000)]              # (search, lambda, max_sad)
SCALES = [1.0, 1.25, 0.6, 0.5]                                # h1 / w1 are no multiples of 16: the padded region is read
MEANS = (102.9801, 115.9465, 122.7717)
PIXEL_SCALE = 0.5


_PAIRS = {}


def reference_pairs(size, params):
    """eleven frames of one clip: luma planes, and rows / SAD of the ten pairs (i, i - 1) by tests/ref_me.py - computed once per (size,
    parameters), shared by every (F, C) of the case.  Chain 0 of a stack is frames 0 .. F, chain 1 frames 1 .. F + 1: different content at
    every (chain, frame) position, ten host searches in all."""
    if (size, params) not in _PAIRS:
        width, height = size
        planes = [ref_me.luma(f) for f in clip(11, width, height, seed=width)]
        with ThreadPoolExecutor(8) as ex:
            ref = list(ex.map(lambda i: ref_me.estimate(planes[i], planes[i - 1], *params), range(1, 11)))
        _PAIRS[(size, params)] = (planes, ref)
    return _PAIRS[(size, params)]


@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("size", SMALL)
def test_chain_search_equals_the_reference_and_the_pair_kernel(hip, size, params):
    """rows and SAD of every pair of (C, F + 1) stacks, F in {1, 3, 9}, C in {1, 2} == ref_me.estimate == hip.mv_estimate of that pair"""
    planes, ref = reference_pairs(size, params)
    search, lam, max_sad = params
    dev = [t(p) for p in planes]
    for i in range(1, 11):
        rows, sad = hip.mv_estimate(dev[i], dev[i - 1], search=search, lam=lam, max_sad=max_sad, return_sad=True)
        np.testing.assert_array_equal(rows.cpu().numpy(), ref[i - 1][0])
        np.testing.assert_array_equal(sad.cpu().numpy(), ref[i - 1][1])
    for F in (1, 3, 9):
        for C in (1, 2):
            stack = plane_stack(planes, [list(range(c, c + F + 1)) for c in range(C)])
            rows, sad = hip.mv_estimate_chain(stack, search=search, lam=lam, max_sad=max_sad, return_sad=True)
            assert rows.dtype == torch.int32 and tuple(rows.shape) == (C, F) + ref[0][0].shape and tuple(sad.shape) == (C, F) + ref[0][1].shape
            rows, sad = rows.cpu().numpy(), sad.cpu().numpy()
            for c in range(C):
                for f in range(1, F + 1):
                    np.testing.assert_array_equal(rows[c, f - 1], ref[c + f - 1][0], err_msg="rows F=%d C=%d pair (%d, %d)" % (F, C, c, f))
                    np.testing.assert_array_equal(sad[c, f - 1], ref[c + f - 1][1], err_msg="SAD F=%d C=%d pair (%d, %d)" % (F, C, c, f))
            # without the optional output
            np.testing.assert_array_equal(hip.mv_estimate_chain(stack, search=search, lam=lam, max_sad=max_sad).cpu().numpy(), rows)


def test_chain_search_with_a_plane_stride_beyond_the_plane(hip):
    """planes 1,024 bytes further apart than they are large; the bytes between them (0xA5) are never part of a sum"""
    size, params = (250, 130), (16, 4, 0)
    planes, ref = reference_pairs(size, params)
    stack = plane_stack(planes, [[0, 1, 2, 3], [1, 2, 3, 4]], stride=250 * 130 + 1024)
    assert stack.stride(1) == 250 * 130 + 1024 and not stack.is_contiguous()
    rows, sad = hip.mv_estimate_chain(stack, *params, return_sad=True)
    for c in range(2):
        for f in range(1, 4):
            np.testing.assert_array_equal(rows[c, f - 1].cpu().numpy(), ref[c + f - 1][0])
            np.testing.assert_array_equal(sad[c, f - 1].cpu().numpy(), ref[c + f - 1][1])


@pytest.mark.parametrize("size,C,F,gap", [((40, 24), 1, 1, 0), ((250, 130), 2, 2, 0), ((37, 23), 1, 2, 12)])
def test_chain_search_on_a_stack_stored_in_reverse(hip, size, C, F, gap):
    """lsfa_mv_estimate_chain with a negative plane stride: plane 0 of the stack is the LAST plane in memory, every other one a padded
    plane size in front of the one before it, so that the chain offset c * (F + 1) is walked backwards too.  Rows and SAD of every pair ==
    hip.mv_estimate of that pair == ref_me.estimate.  40 x 24: one whole block and blocks cut by the right and the bottom edge.  37 x 23:
    W * H % 4 != 0 and the planes a further 12 bytes apart, so the stride exceeds the plane (0xA5 between the planes)."""
    width, height = size
    planes = [ref_me.luma(f) for f in clip(C + F, width, height, seed=width)]
    chains = [list(range(c, c + F + 1)) for c in range(C)]
    in_stack_order = [i for chain in chains for i in chain]
    N, stride = C * (F + 1), -(-height * width // 4) * 4 + gap
    memory = plane_stack(planes, [in_stack_order[::-1]], stride=stride)[0]  # memory plane m holds stack plane N - 1 - m
    assert memory.stride(0) == stride
    dev = [t(p) for p in planes]
    mbh, mbw = -(-height // 16), -(-width // 16)
    zeroed = 0
    for max_sad in (0, 900):
        rows = torch.full((C, F, mbh * mbw, 7), -7, dtype=torch.int32, device=DEV)
        sad = torch.full((C, F, mbh, mbw), -7, dtype=torch.int32, device=DEV)
        rc = hip.lib().lsfa_mv_estimate_chain(memory[N - 1].data_ptr(), -stride, C, F, width, height, 4, 4, max_sad, rows.data_ptr(), sad.data_ptr(), None)
        assert rc == 0, hip.lib().lsfa_last_error()
        torch.cuda.synchronize()
        for c in range(C):
            for f in range(1, F + 1):
                cur, ref = chains[c][f], chains[c][f - 1]
                pair_rows, pair_sad = hip.mv_estimate(dev[cur], dev[ref], 4, 4, max_sad, return_sad=True)
                assert torch.equal(rows[c, f - 1], pair_rows) and torch.equal(sad[c, f - 1], pair_sad), (max_sad, c, f)
                want_rows, want_sad = ref_me.estimate(planes[cur], planes[ref], 4, 4, max_sad)
                np.testing.assert_array_equal(rows[c, f - 1].cpu().numpy(), want_rows, err_msg="rows max_sad %d pair (%d, %d)" % (max_sad, c, f))
                np.testing.assert_array_equal(sad[c, f - 1].cpu().numpy(), want_sad, err_msg="SAD max_sad %d pair (%d, %d)" % (max_sad, c, f))
                zeroed += int((want_sad > max_sad).sum()) if max_sad else 0
    assert zeroed > 0           # the threshold bites somewhere


def test_chain_search_full_size_equals_the_pair_kernel(hip):
    """1000 x 600, F = 9 (21,546 workgroups in one grid): device against device, pair by pair"""
    planes = [ref_me.luma(f) for f in clip(10, 1000, 600, seed=7, m=(-5, 7))]
    stack = plane_stack(planes, [list(range(10))])
    assert stack.is_contiguous()
    rows, sad = hip.mv_estimate_chain(stack, 16, 4, 0, return_sad=True)
    for f in range(1, 10):
        want_rows, want_sad = hip.mv_estimate(stack[0, f], stack[0, f - 1], 16, 4, 0, return_sad=True)
        assert torch.equal(rows[0, f - 1], want_rows) and torch.equal(sad[0, f - 1], want_sad), f
    v = rows[0, :, :, 5:7] - rows[0, :, :, 3:5]
    assert int(((v[..., 0] == -5) & (v[..., 1] == 7)).sum()) >= 9 * 2294         # what tests/test_me_cpu.py derives per pair


# ---- the segment's inputs -------------------------------------------------------------------------------------------------------------------
def per_frame_inputs(hip, frames, search, lam, max_sad, scales, means=MEANS, pixel_scale=PIXEL_SCALE):
    """hip.MotionEstimator over frames[0] (key) .. frames[n]: {scale: (mv (n, 2, h, w), res (n, 3, h, w))}"""
    height, width = frames[0].shape[:2]
    me = hip.MotionEstimator(width, height, DEV, search=search, lam=lam, max_sad=max_sad)
    dev = [t(f) for f in frames]
    me.key_frame(dev[0])
    out = {s: ([], []) for s in scales}
    for f in range(1, len(frames)):
        me.next_frame(dev[f])
        for s in scales:
            mv, res = me.network_inputs(dev[f], dev[0], s, means, pixel_scale)
            out[s][0].append(mv[0].clone())
            out[s][1].append(res[0].clone())
    return {s: (torch.stack(a), torch.stack(b)) for s, (a, b) in out.items()}


def host_inputs(frames, search, lam, max_sad, scale, means=MEANS, pixel_scale=PIXEL_SCALE):
    """ref_me rows, oracle.coviar_accumulate frame by frame, np_ref.transform_mv_res: [(mv (2, h, w), res (3, h, w)) float32 per frame]"""
    height, width = frames[0].shape[:2]
    lum = [ref_me.luma(f) for f in frames]
    accu = oracle.coviar_identity(width, height)
    out = []
    for f in range(1, len(frames)):
        accu = oracle.coviar_accumulate(ref_me.estimate(lum[f], lum[f - 1], search, lam, max_sad)[0], accu)
        mv, res = np_ref.transform_mv_res(-oracle.coviar_mv(accu).astype(np.float32), oracle.coviar_residual(frames[f], frames[0], accu).astype(np.float32),
                                          scale, means, pixel_scale)
        out.append((mv.astype(np.float32)[0], res.astype(np.float32)[0]))
    return out


@pytest.mark.parametrize("size", SMALL)
def test_segment_inputs_equal_the_per_frame_chain_and_the_oracle(hip, size):
    """every frame of F = 9 at every scale == MotionEstimator.network_inputs == np_ref.transform_mv_res of the oracle's accumulation"""
    width, height = size
    frames = clip(10, width, height, seed=width + 1)
    sme = hip.SegmentMotionEstimator(width, height, frames=9, clips=1, device=DEV, search=8, lam=4)
    stack = t(np.stack(frames)[None])
    want = per_frame_inputs(hip, frames, 8, 4, 0, SCALES)
    for s in SCALES:
        mv, res = sme.segment(stack, s, MEANS, PIXEL_SCALE)
        assert tuple(mv.shape) == (9, 1) + tuple(want[s][0].shape[1:]) and tuple(res.shape) == (9, 1) + tuple(want[s][1].shape[1:])
        assert torch.equal(mv[:, 0], want[s][0]) and torch.equal(res[:, 0], want[s][1]), s
        host = host_inputs(frames, 8, 4, 0, s)
        for f in range(9):
            np.testing.assert_array_equal(mv[f, 0].cpu().numpy(), host[f][0], err_msg="mv scale %g frame %d" % (s, f + 1))
            np.testing.assert_array_equal(res[f, 0].cpu().numpy(), host[f][1], err_msg="res scale %g frame %d" % (s, f + 1))
        assert float(mv.abs().max()) > 0
    assert tuple(sme.rows.shape) == (1, 9, sme.mbh * sme.mbw, 7) and tuple(sme.sad.shape) == (1, 9, sme.mbh, sme.mbw)
    lum = [ref_me.luma(f) for f in frames]
    np.testing.assert_array_equal(sme.rows[0, 8].cpu().numpy(), ref_me.estimate(lum[9], lum[8], 8, 4)[0])


def test_segment_inputs_full_size_equal_the_per_frame_chain(hip):
    """1000 x 600, F = 9, every scale: device against device (the host chain costs seconds per pair here)"""
    frames = clip(10, 1000, 600, seed=9, m=(-5, 7))
    sme = hip.SegmentMotionEstimator(1000, 600, frames=9, device=DEV, search=16, lam=4)
    stack = t(np.stack(frames)[None])
    want = per_frame_inputs(hip, frames, 16, 4, 0, SCALES)
    for s in SCALES:
        mv, res = sme.segment(stack, s, MEANS, PIXEL_SCALE)
        assert torch.equal(mv[:, 0], want[s][0]) and torch.equal(res[:, 0], want[s][1]), s
    assert tuple(mv.shape) == (9, 1, 2, 19, 32)


def test_segment_inputs_with_blocks_zeroed_mid_chain(hip):
    """max_sad = 900 on a noisy clip: zero and non-zero vectors in one chain (identity steps of the walk)"""
    width, height = 96, 64
    frames = clip(10, width, height, seed=width)
    sme = hip.SegmentMotionEstimator(width, height, frames=9, device=DEV, search=8, lam=4, max_sad=900)
    mv, res = sme.segment(t(np.stack(frames)[None]), 1.25, MEANS, PIXEL_SCALE)
    v = (sme.rows[0, :, :, 3:5] - sme.rows[0, :, :, 5:7]).cpu().numpy()
    zero = (v == 0).all(axis=2)
    assert zero.any() and not zero.all()
    want = per_frame_inputs(hip, frames, 8, 4, 900, [1.25])[1.25]
    assert torch.equal(mv[:, 0], want[0]) and torch.equal(res[:, 0], want[1])
    for f, (h_mv, h_res) in enumerate(host_inputs(frames, 8, 4, 900, 1.25)):
        np.testing.assert_array_equal(mv[f, 0].cpu().numpy(), h_mv)
        np.testing.assert_array_equal(res[f, 0].cpu().numpy(), h_res)


def test_two_clips_in_lock_step(hip):
    """C = 2: out[f - 1][c] is clip c's frame f - the layout a batch of lock-step clips hands to cur_frame / cur_segment"""
    width, height = 250, 130
    clips = [clip(10, width, height, seed=3), clip(10, width, height, seed=4, m=(-4, 5))]
    sme = hip.SegmentMotionEstimator(width, height, frames=9, clips=2, device=DEV, search=16, lam=4)
    mv, res = sme.segment(t(np.stack([np.stack(c) for c in clips])), 0.6, MEANS, PIXEL_SCALE)
    assert tuple(mv.shape)[:3] == (9, 2, 2) and tuple(res.shape)[:3] == (9, 2, 3)
    for c in range(2):
        want = per_frame_inputs(hip, clips[c], 16, 4, 0, [0.6])[0.6]
        assert torch.equal(mv[:, c], want[0]) and torch.equal(res[:, c], want[1]), c
    assert not torch.equal(mv[:, 0], mv[:, 1])


def test_short_segment(hip):
    """n < frames: a stack of n + 1 frames, or the first n + 1 of a longer one, through an estimator built for nine"""
    width, height = 96, 64
    frames = clip(10, width, height, seed=12)
    sme = hip.SegmentMotionEstimator(width, height, frames=9, device=DEV, search=8, lam=4)
    stack = t(np.stack(frames)[None])
    full_mv, full_res = [x.clone() for x in sme.segment(stack, 1.0, MEANS, PIXEL_SCALE)]
    for n in (1, 4):
        a_mv, a_res = sme.segment(stack, 1.0, MEANS, PIXEL_SCALE, n=n)
        assert tuple(a_mv.shape)[:2] == (n, 1) and torch.equal(a_mv, full_mv[:n]) and torch.equal(a_res, full_res[:n]), n
        assert tuple(sme.rows.shape)[:2] == (1, n)
        b_mv, b_res = sme.segment(stack[:, :n + 1].contiguous(), 1.0, MEANS, PIXEL_SCALE)
        assert torch.equal(b_mv, full_mv[:n]) and torch.equal(b_res, full_res[:n]), n
    with pytest.raises(hip.LsfaError, match="non-key frames"):
        sme.segment(stack, 1.0, MEANS, PIXEL_SCALE, n=10)
    with pytest.raises(hip.LsfaError, match="non-key frames"):
        hip.SegmentMotionEstimator(width, height, frames=4, device=DEV).segment(stack, 1.0)


@pytest.mark.parametrize("size,search", [((1000, 600), 8), ((250, 130), 16)])
def test_translated_texture_through_the_inputs(hip, size, search):
    """test_motion_estimator_chain's clip, m = (3, -2), nine frames: on pixels at least 48 from the border the residual against the key frame
    is 0 and the accumulated vector 9 m.  Read from the inputs of frame 9 at scale 1 with zero means: output cell (Y, X) reads rows 16 Y + 7,
    16 Y + 8 and columns 16 X + 7, 16 X + 8, so the cells wholly inside hold -9 m / 16 (the negated vectors, in stride-16 cells) and 0."""
    width, height = size
    m = (3, -2)
    frames = ref_me.translated_clip(10, width, height, m, seed=width)
    sme = hip.SegmentMotionEstimator(width, height, frames=9, device=DEV, search=search, lam=4)
    mv, res = sme.segment(t(np.stack(frames)[None]), 1.0, (0.0, 0.0, 0.0), 1.0)
    ys = [Y for Y in range(mv.shape[3]) if 16 * Y + 7 >= 48 and 16 * Y + 8 < height - 48]
    xs = [X for X in range(mv.shape[4]) if 16 * X + 7 >= 48 and 16 * X + 8 < width - 48]
    assert len(ys) >= 2 and len(xs) >= 10
    inner_mv = mv[8, 0][:, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1].cpu().numpy()
    inner_res = res[8, 0][:, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1].cpu().numpy()
    assert (inner_mv[0] == -9 * m[0] / 16.0).all() and (inner_mv[1] == -9 * m[1] / 16.0).all()
    assert (inner_res == 0).all()
    assert float(res[8].abs().max()) > 0                      # the border blocks' chain is not exact


def test_rows_outside_the_contract_follow_the_walk(hip):
    """Rows that are not the estimator's - sources outside the frame, vectors far beyond any search - give the walk's own result, checked by
    value: a step whose source leaves the frame is not taken (tests/ref_me_segment.py), and every read stays inside the frames."""
    width, height = 96, 64
    frames = clip(4, width, height, seed=5)
    zero = np.zeros((height, width), np.uint8)
    rows = np.stack([ref_me.estimate(zero, zero, 4, 0)[0]] * 3).copy()          # three frames of zero vectors
    rs = np.random.RandomState(0)
    rows[:, :, 3] += rs.randint(-120, 121, rows.shape[:2])                         # sources anywhere within +-120 pixels: many outside
    rows[:, :, 4] += rs.randint(-80, 81, rows.shape[:2])
    rows[1, 5, 3:5] = (2 ** 31 - 1, -2 ** 31)                                      # and two that overflow a 32-bit difference
    rows[2, 7, 3:5] = (-2 ** 31, 2 ** 31 - 1)
    accus = ref_me_segment.walk(rows, width, height)
    taken = sum(int((a != oracle.coviar_identity(width, height)).any(axis=2).sum()) for a in accus)
    assert 0 < taken < 3 * width * height
    stack = t(np.stack(frames)[None])
    for s in (1.0, 0.6):
        mv, res = hip.mv_segment_inputs(t(rows[None]), stack, s, MEANS, PIXEL_SCALE)
        for f in range(3):
            w_mv, w_res = np_ref.transform_mv_res(-ref_me_segment.field(accus[f]).astype(np.float32),
                                                  ref_me_segment.residual(frames[f + 1], frames[0], accus[f]).astype(np.float32), s, MEANS, PIXEL_SCALE)
            np.testing.assert_array_equal(mv[f].cpu().numpy(), w_mv.astype(np.float32))
            np.testing.assert_array_equal(res[f].cpu().numpy(), w_res.astype(np.float32))


def test_segment_graph_capture(hip):
    """segment captured with torch.cuda.graph on one stream (no parallel branches), replayed on NEW frame contents written into the same
    stack == the eager result on those contents"""
    width, height = 250, 130
    clips = [clip(6, width, height, seed=1, sigma=0.0), clip(6, width, height, seed=2, m=(-4, 5))]
    buf = t(np.stack(clips[0])[None]).clone()
    sme = hip.SegmentMotionEstimator(width, height, frames=5, device=DEV, search=16, lam=4)
    sme.segment(buf, 1.25, MEANS, PIXEL_SCALE)              # warm-up: the outputs are allocated at the first call for a scale and a length
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_mv, out_res = sme.segment(buf, 1.25, MEANS, PIXEL_SCALE)
    eager = hip.SegmentMotionEstimator(width, height, frames=5, device=DEV, search=16, lam=4)
    seen = []
    for k, c in enumerate(clips[::-1] + clips):
        buf.copy_(t(np.stack(c)[None]))
        g.replay()
        torch.cuda.synchronize()
        e_mv, e_res = eager.segment(t(np.stack(c)[None]), 1.25, MEANS, PIXEL_SCALE)
        assert torch.equal(out_mv, e_mv) and torch.equal(out_res, e_res), k
        assert torch.equal(sme.rows, eager.rows) and torch.equal(sme.sad, eager.sad), k
        seen.append(out_mv.clone())
    assert not torch.equal(seen[0], seen[1])


def test_segment_yuv_equals_segment_on_the_converted_frames(hip):
    """segment_yuv (NV12, two clips of four frames in one conversion launch) == segment on yuv420_to_bgr_u8's frames; luma_from='y' searches
    the decoder's Y planes"""
    width, height, C, n = 96, 64, 2, 3
    rs = np.random.RandomState(3)
    N = C * (n + 1)
    base = clip(N, width, height, seed=8)
    y = t(np.stack([ref_me.luma(f) for f in base]))
    uv = t(rs.randint(96, 160, (N, height // 2, width)).astype(np.uint8))
    bgr = hip.yuv420_to_bgr_u8(y, uv).view(C, n + 1, height, width, 3)
    sme = hip.SegmentMotionEstimator(width, height, frames=9, clips=C, device=DEV, search=8, lam=4)
    want_mv, want_res = [x.clone() for x in sme.segment(bgr, 1.0, MEANS, PIXEL_SCALE)]
    mv, res = sme.segment_yuv(y, uv, im_scale=1.0, pixel_means=MEANS, pixel_scale=PIXEL_SCALE)
    assert torch.equal(mv, want_mv) and torch.equal(res, want_res) and torch.equal(sme.bgr, bgr)
    from_y = hip.SegmentMotionEstimator(width, height, frames=9, clips=C, device=DEV, search=8, lam=4, luma_from='y')
    from_y.segment_yuv(y, uv, im_scale=1.0, pixel_means=MEANS, pixel_scale=PIXEL_SCALE)
    assert torch.equal(from_y.rows, hip.mv_estimate_chain(y.view(C, n + 1, height, width), 8, 4, 0))


def test_error_paths(hip):
    """every LSFA_REQUIRE of the two exports: an error code and its message, nothing launched; the wrappers raise LsfaError"""
    L = hip.lib()
    W, H = 96, 64
    luma = torch.zeros((1, 3, H, W), dtype=torch.uint8, device=DEV)
    bgr = torch.zeros((1, 3, H, W, 3), dtype=torch.uint8, device=DEV)
    rows = torch.zeros((1, 2, 24, 7), dtype=torch.int32, device=DEV)
    sad = torch.full((1, 2, 4, 6), -7, dtype=torch.int32, device=DEV)
    mv = torch.full((2, 1, 2, 4, 6), -7.0, device=DEV)
    res = torch.full((2, 1, 3, 4, 6), -7.0, device=DEV)
    rows_before = rows.clone()
    means = (ctypes.c_double * 3)(*MEANS)

    def chain(**kw):
        a = dict(luma=luma.data_ptr(), stride=W * H, C=1, F=2, W=W, H=H, R=16, lam=4, max_sad=0, mvs=rows.data_ptr(), sad=sad.data_ptr())
        a.update(kw)
        return L.lsfa_mv_estimate_chain(a['luma'], a['stride'], a['C'], a['F'], a['W'], a['H'], a['R'], a['lam'], a['max_sad'], a['mvs'], a['sad'], None)

    def inputs(**kw):
        a = dict(mvs=rows.data_ptr(), bgr=bgr.data_ptr(), stride=W * H * 3, C=1, F=2, W=W, H=H, scale=1.0, h1=H, w1=W, rs=16, means=means, ps=1.0,
                 mv=mv.data_ptr(), res=res.data_ptr(), oh=4, ow=6)
        a.update(kw)
        return L.lsfa_mv_segment_inputs(a['mvs'], a['bgr'], a['stride'], a['C'], a['F'], a['W'], a['H'], a['scale'], a['h1'], a['w1'], a['rs'], a['means'],
                                        a['ps'], a['mv'], a['res'], a['oh'], a['ow'], None)

    for call, kw, text in ((chain, dict(luma=None), b"NULL"), (chain, dict(mvs=None), b"NULL"), (chain, dict(W=0), b"bad frame size"),
                           (chain, dict(H=-1), b"bad frame size"), (chain, dict(R=0), b"search 0"), (chain, dict(R=33), b"search 33"),
                           (chain, dict(lam=-1), b"lambda -1"), (chain, dict(lam=(1 << 24) + 1), b"lambda"), (chain, dict(max_sad=-1), b"max_sad -1"),
                           (chain, dict(C=0), b"at least 1"), (chain, dict(F=0), b"at least 1"), (chain, dict(stride=W * H - 4), b"plane stride"),
                           (chain, dict(stride=W * H + 2), b"multiple of 4"), (chain, dict(luma=luma.data_ptr() + 1), b"4-byte aligned"),
                           (chain, dict(C=1 << 16, F=1 << 12), b"exceed one grid"),
                           (inputs, dict(mvs=None), b"NULL"), (inputs, dict(bgr=None), b"NULL"), (inputs, dict(means=None), b"NULL"),
                           (inputs, dict(mv=None), b"NULL"), (inputs, dict(res=None), b"NULL"), (inputs, dict(W=0), b"bad frame size"),
                           (inputs, dict(C=0), b"at least 1"), (inputs, dict(F=0), b"at least 1"), (inputs, dict(stride=W * H * 3 - 1), b"frame stride"),
                           (inputs, dict(h1=0), b"bad shape"), (inputs, dict(w1=-3), b"bad shape"), (inputs, dict(rs=0), b"bad shape"),
                           (inputs, dict(scale=0.0), b"bad shape"), (inputs, dict(oh=5), b"outputs are 5 x 6"), (inputs, dict(ow=7), b"outputs are 4 x 7"),
                           (inputs, dict(h1=H + 16), b"outputs are 4 x 6"), (inputs, dict(C=1 << 12, F=1 << 12), b"exceed one launch")):
        assert call(**kw) != 0, kw
        msg = L.lsfa_last_error()
        assert text in msg and (b"lsfa_mv_estimate_chain" if call is chain else b"lsfa_mv_segment_inputs") in msg, (kw, msg)
    torch.cuda.synchronize()
    assert torch.equal(rows, rows_before) and (sad == -7).all() and (mv == -7).all() and (res == -7).all()        # nothing was launched
    assert chain() == 0 and inputs() == 0
    torch.cuda.synchronize()
    assert (sad == 0).all() and not (mv == -7).any()

    for bad in (dict(search=0), dict(search=33), dict(lam=-1), dict(max_sad=-1)):
        with pytest.raises(hip.LsfaError, match="lsfa_mv_estimate_chain"):
            hip.mv_estimate_chain(luma, **bad)
    with pytest.raises(hip.LsfaError, match="uint8 CUDA stack"):
        hip.mv_estimate_chain(luma.float())
    with pytest.raises(hip.LsfaError, match="uint8 CUDA stack"):
        hip.mv_estimate_chain(luma[0])                        # no chain axis
    with pytest.raises(hip.LsfaError, match="uint8 CUDA stack"):
        hip.mv_estimate_chain(luma[:, :1])                    # a key frame alone
    with pytest.raises(hip.LsfaError, match="uint8 CUDA stack"):
        hip.mv_estimate_chain(luma.cpu())
    with pytest.raises(hip.LsfaError, match="dense frames"):
        hip.mv_estimate_chain(luma[:, :, :, ::2])
    with pytest.raises(hip.LsfaError, match="output buffer"):
        hip.mv_estimate_chain(luma, out=rows[:, :1])
    with pytest.raises(hip.LsfaError, match="rows must be"):
        hip.mv_segment_inputs(rows[:, :1], bgr, 1.0)
    with pytest.raises(hip.LsfaError, match="rows must be"):
        hip.mv_segment_inputs(rows.float(), bgr, 1.0)
    with pytest.raises(hip.LsfaError, match="uint8 CUDA stack"):
        hip.mv_segment_inputs(rows, bgr[..., :2], 1.0)
    with pytest.raises(hip.LsfaError, match="im_scale"):
        hip.mv_segment_inputs(rows, bgr, 0.0)
    with pytest.raises(hip.LsfaError, match="output buffer"):
        hip.mv_segment_inputs(rows, bgr, 1.0, out=(mv, res[:1]))
    with pytest.raises(hip.LsfaError, match="search 40"):
        hip.SegmentMotionEstimator(W, H, device=DEV, search=40)
    with pytest.raises(hip.LsfaError, match="frames 0"):
        hip.SegmentMotionEstimator(W, H, frames=0, device=DEV)
    with pytest.raises(hip.LsfaError, match="luma_from"):
        hip.SegmentMotionEstimator(W, H, device=DEV, luma_from='u')
    sme = hip.SegmentMotionEstimator(W, H, frames=2, device=DEV)
    with pytest.raises(hip.LsfaError, match="uint8 stack"):
        sme.segment(bgr[0], 1.0)
    with pytest.raises(hip.LsfaError, match="uint8 stack"):
        sme.segment(bgr[:, :, :32], 1.0)
    torch.cuda.synchronize()


def test_prof_scope_counts_both_launches(hip):
    luma = torch.zeros((1, 3, 64, 96), dtype=torch.uint8, device=DEV)
    bgr = torch.zeros((1, 3, 64, 96, 3), dtype=torch.uint8, device=DEV)
    hip.prof_enable(True, ops=["mv_estimate"])
    try:
        hip.mv_segment_inputs(hip.mv_estimate_chain(luma), bgr, 1.0)
        ms, n = hip.prof_read()["mv_estimate"]
    finally:
        hip.prof_enable(False)
    assert n == 2 and ms > 0.0


# ---- frames alone into the batched pipeline --------------------------------------------------------------------------------------------------
class PerFrameEstimator(object):
    """hip.MotionEstimator behind SegmentMotionEstimator.segment's interface: the per-frame chain on the same frames"""

    def __init__(self, hip, width, height, **kw):
        self.me = hip.MotionEstimator(width, height, DEV, **kw)

    def segment(self, stack, im_scale, pixel_means, pixel_scale):
        self.me.key_frame(stack[0, 0])
        mvs, ress = [], []
        for f in range(1, int(stack.shape[1])):
            self.me.next_frame(stack[0, f])
            mv, res = self.me.network_inputs(stack[0, f], stack[0, 0], im_scale, pixel_means, pixel_scale)
            mvs.append(mv.clone())
            ress.append(res.clone())
        return torch.stack(mvs), torch.stack(ress)


@pytest.mark.parametrize("segment,key_group", [(9, 2), (0, 1)])
def test_pipeline_from_frames_alone(hip, monkeypatch, segment, key_group):
    """One synthetic clip of 24 frames at key interval 10 (segments of 9, 9 and 2 non-key frames; the last frame is a key frame) through
    pred_eval_pipelined on TestLoader(estimate_mv=...): the same detections, bit for bit, as the same pipeline fed the per-frame
    MotionEstimator's outputs for the same frames."""
    from lsfa_amd.config.config import lsfa_test_config
    from lsfa_amd.core.loader import TestLoader
    from lsfa_amd.function import test_rcnn as T
    from lsfa_amd.symbols import params as P
    from lsfa_amd.utils.synthetic import synthetic_roidb
    H, W = 96, 160
    cfg = lsfa_test_config(key_frame_interval=10)
    arg, aux = P.init_params(cfg, seed=3)
    roidb = synthetic_roidb(1, 24, H, W, 10)
    cfg.TEST.ESTIMATE_MV = dict(search=8, lam=4)             # test_rcnn builds its loader itself: the option reaches it through the config
    calls = []

    class SegmentLoader(TestLoader):
        def _estimate_segment(self, entry, key_f):
            before = self._segment
            TestLoader._estimate_segment(self, entry, key_f)
            if self._segment is not None and self._segment is not before:
                calls.append((key_f, self._segment[1]))

    class PerFrameLoader(TestLoader):
        def _segment_estimator(self, width, height):
            return PerFrameEstimator(hip, width, height, **self.estimate_mv)

    monkeypatch.setattr(T, "TestLoader", SegmentLoader)
    rows_s, ids_s = T.test_rcnn(cfg, roidb, arg, aux, device=DEV, pipeline=True, segment=segment, key_group=key_group)
    assert calls == [(0, 9), (10, 9), (20, 2)]
    monkeypatch.setattr(T, "TestLoader", PerFrameLoader)
    rows_f, ids_f = T.test_rcnn(cfg, roidb, arg, aux, device=DEV, pipeline=True, segment=segment, key_group=key_group)
    np.testing.assert_array_equal(ids_s, ids_f)
    assert len(rows_s) > 0
    np.testing.assert_array_equal(rows_s, rows_f)
    if segment == 0:
        # ... and the estimated inputs are not the clip's own: the detections differ from the default path's
        monkeypatch.setattr(T, "TestLoader", TestLoader)
        rows_d, _ = T.test_rcnn(lsfa_test_config(key_frame_interval=10), roidb, arg, aux, device=DEV, pipeline=True, segment=segment, key_group=key_group)
        assert rows_d.shape != rows_s.shape or not np.array_equal(rows_d, rows_s)
        # the serial loop takes the same loader
        monkeypatch.setattr(T, "TestLoader", SegmentLoader)
        rows_q, ids_q = T.test_rcnn(cfg, roidb, arg, aux, device=DEV, pipeline=False)
        np.testing.assert_array_equal(ids_q, ids_s)
        np.testing.assert_array_equal(rows_q, rows_s)
