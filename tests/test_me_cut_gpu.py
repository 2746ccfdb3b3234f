"""lsfa_mv_cut_score (lsfa_amd/csrc/me_cut.hip), hip.SegmentMotionEstimator / hip.MotionEstimator with cut= and
TestLoader(estimate_mv=dict(cut=...)) on the GPU: the two kernels against tests/ref_me_cut.py bit for bit on the SADs of both searches, the
estimators with the mode on against the same estimators with it off, graph capture, the refusals, and a synthetic clip with two cuts
through both frame loops.  tests/test_me_cut_cpu.py pins the reference and the margin the end-to-end expectations rest on."""
import numpy as np
import pytest
import torch

import me_util
import ref_me
import ref_me_cut as rc
from me_util import plane_stack, t

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MEANS = (102.9801, 115.9465, 122.7717)
PIXEL_SCALE = 0.5


def bgr_two_scenes(width, height, a=3, b=2):
    """the first `a` frames of the three-frame seed-1 translated clip, then the first `b` of the two-frame seed-2 clip (the clips
    tests/test_me_cut_cpu.py records its figures on): a cut between frame a - 1 and frame a"""
    return me_util.clip(3, width, height, seed=1)[:a] + me_util.clip(2, width, height, seed=2)[:b]


def two_scenes(width, height, a=3, b=2):
    """bgr_two_scenes as luma planes"""
    return [ref_me.luma(f) for f in bgr_two_scenes(width, height, a, b)]


def check_cut_score(hip, planes, chains, stack, sad, biases=(rc.BIAS,)):
    """hip.mv_cut_score(stack, sad, bias) == ref_me_cut.cut_score on the same planes and the same SAD, intra and unmatched, bit for bit"""
    host = np.stack([np.stack([planes[i] for i in chain]) for chain in chains])
    C, F = len(chains), len(chains[0]) - 1
    mbh, mbw = -(-host.shape[2] // 16), -(-host.shape[3] // 16)
    seen = []
    for bias in biases:
        intra, unmatched = hip.mv_cut_score(stack, sad, bias)
        assert intra.dtype == torch.int32 and tuple(intra.shape) == (C, F, mbh, mbw)
        assert unmatched.dtype == torch.int32 and tuple(unmatched.shape) == (C, F)
        want_intra, want_un = rc.cut_score(host, sad.cpu().numpy(), bias)
        np.testing.assert_array_equal(intra.cpu().numpy(), want_intra, err_msg="intra, bias %d" % bias)
        np.testing.assert_array_equal(unmatched.cpu().numpy(), want_un, err_msg="unmatched, bias %d" % bias)
        seen.append(want_un)
    return seen


# ---- lsfa_mv_cut_score -----------------------------------------------------------------------------------------------------------------------------
def test_cut_score_small_unaligned_plane(hip):
    """37 x 23, F = 2: rows that are not dword aligned, blocks cut by both edges (5 columns, 7 rows), W * H % 4 != 0 so that the planes lie a
    padded size apart; bias 0, the default and 255.  The second pair is a cut."""
    planes = two_scenes(37, 23, a=2, b=1)
    chains = [[0, 1, 2]]
    stack = plane_stack(planes, chains)
    sad = hip.mv_estimate_chain(stack, 4, 4, 0, return_sad=True)[1]
    un0, un4, un255 = check_cut_score(hip, planes, chains, stack, sad, biases=(0, rc.BIAS, 255))
    assert un4.tolist() == [[4, 6]]                  # the figures tests/test_me_cut_cpu.py records for these two pairs
    assert (un0 >= un4).all() and not un255.any()


@pytest.mark.parametrize("levels", [0, 1])
def test_cut_score_on_both_searches_sad(hip, levels):
    """250 x 130 (10-pixel and 2-row edge blocks), C = 2, F = 3, fed by the full search's SAD and by the pyramid's (L = 1) level-0 SAD; chain 0
    has its cut at f = 3, chain 1 at f = 2"""
    width, height = 250, 130
    planes = two_scenes(width, height)
    chains = [[0, 1, 2, 3], [1, 2, 3, 4]]
    stack = plane_stack(planes, chains)
    if levels == 0:
        sad = hip.mv_estimate_chain(stack, 8, 4, 0, return_sad=True)[1]
    else:
        p1 = hip.luma_pyramid(stack.reshape(8, height, width), 1)[0]
        top = hip.mv_estimate_chain(p1.view(2, 4, p1.shape[1], p1.shape[2]), 8, 4, 0)
        sad = hip.mv_refine_chain(stack, top, 2, 4, 0, return_sad=True)[1]
    un0, un, un255 = check_cut_score(hip, planes, chains, stack, sad, biases=(0, rc.BIAS, 255))
    assert (un0 >= un).all() and un0.sum() > un.sum() and not un255.any()          # the bias decides some blocks
    flags = rc.is_cut(un, 144)
    assert flags.tolist() == [[False, False, True], [False, True, False]], un
    if levels == 0:
        assert int(un[0, 0]) == 9                    # the recorded figure of frames 0 -> 1 of the seed-1 clip
    # ... into the caller's buffers, which are written nowhere else
    intra = torch.full((2, 3, 9, 16), -7, dtype=torch.int32, device=DEV)
    unmatched = torch.full((7,), -7, dtype=torch.int32, device=DEV)
    got = hip.mv_cut_score(stack, sad, out=(intra, unmatched[:6].view(2, 3)))
    assert got[0] is intra and int(unmatched[6]) == -7 and unmatched[:6].tolist() == un.reshape(-1).tolist() and not (intra == -7).any()


def test_cut_score_recorded_cut_pair(hip):
    """the pair behind the figure 131 of 144: frame 1 of the seed-1 clip -> frame 0 of the seed-2 clip, 250 x 130, R = 8; and 96 x 64: 24 of 24"""
    for (width, height), want in (((250, 130), [9, 131]), ((96, 64), [9, 24])):
        planes = two_scenes(width, height, a=2)
        stack = plane_stack(planes, [[0, 1, 2]])
        sad = hip.mv_estimate_chain(stack, 8, 4, 0, return_sad=True)[1]
        assert check_cut_score(hip, planes, [[0, 1, 2]], stack, sad)[0].tolist() == [want]


def test_cut_score_on_a_reversed_pair(hip):
    """the ping-pong form: one pair of 96 x 64 stored in reverse (the current plane in FRONT of the reference plane), the planes 12 bytes
    further apart than they are large - the 0xA5 between them is part of no sum"""
    width, height = 96, 64
    planes = two_scenes(width, height, a=2, b=1)
    stride = width * height + 12
    for ref_i, cur_i in ((0, 1), (1, 2)):
        memory = plane_stack(planes, [[cur_i, ref_i]], stride=stride)[0]           # memory plane 0 = the current frame, plane 1 = the reference
        assert memory.stride(0) == stride
        sad = hip.mv_estimate(memory[0], memory[1], 8, 4, 0, return_sad=True)[1]
        intra = torch.full((4, 6), -7, dtype=torch.int32, device=DEV)
        unmatched = torch.full((2,), -7, dtype=torch.int32, device=DEV)
        code = hip.lib().lsfa_mv_cut_score(memory[1].data_ptr(), -stride, 1, 1, width, height, sad.data_ptr(), rc.BIAS, intra.data_ptr(),
                                           unmatched.data_ptr(), None)
        assert code == 0, hip.lib().lsfa_last_error()
        torch.cuda.synchronize()
        want_intra, want_un = rc.cut_score(np.stack([planes[ref_i], planes[cur_i]])[None], sad.cpu().numpy()[None, None], rc.BIAS)
        np.testing.assert_array_equal(intra.cpu().numpy(), want_intra[0, 0])
        assert unmatched.tolist() == [int(want_un[0, 0]), -7] and int(want_un[0, 0]) == (9 if cur_i == 1 else 24)


def test_cut_score_full_size(hip):
    """1000 x 600, two pairs (the second a cut): 4,788 waves, a bottom row of 8-pixel-high blocks, and more blocks per pair (2,394) than the
    counting workgroup has lanes"""
    width, height = 1000, 600
    planes = two_scenes(width, height, a=2, b=1)
    stack = plane_stack(planes, [[0, 1, 2]])
    sad = hip.mv_estimate_chain(stack, 4, 4, 0, return_sad=True)[1]
    un, = check_cut_score(hip, planes, [[0, 1, 2]], stack, sad)
    assert rc.is_cut(un, 2394).tolist() == [[False, True]], un


def test_cut_score_refusals(hip):
    """every LSFA_REQUIRE of the export: an error code and its message, nothing launched; the wrapper raises LsfaError"""
    L = hip.lib()
    W, H = 96, 64
    luma = torch.zeros((1, 3, H, W), dtype=torch.uint8, device=DEV)
    sad = torch.zeros((1, 2, 4, 6), dtype=torch.int32, device=DEV)
    intra = torch.full((1, 2, 4, 6), -7, dtype=torch.int32, device=DEV)
    unmatched = torch.full((1, 2), -7, dtype=torch.int32, device=DEV)

    def score(**kw):
        a = dict(luma=luma.data_ptr(), stride=W * H, C=1, F=2, W=W, H=H, sad=sad.data_ptr(), bias=4, intra=intra.data_ptr(), un=unmatched.data_ptr())
        a.update(kw)
        return L.lsfa_mv_cut_score(a['luma'], a['stride'], a['C'], a['F'], a['W'], a['H'], a['sad'], a['bias'], a['intra'], a['un'], None)

    for kw, text in ((dict(luma=None), b"NULL"), (dict(sad=None), b"NULL"), (dict(intra=None), b"NULL"), (dict(un=None), b"NULL"),
                     (dict(bias=-1), b"bias -1"), (dict(bias=256), b"bias 256"), (dict(W=0), b"bad frame size"), (dict(H=-1), b"bad frame size"),
                     (dict(C=0), b"at least 1"), (dict(F=0), b"at least 1"), (dict(stride=W * H - 4), b"plane stride"),
                     (dict(stride=-(W * H - 4)), b"plane stride"), (dict(stride=W * H + 2), b"multiple of 4"), (dict(stride=1 << 36), b"2^36"),
                     (dict(luma=luma.data_ptr() + 1), b"4-byte aligned"), (dict(C=1 << 16, F=1 << 12), b"exceed one grid")):
        assert score(**kw) != 0, kw
        msg = L.lsfa_last_error()
        assert text in msg and b"lsfa_mv_cut_score" in msg, (kw, msg)
    torch.cuda.synchronize()
    assert (intra == -7).all() and (unmatched == -7).all()          # nothing was launched
    assert score() == 0
    torch.cuda.synchronize()
    assert (intra == 0).all() and (unmatched == 0).all()             # black planes, zero SAD: no block is unmatched

    with pytest.raises(hip.LsfaError, match="bias"):
        hip.mv_cut_score(luma, sad, bias=256)
    with pytest.raises(hip.LsfaError, match="uint8 CUDA stack"):
        hip.mv_cut_score(luma[0], sad)
    with pytest.raises(hip.LsfaError, match="sad"):
        hip.mv_cut_score(luma, sad[:, :1])
    with pytest.raises(hip.LsfaError, match="sad"):
        hip.mv_cut_score(luma, sad.float())
    with pytest.raises(hip.LsfaError, match="output buffer"):
        hip.mv_cut_score(luma, sad, out=(intra, unmatched[:, :1]))
    with pytest.raises(hip.LsfaError, match="percent"):
        hip.SegmentMotionEstimator(W, H, device=DEV, cut=dict(percent=0))
    with pytest.raises(hip.LsfaError, match="bias"):
        hip.MotionEstimator(W, H, DEV, cut=dict(bias=300))
    with pytest.raises(hip.LsfaError, match="without cut"):
        hip.MotionEstimator(W, H, DEV).is_cut()
    with pytest.raises(hip.LsfaError, match="first_cuts"):
        hip.SegmentMotionEstimator(W, H, device=DEV).first_cuts()
    with pytest.raises(hip.LsfaError, match="first_cuts"):
        hip.SegmentMotionEstimator(W, H, device=DEV, cut=dict()).first_cuts()          # no segment yet


# ---- the estimators --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [0, 1])
def test_segment_estimator_with_cut(hip, levels):
    """cut= changes nothing it returned before - rows, SAD, motion_vector and res_diff equal the same estimator's without it, bit for bit -
    and adds .intra / .unmatched == the reference on the estimator's own SAD, and first_cuts; two clips in lock step, a short segment, and
    the whole call in one captured graph, replayed twice"""
    width, height = 250, 130
    frames = bgr_two_scenes(width, height, 3, 2)
    planes = [ref_me.luma(f) for f in frames]
    chains = [[0, 1, 2, 3], [1, 2, 3, 4]]
    stack = t(np.stack([np.stack([frames[i] for i in chain]) for chain in chains]))
    kw = dict(frames=4, clips=2, device=DEV, search=8, lam=4, levels=levels)
    plain, cut = hip.SegmentMotionEstimator(width, height, **kw), hip.SegmentMotionEstimator(width, height, cut=dict(), **kw)
    assert plain.cut is None and plain.unmatched is None and cut.cut == (rc.BIAS, rc.PERCENT)
    want_mv, want_res = [x.clone() for x in plain.segment(stack, 1.25, MEANS, PIXEL_SCALE)]
    mv, res = cut.segment(stack, 1.25, MEANS, PIXEL_SCALE)
    assert torch.equal(mv, want_mv) and torch.equal(res, want_res) and torch.equal(cut.rows, plain.rows) and torch.equal(cut.sad, plain.sad)
    host = np.stack([np.stack([planes[i] for i in chain]) for chain in chains])
    want_intra, want_un = rc.cut_score(host, cut.sad.cpu().numpy())
    assert tuple(cut.unmatched.shape) == (2, 3) and tuple(cut.intra.shape) == (2, 3, 9, 16)
    np.testing.assert_array_equal(cut.intra.cpu().numpy(), want_intra)
    np.testing.assert_array_equal(cut.unmatched.cpu().numpy(), want_un)
    assert cut.first_cuts() == rc.first_cuts(want_un, 144) == [3, 2]
    assert cut.first_cuts(2) == [None, 2] and cut.first_cuts(1) == [None, None]
    # a stricter decision on the same counts
    assert hip.SegmentMotionEstimator(width, height, cut=dict(percent=100), **kw).cut == (rc.BIAS, 100)

    # one graph, no parallel branch: replayed on new contents and on the first contents again
    buf = stack.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_mv, g_res = cut.segment(buf, 1.25, MEANS, PIXEL_SCALE)
    other = t(np.stack([np.stack([frames[i] for i in chain]) for chain in ([4, 3, 2, 1], [3, 2, 1, 0])]))
    e_mv, e_res = [x.clone() for x in plain.segment(other, 1.25, MEANS, PIXEL_SCALE)]
    e_un = rc.cut_score(host[::-1, ::-1], plain.sad.cpu().numpy())[1]
    for contents, w_mv, w_res, w_un in ((other, e_mv, e_res, e_un), (stack, want_mv, want_res, want_un)):
        buf.copy_(contents)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_mv, w_mv) and torch.equal(g_res, w_res)
        np.testing.assert_array_equal(cut.unmatched.cpu().numpy(), w_un)
    assert not np.array_equal(e_un, want_un)

    # the short segment in front of a clip's last frame: one clip, n = 2 of a stack of four frames
    one = hip.SegmentMotionEstimator(width, height, frames=4, clips=1, device=DEV, search=8, lam=4, levels=levels, cut=dict(bias=0))
    one.segment(stack[:1], 1.0, MEANS, PIXEL_SCALE, n=2)
    assert tuple(one.unmatched.shape) == (1, 2)
    np.testing.assert_array_equal(one.unmatched.cpu().numpy(), rc.cut_score(host[:1, :3], one.sad.cpu().numpy(), 0)[1])
    assert one.first_cuts() == [None]


@pytest.mark.parametrize("levels", [0, 1])
def test_motion_estimator_with_cut(hip, levels):
    """frame by frame on the ping-pong pair (levels = 1: the stack of two is stored in reverse every other frame): rows, SAD and network
    inputs of the estimator without cut=, .unmatched == the reference, is_cut() at the scene change only; 37 x 23 needs the padded plane"""
    for width, height, search in ((250, 130, 8), (37, 23, 4)):
        frames = bgr_two_scenes(width, height, 3, 2)
        planes = [ref_me.luma(f) for f in frames]
        dev = [t(f) for f in frames]
        plain = hip.MotionEstimator(width, height, DEV, search=search, lam=4, levels=levels)
        cut = hip.MotionEstimator(width, height, DEV, search=search, lam=4, levels=levels, cut=dict(bias=rc.BIAS, percent=60))
        assert plain.unmatched is None and tuple(cut.unmatched.shape) == (1,)
        plain.key_frame(dev[0])
        cut.key_frame(dev[0])
        flags = []
        for f in range(1, 5):
            want_rows = plain.next_frame(dev[f])
            rows = cut.next_frame(dev[f])
            assert torch.equal(rows, want_rows) and torch.equal(cut.sad, plain.sad), (width, f)
            w_mv, w_res = plain.network_inputs(dev[f], dev[0], 1.0, MEANS, PIXEL_SCALE)
            mv, res = cut.network_inputs(dev[f], dev[0], 1.0, MEANS, PIXEL_SCALE)
            assert torch.equal(mv, w_mv) and torch.equal(res, w_res), (width, f)
            want_un = rc.cut_score(np.stack([planes[f - 1], planes[f]])[None], cut.sad.cpu().numpy()[None, None])[1]
            assert cut.unmatched.tolist() == [int(want_un[0, 0])], (width, f)
            flags.append(cut.is_cut())
            assert flags[-1] == bool(rc.is_cut(want_un[0, 0], cut.mbh * cut.mbw, 60)), (width, f)
        if width == 250:
            assert flags == [False, False, True, False]


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------
def test_clip_with_cuts_through_both_frame_loops(hip, monkeypatch):
    """The 24-frame synthetic clip of ref_me_cut.E2E (K = 10, new scenes at frames 4 and 17, decisive by tests/test_me_cut_cpu.py's margin
    check): the loader's flags are the plan [0, 4, 14, 17, 23] in the serial loop and in both pipelined forms; pred_eval_pipelined frame by
    frame equals pred_eval bit for bit; with whole segments batched and three key frames grouped the bank check (the key frames announced
    are the ones handed out) does not raise."""
    from lsfa_amd.config.config import lsfa_test_config
    from lsfa_amd.core.loader import TestLoader
    from lsfa_amd.function import test_rcnn as T
    from lsfa_amd.symbols import params as P
    from lsfa_amd.utils.synthetic import synthetic_roidb
    e = rc.E2E
    assert e['clip_id'] == 0
    cfg = lsfa_test_config(key_frame_interval=e['interval'])
    arg, aux = P.init_params(cfg, seed=3)
    roidb = synthetic_roidb(1, e['frames'], e['height'], e['width'], e['interval'], cuts=e['cuts'])
    cfg.TEST.ESTIMATE_MV = dict(search=e['search'], lam=4, cut=dict())
    want_flags = [(0 if f == 0 else 1) if f in e['keys'] else 2 for f in range(e['frames'])]
    runs = []

    class FlagLoader(TestLoader):
        def __init__(self, *a, **kw):
            self.flags = []
            runs.append(self)
            TestLoader.__init__(self, *a, **kw)

        def next(self):
            out = TestLoader.next(self)
            self.flags.append(out[1])
            return out

    monkeypatch.setattr(T, "TestLoader", FlagLoader)
    rows_serial, ids_serial = T.test_rcnn(cfg, roidb, arg, aux, device=DEV, pipeline=False)
    rows_frame, ids_frame = T.test_rcnn(cfg, roidb, arg, aux, device=DEV, pipeline=True, segment=0, key_group=1)
    rows_batch, ids_batch = T.test_rcnn(cfg, roidb, arg, aux, device=DEV, pipeline=True, segment=e['interval'] - 1, key_group=3)
    assert [r.flags for r in runs] == [want_flags] * 3
    assert all(r.cut and not r._segments for r in runs)
    np.testing.assert_array_equal(ids_frame, ids_serial)
    np.testing.assert_array_equal(ids_batch, ids_serial)
    assert len(rows_serial) > 0 and len(rows_batch) > 0
    np.testing.assert_array_equal(rows_frame, rows_serial)


def test_demo_scene_cut(hip, tmp_path):
    """lsfa_amd.demo --frames DIR --estimate-mv --scene-cut on ten PNG frames, scenes of three, two and five (160 x 96, interval 4): the loop's
    running key index gives key frames 0, then 3 and 5 - where the estimator's is_cut() says a scene starts - and 9; the expected cut comes from the
    numpy reference, which is decisive on every pair (at most 25 % / at least 75 % of the blocks unmatched)"""
    from PIL import Image
    from lsfa_amd import demo
    import json
    frames = me_util.clip(3, 160, 96, seed=1) + me_util.clip(5, 160, 96, seed=5)[:2] + me_util.clip(5, 160, 96, seed=6)          # scenes of 3, 2 and 5 frames
    assert len(frames) == 10
    (tmp_path / "frames").mkdir()
    for i, fr in enumerate(frames):
        Image.fromarray(np.ascontiguousarray(fr[:, :, ::-1])).save(str(tmp_path / "frames" / ("%06d.png" % i)))      # PNG holds RGB; the frames are BGR
    planes = [ref_me.luma(f) for f in frames]
    cuts = set()
    for f in range(1, 10):
        sad = ref_me.estimate(planes[f], planes[f - 1], 8, 4, 0)[1]
        un = int(rc.unmatched_blocks(sad, rc.intra(planes[f]), 96, 160).sum())
        assert un * 100 <= 25 * 60 or un * 100 >= 75 * 60, (f, un)
        if rc.is_cut(un, 60):
            cuts.add(f)
    assert cuts == {3, 5}
    # the demo's rule: a key frame every `interval` frames behind the last one, and at every cut (no rule for the last frame)
    keys, last = [], 0
    for f in range(10):
        if f == 0 or f - last == 4 or f in cuts:
            keys.append(f)
            last = f
    assert keys == [0, 3, 5, 9]
    out = tmp_path / "cut.json"
    demo.main(["--frames", str(tmp_path / "frames"), "--estimate-mv", "--search", "8", "--scene-cut", "--interval", "4", "--score", "0.05", "--out", str(out)])
    got = json.loads(out.read_text())
    assert [r["key"] for r in got] == [f in keys for f in range(10)]
    # without --scene-cut: every fourth frame, as ever
    demo.main(["--frames", str(tmp_path / "frames"), "--estimate-mv", "--search", "8", "--interval", "4", "--score", "0.05", "--out", str(out)])
    assert [r["key"] for r in json.loads(out.read_text())] == [f % 4 == 0 for f in range(10)]
    for bad in (["--scene-cut"], ["--frames", str(tmp_path / "frames"), "--estimate-mv", "--scene-cut", "0"],
                ["--frames", str(tmp_path / "frames"), "--estimate-mv", "--scene-cut", "--cut-bias", "256"]):
        with pytest.raises(SystemExit):
            demo.parse_args(bad)
