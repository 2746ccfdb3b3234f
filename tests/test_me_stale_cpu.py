"""Stale key frames without a device: tests/ref_me_stale.py, the numpy statement of the specification (include/lsfa_hip.h, lsfa_mv_key_sad /
lsfa_mv_key_sad_accu; DESIGN.md "Stale key frames"), pinned by cases with a known answer; the walk-back identity between its two forms;
the reference's counts on a dissolve, a pan and a hard cut, each decisive by a stated margin; the loader's plan with the union of both
rules' flags; the parameter refusals and the constructors (stale=None builds nothing); the interface.  The device kernels are compared
with the reference bit for bit in tests/test_me_stale_gpu.py."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import binding_contract as bc
import oracle
import ref_me
import ref_me_cut as rc
import ref_me_segment
import ref_me_stale as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def zero_rows(width, height, frames):
    """the estimator's rows with every vector zero"""
    rows = ref_me.estimate(np.zeros((height, width), np.uint8), np.zeros((height, width), np.uint8), 1, 0)[0]
    return np.stack([rows] * frames)[None]


# ---- known answers ----------------------------------------------------------------------------------------------------------------------------------
def test_identical_planes_and_zero_vectors_cost_nothing():
    y = np.random.RandomState(0).randint(0, 256, (23, 37)).astype(np.uint8)
    sad = rs.key_sad(np.stack([y] * 4)[None], zero_rows(37, 23, 3))
    assert sad.shape == (1, 3, 2, 3) and sad.dtype == np.int32 and not sad.any()


def test_constant_planes_cost_their_distance_on_every_covered_pixel():
    """37 x 23: blocks of 16 x 16, 5 x 16 (right edge), 16 x 7 (bottom edge) and 5 x 7 pixels, each with its own n_b"""
    a, b = np.full((23, 37), 200, np.uint8), np.full((23, 37), 57, np.uint8)
    sad = rs.key_sad(np.stack([a, b, a])[None], zero_rows(37, 23, 2))
    n = rc.block_pixels(23, 37)
    assert n.tolist() == [[256, 256, 80], [112, 112, 35]]
    np.testing.assert_array_equal(sad[0, 0], n * 143)
    assert not sad[0, 1].any()


def clean_blocks(width, height, m, f):
    """(mbh, mbw) bool for frame f of a clip translated by m per frame: the blocks ALL of whose covered pixels walk f steps of -m and stand,
    at every step, in a block whose rectangle shifted by -m lies inside the frame (such a block's best vector is the exact one, SAD 0).
    Geometry alone: nothing of the reference under test."""
    mbh, mbw = -(-height // 16), -(-width // 16)
    good = np.zeros((mbh, mbw), bool)
    for by in range(mbh):
        for bx in range(mbw):
            x0, y0, x1, y1 = 16 * bx, 16 * by, min(16 * bx + 16, width), min(16 * by + 16, height)
            good[by, bx] = x0 - m[0] >= 0 and x1 - m[0] <= width and y0 - m[1] >= 0 and y1 - m[1] <= height
    ys, xs = np.mgrid[0:height, 0:width]
    ok = np.ones((height, width), bool)
    for _ in range(f):
        ok &= good[ys >> 4, xs >> 4]
        xs, ys = np.clip(xs - m[0], 0, width - 1), np.clip(ys - m[1], 0, height - 1)
    full = np.ones((mbh * 16, mbw * 16), bool)
    full[:height, :width] = ok
    return full.reshape(mbh, 16, mbw, 16).all(axis=(1, 3))


def test_translated_white_noise_is_predicted_exactly_outside_the_entering_band():
    """96 x 64 white noise moving by (3, -2) per frame, no noise added, R = 4, five frames behind the key frame: keysad == 0 on every block
    all of whose pixels' walks took every step.  The band where they did not - the left column and the bottom row, where content enters,
    and from frame 2 on the blocks beside them, whose pixels step into them - is 9 of 24 blocks at frame 1 and 16 behind it (geometry: clean_blocks:
    with 3 and 2 pixels per frame a walk of five steps crosses at most one block boundary per axis)"""
    width, height, m = 96, 64, (3, -2)
    ys = [ref_me.luma(f) for f in ref_me.translated_clip(6, width, height, m, seed=7)]
    rows = np.stack([ref_me.estimate(ys[f], ys[f - 1], 4, 4, 0)[0] for f in range(1, 6)])[None]
    sad = rs.key_sad(np.stack(ys)[None], rows)
    band = []
    for f in range(1, 6):
        clean = clean_blocks(width, height, m, f)
        band.append(int((~clean).sum()))
        assert not sad[0, f - 1][clean].any(), f
        assert sad[0, f - 1][~clean].all(), f            # white noise: what was not predicted costs a great deal
    print("blocks outside the clean region per frame:", band)
    assert band == [9, 16, 16, 16, 16]


# ---- the walk-back identity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height,search,max_sad", [(37, 23, 4, 0), (96, 64, 8, 900)])
def test_accu_form_equals_the_walk_form(width, height, search, max_sad):
    """key_sad_accu on oracle.coviar_accumulate's map == key_sad on the rows, bit for bit: under noise at 37 x 23, and at 96 x 64 with max_sad
    zeroing blocks in the middle of the chain"""
    frames = ref_me.translated_clip(6, width, height, (3, -2), seed=width, sigma=3.0)
    ys = [ref_me.luma(f) for f in frames]
    rows = np.stack([ref_me.estimate(ys[f], ys[f - 1], search, 4, max_sad)[0] for f in range(1, 6)])
    if max_sad:
        zero = (rows[:, :, 3:5] == rows[:, :, 5:7]).all(axis=2)
        assert zero.any() and not zero.all()
    want = rs.key_sad(np.stack(ys)[None], rows[None])
    accu = oracle.coviar_identity(width, height)
    for f in range(1, 6):
        accu = oracle.coviar_accumulate(rows[f - 1], accu)
        np.testing.assert_array_equal(rs.key_sad_accu(ys[f], ys[0], accu), want[0, f - 1], err_msg="frame %d" % f)
    assert want.any()


def test_accu_entries_outside_the_plane_read_as_zero():
    y = np.full((23, 37), 9, np.uint8)
    accu = oracle.coviar_identity(37, 23).copy()
    accu[0, 0] = (-1, 0)
    accu[22, 36] = (36, 23)
    accu[5, 20] = (37, 5)
    got = rs.key_sad_accu(y, y, accu)
    assert got.tolist() == [[9, 9, 0], [0, 0, 9]]


# ---- the recorded counts and their margin ----------------------------------------------------------------------------------------------------------
# (pair rule's counts, key rule's counts) per frame f = 1.. as the numpy reference gives them: lambda 4, bias 4, R = 4
DISSOLVE = ([0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 5, 17, 22, 23], 24)          # frames 2..6 are the dissolve
HARD_CUT = ([0, 0, 0, 21, 0, 0], [0, 0, 0, 21, 22, 22], 24)
PAN = ([1, 1, 4, 2, 1, 1, 1, 2], [1, 14, 17, 23, 22, 23, 22, 26], 144)
MARGIN = 20          # every deciding count lies at least 20 % of the blocks from percent = 50: at most 30 % or at least 70 %


def decisive(counts, blocks):
    return all(c * 100 <= (50 - MARGIN) * blocks or c * 100 >= (50 + MARGIN) * blocks for c in counts)


def test_dissolve_is_seen_by_the_key_rule_only():
    """96 x 64, two frames of scene A, a five-frame linear blend into scene B, one of B: the pair rule flags no frame (no single pair crosses
    it); against the key frame the unmatched blocks are 0, 0, 0, 5, 17, 22, 23 of 24 at frames 1..7 and frame 5, the fourth of the dissolve, is stale"""
    pair, key, blocks = got = rs.chain_counts(rs.dissolve_clip(), 4)
    print("dissolve:", got)
    assert got == DISSOLVE and decisive(pair, blocks) and decisive(key, blocks)
    assert rc.first_cuts(np.array([pair]), blocks) == [None]
    assert rc.first_cuts(np.array([key]), blocks) == [5] and 2 < 5 < 6            # strictly inside the dissolve (frames 2..6)
    assert rs.first_flagged(rc.is_cut([pair], blocks), rc.is_cut([key], blocks)) == [5]


def test_quiet_pan_is_flagged_by_neither_rule():
    """250 x 130 moving by (2, -1) per frame over eight frames: the band that enters costs at most 26 of 144 blocks against the key frame"""
    pair, key, blocks = got = rs.chain_counts(rs.pan_clip(), 4)
    print("pan:", got)
    assert got == PAN and decisive(pair, blocks) and decisive(key, blocks)
    assert rc.first_cuts(np.array([pair]), blocks) == [None] and rc.first_cuts(np.array([key]), blocks) == [None]


def test_hard_cut_is_flagged_by_both_rules():
    pair, key, blocks = got = rs.chain_counts(rs.cut_clip(), 4)
    print("hard cut:", got)
    assert got == HARD_CUT and decisive(pair, blocks) and decisive(key, blocks)
    assert rc.first_cuts(np.array([pair]), blocks) == [4] == rc.first_cuts(np.array([key]), blocks)
    assert rc.is_cut(key, blocks).tolist() == [False, False, False, True, True, True]      # the key frame stays lost behind the cut


# ---- the loader's plan with the union of both rules' flags -----------------------------------------------------------------------------------------
def union_plan_brute(length, interval, pair_flags, key_flags):
    """frame by frame: frame f is a key frame iff it is the first or the last frame, `interval` frames behind the key frame in front of it,
    flagged by the pair rule (a set of frames), or flagged by the key rule for the segment that started at that key frame (key_flags:
    {key frame: set of frames})"""
    keys, last = [], None
    for f in range(length):
        if f == 0 or f == length - 1 or f - last == interval or f in pair_flags or f in key_flags.get(last, ()):
            keys.append(f)
            last = f
    return keys


def test_plan_with_the_union_of_flags_against_brute_force():
    """what TestLoader does with first_cuts() of either rule: next_key_frame is handed the first flagged frame of the segment behind the key
    frame - from the pair rule's set or from the key rule's flags of THAT segment - and nothing else"""
    from lsfa_amd.core.loader import next_key_frame
    r = np.random.RandomState(5)
    for L in range(2, 13):
        for K in range(1, 6):
            for _ in range(12):
                pair_flags = set(f for f in range(1, L) if r.rand() < 0.15)
                key_flags = {k: set(f for f in range(k + 1, L) if r.rand() < 0.2) for k in range(L)}
                keys = [0]
                while keys[-1] < L - 1:
                    k = keys[-1]
                    n = min(k + K - 1, L - 2) - k
                    flagged = [f for f in range(k + 1, k + n + 1) if f in pair_flags or f in key_flags[k]]          # the estimator's segment
                    keys.append(next_key_frame(k, L, K, flagged[:1]))
                assert keys == union_plan_brute(L, K, pair_flags, key_flags), (L, K, pair_flags, key_flags)


class StubEstimator(object):
    """stands in for hip.SegmentMotionEstimator(stale=...): reports the first flagged frame it was told of for the segment's key frame"""

    def __init__(self, roidb, flags):
        self.roidb, self.flags, self.last, self.reads = roidb, flags, None, 0

    def segment(self, stack, im_scale, pixel_means, pixel_scale):
        n = int(stack.shape[1]) - 1
        k, = [k for k in range(self.roidb[0]['frame_seg_len']) if torch.equal(self.roidb[0]['clip'].frame_u8(k), stack[0, 0])]
        self.last = (k, n)
        return torch.zeros((n, 1, 2, 2, 3)), torch.zeros((n, 1, 3, 2, 3))

    def first_cuts(self, n=None):
        k, have = self.last
        self.reads += 1
        hits = [f for f in range(1, have + 1) if k + f in self.flags.get(k, ())]
        return [hits[0] if hits else None]


@pytest.mark.parametrize("estimate_mv", [dict(search=8, stale=dict(percent=40)), dict(search=8, cut=dict(), stale=dict())])
def test_loader_places_key_frames_at_stale_frames(estimate_mv):
    """estimate_mv with stale= (alone or beside cut=) switches the loader's early segment end on: the flags follow the frames the estimator's
    first_cuts reports segment by segment, upcoming_key_frames announces them, one readback per estimated segment"""
    from lsfa_amd.config.config import lsfa_test_config
    from lsfa_amd.core.loader import TestLoader
    from lsfa_amd.utils.synthetic import synthetic_roidb
    K, n = 4, 11
    flags = {0: {2}, 2: {3, 5}, 3: set(), 7: {9}}          # per key frame: the frames its segment flags
    roidb = synthetic_roidb(1, n, 32, 48, K)
    stubs = []

    class Loader(TestLoader):
        def _segment_estimator(self, width, height):
            stubs.append(StubEstimator(roidb, flags))
            return stubs[-1]

    loader = Loader(roidb, lsfa_test_config(key_frame_interval=K), device='cpu', estimate_mv=estimate_mv)
    assert loader.cut
    want = union_plan_brute(n, K, set(), flags)
    assert want == [0, 2, 3, 7, 9, 10]
    got, announced = [], None
    for f, (im_info, flag, batch) in enumerate(loader):
        got.append(flag)
        if flag != 2:
            if announced is not None:
                assert announced[:1] == [k for k in want if k >= f][:1] or not announced
            announced = [k for k in want if k > f][:2]
            assert len(loader.upcoming_key_frames(2)) == len(announced)
    assert got == [(0 if f == 0 else 1) if f in want else 2 for f in range(n)]
    assert sum(s.reads for s in stubs) == len([k for k in want if min(k + K - 1, n - 2) - k >= 1])


def test_loader_takes_stale_from_the_config():
    from lsfa_amd.config.config import lsfa_test_config
    from lsfa_amd.core.loader import TestLoader
    from lsfa_amd.utils.synthetic import synthetic_roidb
    cfg = lsfa_test_config(key_frame_interval=3)
    cfg.TEST.ESTIMATE_MV = dict(search=8, stale=dict(bias=2, percent=40))
    roidb = synthetic_roidb(1, 5, 32, 48, 3)

    class Loader(TestLoader):
        def _segment_estimator(self, width, height):
            return StubEstimator(roidb, {0: {2}})

    loader = Loader(roidb, cfg, device='cpu')
    assert loader.cut and loader.estimate_mv['stale'] == dict(bias=2, percent=40)
    assert [flag for _, flag, _ in loader] == [0, 2, 1, 2, 1]


# ---- the synthetic clip with dissolves --------------------------------------------------------------------------------------------------------------
def test_synthetic_dissolves_blend_into_a_new_scene_and_the_default_has_none():
    from lsfa_amd.utils.synthetic import SyntheticClip, synthetic_roidb
    plain, cut, dis = SyntheticClip(1, 10, 48, 64), SyntheticClip(1, 10, 48, 64, cuts=(3,)), SyntheticClip(1, 10, 48, 64, dissolves=((3, 4),))
    assert plain.dissolves == () and dis.dissolves == ((3, 4),)
    for f in range(10):
        assert torch.equal(plain.frame(f), dis.frame(f)) == (f < 3), f
        assert torch.equal(cut.frame(f), dis.frame(f)) == (f < 3 or f >= 7), f          # behind the dissolve: the scene a cut would have started
    # inside: between the two scenes, nearer the old one first (the noise is the frame's own in all three clips)
    for f, nearer_old in ((3, True), (6, False)):
        d_old = (dis.frame(f) - plain.frame(f)).abs().mean()
        d_new = (dis.frame(f) - cut.frame(f)).abs().mean()
        assert (d_old < d_new) == nearer_old, (f, float(d_old), float(d_new))
    both = SyntheticClip(1, 10, 48, 64, cuts=(2,), dissolves=((4, 3),))
    assert torch.equal(both.frame(3), SyntheticClip(1, 10, 48, 64, cuts=(2,)).frame(3))
    assert [e['clip'].dissolves for e in synthetic_roidb(2, 10, 48, 64, 4, dissolves=((5, 2),))] == [((5, 2),)] * 2
    for bad in (dict(dissolves=((0, 2),)), dict(dissolves=((8, 3),)), dict(dissolves=((3, 0),)), dict(cuts=(4,), dissolves=((3, 3),)),
                dict(dissolves=((3, 3), (5, 2)))):
        with pytest.raises(ValueError):
            SyntheticClip(0, 10, 48, 64, **bad)


# ---- the end-to-end clip's margin -----------------------------------------------------------------------------------------------------------------
# the clip tests/test_me_stale_gpu.py runs through the loader and both frame loops (ref_me_cut.E2E is the model): 24 frames of 128 x 192,
# K = 10, search 8, a three-frame dissolve from frame 3 and a hard cut at frame 18, the key rule alone (stale=dict())
E2E = dict(clip_id=0, frames=24, height=128, width=192, interval=10, dissolves=((3, 3),), cuts=(18,), search=8, keys=[0, 3, 4, 5, 6, 16, 18, 23])
E2E_MARGIN = 15


def e2e_planes():
    from lsfa_amd.utils.synthetic import SyntheticClip
    e = E2E
    clip = SyntheticClip(e['clip_id'], e['frames'], e['height'], e['width'], e['interval'], cuts=e['cuts'], dissolves=e['dissolves'])
    return [ref_me.luma(clip.frame_u8(f).numpy()) for f in range(e['frames'])]


def test_end_to_end_clip_is_decisive():
    """the reference's plan on the E2E clip, segment by segment as the loader estimates them: every count up to and including a segment's
    first flagged frame (the counts behind it decide nothing: those pairs are discarded) lies at most 35 % or at least 65 % of the blocks"""
    e = E2E
    keys, counts = rs.plan(e2e_planes(), e['interval'], e['search'], None, (rs.BIAS, rs.PERCENT))
    print("key frames", keys)
    for k in sorted(counts):
        print("  segment behind", k, counts[k][1])
    assert keys == e['keys']
    for k, (_, key_un) in counts.items():
        flags = rc.is_cut(key_un, 96).tolist()
        deciding = key_un[:flags.index(True) + 1] if True in flags else key_un
        assert all(c * 100 <= (50 - E2E_MARGIN) * 96 or c * 100 >= (50 + E2E_MARGIN) * 96 for c in deciding), (k, key_un)


# ---- the parameters and the constructors -----------------------------------------------------------------------------------------------------------
@pytest.fixture
def fake(monkeypatch):
    """hip.py's classes on a machine without a GPU: allocations on cuda:0 become host tensors that claim to be there, launches are recorded"""
    from lsfa_amd import hip
    with bc.fake_cuda(monkeypatch):
        spy = bc.Spy(hip.lib())
        monkeypatch.setattr(hip, "lib", lambda: spy)
        yield hip, spy


def test_parameter_refusals(fake):
    hip, spy = fake
    for bad in (dict(bias=4, percent=50, extra=1), dict(bias=300), dict(percent=0), dict(bias=-1), dict(percent=101), 50):
        with pytest.raises(hip.LsfaError, match="stale"):
            hip.SegmentMotionEstimator(96, 64, device=bc.CUDA0, stale=bad)
        with pytest.raises(hip.LsfaError, match="stale"):
            hip.MotionEstimator(96, 64, bc.CUDA0, stale=bad)
    with pytest.raises(hip.LsfaError, match="cut takes"):          # the pair rule's own message keeps its keyword
        hip.SegmentMotionEstimator(96, 64, device=bc.CUDA0, cut=dict(percent=0), stale=dict())
    assert not [c for c in spy.launched() if c not in ("lsfa_mv_identity",)]


def test_constructors(fake):
    """stale=None builds nothing: no buffer, .cut as it was; stale=dict() takes the defaults, either key may be left out, and every buffer of
    the mode exists after construction - for MotionEstimator also the third level-0 plane"""
    hip, spy = fake
    for make in (lambda **kw: hip.SegmentMotionEstimator(96, 64, frames=3, clips=2, device=bc.CUDA0, **kw), lambda **kw: hip.MotionEstimator(96, 64, bc.CUDA0, **kw)):
        off = make(cut=dict(percent=60))
        s = off._search
        assert off.stale is None and off.cut == (4, 60) and off.keysad is None and off.key_unmatched is None
        assert s.stale is None and s.keysad is None and s.key_intra is None and s.key_unmatched is None and s.key_plane is None
        assert s.unmatched is not None and s._counts.numel() == s.unmatched.numel()
        none = make()
        assert none.cut is None and none.stale is None and none._search._counts is None and none._search.unmatched is None
        on = make(stale=dict())
        assert on.stale == (hip.ME_STALE_BIAS, hip.ME_STALE_PERCENT) == (4, 50) and on.cut is None and on._search.unmatched is None
        assert make(stale=dict(bias=9)).stale == (9, 50) and make(stale=dict(percent=7)).stale == (4, 7)
        both = make(cut=dict(), stale=dict(bias=1, percent=2))
        s = both._search
        pairs = s.key_unmatched.numel()
        assert both.cut == (4, 50) and both.stale == (1, 2)
        assert s.keysad.numel() == s.key_intra.numel() == pairs * 24 and s.unmatched.numel() == pairs and s._counts.numel() == 2 * pairs
    seg, me = hip.SegmentMotionEstimator(96, 64, frames=3, clips=2, device=bc.CUDA0, stale=dict()), hip.MotionEstimator(96, 64, bc.CUDA0, stale=dict())
    assert seg._search.key_plane is None and seg._search.key_unmatched.numel() == 6
    assert me._search.key_plane.numel() == 96 * 64 and tuple(me.key_unmatched.shape) == (1,) and tuple(me.keysad.shape) == (4, 6)
    with pytest.raises(hip.LsfaError, match="first_cuts"):
        seg.first_cuts()                                     # no segment yet
    with pytest.raises(hip.LsfaError, match="first_cuts"):
        hip.SegmentMotionEstimator(96, 64, device=bc.CUDA0).first_cuts()


def test_launches_of_the_mode(fake):
    """what the mode adds, as the recording library sees it: the segment form behind the search and in front of the inputs; frame by frame a
    copy of the key plane, then the accu form behind the accumulation; nothing of it without stale="""
    hip, spy = fake
    env = bc.Env(fake=True)
    stack = env.u8(1, 3, 16, 32, 3)

    def segment(**kw):
        sme = hip.SegmentMotionEstimator(32, 16, frames=2, device=bc.CUDA0, search=4, **kw)
        del spy.calls[:]
        sme.segment(stack, 1.0)
        return spy.launched()

    plain, on, both = segment(), segment(stale=dict(bias=7)), segment(cut=dict(), stale=dict())
    assert plain == ["lsfa_luma_u8", "lsfa_mv_estimate_chain", "lsfa_mv_segment_inputs"]
    assert on == ["lsfa_luma_u8", "lsfa_mv_estimate_chain", "lsfa_mv_key_sad", "lsfa_mv_cut_score", "lsfa_mv_segment_inputs"]
    assert both == ["lsfa_luma_u8", "lsfa_mv_estimate_chain", "lsfa_mv_cut_score", "lsfa_mv_key_sad", "lsfa_mv_cut_score", "lsfa_mv_segment_inputs"]
    v = spy.values("lsfa_mv_key_sad")
    assert (v["n_chains"], v["n_frames"], v["width"], v["height"], v["plane_stride"]) == (1, 2, 32, 16, 512)

    def frames(**kw):
        me = hip.MotionEstimator(32, 16, bc.CUDA0, search=4, **kw)
        del spy.calls[:]
        me.key_frame(env.u8(16, 32, 3))
        me.next_frame(env.u8(16, 32, 3))
        return spy.launched(), me

    plain, _ = frames()
    on, me = frames(stale=dict(bias=7))
    assert plain == ["lsfa_luma_u8", "lsfa_mv_identity", "lsfa_luma_u8", "lsfa_mv_estimate", "lsfa_mv_accumulate"]
    assert on == ["lsfa_luma_u8", "lsfa_copy_many", "lsfa_mv_identity", "lsfa_luma_u8", "lsfa_mv_estimate", "lsfa_mv_accumulate", "lsfa_mv_key_sad_accu",
                  "lsfa_mv_cut_score"]
    v = spy.values("lsfa_mv_key_sad_accu")
    s = me._search
    assert v["luma_key"] == s.key_plane.data_ptr() and v["luma_cur"] == s.flat[0].data_ptr() + 512 and v["accu"] == me.acc.accu.data_ptr()
    score = [a for name, a in spy.calls if name == "lsfa_mv_cut_score"][0]
    assert dict(zip(bc.param_names("lsfa_mv_cut_score"), score))["bias"] == 7


# ---- the interface ----------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_the_binding_derives_both_exports():
    import ctypes
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsfa_hip.h")).read(), flags=re.S)
    from lsfa_amd import hip
    for name, want in (("lsfa_mv_key_sad", [ctypes.c_void_p, ctypes.c_longlong] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3),
                       ("lsfa_mv_key_sad_accu", [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 2)):
        assert re.search(r"\bint\s+%s\s*\(" % name, text)
        ret, params = hip._PROTOTYPES[name]
        assert ret.strip() == "int" and [hip._ctype(p) for p in params] == want
    for name in ("ME_STALE_BIAS", "ME_STALE_PERCENT"):
        assert hasattr(hip, name), name
    # the exports are named by _MotionSearch alone, which hands the library no tensor of the caller's (tests/binding_contract.py)
    import test_abi
    by_export = test_abi.wrappers_by_export()
    assert by_export["lsfa_mv_key_sad"] == {"_MotionSearch"} == by_export["lsfa_mv_key_sad_accu"]
    src = open(os.path.join(ROOT, "lsfa_amd", "core", "loader.py")).read() + open(os.path.join(ROOT, "lsfa_amd", "demo.py")).read()
    assert "lsfa_mv_key_sad" not in src
