"""Scene cuts without a device: tests/ref_me_cut.py, the numpy statement of the specification (include/lsfa_hip.h, lsfa_mv_cut_score; DESIGN.md
"Scene cuts"), pinned by cases with a known answer and by the figures recorded from it; the key plan against a brute-force restatement;
TestLoader(estimate_mv=dict(cut=...)) on a stub estimator; the margin the GPU end-to-end test's expected flags rest on.
tests/test_me_cut_gpu.py compares the kernels with this reference."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import ref_me
import ref_me_cut as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- known answers of the specification ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [0, 1, 200, 255])
def test_constant_plane_has_no_intra_cost(value):
    for h, w in ((16, 16), (23, 37), (130, 250)):
        cost = rc.intra(np.full((h, w), value, np.uint8))
        assert cost.shape == (-(-h // 16), -(-w // 16)) and not cost.any()


@pytest.mark.parametrize("h", [2, 10, 100])
def test_two_values_half_and_half_cost_half_their_distance_per_pixel(h):
    """columns alternate between v and v + h: every block of even width holds them half and half, its mean is v + h / 2 and
    intra = n_b * h / 2 - with the block's OWN n_b in the blocks cut by the right (4 wide) and bottom (2 high) edges"""
    y = np.empty((18, 20), np.uint8)
    y[:, 0::2], y[:, 1::2] = 40, 40 + h
    n = rc.block_pixels(18, 20)
    np.testing.assert_array_equal(n, [[256, 64], [32, 8]])
    np.testing.assert_array_equal(rc.intra(y), n * h // 2)


def test_mean_is_rounded_over_the_blocks_own_pixels():
    y = np.zeros((18, 20), np.uint8)
    y[3, 5] = 255            # the whole block: m = (255 + 128) / 256 = 1, intra = 254 + 255 * 1
    y[17, 19] = 4            # the 4 x 2 corner block: m = (4 + 4) / 8 = 1, intra = 3 + 7 (with n = 256 it would be m = 0, intra = 4)
    y[16, 0] = 15            # the 16 x 2 bottom block: m = (15 + 16) / 32 = 0, intra = 15
    np.testing.assert_array_equal(rc.intra(y), [[509, 0], [15, 10]])


def test_the_two_inequalities_are_strict():
    """unmatched iff inter > intra + bias * n_b; a cut iff unmatched * 100 > percent * blocks"""
    n = rc.block_pixels(18, 20)
    cost = np.array([[100, 7], [0, 3]], np.int32)
    for bias in (0, 4, 255):
        edge = (cost + bias * n).astype(np.int32)
        assert not rc.unmatched_blocks(edge, cost, 18, 20, bias).any()
        assert rc.unmatched_blocks(edge + 1, cost, 18, 20, bias).all()
    assert not rc.is_cut(12, 24, 50) and rc.is_cut(13, 24, 50)
    assert not rc.is_cut(24, 24, 100) and rc.is_cut(1, 24, 1) and not rc.is_cut(0, 24, 1)
    assert rc.first_cuts(np.array([[0, 13, 24], [12, 12, 0]]), 24, 50) == [2, None]


# ---- the figures recorded from the specification -------------------------------------------------------------------------------------------------
def recorded_pairs(width, height):
    """(translated pair, cut pair) of luma planes: frames 0 -> 1 of the seed-1 translated clip (three frames, sigma 3, m = (3, -2)), and that
    clip's frame 1 -> frame 0 of the seed-2 clip (two frames)"""
    a = ref_me.translated_clip(3, width, height, (3, -2), seed=1, sigma=3.0)
    b = ref_me.translated_clip(2, width, height, (3, -2), seed=2, sigma=3.0)
    y0, y1, z0 = ref_me.luma(a[0]), ref_me.luma(a[1]), ref_me.luma(b[0])
    return (y1, y0), (z0, y1)


@pytest.mark.parametrize("width,height,search,same,cut,blocks", [(250, 130, 8, 9, 131, 144), (96, 64, 8, 9, 24, 24), (37, 23, 4, 4, 6, 6)])
def test_recorded_counts(width, height, search, same, cut, blocks):
    """lambda 4, bias 4: the translated pair leaves the band where new content enters unmatched, the cut pair nearly everything"""
    got = []
    for cur, ref in recorded_pairs(width, height):
        _, sad = ref_me.estimate(cur, ref, search, 4, 0)
        planes = np.stack([ref, cur])[None]
        cost, un = rc.cut_score(planes, sad[None, None], 4)
        assert cost.shape == (1, 1) + sad.shape and un.shape == (1, 1) and sad.size == blocks
        np.testing.assert_array_equal(cost[0, 0], rc.intra(cur))
        got.append(int(un[0, 0]))
    assert got == [same, cut]
    if blocks >= 24:          # 37 x 23 is too small for the frame decision
        assert [bool(rc.is_cut(g, blocks, 50)) for g in got] == [False, True]


# ---- the key plan ----------------------------------------------------------------------------------------------------------------------------------
def test_key_plan_against_brute_force():
    from lsfa_amd.core.loader import key_plan, next_key_frame
    for L in range(1, 15):
        for K in range(1, 6):
            for r in range(4):
                for cuts in itertools.combinations(range(1, L), r):
                    plan = key_plan(L, K, set(cuts))
                    assert plan == rc.key_plan_brute(L, K, set(cuts)), (L, K, cuts)
                    assert all(next_key_frame(a, L, K, set(cuts)) == b for a, b in zip(plan, plan[1:]))
    assert key_plan(24, 10, {4, 17}) == [0, 4, 14, 17, 23] == rc.E2E['keys']
    assert key_plan(24, 10, ()) == [0, 10, 20, 23]
    assert key_plan(24, 10, {10, 22, 23}) == [0, 10, 20, 22, 23]


# ---- TestLoader on a stub estimator -------------------------------------------------------------------------------------------------------------
class StubCutEstimator(object):
    """stands in for hip.SegmentMotionEstimator(cut=...): names the frames like tests/test_me_segment_cpu.py's stub and reports the cut
    frames it was told of - it finds out which frames a stack holds by looking them up in the clips"""

    def __init__(self, log, roidb, cuts):
        self.log, self.roidb, self.cuts = log, roidb, cuts
        self.buf, self.last, self.reads = {}, None, 0

    def segment(self, stack, im_scale, pixel_means, pixel_scale):
        n = int(stack.shape[1]) - 1
        where = [(v, k) for v, e in enumerate(self.roidb) for k in range(e['frame_seg_len']) if torch.equal(e['clip'].frame_u8(k), stack[0, 0])]
        assert len(where) == 1
        (v, k), = where
        for g in range(n + 1):
            assert torch.equal(stack[0, g], self.roidb[v]['clip'].frame_u8(k + g)), (v, k, g)
        self.log.append((v, k, n))
        self.last = (v, k, n)
        mv, res = self.buf.setdefault(n, (torch.empty((n, 1, 2, 2, 3)), torch.empty((n, 1, 3, 2, 3))))      # reused from call to call
        for f in range(n):
            mv[f] = float(stack[0, f + 1].sum())
            res[f] = float(stack[0, 0].sum()) + f + 1
        return mv, res

    def first_cuts(self, n=None):
        v, k, have = self.last
        self.reads += 1
        hits = [f for f in range(1, have + 1) if k + f in self.cuts[v]]
        return [hits[0] if hits else None]


def cut_loader(K, n, cuts, estimate_mv):
    from lsfa_amd.config.config import lsfa_test_config
    from lsfa_amd.core.loader import TestLoader
    from lsfa_amd.utils.synthetic import synthetic_roidb
    log, stubs = [], []
    roidb = synthetic_roidb(len(cuts), n, 32, 48, K)

    class Loader(TestLoader):
        def _segment_estimator(self, width, height):
            stubs.append(StubCutEstimator(log, roidb, cuts))
            return stubs[-1]

    return Loader(roidb, lsfa_test_config(key_frame_interval=K), device='cpu', estimate_mv=estimate_mv), roidb, log, stubs


@pytest.mark.parametrize("K,n,cuts,ahead", [(10, 24, [{4, 17}, set()], 2), (4, 11, [{2, 3, 9}, {5}], 0), (4, 11, [{2, 3, 9}, {5}], 3),
                                            (3, 8, [{3, 6}, {1, 7}], 1), (5, 9, [{8}, {4, 7}], 4), (1, 4, [{2}, set()], 2)])
def test_loader_places_key_frames_at_cuts(K, n, cuts, ahead):
    """flags == key_plan of the cut frames the estimator reports; every non-key frame receives its own segment's slice (the pairs estimated
    beyond a cut are never handed out); upcoming_key_frames(ahead), asked after every key frame, announces exactly the tensors handed out
    at the next key frames, in order; a segment is estimated once, whether the iteration or the look-ahead reached it first"""
    from lsfa_amd.core.loader import key_plan
    loader, roidb, log, stubs = cut_loader(K, n, cuts, dict(search=8, cut=dict(percent=50)))
    assert loader.cut
    plans = [key_plan(n, K, c) for c in cuts]
    announced, i = [], 0
    for im_info, flag, batch in loader:
        d = dict(zip(loader.data_name, batch.data[0]))
        v, f = divmod(i, n)
        clip, keys = roidb[v]['clip'], plans[v]
        assert flag == (2 if f not in keys else (0 if f == 0 else 1)), (v, f, flag, keys)
        if flag == 2:
            key_f = max(k for k in keys if k < f)
            assert float(d['motion_vector'].flatten()[0]) == float(clip.frame_u8(f).sum()), (v, f)
            assert float(d['res_diff'].flatten()[0]) == float(clip.frame_u8(key_f).sum()) + (f - key_f), (v, f, key_f)
            assert tuple(d['motion_vector'].shape) == (1, 2, 2, 3) and tuple(d['res_diff'].shape) == (1, 3, 2, 3)
        else:
            if flag == 0:
                assert not announced, (v, announced)          # a video's announcements end with the video
            if announced:
                want_f, want = announced.pop(0)
                assert want_f == f and d['data'] is want, (v, f, want_f)
            assert d['data_key'] is d['data']
            if ahead:
                coming = [k for k in keys if k > f][:ahead]
                got = loader.upcoming_key_frames(ahead)
                assert len(got) == len(coming), (v, f, coming)
                for k, t in zip(coming, got):
                    assert torch.equal(t, clip.frame(k)), (v, f, k)
                # frames announced before are announced again as the SAME tensors
                for (pf, pt), t in zip(announced, got):
                    assert pt is t, (v, f, pf)
                announced = list(zip(coming, got))
        i += 1
    assert i == len(cuts) * n and not announced
    # one estimate per key frame that has a non-key candidate behind it, on key .. min(key + K - 1, n - 2)
    want = [(v, k, min(k + K - 1, n - 2) - k) for v in range(len(cuts)) for k in plans[v] if min(k + K - 1, n - 2) - k >= 1]
    assert sorted(log) == want and (ahead or log == want), (log, want)
    assert sum(s.reads for s in stubs) == len(want)           # one readback per estimated segment
    assert len(loader._segments) <= 1                          # nothing of the segments passed is kept


def test_loader_without_cut_never_reads_back_or_estimates_ahead():
    """cut absent: one estimate per key frame when it is handed out, upcoming_key_frames announces every K-th frame without estimating
    anything, first_cuts is never called"""
    loader, roidb, log, stubs = cut_loader(4, 11, [set(), set()], dict(search=8))
    assert not loader.cut
    seen = 0
    for i, (im_info, flag, batch) in enumerate(loader):
        if flag != 2:
            before = list(log)
            got = loader.upcoming_key_frames(3)
            assert log == before
            f = i % 11
            assert len(got) == len([k for k in (4, 8, 10) if k > f])
            seen += 1
    assert seen == 8 and log == [(v, k, m) for v in (0, 1) for k, m in ((0, 3), (4, 3), (8, 1))]
    assert sum(s.reads for s in stubs) == 0


def test_loader_takes_cut_from_the_config():
    from lsfa_amd.config.config import lsfa_test_config
    from lsfa_amd.core.loader import TestLoader
    from lsfa_amd.utils.synthetic import synthetic_roidb
    cfg = lsfa_test_config(key_frame_interval=3)
    cfg.TEST.ESTIMATE_MV = dict(search=8, cut=dict(bias=2, percent=40))
    roidb = synthetic_roidb(1, 5, 32, 48, 3)
    log = []

    class Loader(TestLoader):
        def _segment_estimator(self, width, height):
            return StubCutEstimator(log, roidb, [{2}])

    loader = Loader(roidb, cfg, device='cpu')
    assert loader.cut and loader.estimate_mv['cut'] == dict(bias=2, percent=40)
    assert [flag for _, flag, _ in loader] == [0, 2, 1, 2, 1]


# ---- the synthetic clip with cuts -----------------------------------------------------------------------------------------------------------------
def test_synthetic_cuts_redraw_the_scene_and_the_default_has_none():
    from lsfa_amd.utils.synthetic import SyntheticClip, synthetic_roidb
    plain, cut = SyntheticClip(1, 8, 48, 64), SyntheticClip(1, 8, 48, 64, cuts=(3, 6))
    assert plain.cuts == () and cut.cuts == (3, 6)
    for f in range(8):
        same = torch.equal(plain.frame(f), cut.frame(f))
        assert same == (f < 3), f
        assert torch.equal(plain.res_diff(f), cut.res_diff(f))
    assert not torch.equal(cut.frame_u8(5), SyntheticClip(1, 8, 48, 64, cuts=(3,)).frame_u8(6))
    assert torch.equal(cut.frame(5), SyntheticClip(1, 8, 48, 64, cuts=(3,)).frame(5))          # a scene depends on its number alone
    assert torch.equal(cut.frame(2), plain.frame(2))                                            # and looking back selects the earlier scene again
    assert [e['clip'].cuts for e in synthetic_roidb(2, 8, 48, 64, 4, cuts=(5,))] == [(5,), (5,)]
    with pytest.raises(ValueError):
        SyntheticClip(0, 8, 48, 64, cuts=(8,))


# ---- the margin under the GPU end-to-end test ---------------------------------------------------------------------------------------------------
def test_end_to_end_clip_is_decisive():
    """on the clip tests/test_me_cut_gpu.py runs end to end, the reference leaves at most 25 % of the blocks unmatched on every pair inside a
    scene and at least 75 % on every cut pair: the expected key frames rest on a margin, not on a boundary of percent = 50"""
    from lsfa_amd.core.loader import key_plan
    e = rc.E2E
    counts, blocks = rc.e2e_unmatched()
    print("unmatched of %d blocks per pair:" % blocks, counts)
    for f, c in enumerate(counts, start=1):
        if f in e['cuts']:
            assert c * 100 >= 75 * blocks, (f, c)
        else:
            assert c * 100 <= 25 * blocks, (f, c)
    found = {f for f, c in enumerate(counts, start=1) if rc.is_cut(c, blocks, rc.PERCENT)}
    assert found == set(e['cuts']) and key_plan(e['frames'], e['interval'], found) == e['keys']


# ---- the interface ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_the_binding_derives_the_export():
    import ctypes
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsfa_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+lsfa_mv_cut_score\s*\(", text)
    from lsfa_amd import hip
    ret, params = hip._PROTOTYPES["lsfa_mv_cut_score"]
    assert ret.strip() == "int"
    assert [hip._ctype(p) for p in params] == [ctypes.c_void_p, ctypes.c_longlong] + [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_int] + \
        [ctypes.c_void_p] * 3
    for name in ("mv_cut_score", "cut_flags", "ME_CUT_BIAS", "ME_CUT_PERCENT"):
        assert hasattr(hip, name), name
    assert (hip.ME_CUT_BIAS, hip.ME_CUT_PERCENT) == (rc.BIAS, rc.PERCENT)
    assert "me_cut.hip" in __import__("lsfa_amd.build", fromlist=["SOURCES"]).SOURCES
    with pytest.raises(hip.LsfaError):
        hip._cut_params("test", dict(bias=256))
    with pytest.raises(hip.LsfaError):
        hip._cut_params("test", dict(percent=0))
    with pytest.raises(hip.LsfaError):
        hip._cut_params("test", dict(threshold=3))
    assert hip._cut_params("test", dict()) == (4, 50) and hip._cut_params("test", None) is None
    np.testing.assert_array_equal(hip.cut_flags([12, 13], 24, 50), [False, True])
