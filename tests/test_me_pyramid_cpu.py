"""The pyramid motion search without a device: tests/ref_me_pyramid.py, the numpy statement of the specification (include/lsfa_hip.h,
lsfa_luma_pyramid / lsfa_mv_refine_chain; DESIGN.md "Pyramid search"), pinned by cases with a known answer.  tests/test_me_pyramid_gpu.py
compares the kernels with it bit for bit."""
import numpy as np
import pytest

import oracle
import ref_me
import ref_me_pyramid as rp
import ref_me_segment


# ---- the pyramid ---------------------------------------------------------------------------------------------------------------------------------
def test_a_constant_plane_stays_constant():
    for shape in ((5, 3), (16, 16), (37, 23)):
        levels = rp.pyramid(np.full(shape, 201, np.uint8), 2)
        assert [p.shape for p in levels] == [shape, (-(-shape[0] // 2), -(-shape[1] // 2)), (-(-shape[0] // 4), -(-shape[1] // 4))]
        assert all((p == 201).all() and p.dtype == np.uint8 for p in levels)


def test_five_by_three_by_hand():
    """5 wide, 3 high -> 3 x 2; the last column and the last row repeat their only tap"""
    p = np.array([[10, 20, 30, 40, 50],
                  [60, 70, 80, 90, 100],
                  [110, 120, 130, 140, 150]], np.uint8)
    want = np.array([[(10 + 20 + 60 + 70 + 2) >> 2, (30 + 40 + 80 + 90 + 2) >> 2, (50 + 50 + 100 + 100 + 2) >> 2],
                     [(110 + 120 + 110 + 120 + 2) >> 2, (130 + 140 + 130 + 140 + 2) >> 2, (150 * 4 + 2) >> 2]], np.uint8)
    got = rp.down(p)
    assert got.shape == (2, 3)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(want, [[40, 60, 75], [115, 135, 150]])


def test_the_rounding():
    assert rp.down(np.array([[0, 0], [0, 1]], np.uint8)).tolist() == [[0]]          # (1 + 2) >> 2
    assert rp.down(np.array([[0, 0], [1, 1]], np.uint8)).tolist() == [[1]]          # (2 + 2) >> 2
    assert rp.down(np.array([[255, 255], [255, 255]], np.uint8)).tolist() == [[255]]


def test_level_two_is_two_steps_not_one():
    rs = np.random.RandomState(0)
    p = rs.randint(0, 256, (5, 7)).astype(np.uint8)         # 7 wide, 5 high
    levels = rp.pyramid(p, 2)
    assert levels[2].shape == (2, 2)
    np.testing.assert_array_equal(levels[2], rp.down(rp.down(p)))
    # ... and the two roundings show: a 4 x 4 mean in one step differs somewhere on random planes
    q = rs.randint(0, 256, (64, 64)).astype(np.uint8)
    one_step = ((q.astype(np.int64).reshape(16, 4, 16, 4).sum(axis=(1, 3)) + 8) >> 4).astype(np.uint8)
    assert (rp.pyramid(q, 2)[2] != one_step).any()


# ---- levels = 0 -----------------------------------------------------------------------------------------------------------------------------------
def test_levels_zero_is_the_full_search():
    frames = ref_me.translated_clip(2, 70, 45, (3, -2), seed=1, sigma=3.0)
    cur, ref = ref_me.luma(frames[1]), ref_me.luma(frames[0])
    for search, lam, max_sad in ((4, 0, 0), (8, 4, 0), (8, 4, 1500)):
        rows, sad = rp.estimate(cur, ref, 0, search, lam, max_sad)
        want_rows, want_sad = ref_me.estimate(cur, ref, search, lam, max_sad)
        np.testing.assert_array_equal(rows, want_rows)
        np.testing.assert_array_equal(sad, want_sad)
    assert rp.reach(0, 16, 2) == 16 and rp.reach(1, 16, 2) == 34 and rp.reach(2, 8, 2) == 38 and rp.reach(2, 32, 3) == 137


# ---- a known answer beyond the full search's reach ------------------------------------------------------------------------------------------------
KNOWN, known_answer_case = rp.KNOWN, rp.known_answer_case


def test_known_answer_beyond_the_old_reach():
    k = KNOWN
    ref, cur, ok = known_answer_case()
    assert ok.shape == (12, 16) and ok.sum() * 3 > ok.size, int(ok.sum())        # more than a third of the 192 blocks
    assert int(ok.sum()) == 96                                                  # bx 4..15, by 0..7, by the arithmetic of the three levels
    rows, sad = rp.estimate(cur, ref, k['levels'], k['search'], k['lam'], 0, k['refine'])
    v = ref_me.vectors(rows, 12, 16)
    hit = (v[..., 0] == k['m'][0]) & (v[..., 1] == k['m'][1])
    assert hit[ok].all(), "eligible blocks without the translation: %s" % np.argwhere(ok & ~hit).tolist()
    assert (sad[ok] == 0).all()
    # the point of the feature: no parameter of the full search expresses this vector
    full = ref_me.vectors(ref_me.estimate(cur, ref, 32, k['lam'], 0)[0], 12, 16)
    assert not ((full[..., 0] == k['m'][0]) & (full[..., 1] == k['m'][1])).any()
    assert np.abs(full).max() <= 32 < rp.reach(k['levels'], k['search'], k['refine'])


# ---- the refinement's rules -----------------------------------------------------------------------------------------------------------------------
def forced_parent_rows(width, height, vec):
    """rows of the level above a (height, width) plane, every block with the vector `vec` (src - dst)"""
    h1, w1 = -(-height // 2), -(-width // 2)
    z = np.zeros((h1, w1), np.uint8)
    rows = ref_me.estimate(z, z, 1, 0)[0].copy()
    rows[:, 3] += vec[0]
    rows[:, 4] += vec[1]
    return rows


@pytest.mark.parametrize("vec", [(3, -2), (-9, 7), (40, 40)])
def test_zero_candidate_on_a_static_frame(vec):
    """a parent field forced to nonzero vectors: the window never holds (0, 0) for |2 v| > refine, yet a static frame returns all zeros"""
    rs = np.random.RandomState(2)
    p = rs.randint(0, 256, (45, 70)).astype(np.uint8)
    rows, sad = rp.refine(p, p, forced_parent_rows(70, 45, vec), 2, 4, 0)
    assert rows.shape == (3 * 5, 7)
    assert (rows[:, 3:5] == rows[:, 5:7]).all() and (sad == 0).all()


def test_max_sad_zeroes_level_zero_winners_only():
    frames = ref_me.translated_clip(2, 96, 64, (6, -4), seed=3, sigma=6.0)
    cur, ref = ref_me.luma(frames[1]), ref_me.luma(frames[0])
    rows_off, sad_off, lv_off = rp.estimate(cur, ref, 2, 4, 4, 0, 2, return_levels=True)
    moved = (rows_off[:, 3:5] != rows_off[:, 5:7]).any(axis=1)
    thr = int(np.median(sad_off.reshape(-1)[moved]))
    rows_on, sad_on, lv_on = rp.estimate(cur, ref, 2, 4, 4, thr, 2, return_levels=True)
    np.testing.assert_array_equal(sad_on, sad_off)                       # the SAD output keeps the winner's
    for k in (1, 2):
        np.testing.assert_array_equal(lv_on[k], lv_off[k])               # the levels above are searched without the threshold
    intra = sad_off.reshape(-1) > thr
    assert (intra & moved).any() and (~intra & moved).any()
    assert (rows_on[intra, 3:5] == rows_on[intra, 5:7]).all()
    np.testing.assert_array_equal(rows_on[~intra], rows_off[~intra])


def test_cost_is_on_the_absolute_vector():
    """a flat frame: every candidate has SAD 0, so with lambda > 0 the zero vector wins whatever the parent says; with lambda = 0 the tie
    goes to the shortest valid candidate, (0, 0) again"""
    p = np.full((64, 96), 77, np.uint8)
    for lam in (0, 4):
        rows, _ = rp.refine(p, p, forced_parent_rows(96, 64, (5, 5)), 3, lam, 0)
        assert (rows[:, 3:5] == rows[:, 5:7]).all()


# ---- odd sizes and the walk-back contract ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("width,height", [(37, 23), (250, 130)])
def test_odd_sizes_stay_inside_the_walk_back_contract(width, height, levels):
    """one row per level-0 block, every source rectangle inside the frame, and tests/ref_me_segment.py's walk over these rows equals
    oracle.coviar_accumulate chained over them, bit for bit (the pin of tests/test_me_segment_cpu.py, on the new rows)"""
    frames = ref_me.translated_clip(4, width, height, (7, -5), seed=width + levels, sigma=3.0)
    lum = [ref_me.luma(f) for f in frames]
    rows = np.stack([rp.estimate(lum[f], lum[f - 1], levels, 4, 4, 0, 2)[0] for f in range(1, 4)])
    mbh, mbw = -(-height // 16), -(-width // 16)
    assert rows.shape == (3, mbh * mbw, 7)
    for r in rows:
        assert (r[:, 0] == -1).all() and (r[:, 1:3] == 16).all()
        np.testing.assert_array_equal(r[:, 5], np.tile(16 * np.arange(mbw) + 8, mbh))
        np.testing.assert_array_equal(r[:, 6], np.repeat(16 * np.arange(mbh) + 8, mbw))
        x0, y0 = r[:, 3] - 8, r[:, 4] - 8                                # the source rectangle of the covered part
        bw, bh = np.minimum(16, width - (r[:, 5] - 8)), np.minimum(16, height - (r[:, 6] - 8))
        assert (x0 >= 0).all() and (y0 >= 0).all() and (x0 + bw <= width).all() and (y0 + bh <= height).all()
    assert (rows[:, :, 3:5] != rows[:, :, 5:7]).any()
    walked = ref_me_segment.walk(rows, width, height)
    accu = oracle.coviar_identity(width, height)
    for f in range(3):
        accu = oracle.coviar_accumulate(rows[f], accu)
        np.testing.assert_array_equal(walked[f], accu, err_msg="frame %d" % (f + 1))
