"""The motion-estimation specification pinned on the CPU (tests/ref_me.py): known motion is recovered exactly, the tie-break, partial
blocks, the frame-edge rule and max_sad behave as written.  The device kernels (tests/test_me_gpu.py) are compared with this reference
bit for bit, so it is checked here against cases whose answer is known without running it."""
import os
import re

import numpy as np
import pytest

import oracle
import ref_me

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

W, H = 1000, 600
MBW, MBH = 63, 38


def true_source_inside(m, width=W, height=H):
    """(mbh, mbw) bool: the block's covered rectangle shifted by -m (where its content was one frame earlier) lies inside the frame"""
    mbh, mbw = -(-height // 16), -(-width // 16)
    x0, y0 = 16 * np.arange(mbw)[None, :], 16 * np.arange(mbh)[:, None]
    x1, y1 = np.minimum(x0 + 16, width) - 1, np.minimum(y0 + 16, height) - 1
    return (x0 - m[0] >= 0) & (x1 - m[0] <= width - 1) & (y0 - m[1] >= 0) & (y1 - m[1] <= height - 1)


@pytest.mark.parametrize("m,sigma", [((3, -2), 0.0), ((-5, 7), 0.0), ((3, -2), 3.0), ((-5, 7), 3.0)])
def test_translation_is_recovered_exactly(m, sigma):
    """Frames cut from one uniform random texture at offset -m * f: every block whose true source block lies inside the frame returns
    exactly m (dst - src).  A wrong candidate's SAD is about 256 * 85 there, far above any lambda * 64 and above sigma-3 noise (about
    256 * 3.4), so this is a derivation, not a tuned threshold.  2,294 of 2,394 blocks: all but one border column (38) and one border
    row (63) that share a corner."""
    f0, f1 = ref_me.translated_clip(2, W, H, m, seed=11, sigma=sigma)
    rows, sad = ref_me.estimate(ref_me.luma(f1), ref_me.luma(f0), 16, 4)
    assert rows.shape == (MBH * MBW, 7) and sad.shape == (MBH, MBW)
    inside = true_source_inside(m)
    assert int(inside.sum()) == 2294
    v = ref_me.vectors(rows, MBH, MBW)
    exact = (v[..., 0] == m[0]) & (v[..., 1] == m[1])
    assert int((exact & inside).sum()) == 2294
    if sigma == 0.0:
        assert (sad[inside] == 0).all()
    # the fixed columns of every row
    np.testing.assert_array_equal(rows[:, :3], np.tile(np.array([-1, 16, 16], np.int32), (MBH * MBW, 1)))
    np.testing.assert_array_equal(rows[:, 5].reshape(MBH, MBW), np.tile(16 * np.arange(MBW) + 8, (MBH, 1)))
    np.testing.assert_array_equal(rows[:, 6].reshape(MBH, MBW), np.tile((16 * np.arange(MBH) + 8)[:, None], (1, MBW)))


def test_nine_chained_frames_accumulate_to_nine_m():
    """A key frame + nine frames of m = (3, -2) chained through coviar_accumulate: the accumulated vector is 9 m on every pixel at least
    48 from the border (a wrong border block reaches at most 16 + 9 * 3 = 43 pixels inward).  R = 8 keeps the host time down."""
    m, n = (3, -2), 10
    frames = ref_me.translated_clip(n, W, H, m, seed=5)
    accu = oracle.coviar_identity(W, H)
    lum = [ref_me.luma(f) for f in frames]
    for f in range(1, n):
        rows, _ = ref_me.estimate(lum[f], lum[f - 1], 8, 4)
        accu = oracle.coviar_accumulate(rows, accu)
    mv = oracle.coviar_mv(accu)[48:H - 48, 48:W - 48]
    assert mv.shape[0] * mv.shape[1] == 455616
    assert (mv[..., 0] == 9 * m[0]).all() and (mv[..., 1] == 9 * m[1]).all()


def test_flat_frames_give_zero_vectors():
    y = np.full((H, W), 77, np.uint8)
    rows, sad = ref_me.estimate(y, y.copy(), 16, 4)
    assert (ref_me.vectors(rows, MBH, MBW) == 0).all() and (sad == 0).all()
    rows, sad = ref_me.estimate(y, y.copy(), 16, 0)          # lambda 0: every candidate costs 0, the order (|dx| + |dy|, dy, dx) decides
    assert (ref_me.vectors(rows, MBH, MBW) == 0).all() and (sad == 0).all()


def test_luma_formula():
    bgr = np.array([[[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30]]], np.uint8)
    want = [0, 255, (29 * 255 + 128) >> 8, (150 * 255 + 128) >> 8, (77 * 255 + 128) >> 8, (290 + 3000 + 2310 + 128) >> 8]
    assert ref_me.luma(bgr).tolist() == [want]


def test_tie_break_order():
    """Candidates with equal cost: (|dx| + |dy|, dy, dx) decides.  A random patch (values >= 100) on black is the current block; the
    reference holds exact copies of it at chosen shifts on black, so exactly those candidates have SAD 0."""
    patch = np.random.RandomState(3).randint(100, 256, (16, 16)).astype(np.uint8)
    ref3 = np.zeros((32, 48), np.uint8)
    cur3 = np.zeros((32, 48), np.uint8)
    cur3[16:, 16:32] = patch                          # block (1, 1) of a 48-wide plane: x in [16, 32), y in [16, 32)
    ref3[0:16, 0:16] = patch                          # (dx, dy) = (-16, -16): length 32
    ref3[0:16, 32:48] = patch                         # (dx, dy) = (+16, -16): length 32, same dy, larger dx
    rows, sad = ref_me.estimate(cur3, ref3, 16, 4)
    v = ref_me.vectors(rows, 2, 3)[1, 1]
    assert sad[1, 1] == 0 and (v[0], v[1]) == (16, 16)        # dst - src = -(dx, dy): dx = -16 won over dx = +16
    ref4 = np.zeros((48, 48), np.uint8)
    cur4 = np.zeros((48, 48), np.uint8)
    cur4[16:32, 16:32] = patch
    ref4[0:16, 16:32] = patch                         # (dx, dy) = (0, -16): length 16
    ref4[16:32, 32:48] = patch                        # (dx, dy) = (+16, 0): length 16, larger dy loses
    ref4[32:48, 0:16] = patch                         # (dx, dy) = (-16, +16): length 32 loses on length at equal SAD once lambda > 0
    for lam in (0, 4):
        rows, sad = ref_me.estimate(cur4, ref4, 16, lam)
        v = ref_me.vectors(rows, 3, 3)[1, 1]
        assert sad[1, 1] == 0 and (v[0], v[1]) == (0, 16), lam     # (dx, dy) = (0, -16)
    # lambda 0, lengths differ: ref5 holds the patch at (-16, +16) (length 32) and at (+16, 0) (length 16): cost 0 both, the shorter wins
    ref5 = np.zeros((48, 48), np.uint8)
    ref5[32:48, 0:16] = patch
    ref5[16:32, 32:48] = patch
    rows, sad = ref_me.estimate(cur4, ref5, 16, 0)
    v = ref_me.vectors(rows, 3, 3)[1, 1]
    assert sad[1, 1] == 0 and (v[0], v[1]) == (-16, 0)


def test_lambda_trades_sad_for_length():
    """A copy 16 pixels away with SAD 0 against the co-located block with SAD s: the far one wins iff 16 lambda < s (equal cost: the
    shorter vector, i.e. (0, 0), wins)."""
    rs = np.random.RandomState(4)
    patch = rs.randint(100, 200, (16, 16)).astype(np.uint8)
    cur = np.zeros((48, 48), np.uint8)
    cur[16:32, 16:32] = patch
    ref = np.zeros((48, 48), np.uint8)
    ref[16:32, 32:48] = patch                       # (dx, dy) = (+16, 0), SAD 0
    near = patch.copy()
    near[0, :10] += 8                               # co-located copy with SAD 80
    ref[16:32, 16:32] = near
    for lam, want in ((4, (-16, 0)), (5, (0, 0)), (6, (0, 0))):
        rows, sad = ref_me.estimate(cur, ref, 16, lam)
        v = ref_me.vectors(rows, 3, 3)[1, 1]
        assert (v[0], v[1]) == want, lam
        assert sad[1, 1] == (0 if want != (0, 0) else 80)


def test_max_sad_turns_a_block_to_zero():
    f0, f1 = ref_me.translated_clip(2, 96, 64, (3, -2), seed=2)
    y0, y1 = ref_me.luma(f0), ref_me.luma(f1)
    y1 = y1.copy()
    y1[16:32, 32:48] = np.random.RandomState(9).randint(0, 256, (16, 16))       # block (2, 1): nothing in the reference matches it
    rows, sad = ref_me.estimate(y1, y0, 16, 4)
    rows_t, sad_t = ref_me.estimate(y1, y0, 16, 4, max_sad=5000)
    v, vt = ref_me.vectors(rows, 4, 6), ref_me.vectors(rows_t, 4, 6)
    assert sad[1, 2] > 5000 and (vt[1, 2] == 0).all()
    np.testing.assert_array_equal(sad, sad_t)                   # the SAD output keeps the winner's
    keep = sad <= 5000
    assert keep.sum() >= 10 and (v[keep] == vt[keep]).all() and (vt[~keep] == 0).all()


def test_partial_block_uses_only_its_covered_rows():
    """H = 40: the last block row covers 8 rows.  Its match must come from those rows alone: the block is found at its true shift although
    the 8 rows below the frame do not exist, and its SAD is 0."""
    m = (2, 3)
    f0, f1 = ref_me.translated_clip(2, 64, 40, m, seed=8)
    rows, sad = ref_me.estimate(ref_me.luma(f1), ref_me.luma(f0), 8, 4)
    v = ref_me.vectors(rows, 3, 4)
    inside = true_source_inside(m, 64, 40)
    assert inside[2].sum() == 3 and (v[2][inside[2]] == np.array(m)).all() and (sad[2][inside[2]] == 0).all()
    # W = 40: the same for the last block column (8 covered columns)
    f0, f1 = ref_me.translated_clip(2, 40, 64, m, seed=8)
    rows, sad = ref_me.estimate(ref_me.luma(f1), ref_me.luma(f0), 8, 4)
    v = ref_me.vectors(rows, 4, 3)
    inside = true_source_inside(m, 40, 64)
    assert (v[inside] == np.array(m)).all() and (sad[inside] == 0).all() and inside[:, 2].sum() == 3


def test_a_candidate_that_leaves_the_frame_is_never_chosen():
    """Pure noise against pure noise: every block picks SOME candidate; none of them may move the covered rectangle out of the frame - also
    where the zero padding outside it would have matched better (a black current frame against a bright reference: out-of-frame zeros
    would have SAD 0)."""
    rs = np.random.RandomState(1)
    for (w, h, r) in ((96, 64, 16), (37, 23, 32), (40, 40, 4)):
        for cur, ref in ((rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h, w)).astype(np.uint8)),
                         (np.zeros((h, w), np.uint8), rs.randint(128, 256, (h, w)).astype(np.uint8))):
            rows, _ = ref_me.estimate(cur, ref, r, 0)
            mbh, mbw = -(-h // 16), -(-w // 16)
            dx, dy = (rows[:, 3] - rows[:, 5]).reshape(mbh, mbw), (rows[:, 4] - rows[:, 6]).reshape(mbh, mbw)
            x0, y0 = 16 * np.arange(mbw)[None, :], 16 * np.arange(mbh)[:, None]
            x1, y1 = np.minimum(x0 + 16, w) - 1, np.minimum(y0 + 16, h) - 1
            assert (x0 + dx >= 0).all() and (x1 + dx <= w - 1).all() and (y0 + dy >= 0).all() and (y1 + dy <= h - 1).all()
            assert (np.abs(dx) <= r).all() and (np.abs(dy) <= r).all()


def test_header_and_binding_declare_the_feature():
    text = open(os.path.join(ROOT, "include", "lsfa_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("lsfa_luma_u8", "lsfa_mv_estimate"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert "LSFA_OP_MV_ESTIMATE" in text
    from lsfa_amd import hip
    assert "mv_estimate" in hip.OP_NAMES
    for name in ("luma_u8", "mv_estimate", "MotionEstimator"):
        assert hasattr(hip, name), name
