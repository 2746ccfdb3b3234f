"""The inputs of tests/test_iou_sliver_gpu.py, and the proof on the CPU that they hold what they claim.

iou_test.h decides a pair of boxes without dividing unless d = fma(-thresh, uni, inter) lies in the sliver
0 < d < thresh * 2^-22 * uni (2^-51 in float64), the union is not positive, or the threshold is outside the fast range;
five call sites then redo their work with the division.  Every input set built here puts pairs of a stated kind
(tests/ref_iou.py) at stated sorted positions - a diagonal 64 x 64 tile, an off-diagonal one, the partial last tile as a
row and as a column - among ordinary boxes, and this file asserts per set:

  * each placed pair is of its kind, at its position, and DECIDES a survivor: flipping that one pair's answer in
    ref_iou's sweep changes the keep list;
  * the oracle and ref_iou's sweep on the division's answer give the same survivors;
  * a fast test that answers from the sign of d alone, and a caller that never redoes, each give other survivors - so
    the GPU tests fail for either mistake.  Where a set cannot tell one of them (stated at the set), that is asserted too.

These are conditions of the tests, not measurements: a set that does not meet them fails here, without a GPU.
"""
import numpy as np
import pytest

import oracle
import ref_iou

K, S, D = "sliver_keep", "sliver_suppress", "degenerate"

# ---- the known sliver pairs: (A, B) as [x1, y1, x2, y2] with y = 0; B ranks below A -------------------------------------------
# float32 0.7 keep: IoU = 60928 / 87040 = 7/10 > 0.7f, the quotient rounds to 0.7f.  The others are p / q just above the
# threshold as one-row boxes of width W shifted by dx (inter = W - dx, uni = W + dx).


def _row_pair(W, dx):
    return [0, 0, W - 1, 0], [dx, 0, dx + W - 1, 0]


SLIVER_PAIRS = {
    ("float32", 0.7, K): ([0, 0, 271, 271], [48, 0, 319, 271]),
    ("float32", 0.7, S): _row_pair(850006, 150001),                         # 700005 / 1000007
    ("float32", 0.3, K): _row_pair(2423384, 1304899),                       # 1118485 / 3728283: rounds to 0.3f
    ("float32", 0.3, S): _row_pair(1300002, 700001),                        # 600001 / 2000003
    ("float64", 0.3, K): ([0, 0, 5, 0], [3, 0, 9, 0]),                      # 3 / 10 > 0.3 as doubles
    ("float64", 0.3, S): _row_pair(1950000000000002, 1050000000000001),     # 900000000000001 / 3000000000000003
    ("float64", 0.7, K): ([0, 0, 7, 0], [1, 0, 9, 0]),                      # 7 / 10 > 0.7 as doubles
    ("float64", 0.7, S): _row_pair(1700000000000006, 300000000000001),      # 1400000000000005 / 2000000000000007
}
DEGENERATE_BOX = {
    "zero": [5, 0, 4, 4],            # x2 = x1 - 1: area 0; two of them: 0 / 0
    "negative": [10, 0, 8.5, 0],     # area -0.5 (less than any other box has); two of them: union -1
    "infinite": [0, 0, np.inf, 10],  # area inf; two of them: inf - inf
}


def ordinary_boxes(rs, n, dtype):
    """Clusters of overlapping boxes in [0, 1000) x [0, 600): some pairs suppress, some do not."""
    k = max(3, n // 12)
    cx = rs.uniform(50, 950, k)[rs.randint(0, k, n)] + rs.normal(0, 14, n)
    cy = rs.uniform(50, 550, k)[rs.randint(0, k, n)] + rs.normal(0, 14, n)
    w, h = rs.uniform(30, 200, n), rs.uniform(30, 200, n)
    b = np.stack([np.clip(cx - w / 2, 0, 999), np.clip(cy - h / 2, 0, 599), np.clip(cx + w / 2, 0, 999), np.clip(cy + h / 2, 0, 599)], 1)
    return b.astype(dtype)


def place(boxes, placements, dtype, thresh, degenerate=None):
    """Overwrite rows of `boxes` (sorted positions) with the placed pairs.  Every sliver pair gets rows of its own far
    below the ordinary boxes (an integer shift in y is exact), so that it overlaps nothing else: A always survives and B's
    fate is that pair's answer.  The degenerate boxes all sit on one row: any two of them are a degenerate pair."""
    name = np.dtype(dtype).name
    for k, (i, j, kind) in enumerate(placements):
        if kind == D:
            continue
        a, b = SLIVER_PAIRS[(name, thresh, kind)]
        y = 20000 + 1000 * k
        boxes[i] = [a[0], a[1] + y, a[2], a[3] + y]
        boxes[j] = [b[0], b[1] + y, b[2], b[3] + y]
    if degenerate:
        g = DEGENERATE_BOX[degenerate]
        for i in sorted(set(p for i, j, kind in placements if kind == D for p in (i, j))):
            boxes[i] = [g[0], g[1] + 10000, g[2], g[3] + 10000]
    return boxes


# layouts: n -> name -> placements (row position, column position, kind); tiles are (row // 64, column // 64)
_BASE = [(3, 40, K), (10, 55, S), (20, 70, K), (30, 100, S)]          # the diagonal tile (0, 0), the off-diagonal (0, 1)
NMS_LAYOUTS = {
    130: {      # three column blocks, the last tile has 2 columns
        "column": _BASE + [(90, 128, K), (110, 129, S)],      # the partial tile as a column: tile (1, 2)
        "row_keep": _BASE + [(128, 129, K)],                  # ... as a row: its own diagonal tile (2, 2) holds one pair
        "row_suppress": _BASE + [(128, 129, S)],
    },
    65: {       # the last tile has 1 column
        "column_keep": [(3, 40, K), (10, 55, S), (20, 64, K)],
        "column_suppress": [(3, 40, K), (10, 55, S), (20, 64, S)],
    },
    64: {"full": [(3, 40, K), (10, 55, S), (0, 63, K), (1, 62, S)]},
}
# degenerate boxes at 5, 33 and 129: a pair in the diagonal tile (5, 33) and two in the partial column tile ((5, 129), and
# (33, 129), which decides nothing where 5 suppresses 33), each tile with a sliver pair and ordinary pairs beside it;
# (72, 100) is a sliver pair in a tile (1, 1) that holds no degenerate pair
DEGENERATE_LAYOUT = [(3, 40, K), (5, 33, D), (5, 129, D), (20, 70, S), (72, 100, K), (50, 128, S)]
FAST_THRESHOLDS = (0.3, 0.7)
SLOW_THRESHOLDS = {"float32": (0.0, -0.1, 1e-31), "float64": (0.0, -0.1, 1e-301)}


def nms_set(n, layout, dtype, thresh):
    """(boxes (n, 4) in score order, placements)"""
    boxes = ordinary_boxes(np.random.RandomState(n), n, dtype)
    placements = NMS_LAYOUTS[n][layout]
    return place(boxes, placements, dtype, thresh), placements


def nms_degenerate_set(kind, dtype, thresh):
    boxes = ordinary_boxes(np.random.RandomState(7), 130, dtype)
    return place(boxes, DEGENERATE_LAYOUT, dtype, thresh, degenerate=kind), DEGENERATE_LAYOUT


def nms_slow_set(dtype):
    """Thresholds outside the fast range divide everywhere: the boxes of the 0.7 column layout."""
    return nms_set(130, "column", dtype, 0.7)[0]


def with_scores(boxes):
    """(n, 5) dets: strictly falling scores, so that the order is the index order for every sort."""
    n = boxes.shape[0]
    s = (1.0 - np.arange(n) / (2.0 * n)).astype(boxes.dtype)
    return np.concatenate([boxes, s[:, None]], 1)


def oracle_keep(boxes, thresh):
    if boxes.dtype == np.float32:
        return oracle.nms_sorted(boxes, thresh)
    return oracle.nms_f64(with_scores(boxes), thresh)


NMS_SETS = [(n, layout) for n in (130, 65, 64) for layout in NMS_LAYOUTS[n]]
DTYPES = ("float32", "float64")


def check_placed(c, placements):
    """Every placed pair is of its kind and decides a survivor."""
    keep = ref_iou.sweep(c.div)
    for i, j, kind in placements:
        assert getattr(c, kind)[i, j], "pair (%d, %d) is not %s" % (i, j, kind)
        assert i in keep, "row box %d of pair (%d, %d) does not survive" % (i, i, j)
        assert not np.array_equal(ref_iou.sweep(ref_iou.flip(c.div, i, j)), keep), "pair (%d, %d) decides nothing" % (i, j)
    return keep


def tiles_of(c, kind):
    i, j = np.nonzero(np.triu(getattr(c, kind), 1))
    return set(zip((i // 64).tolist(), (j // 64).tolist()))


# ---- ref_iou on the known pairs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(SLIVER_PAIRS, key=str), ids=lambda k: "%s-%s-%s" % k)
def test_known_pairs_are_what_they_claim(key):
    name, thresh, kind = key
    a, b = SLIVER_PAIRS[key]
    for boxes in ([a, b], [b, a]):                  # row and column swapped
        c = ref_iou.classify(np.array(boxes, name), thresh, name)
        assert getattr(c, kind)[0, 1] and getattr(c, kind)[1, 0]
        assert c.unsure[0, 1] and c.pos[0, 1] and not c.fast_answer[0, 1]
        assert bool(c.div[0, 1]) == (kind == S)
        assert list(oracle_keep(np.array([a, b], name), thresh)) == ([0] if kind == S else [0, 1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sorted(DEGENERATE_BOX))
def test_degenerate_pairs_divide(dtype, kind):
    """Zero and NaN unions: float32 keeps the second box (NaN > thresh is false), float64 suppresses it (numpy's rule).  A
    negative union: the fast test would say "suppress" (d > 0 and clear), the division keeps."""
    g = DEGENERATE_BOX[kind]
    c = ref_iou.classify(np.array([g, g], dtype), 0.7, dtype)
    assert c.degenerate[0, 1] and c.unsure[0, 1]
    assert bool(c.div[0, 1]) == (dtype == "float64" and kind != "negative")
    assert bool(c.fast_answer[0, 1]) == (kind == "negative")
    assert len(oracle_keep(np.array([g, g], dtype), 0.7)) == (1 if c.div[0, 1] else 2)


def test_round_to_format_is_one_rounding():
    from fractions import Fraction
    rs = np.random.RandomState(0)
    for _ in range(2000):
        x = float(rs.randn() * 10.0 ** rs.randint(-5, 6))
        assert ref_iou.round_to_format(Fraction(x), 24) == Fraction(float(np.float32(x)))
        assert ref_iou.round_to_format(Fraction(x), 53) == Fraction(x)
    half = Fraction(1) + Fraction(1, 2 ** 24)          # a tie between 1 and 1 + 2^-23: to even
    assert ref_iou.round_to_format(half, 24) == 1 and ref_iou.round_to_format(half + Fraction(1, 2 ** 23), 24) == 1 + Fraction(1, 2 ** 22)


# ---- the NMS sets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thresh", FAST_THRESHOLDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,layout", NMS_SETS)
def test_nms_sets_hold_deciding_sliver_pairs_at_each_position(n, layout, dtype, thresh):
    boxes, placements = nms_set(n, layout, dtype, thresh)
    c = ref_iou.classify(boxes, thresh, dtype)
    keep = check_placed(c, placements)
    assert not c.degenerate.any()                   # nothing but a sliver makes a tile of these sets divide
    # the placed pairs are the only slivers, so the positions are exactly the layout's
    assert tiles_of(c, K) == set((i // 64, j // 64) for i, j, k in placements if k == K)
    assert tiles_of(c, S) == set((i // 64, j // 64) for i, j, k in placements if k == S)
    assert (0, 0) in tiles_of(c, K) and (0, 0) in tiles_of(c, S)
    if n == 130:
        assert (0, 1) in tiles_of(c, K) and (0, 1) in tiles_of(c, S)
        want = {"column": [(1, 2, K), (1, 2, S)], "row_keep": [(2, 2, K)], "row_suppress": [(2, 2, S)]}[layout]
        for rb, cb, kind in want:
            assert (rb, cb) in tiles_of(c, kind)
    if n == 65:
        assert (0, 1) in tiles_of(c, K if layout == "column_keep" else S)
    # ordinary pairs of both outcomes beside the slivers, in every tile the slivers sit in
    for rb, cb in tiles_of(c, K) | tiles_of(c, S):
        sl = (slice(rb * 64, rb * 64 + 64), slice(cb * 64, cb * 64 + 64))
        if min(n - rb * 64, n - cb * 64) >= 32:
            assert c.plain_suppress[sl].any() and c.plain_keep[sl].any()
    assert 1 < len(keep) < n
    np.testing.assert_array_equal(oracle_keep(boxes, thresh), keep)
    assert not np.array_equal(ref_iou.sweep(ref_iou.sign_only_answer(c, tile_redo=True)), keep)
    assert not np.array_equal(ref_iou.sweep(ref_iou.never_redo_answer(c)), keep)


@pytest.mark.parametrize("thresh", FAST_THRESHOLDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sorted(DEGENERATE_BOX))
def test_nms_degenerate_sets(kind, dtype, thresh):
    """A degenerate pair in the diagonal tile and in the partial column tile, each beside a sliver pair and ordinary pairs,
    every one deciding.  A caller that never redoes differs through the sliver pairs in every set, and through the
    degenerate pairs themselves where the fast answer is not the division's (float64 zero / NaN unions, negative unions);
    a sign-only fast test differs through the sliver pair of tile (1, 1), which no degenerate pair makes divide."""
    boxes, placements = nms_degenerate_set(kind, dtype, thresh)
    c = ref_iou.classify(boxes, thresh, dtype)
    keep = check_placed(c, placements)
    assert tiles_of(c, D) == {(0, 0), (0, 2)}
    for tile in ((0, 0), (0, 2)):
        assert tile in tiles_of(c, K) | tiles_of(c, S)
        sl = (slice(tile[0] * 64, tile[0] * 64 + 64), slice(tile[1] * 64, tile[1] * 64 + 64))
        assert c.plain_keep[sl].any()
    assert c.plain_suppress[:64, :64].any()      # (the partial tile's two columns are both placed boxes: nothing else suppresses them)
    assert (1, 1) in tiles_of(c, K) and (1, 1) not in tiles_of(c, D)
    np.testing.assert_array_equal(oracle_keep(boxes, thresh), keep)
    assert not np.array_equal(ref_iou.sweep(ref_iou.sign_only_answer(c, tile_redo=True)), keep)
    assert not np.array_equal(ref_iou.sweep(ref_iou.never_redo_answer(c)), keep)
    only_degenerate = np.where(c.degenerate, c.fast_answer, c.div)       # the fast answer stands for degenerate unions alone
    differs = not np.array_equal(ref_iou.sweep(only_degenerate), keep)
    assert differs == (kind == "negative" or dtype == "float64")


@pytest.mark.parametrize("dtype", DTYPES)
def test_nms_slow_thresholds_divide_everywhere(dtype):
    boxes = nms_slow_set(dtype)
    for thresh in SLOW_THRESHOLDS[dtype]:
        c = ref_iou.classify(boxes, thresh, dtype)
        assert not c.fast and c.unsure.all()
        np.testing.assert_array_equal(oracle_keep(boxes, thresh), ref_iou.sweep(c.div))
    assert len(ref_iou.sweep(ref_iou.classify(boxes, -0.1, dtype).div)) == 1       # every IoU, 0 included, is > -0.1


@pytest.mark.parametrize("dtype", DTYPES)
def test_identical_boxes_at_thresh_one_are_all_kept(dtype):
    """IoU = 1 and d == 0: not positive, nothing suppresses.  A test on d >= 0 would keep one box."""
    boxes = identical_boxes(dtype)
    c = ref_iou.classify(boxes, 1.0, dtype)
    assert c.fast and c.plain_keep.all() and not c.pos.any()
    assert np.array_equal(c.inter, c.uni)
    np.testing.assert_array_equal(ref_iou.sweep(c.div), np.arange(130))
    np.testing.assert_array_equal(oracle_keep(boxes, 1.0), np.arange(130))


def identical_boxes(dtype):
    return np.tile(np.array([[10, 20, 109, 79]], dtype), (130, 1))


# ---- Proposal ----------------------------------------------------------------------------------------------------------------
# One ratio-1 anchor per cell on stride 16, a 12 x 14 map, threshold 0.7, rpn_min_size 0.  Four cells decode to two pairs of
# big boxes; every other cell gets dw = dh so negative that its box is a few pixels around its anchor's centre, overlaps no
# other small box, is a sliver of a big box's area and survives - so a big box can be ranked below any number of survivors.
#   keep:     scale 17, a 272 x 272 anchor; with zero deltas, cells three apart decode to the float32 0.7 keep pair (cells
#             with index >= 8 are not clipped at 0).  No other two of the four big boxes exceed 0.7.
#   suppress: scale 86, a 1376 x 1376 anchor.  Two such boxes offset by (183, 69) have inter = 1193 * 1307 = 1559251 and
#             uni = 2227501: 10 p - 7 q = 3, the quotient rounds to the float after 0.7f.  Found by solving
#             17 (L - ox)(L - oy) = 14 L^2 + k over L = 16 * scale and small k; the offsets come from dx, dy in steps of 1 / 32
#             (43 pixels, exact in float32) and whole cells: 183 = 5 * 43 - 2 * 16, 69 = 7 * 16 - 43.  dx = dy = 1 / 2 puts
#             a box's corner at (8 + 16 w, 8 + 16 h); the second pair sits 33 steps (1419 pixels) further down.
PROPOSAL = dict(H=12, W=14, ratios=(1,), feature_stride=16, threshold=0.7, rpn_min_size=0)
PROPOSAL_IM_INFO = (4096.0, 4096.0, 1.0)
PROPOSAL_SIDES = {      # scales, dw = dh of the small boxes, ((h, w), (dx, dy)) of A1, B1, A2, B2, the pairs' kind
    "keep": dict(scales=(17,), small=-3.0, kind=K,
                 big=(((8, 8), (0, 0)), ((8, 11), (0, 0)), ((11, 9), (0, 0)), ((11, 12), (0, 0)))),
    "suppress": dict(scales=(86,), small=-6.0, kind=S,
                     big=(((0, 2), (16 / 32, 16 / 32)), ((7, 0), (21 / 32, 15 / 32)), ((1, 3), (16 / 32, 49 / 32)), ((8, 1), (21 / 32, 48 / 32)))),
}
# sorted positions (A1, B1, A2, B2) of the four big boxes
PROPOSAL_CASES = {
    "top": (0, 1, 70, 130),          # first and second; A below 64 survivors and B a block further down
    "boundary": (62, 66, 5, 140),    # across the boundary of the first two 64-candidate blocks; first block against the last
    "degenerate": (0, 1, 70, 130),   # + two zero-area boxes (dw = -20), see proposal_image
}
ZERO_CELLS = ((2, 3), (5, 9))
ZERO_POSITIONS = (10, 100)


def proposal_image(side, case):
    """cls_prob (2, H, W), bbox_pred (4, H, W) of one image, and the sorted positions of the big boxes."""
    H, W = PROPOSAL["H"], PROPOSAL["W"]
    geo = PROPOSAL_SIDES[side]
    deltas = np.zeros((4, H, W), np.float32)
    deltas[2:] = geo["small"]
    for (h, w), (dx, dy) in geo["big"]:
        deltas[:, h, w] = [dx, dy, 0.0, 0.0]
    ranked = dict(zip(PROPOSAL_CASES[case], [cell for cell, _ in geo["big"]]))
    if case == "degenerate":
        # dw = -20: the decoded width (anchor * e^-20) vanishes against the centre, x1 = ctr + 0.5 and x2 = ctr - 0.5 after
        # rounding, x2 - x1 + 1 = 0.  rpn_min_size = 0 lets it through (0 < 0 is false); two such boxes have union 0.
        for (h, w), p in zip(ZERO_CELLS, ZERO_POSITIONS):
            deltas[2, h, w] = -20.0
            ranked[p] = (h, w)
    rest = [(h, w) for h in range(H) for w in range(W) if (h, w) not in ranked.values()]
    order = []
    for p in range(H * W):
        order.append(ranked[p] if p in ranked else rest.pop(0))
    prob = np.zeros((2, H, W), np.float32)
    for p, (h, w) in enumerate(order):
        prob[1, h, w] = np.float32(0.95 - 0.005 * p)
    prob[0] = 1 - prob[1]
    return prob, deltas, PROPOSAL_CASES[case]


def proposal_batch(side, cases):
    imgs = [proposal_image(side, c) for c in cases]
    prob = np.stack([i[0] for i in imgs])
    deltas = np.stack([i[1] for i in imgs])
    im_info = np.array([PROPOSAL_IM_INFO] * len(cases), np.float32)
    return prob, deltas, im_info


def proposal_kwargs(side):
    return dict(feature_stride=PROPOSAL["feature_stride"], scales=PROPOSAL_SIDES[side]["scales"], ratios=PROPOSAL["ratios"],
                threshold=PROPOSAL["threshold"], rpn_min_size=PROPOSAL["rpn_min_size"])


def inter_uni_of(two_boxes):
    inter, uni = ref_iou.inter_uni(np.ascontiguousarray(two_boxes, np.float32))
    return float(inter[0, 1]), float(uni[0, 1])


@pytest.mark.parametrize("case", sorted(PROPOSAL_CASES))
@pytest.mark.parametrize("side", sorted(PROPOSAL_SIDES))
def test_proposal_sets_rank_deciding_pairs_where_they_claim(side, case):
    """Through the oracle's own decoded boxes and order.  An image holds pairs of one side only (an operator has one set of
    scales): the keep side tells a sign-only fast test from the right one and not a caller that never redoes, the suppress
    side the other way round - both asserted, so that nobody takes one side for a proof against both mistakes."""
    geo = PROPOSAL_SIDES[side]
    prob, deltas, im_info = proposal_batch(side, [case])
    positions = proposal_image(side, case)[2]
    kw = proposal_kwargs(side)
    rois, scores, order, keep_o, nkeep = oracle.proposal(prob, deltas, im_info, return_debug=True, **kw)
    dec = oracle.proposal_decode(prob, deltas, im_info, feature_stride=16, scales=kw["scales"], ratios=kw["ratios"], rpn_min_size=0)[0]
    n = PROPOSAL["H"] * PROPOSAL["W"]
    assert order.shape == (1, n)
    boxes = dec[order[0], :4]
    for p, ((h, w), _) in zip(positions, geo["big"]):
        assert order[0, p] == h * PROPOSAL["W"] + w
    a1, b1, a2, b2 = positions
    if side == "keep":
        for p, ((h, w), _) in zip(positions, geo["big"]):
            np.testing.assert_array_equal(boxes[p], np.array([16 * w - 128, 16 * h - 128, 16 * w + 143, 16 * h + 143], np.float32))
    else:
        for a, b in ((a1, b1), (a2, b2)):
            np.testing.assert_array_equal(boxes[b] - boxes[a], np.array([183, 69, 183, 69], np.float32))
            np.testing.assert_array_equal(boxes[a, 2:] - boxes[a, :2], np.array([1375, 1375], np.float32))
            assert boxes[a].min() >= 0 and boxes[b].max() < 4095          # nothing clipped
            assert inter_uni_of(boxes[[a, b]]) == (1559251.0, 2227501.0)
    c = ref_iou.classify(boxes, 0.7, "float32")
    placements = [(a1, b1, geo["kind"]), (a2, b2, geo["kind"])]
    if case == "degenerate":
        placements.append((ZERO_POSITIONS[0], ZERO_POSITIONS[1], D))
        for p in ZERO_POSITIONS:
            assert ref_iou.box_area(boxes[p:p + 1])[0] == 0
        assert tiles_of(c, D) == {(0, 1)}
    else:
        assert not c.degenerate.any()
    keep = check_placed(c, placements)
    assert np.count_nonzero(np.triu(getattr(c, geo["kind"]), 1)) == 2
    assert np.count_nonzero(np.triu(c.sliver_keep | c.sliver_suppress, 1)) == 2
    if case != "boundary":
        assert np.count_nonzero(keep < a2) >= 64 and a2 // 64 != b2 // 64      # A2 is the 65th survivor or later, B2 a block further
    assert np.count_nonzero(np.triu(c.plain_suppress, 1)) == 0 and len(keep) == (n if side == "keep" else n - 2)
    np.testing.assert_array_equal(keep_o[0, :nkeep[0]], keep)
    sign_only = ref_iou.sweep(ref_iou.sign_only_answer(c, tile_redo=(case == "degenerate")))
    never_redo = ref_iou.sweep(ref_iou.never_redo_answer(c))
    assert np.array_equal(sign_only, keep) == (side == "suppress")
    assert np.array_equal(never_redo, keep) == (side == "keep")


# ---- detection post-processing ---------------------------------------------------------------------------------------------
# R = 70 rois, zero deltas (the decoded float64 boxes are the rois), 3 classes: class 1 ranks the rois in index order, so
# roi index = sorted position and positions 0..63 against 64..69 are the off-diagonal tile; class 2 ranks them at random.
DET = dict(R=70, ncls=3, im_h=600.0, im_w=1000.0, scale=1.0)
DET_LAYOUTS = {
    "sliver": [(3, 40, K), (20, 66, K), (30, 50, K), (64, 69, K)],
    "zero_diagonal": [(3, 40, K), (20, 66, K), (5, 33, D)],
    "zero_off_diagonal": [(3, 40, K), (20, 66, K), (10, 68, D)],
    "suppress": [(3, 40, S), (3, 66, S), (20, 50, K)],       # thresh 0.7 only; one row box against a column in each tile
}
# A float64 suppress-side sliver from float32 rois: p / q must lie within 2^-51 of the threshold, so q is near 1e15 and the
# boxes' extents are beyond 2^24, where float32 holds even numbers only (multiples of 4 beyond 2^25).  Two L x L boxes offset
# by (ox, oy) have p = (L - ox)(L - oy), q = 2 L^2 - p; 10 p - 7 q = k means 17 p = 14 L^2 + k.  k = 1 has no solution
# (6 is no square mod 17) and k = 3 needs L > 3.1e7; the first L with a factorisation whose corners are all float32 values
# is below.  At 0.3 the same form needs 13 p = 6 L^2 + 1, and 2 is no square mod 13 (k = 3 needs L > 4e7, where float32
# holds multiples of 4 only: not searched): no such pair is built for 0.3.  The image is 2^30 wide and high for this layout, so that nothing is clipped.
DET_SUPPRESS_07 = dict(L=31000283, ox=5118250, oy=422074)
DET_CASES = [(layout, thresh) for layout in sorted(DET_LAYOUTS) for thresh in FAST_THRESHOLDS if (layout, thresh) != ("suppress", 0.3)]


def det_image(layout):
    """(im_h, im_w, scale)"""
    side = float(2 ** 30) if layout == "suppress" else None
    return (side or DET["im_h"], side or DET["im_w"], DET["scale"])


def det_set(layout, thresh):
    """rois (R, 5), deltas (R, 8), probs (R, 3), placements.  The redo's "suppress" outcome is the zero-area pair in the
    'zero_*' layouts and the big pair of DET_SUPPRESS_07 (once as it is, once with x and y swapped) in 'suppress'."""
    R = DET["R"]
    g = DET_SUPPRESS_07
    big = [[g["ox"], g["oy"], g["ox"] + g["L"] - 1, g["oy"] + g["L"] - 1], [g["oy"], g["ox"], g["oy"] + g["L"] - 1, g["ox"] + g["L"] - 1]]
    rs = np.random.RandomState(70)
    boxes = np.floor(ordinary_boxes(rs, R, np.float64) * np.array([1, 0.6, 1, 0.6]))          # y < 360
    placements = DET_LAYOUTS[layout]
    boxes[65] = boxes[7] + [1, 0, 1, 0]         # an ordinary pair that suppresses across the two blocks
    for k, (i, j, kind) in enumerate(placements):
        y = 400 + 10 * k
        if kind == D:      # x2 = x1 - 1: two zero-area boxes, apart from each other
            boxes[i], boxes[j] = [700, y, 699, y + 4], [300, y, 299, y + 4]
        elif kind == S:
            assert thresh == 0.7
            boxes[i], boxes[j] = [0, 0, g["L"] - 1, g["L"] - 1], big.pop(0)
        else:
            a, b = SLIVER_PAIRS[("float64", thresh, K)]
            boxes[i], boxes[j] = [a[0], y, a[2], y], [b[0], y, b[2], y]
    rois = np.zeros((R, 5), np.float32)
    rois[:, 1:] = boxes
    deltas = np.zeros((R, 8), np.float32)
    probs = np.zeros((R, 3), np.float32)
    probs[:, 1] = 0.9 - 0.01 * np.arange(R)
    probs[:, 2] = rs.permutation(R) * 0.01 + 0.05
    probs[:, 0] = 0.01
    return rois, deltas, probs, placements


@pytest.mark.parametrize("layout,thresh", DET_CASES)
def test_det_sets(layout, thresh):
    rois, deltas, probs, placements = det_set(layout, thresh)
    im = det_image(layout)
    pred = oracle.bbox_pred_clip(rois, deltas, *im)
    boxes = pred[:, 4:8]
    np.testing.assert_array_equal(boxes, rois[:, 1:].astype(np.float64))
    w_d, w_c, w_k = oracle.det_postprocess(rois, deltas, probs, *im, nms_thresh=thresh, max_per_image=0)
    for cls in (1, 2):
        order = np.argsort(-probs[:, cls].astype(np.float64), kind="stable")
        c = ref_iou.classify(boxes[order], thresh, "float64")
        keep = ref_iou.sweep(c.div)
        np.testing.assert_array_equal(w_k[cls, :w_c[cls]], order[keep])
        assert 1 < len(keep) < DET["R"]
        if cls == 1:
            np.testing.assert_array_equal(order, np.arange(DET["R"]))
            check_placed(c, placements)
            assert {(0, 0), (0, 1)} <= tiles_of(c, S if layout == "suppress" else K)
            assert c.sliver_suppress.any() == (layout == "suppress")
            if layout == "suppress":
                g = DET_SUPPRESS_07
                p = (g["L"] - g["ox"]) * (g["L"] - g["oy"])
                assert 17 * p == 14 * g["L"] ** 2 + 3 and c.inter[3, 40] == c.inter[3, 66] == p and c.uni[3, 40] == 2 * g["L"] ** 2 - p
                assert not c.degenerate.any() and 40 not in keep and 66 not in keep
                assert not np.array_equal(ref_iou.sweep(ref_iou.never_redo_answer(c)), keep)
                assert not np.array_equal(ref_iou.sweep(ref_iou.sign_only_answer(c, tile_redo=True)), keep)      # through (20, 50)
            elif layout == "sliver":
                assert not c.degenerate.any() and (1, 1) in tiles_of(c, K)
                assert not np.array_equal(ref_iou.sweep(ref_iou.sign_only_answer(c, tile_redo=True)), keep)
            else:
                (i, j), = [(i, j) for i, j, kind in placements if kind == D]
                assert c.div[i, j] and not c.fast_answer[i, j] and j not in keep
                assert tiles_of(c, D) == {(0, 0) if layout == "zero_diagonal" else (0, 1)}
                assert not np.array_equal(ref_iou.sweep(ref_iou.never_redo_answer(c)), keep)
            assert c.plain_suppress[:64, :64].any() and c.plain_keep[:64, 64:].any() and c.plain_suppress[:64, 64:].any()
