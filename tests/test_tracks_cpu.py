"""The tracker's specification (include/lsfa_hip.h "Tracks"), as tests/ref_tracks.py states it, pinned by cases whose answers are known by
construction - what prediction from block rows buys, ageing, births, ties, overflow, eligibility - and the ids variant of the overlay plan.
tests/test_tracks_gpu.py holds lsfa_track_steps to ref_tracks.py bit for bit; this file says that ref_tracks.py is the specification."""
import numpy as np

import ref_overlay
import ref_tracks as ref

NCLS, R = 3, 4


def frame(objects, ncls=NCLS, rows=R, score=0.9):
    """{class: [box, ..]} -> dets (ncls, rows, 5), counts (ncls); a box is (x1, y1, x2, y2) or (x1, y1, x2, y2, score)"""
    dets, counts = np.zeros((ncls, rows, 5)), np.zeros(ncls, np.int32)
    for j, boxes in objects.items():
        for r, b in enumerate(boxes):
            dets[j, r] = tuple(b) + (score,) * (5 - len(b))
        counts[j] = len(boxes)
    return dets, counts


def grid_rows(W, H, vector_at):
    """the rows of a 16 x 16 block grid: block centres (16 bx + 8, 16 by + 8) are dst, src = dst - vector_at(dst); a block whose
    vector_at is None gives no row"""
    out = []
    for by in range(H // 16):
        for bx in range(W // 16):
            dx_, dy_ = 16 * bx + 8, 16 * by + 8
            v = vector_at(dx_, dy_)
            if v is not None:
                out.append((-1, 16, 16, dx_ - v[0], dy_ - v[1], dx_, dy_))
    return np.array(out, np.int32).reshape(-1, 7)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def test_prediction_holds_an_identity_that_plain_iou_loses():
    box = lambda f: (100 + 32 * f, 100, 139 + 32 * f, 139)          # noqa: E731
    # consecutive boxes share 8 x 40 pixels: IoU 320 / (3200 - 320) = 0.111 < 0.3
    assert abs(float(ref.iou(np.array(box(0), np.float64), np.array(box(1), np.float64))) - 320.0 / 2880.0) < 1e-15
    plain, guided = ref.Tracker(NCLS, R, iou_thresh=0.3), ref.Tracker(NCLS, R, iou_thresh=0.3)
    rows = grid_rows(400, 304, lambda x, y: (32, 0))
    got_plain, got_guided = [], []
    for f in range(6):
        dets, counts = frame({1: [box(f)]})
        got_plain.append(int(plain.step(dets, counts)[0][1, 0]))
        ids, n = guided.step(dets, counts, rows if f else None, len(rows) if f else None)
        got_guided.append(int(ids[1, 0]))
        if f:
            assert tuple(n) == (1, 1, 0, 0)
    assert got_plain == [1, 2, 3, 4, 5, 6]
    assert got_guided == [1] * 6
    # the nine rows with src centres 104, 120, 136 each way give dx = 288 / 9 = 32 exactly: the predicted box IS the detection
    t = ref.Tracker(NCLS, R)
    t.step(*frame({1: [box(0)]}))
    t.step(*frame({}), rows=rows, row_n=len(rows))
    assert t.tbox[0, 0, :4].tolist() == [132.0, 100.0, 171.0, 139.0] and t.tint[0, 0].tolist() == [1, 1, 1, 1]


def test_two_boxes_of_a_class_that_cross_paths_keep_their_ids_with_rows():
    """A moves +48 a frame, B -48; between frames 2 and 3 each lands exactly where the other was, so plain IoU hands each the other's id"""
    xa, xb = [100, 148, 196, 244, 292], [340, 292, 244, 196, 148]
    box = lambda x: (x, 96, x + 47, 143)          # noqa: E731
    t = ref.Tracker(NCLS, R)
    for f in range(5):
        rows = None
        if f:
            def vector_at(x, y, f=f):          # a block on an object came from 48 px behind it
                if 96 <= y <= 143 and xa[f] <= x <= xa[f] + 47:
                    return (48, 0)
                if 96 <= y <= 143 and xb[f] <= x <= xb[f] + 47:
                    return (-48, 0)
                return None
            rows = grid_rows(512, 304, vector_at)
            assert len(rows) == 18
        dets, counts = frame({1: [box(xa[f]), box(xb[f])]} if f % 2 == 0 else {1: [box(xb[f]), box(xa[f])]})          # the draw order alternates
        ids, n = t.step(dets, counts, rows, None if rows is None else len(rows))
        a, b = (ids[1, 0], ids[1, 1]) if f % 2 == 0 else (ids[1, 1], ids[1, 0])
        assert (int(a), int(b)) == (1, 2), f
    assert t.issued[0] == 2


def test_a_detection_missing_for_max_age_frames_resumes_its_id_and_one_frame_longer_gets_a_new_one():
    box = (10, 10, 50, 50)
    for gap, want, issued in ((3, 1, 1), (4, 2, 2)):
        t = ref.Tracker(NCLS, R, max_age=3)
        assert t.step(*frame({2: [box]}))[0][2, 0] == 1
        for k in range(gap):
            ids, n = t.step(*frame({}))
            assert tuple(n) == (0, 0, 0, 0)
            assert t.tint[0, 0].tolist() == ([1, 2, 1, k + 1] if k < 3 else [0, 0, 0, 0])
        if gap == 4:
            assert not t.tbox.any() and not t.tint.any()          # freed: all nine values zero
        ids, n = t.step(*frame({2: [box]}))
        assert ids[2, 0] == want and t.issued[0] == issued
        assert t.tint[0, 0].tolist() == [want, 2, 2 if gap == 3 else 1, 0]          # the same slot either way
        assert not t.tint[0, 1:].any()


def test_min_hits_three_reads_zero_zero_then_the_id():
    t = ref.Tracker(NCLS, R, min_hits=3)
    got = [int(t.step(*frame({1: [(10, 10, 50, 50)]}))[0][1, 0]) for _ in range(4)]
    assert got == [0, 0, 1, 1]


def test_the_same_box_in_two_classes_is_two_tracks():
    t = ref.Tracker(NCLS, R)
    for _ in range(2):
        ids, n = t.step(*frame({1: [(10, 10, 50, 50)], 2: [(10, 10, 50, 50)]}))
        assert (ids[1, 0], ids[2, 0]) == (1, 2)
    assert tuple(n) == (2, 2, 0, 0) and t.tint[0, :2, 1].tolist() == [1, 2]


def test_ties_go_to_the_lowest_slot_and_to_the_first_detection():
    t = ref.Tracker(NCLS, R)
    t.tbox[0, 1] = t.tbox[0, 2] = (10, 10, 50, 50, 0.5)          # two identical tracks, in slots 1 and 2
    t.tint[0, 1], t.tint[0, 2] = (7, 1, 1, 0), (8, 1, 1, 0)
    t.issued[0] = 8
    ids, n = t.step(*frame({1: [(12, 10, 52, 50)]}))
    assert ids[1, 0] == 7 and tuple(n) == (1, 1, 0, 0) and t.tint[0, 1].tolist() == [7, 1, 2, 0] and t.tint[0, 2].tolist() == [8, 1, 1, 1]
    # two identical detections: the first in draw order takes the track, the second is born (into slot 1, the lowest free one)
    t = ref.Tracker(NCLS, R)
    t.step(*frame({1: [(10, 10, 50, 50)]}))
    ids, n = t.step(*frame({1: [(11, 10, 51, 50), (11, 10, 51, 50)]}))
    assert ids[1, :2].tolist() == [1, 2] and tuple(n) == (2, 1, 1, 0) and t.tint[0, :2, 0].tolist() == [1, 2]


def test_two_slots_and_three_objects_drop_one_without_spending_an_id():
    boxes = [(10, 10, 50, 50), (110, 10, 150, 50), (210, 10, 250, 50)]
    t = ref.Tracker(NCLS, R, max_tracks=2, max_age=0)
    ids, n = t.step(*frame({1: boxes}))
    assert ids[1, :3].tolist() == [1, 2, 0] and tuple(n) == (3, 0, 2, 1) and t.issued[0] == 2
    ids, n = t.step(*frame({1: boxes}))
    assert ids[1, :3].tolist() == [1, 2, 0] and tuple(n) == (3, 2, 0, 1) and t.issued[0] == 2
    ids, n = t.step(*frame({1: boxes[1:]}))          # the first object is gone: its slot is freed in step 4 and taken in step 5 of the same frame
    assert ids[1, :2].tolist() == [2, 3] and tuple(n) == (2, 1, 1, 0) and t.issued[0] == 3
    assert t.tint[0, :, 0].tolist() == [3, 2]


def test_rows_that_are_not_eligible_read_minus_one_and_start_no_track():
    nan, inf = float("nan"), float("inf")
    good = (10, 10, 50, 50, 0.9)
    junk = [(nan, 10, 50, 50, 0.9), (10, inf, 50, 50, 0.9), (10, 10, 50, -inf, 0.9), (10, 10, 50, 50, nan), (10, 10, 50, 50, np.nextafter(0.5, 0)),
            (50, 10, 10, 50, 0.9), (10, 50, 50, 10, 0.9)]
    for row in junk:
        t = ref.Tracker(NCLS, R, score_thresh=0.5)
        ids, n = t.step(*frame({1: [row]}))
        assert (ids == -1).all() and tuple(n) == (0, 0, 0, 0) and not t.tint.any(), row
    t = ref.Tracker(NCLS, R, score_thresh=0.5)
    ids, n = t.step(*frame({1: [(10, 10, 50, 50, 0.5)], 2: [(30, 30, 30, 30, 0.9)]}))          # score == thresh and a one-pixel box are eligible
    assert ids[1, 0] == 1 and ids[2, 0] == 2 and tuple(n) == (2, 0, 2, 0)
    # rows at and beyond counts, counts negative or above R, class 0
    dets = np.zeros((NCLS, R, 5))
    dets[:] = good
    for counts, want in (((R, 2, 0), [(1, 0), (1, 1)]), ((R, -3, 1), [(2, 0)]), ((R, R + 5, 0), [(1, r) for r in range(R)]), ((R, 0, 0), [])):
        t = ref.Tracker(NCLS, R, iou_thresh=2.0)          # nothing matches: every eligible row is born
        ids, n = t.step(dets, np.array(counts, np.int32))
        assert sorted(zip(*np.nonzero(ids >= 0))) == want and (ids[ids < 0] == -1).all() and n[0] == n[2] == len(want) and (ids[0] == -1).all()


def test_zero_sum_rows_leave_tbox_bit_identical():
    t = ref.Tracker(NCLS, R)
    t.tbox[0, 0] = (-0.0, 0.1 + 0.2, 47.3, 31.9, 0.7)
    t.tint[0, 0] = (1, 1, 1, 0)
    t.issued[0] = 1
    before = bits(t.tbox).copy()
    assert before[0, 0, 0] == np.int64(-2 ** 63)          # -0.0
    rows = np.array([(0, 0, 0, 8, 8, 13, 3), (0, 0, 0, 24, 8, 19, 13), (0, 0, 0, 500, 8, 0, 0)], np.int32)          # +5 and -5; the third is outside
    t.step(*frame({}), rows=rows, row_n=3)
    assert (bits(t.tbox) == before).all() and t.tint[0, 0].tolist() == [1, 1, 1, 1]
    t.step(*frame({}), rows=rows, row_n=1)          # x sum 5, y sum -5, one row
    assert t.tbox[0, 0, :4].tolist() == [5.0, (0.1 + 0.2) - 5.0, 47.3 + 5.0, 31.9 - 5.0]
    t.step(*frame({}), rows=rows, row_n=0)
    assert t.tbox[0, 0, 0] == 5.0


def scene(seed, F, ncls=NCLS, rows=R):
    rs = np.random.RandomState(seed)
    dets, counts = np.zeros((F, ncls, rows, 5)), np.zeros((F, ncls), np.int32)
    pos = rs.randint(0, 200, (ncls, rows, 2)).astype(np.float64)
    vel = rs.randint(-6, 7, (ncls, rows, 2)).astype(np.float64)
    for f in range(F):
        pos += vel
        dets[f, ..., 0:2] = pos
        dets[f, ..., 2:4] = pos + 40
        dets[f, ..., 4] = rs.uniform(0.3, 1.0, (ncls, rows))
        counts[f] = rs.randint(0, rows + 1, ncls)
    return dets, counts


def test_steps_over_five_frames_equal_five_step_calls():
    dets, counts = scene(1, 5)
    rows = np.stack([grid_rows(256, 256, lambda x, y, f=f: (f - 2, 1)) for f in range(5)])
    row_n = np.array([0, 256, 100, 1, 256], np.int32)
    a, b = ref.Tracker(NCLS, R, max_tracks=6, max_age=1), ref.Tracker(NCLS, R, max_tracks=6, max_age=1)
    ids, n = a.steps(dets[None], counts[None], rows[None], row_n[None])
    for f in range(5):
        ids_f, n_f = b.step(dets[f], counts[f], rows[f], row_n[f])
        assert (ids[0, f] == ids_f).all() and (n[0, f] == n_f).all()
    assert all((bits(x) == bits(y)).all() if x.dtype == np.float64 else (x == y).all() for x, y in zip(a.state(), b.state()))
    assert n[0, :, 1].sum() > 0 and n[0, :, 2].sum() > 0 and n[0, :, 3].sum() > 0


def test_two_streams_equal_two_single_stream_runs():
    d0, c0 = scene(2, 4)
    d1, c1 = scene(3, 4)
    both = ref.Tracker(NCLS, R, max_tracks=8, streams=2)
    ids, n = both.steps(np.stack([d0, d1]), np.stack([c0, c1]))
    for s, (d, c) in enumerate(((d0, c0), (d1, c1))):
        one = ref.Tracker(NCLS, R, max_tracks=8)
        ids_s, n_s = one.steps(d[None], c[None])
        assert (ids[s] == ids_s[0]).all() and (n[s] == n_s[0]).all()
        assert (bits(both.tbox[s]) == bits(one.tbox[0])).all() and (both.tint[s] == one.tint[0]).all() and both.issued[s] == one.issued[0]


def test_plan_ids_records_carry_the_tracks_colour_and_number():
    ncls = 4
    dets, counts = frame({1: [(10, 20, 50, 60), (5, 5, 30, 30)], 3: [(60, 10, 90, 40, 0.75), (0, 0, 20, 20), (1, 1, 9, 9)]}, ncls=ncls, rows=3)
    ids = np.full((ncls, 3), -1, np.int32)
    ids[1, :2] = (5, 0)                          # 0: tentative, not drawn
    ids[3, :3] = (1234567, -1, 3)                # 1234567 % 100000 = 34567
    names = np.full((ncls, ref_overlay.NAME_LEN), 0xFF, np.uint8)
    names[1, :3] = (13, 11, 28)                  # "car"
    names[3, :12] = np.arange(11, 23)            # twelve letters
    recs, n = ref.plan_ids(dets, counts, ids, 0.5, 100, 120, names=names)
    plain, _ = ref_overlay.plan(dets, counts, 0.5, 100, 120, names=names)
    assert n == (3, 3) and len(plain) == 5
    assert recs[:, :4].tolist() == [[10, 20, 50, 60], [60, 10, 90, 40], [1, 1, 9, 9]]
    assert recs[:, 8].tolist() == [1 + (5 - 1) % 3, 1 + (1234567 - 1) % 3, 1 + (3 - 1) % 3]

    def chars(rec):
        return [(rec[10 + k // 4] >> (8 * (k % 4))) & 255 for k in range(rec[9])]
    z, dot, dash = ref_overlay.ZERO, ref_overlay.DOT, ref.DASH
    assert chars(recs[0]) == [13, 11, 28, dash, z + 5, 0, z, dot, z + 9, z, z]
    assert chars(recs[1]) == list(range(11, 23)) + [dash, z + 3, z + 4, z + 5, z + 6, z + 7, 0, z, dot, z + 7, z + 5, z] and recs[1, 9] == 24
    assert chars(recs[2]) == list(range(11, 23)) + [dash, z + 3, 0, z, dot, z + 9, z, z]
    # the label rectangle follows the longer text
    assert recs[0, 6] == 2 * (6 * 11 + 1) and recs[1, 6] == 2 * (6 * 24 + 1)
    recs, n = ref.plan_ids(dets, counts, ids, 0.5, 100, 120, names=None, with_score=False, label_scale=1, max_boxes=2)
    assert n == (2, 3) and chars(recs[0]) == [z + 1, dash, z + 5] and chars(recs[1]) == [z + 3, dash, z + 3, z + 4, z + 5, z + 6, z + 7]
    recs, n = ref.plan_ids(dets, counts, ids, 0.5, 100, 120, label_scale=0)
    assert recs[:, 9].tolist() == [0, 0, 0] and not recs[:, 4:8].any()
    # every record paints with the overlay's own painter
    index = ref_overlay.cover(ref.plan_ids(dets, counts, ids, 0.5, 100, 120, names=names)[0], 100, 120, ncls, np.ones((42, 8), np.uint8) * 31)
    assert set(np.unique(index)) <= {-1, 1, 2, 3, ncls} and (index == 2).any() and (index == 3).any()
