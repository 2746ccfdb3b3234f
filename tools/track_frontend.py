#!/usr/bin/env python
"""Time of the tracker (lsfa_amd/tracks.py: lsfa_track_steps, one launch per call) and of the overlay's ids variant, next to what they
have to be small against (device events, same process; profiles/r17/track_frontend.txt), at 1000x600, 31 classes x 300 rows:

    steps_f1_30[_rows]             one frame a call, 30 eligible detections, without and with 2,394 block rows
    steps_f9_{5,30,300}[_rows]     nine frames a call - the non-key frames of a segment - with 5 / 30 / 300 eligible detections a frame dealt
                                   to the classes in turn, tracked in the steady state (every detection matched)
    steps_f9_300_one_class[_rows]  the 300 in ONE class: one wave walks them one after the other
    steps_f9_30_churn              nothing ever matches (iou_thresh 2, max_age 0): every frame frees and bears 30 tracks
    plan_paint_30, plan_ids_paint_30   lsfa_overlay_plan + paint against lsfa_overlay_plan_ids + paint, BGR, 30 detections
    one non-key frame              tools/me_frontend.py's non_key_frame at 1000x600, eager

Every form is timed in turn, round by round, as tools/overlay_frontend.py does; min, median and max over the rounds, in microseconds per
call, and for the nine-frame calls per frame.  The goal to read off (reported, not gated): a frame of steps_f9_30_rows costs less than a
tenth of the non-key frame the same run measures.  --kernels-only runs the launches a few times without timing.  Prints one JSON object."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lsfa_amd import overlay, tracks
from overlay_frontend import DEV, NCLS, ROWS, alternating, detections

W, H = 1000, 600
BLOCKS = -(-W // 16) * -(-H // 16)          # 2,394
SLOTS = 512


def one_class(n, seed=0):
    rs = np.random.RandomState(seed)
    dets, counts = np.zeros((NCLS, ROWS, 5)), np.zeros(NCLS, np.int32)
    for k in range(n):
        w, h = rs.uniform(0.04, 0.3) * W, rs.uniform(0.06, 0.4) * H
        x1, y1 = rs.uniform(0, W - w), rs.uniform(0, H - h)
        dets[1, k] = (x1, y1, x1 + w, y1 + h, rs.uniform(0.7, 1.0))
    counts[1] = n
    return torch.from_numpy(dets).to(DEV), torch.from_numpy(counts).to(DEV)


def block_rows(F):
    """(1, F, BLOCKS, 7): the grid of a 1000x600 frame, every block moved by (2, 1)"""
    rows = np.zeros((BLOCKS, 7), np.int32)
    bx, by = np.meshgrid(np.arange(-(-W // 16)), np.arange(-(-H // 16)))
    rows[:, 0], rows[:, 1], rows[:, 2] = -1, 16, 16
    rows[:, 5], rows[:, 6] = 16 * bx.ravel() + 8, 16 * by.ravel() + 8
    rows[:, 3], rows[:, 4] = rows[:, 5] - 2, rows[:, 6] - 1
    return torch.from_numpy(np.broadcast_to(rows, (1, F, BLOCKS, 7)).copy()).to(DEV)


def tracker_form(F, dets, counts, with_rows, expect, **kw):
    tr = tracks.Tracker(NCLS, ROWS, max_tracks=SLOTS, score_thresh=0.7, frames=F, device=DEV, **kw)
    d = dets[None, None].expand(1, F, NCLS, ROWS, 5).contiguous()
    c = counts[None, None].expand(1, F, NCLS).contiguous()
    rows = block_rows(F) if with_rows else None
    fn = lambda: tr.steps(d, c, rows)          # noqa: E731
    fn()
    fn()
    got = tr.stats()[0, -1].tolist()          # the steady state: a box moved by the rows may lose its detection to a near twin
    assert got[0] == expect[0] and got[3] == 0 and abs(got[1] - expect[1]) <= expect[0] // 20, (got, expect)
    return fn


def forms():
    out = []
    for F, counts_ in ((1, (30,)), (9, (5, 30, 300))):
        for n in counts_:
            dets, counts = detections(n, W, H)
            for with_rows in (False, True):
                out.append(('steps_f%d_%d%s' % (F, n, '_rows' if with_rows else ''), tracker_form(F, dets, counts, with_rows, [n, n, 0, 0])))
    dets, counts = one_class(300)
    for with_rows in (False, True):
        out.append(('steps_f9_300_one_class%s' % ('_rows' if with_rows else ''), tracker_form(9, dets, counts, with_rows, [300, 300, 0, 0])))
    dets, counts = detections(30, W, H)
    out.append(('steps_f9_30_churn', tracker_form(9, dets, counts, False, [30, 0, 30, 0], iou_thresh=2.0, max_age=0)))
    bgr = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=DEV)
    ov = overlay.Overlay(NCLS, ROWS, max_boxes=512, device=DEV)
    tr = tracks.Tracker(NCLS, ROWS, max_tracks=SLOTS, score_thresh=0.7, device=DEV)
    ids = tr.step(dets, counts).clone()
    out.append(('plan_paint_30', lambda: ov.draw_bgr(bgr, dets, counts, 0.7)))
    out.append(('plan_ids_paint_30', lambda: ov.draw_bgr(bgr, dets, counts, 0.7, ids=ids)))
    out[-1][1]()
    assert int(ov.drawn()[0, 0]) == 30, ov.drawn()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50, help='calls per graph and per eager window')
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--skip-non-key', action='store_true')
    args = ap.parse_args()
    if args.kernels_only:
        for _, fn in forms():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        return
    out = dict(device=torch.cuda.get_device_name(0), classes=NCLS - 1, rows=ROWS, slots=SLOTS, block_rows=BLOCKS, calls_per_window=args.reps, rounds=args.rounds,
               unit='us per call')
    out['1000x600'] = r = alternating(forms(), args.reps, args.rounds)
    out['us_per_frame_of_a_nine_frame_call'] = {k: dict(graph=round(v['graph']['median'] / 9, 2), eager=round(v['eager']['median'] / 9, 2))
                                                for k, v in r.items() if k.startswith('steps_f9_')}
    if not args.skip_non_key:
        from me_frontend import non_key_frame
        out['non_key_frame_1000x600'] = non_key_frame(30)
        cur = out['non_key_frame_1000x600']['eager_us']
        per = out['us_per_frame_of_a_nine_frame_call']
        out['goal_a_frame_of_30_detections_below_a_tenth_of_the_non_key_frame'] = {
            k: dict(eager_us=per[k]['eager'], graph_us=per[k]['graph'], tenth_us=round(cur / 10, 1), met=bool(per[k]['eager'] < cur / 10))
            for k in ('steps_f9_30', 'steps_f9_30_rows')}
        out['overlay_pair_30'] = dict(plan_us=r['plan_paint_30'], plan_ids_us=r['plan_ids_paint_30'], tenth_us=round(cur / 10, 1))
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main()
