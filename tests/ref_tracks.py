"""The tracker's specification (include/lsfa_hip.h "Tracks"; DESIGN.md "Tracks") stated once in plain numpy / Python float64: loops, one
rounding per operation, nothing vectorised that could reorder the arithmetic.  It is what lsfa_track_steps is compared with bit for bit;
tests/test_tracks_cpu.py pins it by cases whose answers are known by construction.  Comparable with nothing in the reference, which has no
tracker.

`Tracker` holds the state of S streams as the device does (tbox (S, T, 5) float64, tint (S, T, 4) int32, issued (S) int32) and advances it
with `step` (one frame of one stream) or `steps` ((S, F, ..)).  `plan_ids` is lsfa_overlay_plan_ids: ref_overlay.plan for rows that carry a
track id; its records go to ref_overlay.cover and the painters as they are."""
import math

import numpy as np

import ref_overlay

DASH = 38


def wrap32(v):
    """a Python int as the int32 the device holds"""
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def eligible(row, score_thresh):
    x1, y1, x2, y2, score = (float(v) for v in row)
    return all(math.isfinite(v) for v in (x1, y1, x2, y2, score)) and score >= score_thresh and x2 >= x1 and y2 >= y1


def lesser(a, b):
    return b if b < a else a


def greater(a, b):
    return b if b > a else a


def iou(a, b):
    """py_nms's arithmetic on two [x1, y1, x2, y2, ..] of np.float64; min and max are comparisons, so a NaN goes where they put it"""
    one, zero = np.float64(1.0), np.float64(0.0)
    area_a = (a[2] - a[0] + one) * (a[3] - a[1] + one)
    area_b = (b[2] - b[0] + one) * (b[3] - b[1] + one)
    ww = lesser(a[2], b[2]) - greater(a[0], b[0]) + one
    hh = lesser(a[3], b[3]) - greater(a[1], b[1]) + one
    w = ww if ww > zero else zero
    h = hh if hh > zero else zero
    inter = w * h
    return inter / (area_a + area_b - inter)


class Tracker(object):
    def __init__(self, ncls, R, max_tracks=256, score_thresh=0.5, iou_thresh=0.3, max_age=10, min_hits=1, streams=1):
        self.ncls, self.R, self.T, self.S = ncls, R, max_tracks, streams
        self.score_thresh, self.iou_thresh, self.max_age, self.min_hits = float(score_thresh), float(iou_thresh), max_age, min_hits
        self.tbox = np.zeros((streams, max_tracks, 5), np.float64)
        self.tint = np.zeros((streams, max_tracks, 4), np.int32)
        self.issued = np.zeros(streams, np.int32)

    def step(self, dets, counts, rows=None, row_n=None, stream=0):
        """one frame of one stream: dets (ncls, R, 5), counts (ncls); rows (>= row_n, 7) int32 or None -> ids (ncls, R) int32, n (4) int32"""
        with np.errstate(all="ignore"):          # a slot the caller filled with garbage may overflow or divide by zero: the bits are the answer
            return self._step(dets, counts, rows, row_n, stream)

    def _step(self, dets, counts, rows, row_n, stream):
        dets, counts = np.asarray(dets, np.float64), np.asarray(counts)
        tbox, tint = self.tbox[stream], self.tint[stream]
        ncls, R, T = self.ncls, self.R, self.T
        assert dets.shape == (ncls, R, 5) and counts.shape == (ncls,)
        ids = np.full((ncls, R), -1, np.int32)
        # 1: the eligible detections, in draw order
        E = []
        for j in range(1, ncls):
            for r in range(min(max(int(counts[j]), 0), R)):
                if eligible(dets[j, r], self.score_thresh):
                    E.append((j, r))
        # 2: predict
        nrow = 0 if rows is None or row_n is None else max(int(row_n), 0)
        if nrow > 0:
            rows = np.asarray(rows).reshape(-1, 7)
            nrow = min(nrow, rows.shape[0])          # row_n is clamped to n_max
            for t in range(T):
                if tint[t, 0] == 0:
                    continue
                x1, y1, x2, y2 = tbox[t, :4]
                c = sx = sy = 0
                for k in range(nrow):
                    srcx, srcy, dstx, dsty = (int(v) for v in rows[k, 3:7])
                    if x1 <= np.float64(srcx) <= x2 and y1 <= np.float64(srcy) <= y2:
                        c += 1
                        sx += dstx - srcx
                        sy += dsty - srcy
                if c > 0 and sx != 0:
                    dx = np.float64(sx) / np.float64(c)
                    tbox[t, 0] = x1 + dx
                    tbox[t, 2] = x2 + dx
                if c > 0 and sy != 0:
                    dy = np.float64(sy) / np.float64(c)
                    tbox[t, 1] = y1 + dy
                    tbox[t, 3] = y2 + dy
        # 3: associate
        taken, unmatched = set(), []
        for j, r in E:
            best, slot = None, None
            for t in range(T):
                if tint[t, 0] == 0 or int(tint[t, 1]) != j or t in taken:
                    continue
                v = iou(dets[j, r], tbox[t])
                if v >= self.iou_thresh and (slot is None or v > best):
                    best, slot = v, t
            if slot is None:
                unmatched.append((j, r))
                continue
            taken.add(slot)
            tbox[slot] = dets[j, r]
            tint[slot, 2] = wrap32(int(tint[slot, 2]) + 1)
            tint[slot, 3] = 0
            ids[j, r] = tint[slot, 0] if tint[slot, 2] >= self.min_hits else 0
        # 4: age
        for t in range(T):
            if tint[t, 0] != 0 and t not in taken:
                misses = wrap32(int(tint[t, 3]) + 1)
                if misses > self.max_age:
                    tbox[t] = 0.0
                    tint[t] = 0
                else:
                    tint[t, 3] = misses
        # 5: birth
        free = [t for t in range(T) if tint[t, 0] == 0]
        born = 0
        for j, r in unmatched:
            if born < len(free):
                slot = free[born]
                born += 1
                self.issued[stream] = wrap32(int(self.issued[stream]) + 1)
                tbox[slot] = dets[j, r]
                tint[slot] = (self.issued[stream], j, 1, 0)
                ids[j, r] = self.issued[stream] if 1 >= self.min_hits else 0
            else:
                ids[j, r] = 0
        n = np.array([len(E), len(E) - len(unmatched), born, len(unmatched) - born], np.int32)
        return ids, n

    def steps(self, dets, counts, rows=None, row_n=None):
        """dets (S, F, ncls, R, 5), counts (S, F, ncls); rows (S, F, >= n, 7) and row_n (S, F), or None -> ids (S, F, ncls, R), n (S, F, 4)"""
        dets, counts = np.asarray(dets, np.float64), np.asarray(counts)
        S, F = dets.shape[:2]
        assert S == self.S
        ids, n = np.zeros((S, F, self.ncls, self.R), np.int32), np.zeros((S, F, 4), np.int32)
        for s in range(S):
            for f in range(F):
                r = None if rows is None or row_n is None else rows[s][f]
                ids[s, f], n[s, f] = self.step(dets[s, f], counts[s, f], r, None if r is None else row_n[s][f], stream=s)
        return ids, n

    def state(self):
        return self.tbox.copy(), self.tint.copy(), self.issued.copy()


def plan_ids(dets, counts, ids, thresh, H, W, thickness=3, label_scale=2, with_score=True, names=None, max_boxes=256):
    """lsfa_overlay_plan_ids of one image: ref_overlay.plan's records for the rows with ids[j][r] > 0, the colour field 1 + (id - 1) % (ncls - 1)
    and "-" and the digits of id % 100000 between the name and the score -> (records (k, REC_INTS) int32, (recorded, eligible and not skipped))"""
    dets, counts, ids = np.asarray(dets, np.float64), np.asarray(counts), np.asarray(ids)
    ncls, R = dets.shape[:2]
    assert ncls >= 2 and ids.shape == (ncls, R)
    o, i = ref_overlay.ring(thickness)
    recs, kept = [], 0
    for j in range(1, ncls):
        for r in range(min(max(int(counts[j]), 0), R)):
            row = dets[j, r]
            if not np.isfinite(row).all() or not row[4] >= thresh:
                continue
            x1, y1, x2, y2 = (int(min(max(float(v), -ref_overlay.LIMIT), ref_overlay.LIMIT)) for v in row[:4])
            if x2 < x1 or y2 < y1 or x2 < 0 or y2 < 0 or x1 > W - 1 or y1 > H - 1:
                continue
            tid = int(ids[j, r])
            if tid <= 0:
                continue
            kept += 1
            if kept > max_boxes:
                continue
            ch = []
            if label_scale:
                ch = ref_overlay.characters(j, row[4], label_scale, False, names)
                ch += [DASH] + [ref_overlay.ZERO + int(d) for d in str(tid % 100000)]
                if with_score:
                    ch += ref_overlay.characters(j, row[4], label_scale, True, names)[-6:]
            L = len(ch)
            lx = ly = w = h = 0
            if L:
                w, h = label_scale * (6 * L + 1), 9 * label_scale
                lx, ly = x1 - o, y1 - o - h
                if ly < 0:
                    ly = y1 + i
                if lx + w > W:
                    lx = W - w
                if lx < 0:
                    lx = 0
            packed = [0] * (ref_overlay.REC_INTS - 10)
            for k, g in enumerate(ch):
                packed[k // 4] |= g << (8 * (k % 4))
            recs.append([x1, y1, x2, y2, lx, ly, w, h, 1 + (tid - 1) % (ncls - 1), L] + packed)
    return np.array(recs, np.int64).reshape(-1, ref_overlay.REC_INTS).astype(np.int32), (min(kept, max_boxes), kept)
