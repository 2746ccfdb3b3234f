"""Tracks on torch tensors: the ctypes wrapper of lsfa_track_steps (lsfa_amd/csrc/tracks.hip; include/lsfa_hip.h, "Tracks").  Built on
lsfa_amd/hip.py's binding and checkers and under its rule: every tensor is validated before its pointer is taken, and there is no fallback -
a missing library or a refused call is an LsfaError.

The detections stay where lsfa_det_postprocess(_batch) left them - dets (ncls, R, 5) float64 and counts (ncls) int32 - and every row gets a
track id on the device: ids (ncls, R) int32, -1 for a row that is not eligible, 0 for a tentative or dropped one, else the id, which
Overlay.draw_bgr / draw_yuv420 take as `ids=` for one colour and one number per object.  The block rows of MotionEstimator /
SegmentMotionEstimator, if given, predict where last frame's boxes went; they are read in place through their strides.  A call is one launch,
allocates nothing and reads nothing back, so it can be captured in a graph; state() and stats() are the only synchronising calls.

This is the project's own float64 / integer specification (the header; DESIGN.md "Tracks"; tests/ref_tracks.py in numpy).  The reference has
no tracker; it is not SORT, Seq-NMS or a Kalman filter, and the defaults below are not tuned values."""
import math

import torch

from lsfa_amd import hip
from lsfa_amd.hip import LsfaError, _check, _ptr, _tensor

MAX_TRACKS = 1024           # LSFA_TRACK_MAX_TRACKS
MAX_CLASSES = 4096          # LSFA_OVERLAY_MAX_CLASSES
MAX_FRAMES = 4096


class Tracker(object):
    """Tracks the detections of `streams` independent clips of `ncls` classes x `R` rows, `frames` frames a call.  Owns the state - tbox
    (S, T, 5) float64 [x1, y1, x2, y2, score], tint (S, T, 4) int32 [id, class, hits, misses], issued (S) int32; all zero is the empty
    tracker - and the outputs ids (S, F, ncls, R) int32 and n (S, F, 4) int32 {eligible, matched, born, dropped}.
      score_thresh: rows below it are not tracked (the caller's display threshold); iou_thresh: the least IoU of a match
      max_age: a track unmatched for more than max_age frames is freed; min_hits: ids read 0 until a track was matched min_hits times"""

    def __init__(self, ncls, R, max_tracks=256, score_thresh=0.5, iou_thresh=0.3, max_age=10, min_hits=1, streams=1, frames=1, device='cuda:0'):
        for what, v, lo, hi in (("ncls", ncls, 1, MAX_CLASSES), ("R", R, 1, 1 << 24), ("max_tracks", max_tracks, 1, MAX_TRACKS), ("max_age", max_age, 0, 1 << 30),
                                ("min_hits", min_hits, 1, 1 << 30), ("streams", streams, 1, 65535), ("frames", frames, 1, MAX_FRAMES)):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise LsfaError("Tracker: %s %r is not an int in %d..%d" % (what, v, lo, hi))
        if (ncls - 1) * R >= 1 << 31:
            raise LsfaError("Tracker: %d classes x %d rows: (ncls - 1) * R must stay below 2^31" % (ncls, R))
        for what, v in (("score_thresh", score_thresh), ("iou_thresh", iou_thresh)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise LsfaError("Tracker: %s %r is not a finite number" % (what, v))
        self.ncls, self.R, self.max_tracks, self.max_age, self.min_hits, self.streams, self.frames = ncls, R, max_tracks, max_age, min_hits, streams, frames
        self.score_thresh, self.iou_thresh = float(score_thresh), float(iou_thresh)
        self.device = torch.device(device)
        self.tbox = torch.zeros((streams, max_tracks, 5), dtype=torch.float64, device=self.device)
        self.tint = torch.zeros((streams, max_tracks, 4), dtype=torch.int32, device=self.device)
        self.issued = torch.zeros((streams,), dtype=torch.int32, device=self.device)
        self.ids = torch.zeros((streams, frames, ncls, R), dtype=torch.int32, device=self.device)
        self.n = torch.zeros((streams, frames, 4), dtype=torch.int32, device=self.device)
        self._all_rows = torch.zeros((streams, frames), dtype=torch.int32, device=self.device)          # row_n of a call that gives rows alone
        self._all_rows_value = 0

    def _launch(self, who, S, F, dets, counts, rows, row_n, n_max, stream_stride, frame_stride):
        """validates what a call does not own alone - the state and the outputs may have been replaced - and launches lsfa_track_steps"""
        T = self.max_tracks
        _tensor(who, "tbox", self.tbox, torch.float64, (self.streams, T, 5), self.device)
        _tensor(who, "tint", self.tint, torch.int32, (self.streams, T, 4), self.device)
        _tensor(who, "issued", self.issued, torch.int32, (self.streams,), self.device)
        _tensor(who, "ids", self.ids, torch.int32, (self.streams, self.frames, self.ncls, self.R), self.device)
        _tensor(who, "n", self.n, torch.int32, (self.streams, self.frames, 4), self.device)
        if rows is not None:
            if row_n is None:
                if self._all_rows_value != n_max:
                    self._all_rows.fill_(n_max)
                    self._all_rows_value = n_max
                row_n = self._all_rows
            _tensor(who, "row_n", row_n, torch.int32, (self.streams, self.frames), self.device)
        elif row_n is not None:
            raise LsfaError("%s: row_n without rows" % who)
        _check(hip.lib().lsfa_track_steps(_ptr(dets), _ptr(counts), S, F, self.ncls, self.R, _ptr(rows), _ptr(row_n), n_max, stream_stride, frame_stride,
                                          self.score_thresh, self.iou_thresh, self.max_age, self.min_hits, T, _ptr(self.tbox), _ptr(self.tint),
                                          _ptr(self.issued), _ptr(self.ids), _ptr(self.n), hip._stream()), "lsfa_track_steps")

    def _rows(self, who, rows, lead):
        """rows (lead.., blocks, 7) int32 with rows of 7 consecutive ints 7 ints apart; the leading axes may be strided -> (n_max, strides)"""
        dims = len(lead) + 2
        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int32 or rows.device != self.device or rows.dim() != dims or \
                tuple(rows.shape[:-2]) != tuple(lead) or int(rows.shape[-1]) != 7 or int(rows.shape[-2]) < 1 or rows.stride(-1) != 1 or \
                (int(rows.shape[-2]) > 1 and rows.stride(-2) != 7) or any(st < 0 for st in rows.stride()):
            raise LsfaError("%s: rows must be a (%s) int32 tensor on %s whose rows are 7 consecutive ints, 7 ints apart, got %s strides %s" %
                            (who, ", ".join([str(v) for v in lead] + ["blocks", "7"]), self.device, hip._arrived(rows),
                             tuple(rows.stride()) if isinstance(rows, torch.Tensor) else None))
        return int(rows.shape[-2]), [int(st) for st in rows.stride()[:-2]]

    @hip._on_tensor_device
    def step(self, dets, counts, rows=None, row_n=None):
        """One frame of one stream (a Tracker of streams=1, frames=1): dets (ncls, R, 5) float64, counts (ncls) int32; rows (blocks, 7) int32,
        e.g. MotionEstimator.rows as it stands, predicts from all its rows, or from the first row_n ((1, 1) int32 on the device) of them.
        Returns ids (ncls, R) int32, a view of self.ids that the next call overwrites."""
        who = "Tracker.step"
        if self.streams != 1 or self.frames != 1:
            raise LsfaError("%s: this Tracker was made for %d streams x %d frames a call; use steps" % (who, self.streams, self.frames))
        _tensor(who, "dets", dets, torch.float64, (self.ncls, self.R, 5), self.device)
        _tensor(who, "counts", counts, torch.int32, (self.ncls,), self.device)
        n_max = 0
        if rows is not None:
            n_max, _ = self._rows(who, rows, ())
        self._launch(who, 1, 1, dets, counts, rows, row_n, n_max, 0, 0)
        return self.ids[0, 0]

    @hip._on_tensor_device
    def steps(self, dets, counts, rows=None, row_n=None):
        """`frames` frames of every stream in one launch: dets (S, F, ncls, R, 5) float64, counts (S, F, ncls) int32; rows (S, F, blocks, 7)
        int32, e.g. SegmentMotionEstimator.rows (C, n, blocks, 7) as it stands or a strided view of it, read in place; row_n (S, F) int32 on
        the device says how many rows of each frame predict (0: none, a key frame that starts a new chain), None: all of them.
        Returns ids (S, F, ncls, R) int32, self.ids."""
        who = "Tracker.steps"
        S, F = self.streams, self.frames
        _tensor(who, "dets", dets, torch.float64, (S, F, self.ncls, self.R, 5), self.device)
        _tensor(who, "counts", counts, torch.int32, (S, F, self.ncls), self.device)
        n_max, strides = 0, [0, 0]
        if rows is not None:
            n_max, strides = self._rows(who, rows, (S, F))
        self._launch(who, S, F, dets, counts, rows, row_n, n_max, strides[0], strides[1])
        return self.ids

    def reset(self, stream=None):
        """the empty tracker again, for every stream or for stream `stream`; no synchronisation"""
        if stream is None:
            parts = (self.tbox, self.tint, self.issued)
        else:
            if isinstance(stream, bool) or not isinstance(stream, int) or not 0 <= stream < self.streams:
                raise LsfaError("Tracker.reset: stream %r is not an int in 0..%d" % (stream, self.streams - 1))
            parts = (self.tbox[stream], self.tint[stream], self.issued[stream:stream + 1])
        for t in parts:
            t.zero_()

    def state(self):
        """(tbox, tint, issued) read back as numpy; synchronises"""
        return self.tbox.cpu().numpy(), self.tint.cpu().numpy(), self.issued.cpu().numpy()

    def stats(self):
        """n of the last call read back: (S, F, 4) int32 numpy {eligible, matched, born, dropped}; synchronises"""
        return self.n.cpu().numpy()
