"""TestLoader: key-frame scheduling and the per-frame input dict.

Mirror of dff_rfcn/core/loader.py:24-141: flag 0 = first frame of a
video, 1 = key frame (every TEST.KEY_FRAME_INTERVAL frames AND the last frame of every video),
2 = non-key frame; input order `data_name` (:41); placeholders of shape (1, DFF_FEAT_DIM, 1, 1)
for feat_key_old / feat_key (:138-139); `data_key` persists across videos while the first frame of
each video overrides `data_key_old` with itself (:119-122).  Frames come from the roidb
entry's clip generator (lsfa_amd.utils.synthetic) and live on the device.

estimate_mv, or config.TEST.ESTIMATE_MV where it is None (not in the reference; default None = the clip's own `motion_vector` /
`res_diff`): a dict of
hip.SegmentMotionEstimator's parameters (search, lam, max_sad; levels, refine for the pyramid search).  When a key frame is handed out, the
uint8 frames of it and of the non-key frames behind it are uploaded and the whole segment's inputs are estimated from
them on the current stream, in three launches (levels + 4 with the pyramid); each of those non-key frames then receives its slice.

estimate_mv=dict(..., cut=dict(bias=..., percent=...)) (not in the reference either: its dataset has no cuts) places a key frame where the
search says a new scene starts (hip.SegmentMotionEstimator(cut=...), DESIGN.md "Scene cuts"): the key frames of a video are key_plan() of
its cut frames.  A cut frame is handed out with flag 1 like any key frame and the segment behind it is estimated from it; the pairs a
segment estimated beyond its first cut are discarded.  Finding a segment's cut costs one readback (4 bytes per frame), and
upcoming_key_frames estimates the coming segments ahead, as far as it has to, to announce the key frames that will really come.

estimate_mv=dict(..., stale=dict(bias=..., percent=...)) (hip.SegmentMotionEstimator(stale=...), DESIGN.md "Stale key frames") also places
one where the segment's key frame has stopped predicting the frame - a fade, a dissolve, content that pans in.  A stale frame is treated
exactly like a cut frame: everything said of `cut` here holds for "cut or stale", and the frame the loader acts on is the first of a
segment flagged by either rule (the estimator's first_cuts).  The key rule depends on where the segment started, so a video's key frames
are no longer a function of a fixed set of frames: key_plan / next_key_frame are given, per segment, the first flagged frame behind its
key frame - all the loader uses.
"""
import collections

import numpy as np
import torch

from lsfa_amd.utils.motion_options import ends_early

# the estimated segment behind a key frame: tag = (roidb index, key frame), n non-key frames, mv (n, 1, 2, h, w), res (n, 1, 3, h, w), cut frame or None
Segment = collections.namedtuple('Segment', 'tag n mv res cut_f')


def next_key_frame(key_f, length, interval, cuts):
    """The key frame behind key frame key_f of a video of `length` frames: the smallest of key_f + interval, the video's last frame and
    the first cut frame in key_f + 1 .. min(key_f + interval - 1, length - 2).  `cuts`: the frames f whose pair (f, f - 1) is a cut."""
    last = min(key_f + interval, length - 1)
    return min([f for f in cuts if key_f < f < last] + [last])


def key_plan(length, interval, cuts):
    """Every key frame of a video, in order: a pure function of (length, interval, set of cut frames) - cut flags belong to consecutive
    pairs, so they do not depend on where the segments start.  It is what TestLoader's flags follow (next() and get_batch() move the key
    frame on by the same three rules, a segment's first cut taken from its estimate) and what upcoming_key_frames announces, one
    next_key_frame at a time."""
    keys = [0]
    while keys[-1] < length - 1:
        keys.append(next_key_frame(keys[-1], length, interval, cuts))
    return keys


class DataBatch(object):
    """mx.io.DataBatch stand-in: data = [[tensor per data_name]] (one list per device)."""

    def __init__(self, data, label=None, pad=0, index=0, provide_data=None, provide_label=None):
        self.data, self.label, self.pad, self.index = data, label, pad, index
        self.provide_data, self.provide_label = provide_data, provide_label


class TestLoader(object):
    def __init__(self, roidb, config, batch_size=1, shuffle=False, has_rpn=False, device='cuda:0', estimate_mv=None):
        assert batch_size == 1 and not shuffle
        if estimate_mv is None:           # the drivers that build their loader themselves (test_rcnn) are reached through the config
            estimate_mv = config.TEST.get('ESTIMATE_MV')
        self.estimate_mv = None if estimate_mv is None else dict(estimate_mv)
        self._estimators = {}           # (width, height) -> SegmentMotionEstimator
        # `cut` below: the pair rule (cut=) or the key rule (stale=) is on - a segment may end early, at its first flagged frame
        self.cut = ends_early(self.estimate_mv)
        self._segment = None            # the Segment under way
        self._segments = {}             # `cut`: (roidb index, key frame) -> Segment (None: nothing to estimate), the segments estimated ahead
        self.cfg, self.roidb, self.batch_size, self.shuffle, self.has_rpn = config, roidb, batch_size, shuffle, has_rpn
        self.device = device
        self.size = int(np.sum([x['frame_seg_len'] for x in self.roidb]))
        self.index = np.arange(self.size)
        self.data_name = ['data', 'im_info', 'data_key', 'data_key_old', 'motion_vector', 'res_diff', 'feat_key_old',
                          'feat_key']
        self.label_name = None
        self.cur_roidb_index = 0
        self.cur_frameid = 0
        self.data_key = None
        self.data_key_old = None
        self.key_frameid = 0
        self.cur_seg_len = 0
        self.key_frame_flag = -1
        self.cur = 0
        self.data = None
        self.label = []
        self.im_info = None
        self._ahead = {}
        self.reset()
        self.get_batch()

    @property
    def provide_data(self):
        return [[(k, tuple(v.shape)) for k, v in zip(self.data_name, idata)] for idata in self.data]

    @property
    def provide_label(self):
        return [None for _ in range(len(self.data))]

    @property
    def provide_data_single(self):
        return [(k, tuple(v.shape)) for k, v in zip(self.data_name, self.data[0])]

    @property
    def provide_label_single(self):
        return None

    def reset(self):
        self.cur = 0

    def iter_next(self):
        return self.cur < self.size

    def __iter__(self):
        return self

    def __next__(self):
        return self.next()

    def next(self):
        if self.iter_next():
            self.get_batch()
            self.cur += self.batch_size
            self.cur_frameid += 1
            if self.cur_frameid == self.cur_seg_len:
                self.cur_roidb_index += 1
                self.cur_frameid = 0
                self.key_frameid = 0
            elif self.cur_frameid - self.key_frameid == self.cfg.TEST.KEY_FRAME_INTERVAL or self._cut_at(self.key_frameid) == self.cur_frameid:
                self.key_frameid = self.cur_frameid
            return self.im_info, self.key_frame_flag, DataBatch(data=self.data, label=self.label, pad=0,
                                                                index=self.cur // self.batch_size,
                                                                provide_data=self.provide_data,
                                                                provide_label=self.provide_label)
        raise StopIteration

    def _frame_inputs(self, entry, f, key_f):
        clip = entry['clip']
        data = self._ahead.pop((self.cur_roidb_index, f), None)      # an image upcoming_key_frames already produced: the SAME tensor
        if data is None:
            data = clip.frame(f, self.device)
        d = {'data': data, 'im_info': torch.from_numpy(clip.im_info()).to(self.device)}
        if self.estimate_mv is not None and self._is_non_key(entry, f, key_f):
            d['motion_vector'], d['res_diff'] = self._estimated(entry, f, key_f)
        else:
            if self.estimate_mv is not None:
                self._estimate_segment(entry, f)
            d['motion_vector'], d['res_diff'] = clip.motion_vector(f, key_f, self.device), clip.res_diff(f, self.device)
        return d

    @staticmethod
    def _is_non_key(entry, f, key_f):
        """get_batch's rule: frame key_f is a key frame and so is the video's last"""
        return f != key_f and f + 1 != entry['frame_seg_len']

    def _segment_estimator(self, width, height):
        """the estimator of a frame size, built once: a segment holds at most KEY_FRAME_INTERVAL - 1 non-key frames of one clip"""
        from lsfa_amd import hip
        return hip.SegmentMotionEstimator(width, height, frames=max(self.cfg.TEST.KEY_FRAME_INTERVAL - 1, 1), clips=1, device=self.device,
                                          **self.estimate_mv)

    def _compute_segment(self, index, entry, key_f):
        """One SegmentMotionEstimator.segment call on the current stream for key frame key_f of video `index` and the non-key frames behind
        it - key_f + 1 .. key_f + n with n = KEY_FRAME_INTERVAL - 1, fewer in front of the video's last frame (a key frame) -> a Segment,
        or None where no frame follows the key frame.  The result is copied out of the estimator's buffers: a pipeline that groups key
        frames holds a segment's inputs while the next segment is estimated.  With `cut` the segment ends in front of its first cut
        frame (one readback) and the pairs from there on are dropped."""
        n = min(key_f + self.cfg.TEST.KEY_FRAME_INTERVAL - 1, entry['frame_seg_len'] - 2) - key_f
        if n < 1:
            return None
        clip = entry['clip']
        key = (clip.width, clip.height)
        if key not in self._estimators:
            self._estimators[key] = self._segment_estimator(clip.width, clip.height)
        stack = torch.stack([clip.frame_u8(g) for g in range(key_f, key_f + n + 1)]).unsqueeze(0).to(self.device)
        mv, res = self._estimators[key].segment(stack, float(clip.im_info()[0, 2]), self.cfg.network.PIXEL_MEANS, self.cfg.network.PIXEL_SCALE)
        cut_f = None
        if self.cut:
            first = self._estimators[key].first_cuts()[0]
            if first is not None:        # frame key_f + first starts a new scene: it becomes a key frame
                cut_f, n = key_f + first, first - 1
        return Segment((index, key_f), n, mv[:n].clone(), res[:n].clone(), cut_f)

    def _estimate_segment(self, entry, key_f):
        """Key frame key_f is being handed out: the segment behind it becomes the one under way - estimated now, or taken from what
        upcoming_key_frames estimated ahead (`cut` only)."""
        tag = (self.cur_roidb_index, key_f)
        if self._segment is not None and self._segment.tag == tag:
            return                       # get_batch runs twice for the very first frame (the constructor's shape probe)
        self._segment = None
        for old in [t for t in self._segments if t < tag]:       # the iteration has passed them
            del self._segments[old]
        self._segment = self._segments.pop(tag) if tag in self._segments else self._compute_segment(self.cur_roidb_index, entry, key_f)

    def _segment_ahead(self, entry, key_f):
        """`cut`: the segment behind a coming key frame of the current video, estimated once and kept until the iteration reaches it"""
        tag = (self.cur_roidb_index, key_f)
        if self._segment is not None and self._segment.tag == tag:
            return self._segment
        if tag not in self._segments:
            self._segments[tag] = self._compute_segment(self.cur_roidb_index, entry, key_f)
        return self._segments[tag]

    def _cut_at(self, key_f):
        """the cut frame that ends the segment under way behind key frame key_f of the current video, or None"""
        seg = self._segment
        return seg.cut_f if self.cut and seg is not None and seg.tag == (self.cur_roidb_index, key_f) else None

    def _estimated(self, entry, f, key_f):
        seg = self._segment
        if seg is None or seg.tag != (self.cur_roidb_index, key_f) or not 1 <= f - key_f <= seg.n:
            raise RuntimeError("TestLoader: frame %d of video %d is not part of the segment estimated behind key frame %s" %
                               (f, self.cur_roidb_index, None if seg is None else seg.tag))
        return seg.mv[f - key_f - 1], seg.res[f - key_f - 1]

    def upcoming_key_frames(self, n):
        """Call right after a KEY frame was returned: the images of the next `n` key frames of the same video (fewer near its end), for a
        caller that computes the image-only part of several key frames at once (FramePipeline.key_frame(upcoming=...)).  Key frames are
        every KEY_FRAME_INTERVAL-th frame and, by the rule of get_batch above (:106-109), the video's last frame; with `cut` also the cut
        frames (next_key_frame), for which the segments behind the coming key frames are estimated here and kept.  The tensors are kept and
        handed out again when the iteration reaches those frames."""
        if self.cur_frameid == 0:             # the frame just returned was its video's last: nothing ahead in this video
            return []
        entry = self.roidb[self.cur_roidb_index]
        K, L = self.cfg.TEST.KEY_FRAME_INTERVAL, entry['frame_seg_len']
        out, prev = [], self.cur_frameid - 1       # the (key) frame just returned; key_frameid may already point past it (interval 1)
        while len(out) < n and prev < L - 1:
            seg = self._segment_ahead(entry, prev) if self.cut else None
            # the next multiple of the interval, or the video's last frame if that comes first - or, with `cut`, the segment's cut frame
            f = next_key_frame(prev, L, K, () if seg is None or seg.cut_f is None else (seg.cut_f,))
            key = (self.cur_roidb_index, f)
            if key not in self._ahead:
                self._ahead[key] = entry['clip'].frame(f, self.device)
            out.append(self._ahead[key])
            prev = f
        return out

    def get_batch(self):
        cur_roidb = self.roidb[self.cur_roidb_index]
        self.cur_seg_len = cur_roidb['frame_seg_len']
        d = self._frame_inputs(cur_roidb, self.cur_frameid, self.key_frameid)
        if self.key_frameid == self.cur_frameid:       # key frame
            self.data_key_old = self.data_key if self.data_key is not None else d['data']
            self.data_key = d['data']
            if self.key_frameid == 0:
                self.data_key_old = d['data']
                self.key_frame_flag = 0
            else:
                self.key_frame_flag = 1
        elif self.cur_frameid + 1 == self.cur_seg_len:  # the last frame of a video is a key frame
            self.data_key_old = self.data_key if self.data_key is not None else d['data']
            self.data_key = d['data']
            self.key_frame_flag = 1
        else:
            self.key_frame_flag = 2
        dim = self.cfg.network.DFF_FEAT_DIM
        placeholder = torch.zeros((1, dim, 1, 1), device=self.device)
        extend = {'data': d['data'], 'im_info': d['im_info'], 'data_key': self.data_key, 'data_key_old': self.data_key_old,
                  'motion_vector': d['motion_vector'], 'res_diff': d['res_diff'], 'feat_key_old': placeholder,
                  'feat_key': placeholder}
        self.data = [[extend[name] for name in self.data_name]]
        self.im_info = [d['im_info'].cpu().numpy()]
