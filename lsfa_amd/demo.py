#!/usr/bin/env python
"""Counterpart of dff_rfcn/demo.py (:63-158): run the key / non-key frame loop over one clip, print
the running mean time per frame like the reference's tic/toc loop, and report the detections that
score above 0.7 after per-class NMS.

    python -m lsfa_amd.demo                         # synthetic 1000x600 clip, random-init weights
    python -m lsfa_amd.demo --frames DIR [--mv DIR] [--prefix P --epoch E] [--out dets.json]
    python -m lsfa_amd.demo --frames DIR --estimate-mv [--search 16 --mv-lambda 4] [--mv-levels L --mv-refine r] [--dump-mv DIR]
    python -m lsfa_amd.demo --frames DIR --estimate-mv --scene-cut [PERCENT] [--cut-bias B]     # a key frame wherever a new scene starts
    python -m lsfa_amd.demo --frames DIR --estimate-mv --stale-key [PERCENT] [--stale-bias B]   # ... and wherever the key frame stops predicting (fades, pans)

    python -m lsfa_amd.demo --yuv clip.nv12 --size 1280x720 [--yuv-format nv12|i420] [--yuv-matrix bt601|bt709|jpeg] [--estimate-mv ...]
    python -m lsfa_amd.demo --yuv clip.p010 --size 1920x1080 --yuv-format p010|yuv420p10le [--yuv-matrix ...] [--estimate-mv ...]   # 10-bit
    python -m lsfa_amd.demo --yuv cam.yuyv --size 1280x720 --yuv-format yuyv422 [--estimate-mv ...]      # a capture card's packed 4:2:2
    python -m lsfa_amd.demo --yuv clip.yuv --size 1920x1080 --yuv-format yuv422p10le|yuv444p|nv21|... [--yuv-matrix ...] [--estimate-mv ...]

--frames: a directory of *.JPEG / *.jpg / *.png frames in display order (decoded with PIL; the
reference uses cv2.imread, :75).  --mv: one `<frame stem>.npz` per non-key frame holding `mv`
(H, W, 2) and `res` (H, W, 3) in source-image pixels, the arrays lib/utils/image.py:get_image reads
from the compressed stream; without it non-key frames propagate the key feature unchanged (zero
motion, zero residual), which is what the reference's own demo amounts to (it has no MV input).
--estimate-mv: no side data needed - the decoded uint8 frames of the current key-frame interval stay on the device and a
hip.MotionEstimator (16 x 16 block matching against the previous frame, accumulated back to the key frame like the reference's
coviar loader accumulates a decoder's vectors) supplies `motion_vector` / `res_diff`.  The vectors are this project's own
full search, not an MPEG-4 encoder's (DESIGN.md "Motion estimation").  --dump-mv DIR (with --estimate-mv) writes what was
estimated as the `<frame stem>.npz` files --mv reads: `mv` (H, W, 2) int32 is the accumulated field as get_image holds it AFTER
`motion_vector = - motion_vector` (lib/utils/image.py:54), i.e. MINUS lsfa_mv_field's output - the --mv path does not negate -
and `res` (H, W, 3) int32 is lsfa_mv_residual's output as it stands.  Running --mv on such a dump reproduces --estimate-mv.
--yuv FILE --size WxH: a raw YUV 4:2:0 file as `-f rawvideo -pix_fmt nv12` (or yuv420p: --yuv-format i420) writes it - frames back to back, no
header - in place of --frames.  The file is memory-mapped, each frame's 1.5 bytes per pixel are uploaded once and everything behind the
upload runs on the device: `data` is hip.image_resize_transform_yuv420 of the planes, and with --estimate-mv the estimator's *_yuv
methods convert and search them (DESIGN.md "YUV intake"; the conversion is this project's own integer specification).
--yuv-format p010 | yuv420p10le: a 10-bit file of 16-bit little-endian words as `-pix_fmt p010le` (Y plane, then interleaved U, V; the
sample in the high ten bits) or `-pix_fmt yuv420p10le` (Y, U, V planes; the sample in the low ten bits) writes it: 3 bytes per pixel
uploaded, the same path through lsfa_amd/yuv10.py (image_resize_transform_yuv420p10, MotionEstimator10), no host-side conversion.
--yuv-format with any other name of lsfa_amd.yuvfmt.FORMATS (nv21; yuv422p, nv16, nv61, yuyv422 / yuy2, uyvy422; yuv444p, nv24, nv42;
yuv422p10le, p210, yuv444p10le, p410): the file as `-f rawvideo -pix_fmt X` writes it (yuvfmt.frame_bytes: planes back to back, no pitch),
through lsfa_amd/yuvfmt.py (image_resize_transform_yuv, MotionEstimatorYuv).
--draw DIR: the counterpart of draw_boxes + cv2.imwrite (:150-157) - every frame's detections are drawn on the device into its uint8
BGR frame (a --yuv frame converted by the shipped *_to_bgr_u8) by lsfa_amd/overlay.py and the frame is written as DIR/<frame stem>.png
with PIL.  --draw-yuv FILE (--yuv-format nv12 | i420 only): the detections are drawn into a COPY of the frame's planes - the motion
estimator still needs the pristine frames - and the annotated raw stream is written in the input's layout, e.g. for an encoder.
--draw-raw FILE (every --yuv-format of lsfa_amd.yuvfmt.FORMATS: p010, yuyv422, nv21, yuv444p10le, ...): the same for any input layout -
each frame's annotated planes back to back, yuvfmt.frame_bytes per frame, drawn by Overlay.draw_yuv; a ten-bit surface takes the 8-bit
colour in its ten bits, so the stream reads back through the intake as the same BGR.
--classes FILE: one class name per line (the foreground classes, or all with the background first); without it a label is the class
id.  --draw-thickness / --draw-scale: the outline's thickness and the label's scale (0: no label).  The drawing is this project's own
integer specification (DESIGN.md "Detection overlay"), not cv2's, and runs outside the timed region like the reference's.
--track [--track-iou X --track-max-age N --track-min-hits N --track-slots T]: every detection gets a track id on the device, frame by
frame (lsfa_amd/tracks.py; DESIGN.md "Tracks" - the reference has no tracker).  Under --estimate-mv the estimator's block rows of the frame
predict where last frame's boxes went; a key frame that restarts the chain has none, and without --estimate-mv there is no prediction.
With --draw / --draw-yuv / --draw-raw a track keeps one colour and one number (labels read name-id); otherwise the id is the `track` of every
detection of --out (-1: below --score, 0: not reported yet or dropped).
"""
import argparse
import glob
import json
import math
import os
import time

import numpy as np
import torch

from lsfa_amd import overlay, tracks, yuvfmt
from lsfa_amd.config.config import config, lsfa_test_config, update_config, update_network_config
from lsfa_amd.core.graphs import FrameGraphs
from lsfa_amd.symbols import params as P
from lsfa_amd.symbols.resnet_v1_101_flownet_rfcn import resnet_v1_101_flownet_rfcn
from lsfa_amd.utils import motion_options
from lsfa_amd.utils.image import resize, transform, transform_mv_res
from lsfa_amd.utils.load_model import load_param
from lsfa_amd.utils.synthetic import SyntheticClip


YUV_FORMATS = {'nv12': 1, 'i420': 1, 'p010': 2, 'yuv420p10le': 2}          # format -> bytes per sample


def yuv_file_frames(path, width, height, sample_bytes=1, fmt=None):
    """-> the bytes of one width x height 4:2:0 frame of `sample_bytes` bytes per sample - or of format `fmt` (yuvfmt.frame_bytes) - the
    file's size, the frames it holds (None: not a whole number of them, or none)"""
    frame_bytes = (width * height + 2 * (-(-width // 2)) * (-(-height // 2))) * sample_bytes if fmt is None else yuvfmt.frame_bytes(fmt, width, height)
    size = os.path.getsize(path)
    return frame_bytes, size, (None if size == 0 or size % frame_bytes else size // frame_bytes)


class _EstimatedClip(object):
    """What FrameDirClip and YuvFileClip share: mv_res, and behind it the chain of one hip.MotionEstimator over the frames of the current
    key-frame interval.  A clip says what is its own: _new_estimator (the frame size, its extra keywords), _feed (frame i to key_frame* /
    next_frame*), _bgr_pair (frames i and key_i as uint8 BGR, for the dump and network_inputs) and _stems (the names of the .npz files).
    self._kept: frame -> what the clip keeps of it on the device, trimmed in place to the interval under way."""

    def __init__(self, estimate, device, dump_mv):
        if dump_mv is not None and estimate is None:
            raise ValueError('dump_mv writes the ESTIMATED motion vectors: it needs estimate')
        self.estimate, self.device, self.dump_mv = estimate, device, dump_mv
        self._me, self._me_key, self._me_last, self._kept = None, None, None, {}
        if dump_mv is not None:
            os.makedirs(dump_mv, exist_ok=True)

    def _estimated(self, i, key_i):
        from lsfa_amd import hip
        if self._me is None:
            self._me = self._new_estimator(hip, key_i)
        me = self._me
        if self._me_key != key_i or i < self._me_last:        # a new interval (or a step back): start from the key frame again
            for f in [f for f in self._kept if not key_i <= f <= i]:
                del self._kept[f]
            self._feed(me, key_i, True)
            self._me_key, self._me_last = key_i, key_i
        for f in range(self._me_last + 1, i + 1):             # the P-frame chain: every frame against the one before it
            self._feed(me, f, False)
        self._me_last = i
        if motion_options.ends_early(self.estimate) and me.is_cut():
            return None                                       # frame i starts a new scene, or its key frame is stale: the caller makes it a key frame
        cfg, (cur, key) = self.cfg, self._bgr_pair(me, i, key_i)
        if self.dump_mv is not None:
            np.savez(os.path.join(self.dump_mv, self._stems[i] + '.npz'), mv=(-me.acc.motion_vectors()).cpu().numpy(),
                     res=me.acc.residual(cur, key).cpu().numpy())
        mv, res = me.network_inputs(cur, key, self.im_scale, cfg.network.PIXEL_MEANS, cfg.network.PIXEL_SCALE)
        return mv.clone(), res.clone()                        # the estimator reuses its output buffers

    def mv_res(self, i, key_i):
        if self.estimate is not None:
            return self._estimated(i, key_i)
        fh, fw = -(-self.height // 16), -(-self.width // 16)
        return torch.zeros(1, 2, fh, fw), torch.zeros(1, 3, fh, fw)        # zero motion, zero residual

    def last_rows(self):
        """--track: the block rows of the pair (frame, frame before it) the last mv_res estimated, on the device as the estimator holds
        them; None without an estimator"""
        return None if self._me is None else self._me.rows


class FrameDirClip(_EstimatedClip):
    """Frames of one clip from a directory, preprocessed like the reference's demo (:73-82).  estimate: None, or a dict of
    hip.MotionEstimator's parameters (search, lam, max_sad) - motion vectors and residuals are then estimated from the frames on
    `device`; with cut=dict(...) or stale=dict(...) among them mv_res returns None for a frame the estimator finds to start a new scene or to be
    no longer predicted by its key frame; dump_mv: a directory that receives them as the .npz files `mv_dir` is read from."""

    def __init__(self, frame_dir, mv_dir, cfg, estimate=None, device='cuda:0', dump_mv=None):
        from PIL import Image
        names = sorted(sum((glob.glob(os.path.join(frame_dir, e)) for e in ('*.JPEG', '*.jpg', '*.jpeg', '*.png')), []))
        if not names:
            raise FileNotFoundError('no frames under %s' % frame_dir)
        if estimate is not None and mv_dir is not None:
            raise ValueError('either read motion vectors (mv_dir) or estimate them, not both')
        self.names, self.mv_dir, self.cfg = names, mv_dir, cfg
        self._stems = [os.path.splitext(os.path.basename(n))[0] for n in names]
        self._open = Image.open
        self.num_frames = len(names)
        f0, self.im_scale = self._load(0)
        self.height, self.width = f0.shape[2], f0.shape[3]
        _EstimatedClip.__init__(self, estimate, device, dump_mv)
        self._u8 = self._kept           # the decoded frames as (H, W, 3) uint8 BGR

    def _decode(self, i):
        return np.asarray(self._open(self.names[i]).convert('RGB'))          # (H, W, 3) uint8 RGB

    def _load(self, i):
        cfg = self.cfg
        rgb = self._decode(i).astype(np.float32)
        bgr = torch.from_numpy(np.ascontiguousarray(rgb[:, :, ::-1]))
        im, im_scale = resize(bgr, cfg.SCALES[0][0], cfg.SCALES[0][1], stride=cfg.network.IMAGE_STRIDE)
        return transform(im, cfg.network.PIXEL_MEANS, cfg.network.PIXEL_SCALE), im_scale

    def frame(self, i):
        return self._load(i)[0]

    def _frame_u8(self, i):
        """the decoded frame as (H, W, 3) uint8 BGR on the device; the frames of the current interval are kept"""
        if i not in self._u8:
            self._u8[i] = torch.from_numpy(np.ascontiguousarray(self._decode(i)[:, :, ::-1])).to(self.device)
        return self._u8[i]

    def bgr_u8(self, i):
        """a (H, W, 3) uint8 BGR frame on the device that is the caller's to draw into"""
        if i in self._u8:
            return self._u8[i].clone()
        return torch.from_numpy(np.ascontiguousarray(self._decode(i)[:, :, ::-1])).to(self.device)

    def _new_estimator(self, hip, key_i):
        k = self._frame_u8(key_i)
        return hip.MotionEstimator(int(k.shape[1]), int(k.shape[0]), self.device, **self.estimate)

    def _feed(self, me, i, key):
        (me.key_frame if key else me.next_frame)(self._frame_u8(i))

    def _bgr_pair(self, me, i, key_i):
        return self._frame_u8(i), self._frame_u8(key_i)

    def mv_res(self, i, key_i):
        if self.mv_dir is None:
            return _EstimatedClip.mv_res(self, i, key_i)
        z, cfg = np.load(os.path.join(self.mv_dir, self._stems[i] + '.npz')), self.cfg
        return transform_mv_res(z['mv'], z['res'], self.im_scale, cfg.network.PIXEL_MEANS, cfg.network.PIXEL_SCALE)


class YuvFileClip(_EstimatedClip):
    """Frames of one clip from a raw YUV 4:2:0 file (fmt 'nv12': Y plane, then interleaved U, V; 'i420': Y, U, V planes; 'p010' and
    'yuv420p10le': the same two layouts in 16-bit little-endian words holding 10-bit samples, in the high and the low ten bits), frames back to
    back without a header.  Same interface as FrameDirClip: frame(i) is hip.image_resize_transform_yuv420 of the frame's planes on `device`,
    mv_res(i, key_i) the estimator's *_yuv chain when `estimate` (a dict of hip.MotionEstimator's parameters) is given, zero motion and
    zero residual otherwise.  The file is memory-mapped; a frame's bytes are uploaded once and the frames of the current interval are kept.
    A 10-bit format goes through lsfa_amd/yuv10.py instead: the uploaded buffer is viewed as int16 words.  Any other name of
    yuvfmt.FORMATS (4:2:2, 4:4:4, V before U, packed) goes through lsfa_amd/yuvfmt.py: planes(i) lays the file's planes out as its functions
    take them, a packed frame as the one plane y."""

    def __init__(self, path, width, height, cfg, fmt='nv12', matrix='bt601', estimate=None, device='cuda:0', dump_mv=None):
        if fmt not in yuvfmt.FORMATS:
            raise ValueError('fmt %r is not one of %s' % (fmt, ', '.join(sorted(yuvfmt.FORMATS))))
        _, _, layout, sample = yuvfmt.fields(fmt)
        self.other = fmt not in YUV_FORMATS          # not one of the shipped 4:2:0 four: through lsfa_amd/yuvfmt.py
        self.packed = layout >= yuvfmt.YUYV
        self.sample_bytes, self.semi_planar = 1 if sample == yuvfmt.U8 else 2, layout in (yuvfmt.UV, yuvfmt.VU)
        self.src_w, self.src_h, self.fmt, self.matrix, self.cfg = int(width), int(height), fmt, matrix, cfg
        if self.src_w <= 0 or self.src_h <= 0:
            raise ValueError('bad frame size %d x %d' % (self.src_w, self.src_h))
        self.ch, self.cw = yuvfmt.chroma_shape(fmt, self.src_h, self.src_w)
        self.frame_bytes, size, self.num_frames = yuv_file_frames(path, self.src_w, self.src_h, fmt=fmt)
        if self.num_frames is None:
            raise ValueError('%s holds %d bytes: not a whole number of %d x %d %s frames of %d bytes' % (path, size, self.src_w, self.src_h, fmt,
                                                                                                     self.frame_bytes))
        self._map = np.memmap(path, dtype=np.uint8, mode='r')
        self._stems = ['%06d' % i for i in range(self.num_frames)]
        self.names = ['%s/%s' % (os.path.basename(path), stem) for stem in self._stems]
        # `resize`'s scale (lib/utils/image.py:266-280) from the frame size alone
        target, max_size = cfg.SCALES[0][0], cfg.SCALES[0][1]
        lo, hi = min(self.src_h, self.src_w), max(self.src_h, self.src_w)
        self.im_scale = float(target) / float(lo)
        if np.round(self.im_scale * hi) > max_size:
            self.im_scale = float(max_size) / float(hi)
        st = cfg.network.IMAGE_STRIDE
        h1, w1 = int(np.rint(self.src_h * self.im_scale)), int(np.rint(self.src_w * self.im_scale))
        self.height, self.width = (-(-h1 // st) * st, -(-w1 // st) * st) if st else (h1, w1)
        _EstimatedClip.__init__(self, estimate, device, dump_mv)
        self._dev = self._kept          # the frames' bytes as they lie in the file

    def planes(self, i):
        """frame i as the keyword arguments of the hip.*yuv420* (yuv10.*yuv420p10*) functions: views of ONE device tensor holding the
        frame's bytes (its 16-bit words)"""
        if i not in self._dev:
            if self.estimate is None:
                self._dev.clear()                             # nothing looks back at earlier frames
            raw = np.array(self._map[i * self.frame_bytes:(i + 1) * self.frame_bytes])         # one read of the mapped pages
            self._dev[i] = torch.from_numpy(raw).to(self.device)
        return self._views(self._dev[i])

    def _views(self, buf):
        """the planes of one frame's bytes `buf`"""
        n = self.src_w * self.src_h
        if self.sample_bytes == 2:
            buf = buf.view(torch.int16)
        if self.packed:
            return dict(y=buf.view(self.src_h, 4 * self.cw))
        y = buf[:n].view(self.src_h, self.src_w)
        if self.semi_planar:
            return dict(y=y, uv=buf[n:].view(self.ch, 2 * self.cw))
        c = self.ch * self.cw
        return dict(y=y, u=buf[n:n + c].view(self.ch, self.cw), v=buf[n + c:].view(self.ch, self.cw))

    def planes_copy(self, i):
        """-> (a copy of frame i's bytes on the device, its planes as planes(i) gives them): what --draw-yuv draws into and writes"""
        self.planes(i)
        buf = self._dev[i].clone()
        return buf, self._views(buf)

    def bgr_u8(self, i):
        """frame i converted by the shipped *_to_bgr_u8 of its format: a new (H, W, 3) uint8 BGR frame on the device"""
        if self.other:
            return yuvfmt.yuv_to_bgr_u8(self.fmt, matrix=self.matrix, width=self.src_w, **self.planes(i))
        if self.sample_bytes == 2:
            from lsfa_amd import yuv10
            return yuv10.yuv420p10_to_bgr_u8(matrix=self.matrix, msb_aligned=self.fmt == 'p010', **self.planes(i))
        from lsfa_amd import hip
        return hip.yuv420_to_bgr_u8(matrix=self.matrix, **self.planes(i))

    def frame(self, i):
        cfg = self.cfg
        kw = dict(im_scale=self.im_scale, matrix=self.matrix, pixel_means=cfg.network.PIXEL_MEANS, pixel_scale=cfg.network.PIXEL_SCALE,
                  stride=cfg.network.IMAGE_STRIDE)
        if self.other:
            return yuvfmt.image_resize_transform_yuv(self.fmt, width=self.src_w, **kw, **self.planes(i))
        if self.sample_bytes == 2:
            from lsfa_amd import yuv10
            return yuv10.image_resize_transform_yuv420p10(msb_aligned=self.fmt == 'p010', **kw, **self.planes(i))
        from lsfa_amd import hip
        return hip.image_resize_transform_yuv420(**kw, **self.planes(i))

    def _new_estimator(self, hip, key_i):
        if self.other:
            return yuvfmt.MotionEstimatorYuv(self.src_w, self.src_h, self.device, fmt=self.fmt, matrix=self.matrix, **self.estimate)
        if self.sample_bytes == 2:
            from lsfa_amd import yuv10
            return yuv10.MotionEstimator10(self.src_w, self.src_h, self.device, msb_aligned=self.fmt == 'p010', matrix=self.matrix, **self.estimate)
        return hip.MotionEstimator(self.src_w, self.src_h, self.device, matrix=self.matrix, **self.estimate)

    def _feed(self, me, i, key):
        (me.key_frame_yuv if key else me.next_frame_yuv)(**self.planes(i))

    def _bgr_pair(self, me, i, key_i):
        return me.bgr_cur, me.bgr_key            # the estimator converted them

    def _estimated(self, i, key_i):
        if i <= key_i:
            raise ValueError('frame %d has no motion vectors against key frame %d' % (i, key_i))
        return _EstimatedClip._estimated(self, i, key_i)


class _Synthetic(object):
    def __init__(self, n, h, w):
        self.c = SyntheticClip(0, n, h, w)
        self.num_frames, self.height, self.width, self.im_scale = n, h, w, 1.0
        self.names = ['synthetic/%06d' % i for i in range(n)]

    def frame(self, i):
        return self.c.frame(i)

    def bgr_u8(self, i):
        return self.c.frame_u8(i).to('cuda:0')

    def mv_res(self, i, key_i):
        return self.c.motion_vector(i, key_i), self.c.res_diff(i)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='LSFA demo: key / non-key frame loop over one clip')
    ap.add_argument('--cfg', default=None)
    ap.add_argument('--frames', default=None, help='directory of frames (default: a synthetic clip)')
    ap.add_argument('--mv', default=None, help='directory of per-frame .npz with mv / res arrays')
    ap.add_argument('--yuv', default=None, help='a raw YUV file (4:2:0 unless --yuv-format says otherwise; frames back to back, no header) in place of --frames; needs --size')
    ap.add_argument('--size', default=None, help='--yuv: the frame size as WxH, e.g. 1280x720')
    ap.add_argument('--yuv-format', default='nv12', choices=('nv12', 'i420', 'p010', 'yuv420p10le') + tuple(sorted(set(yuvfmt.FORMATS) - set(YUV_FORMATS))),
                    help='--yuv: semi-planar (interleaved U, V) or planar chroma of bytes; p010 / yuv420p10le: the same two of 10-bit samples in '
                         '16-bit words, in the high / the low ten bits; any other name of lsfa_amd.yuvfmt.FORMATS: 4:2:2, 4:4:4, V before U, '
                         'packed YUYV / UYVY, as ffmpeg -f rawvideo -pix_fmt NAME writes it')
    ap.add_argument('--yuv-matrix', default='bt601', choices=('bt601', 'bt709', 'jpeg'), help='--yuv: the colour matrix of the stream')
    motion_options.add_arguments(ap, 'estimate block motion vectors from the frames on the GPU (needs --frames or --yuv)')
    ap.add_argument('--dump-mv', default=None, help='--estimate-mv: write the estimated mv / res as the .npz files --mv reads')
    ap.add_argument('--num', type=int, default=30, help='frames of the synthetic clip')
    ap.add_argument('--interval', type=int, default=10, help='key frame interval (demo.py:68)')
    ap.add_argument('--prefix', default=None)
    ap.add_argument('--epoch', type=int, default=0)
    ap.add_argument('--score', type=float, default=0.7, help='report threshold (demo.py:147)')
    ap.add_argument('--out', default=None, help='write the detections as JSON here')
    ap.add_argument('--no-graph', action='store_true')
    ap.add_argument('--draw', default=None, help='a directory that receives every frame with its detections drawn in, as <frame stem>.png')
    ap.add_argument('--draw-yuv', default=None, help='--yuv with --yuv-format nv12 | i420: write the annotated raw stream, in the input\'s layout, here')
    ap.add_argument('--draw-raw', default=None, help='--yuv with any --yuv-format: write the annotated raw stream, in the input\'s layout, here')
    ap.add_argument('--classes', default=None, help='--draw / --draw-yuv / --draw-raw: a file of class names, one per line; the default labels are class ids')
    ap.add_argument('--draw-thickness', type=int, default=None, help='--draw / --draw-yuv / --draw-raw: the outline\'s thickness in pixels, 1..8 (default 3, the reference\'s)')
    ap.add_argument('--draw-scale', type=int, default=None, help='--draw / --draw-yuv / --draw-raw: the label\'s scale, 1..4, or 0 for no label (default 2)')
    ap.add_argument('--track', action='store_true', help='give every detection a track id on the device (lsfa_amd.tracks); with --estimate-mv the '
                                                         'estimator\'s block rows predict where last frame\'s boxes went')
    ap.add_argument('--track-iou', type=float, default=None, help='--track: the least IoU of a match (default 0.3; not a tuned value)')
    ap.add_argument('--track-max-age', type=int, default=None, help='--track: a track unmatched for more frames than this is dropped (default 10)')
    ap.add_argument('--track-min-hits', type=int, default=None, help='--track: a track is reported from its N-th match on (default 1)')
    ap.add_argument('--track-slots', type=int, default=None, help='--track: the size of the track table, 1..%d (default 256)' % tracks.MAX_TRACKS)
    args = ap.parse_args(argv)
    if args.draw_yuv and not (args.yuv and args.yuv_format in ('nv12', 'i420')):
        ap.error('--draw-yuv writes the input\'s own layout and needs --yuv with --yuv-format nv12 or i420; draw any other input with --draw')
    if args.draw_yuv and os.path.abspath(args.draw_yuv) == os.path.abspath(args.yuv):
        ap.error('--draw-yuv would overwrite its input %s' % args.yuv)
    if args.draw_raw and not args.yuv:
        ap.error('--draw-raw writes the input\'s own layout and needs --yuv')
    if args.draw_raw and os.path.abspath(args.draw_raw) == os.path.abspath(args.yuv):
        ap.error('--draw-raw would overwrite its input %s' % args.yuv)
    if args.draw_raw and args.draw_yuv and os.path.abspath(args.draw_raw) == os.path.abspath(args.draw_yuv):
        ap.error('--draw-raw and --draw-yuv name one file: %s' % args.draw_raw)
    drawing = bool(args.draw or args.draw_yuv or args.draw_raw)
    for name, v in (('--classes', args.classes), ('--draw-thickness', args.draw_thickness), ('--draw-scale', args.draw_scale)):
        if v is not None and not drawing:
            ap.error('%s belongs to --draw / --draw-yuv / --draw-raw' % name)
    if args.draw_thickness is not None and not 1 <= args.draw_thickness <= 8:
        ap.error('--draw-thickness %d is outside 1..8' % args.draw_thickness)
    if args.draw_scale is not None and not 0 <= args.draw_scale <= 4:
        ap.error('--draw-scale %d is outside 0..4' % args.draw_scale)
    for name, v in (('--track-iou', args.track_iou), ('--track-max-age', args.track_max_age), ('--track-min-hits', args.track_min_hits),
                    ('--track-slots', args.track_slots)):
        if v is not None and not args.track:
            ap.error('%s belongs to --track' % name)
    if args.track_iou is not None and not math.isfinite(args.track_iou):
        ap.error('--track-iou %r is not a finite number' % args.track_iou)
    if args.track_max_age is not None and args.track_max_age < 0:
        ap.error('--track-max-age %d is below 0' % args.track_max_age)
    if args.track_min_hits is not None and args.track_min_hits < 1:
        ap.error('--track-min-hits %d is below 1' % args.track_min_hits)
    if args.track_slots is not None and not 1 <= args.track_slots <= tracks.MAX_TRACKS:
        ap.error('--track-slots %d is outside 1..%d' % (args.track_slots, tracks.MAX_TRACKS))
    args.track_iou = 0.3 if args.track_iou is None else args.track_iou
    args.track_max_age = 10 if args.track_max_age is None else args.track_max_age
    args.track_min_hits = 1 if args.track_min_hits is None else args.track_min_hits
    args.track_slots = 256 if args.track_slots is None else args.track_slots
    if args.classes is not None and not os.path.isfile(args.classes):
        ap.error('--classes: no such file: %s' % args.classes)
    args.draw_thickness = 3 if args.draw_thickness is None else args.draw_thickness
    args.draw_scale = 2 if args.draw_scale is None else args.draw_scale
    if args.yuv and args.frames:
        ap.error('--yuv excludes --frames')
    if args.yuv and args.mv:
        ap.error('--mv names the frames of --frames; with --yuv use --estimate-mv')
    args.yuv_size = None
    if args.yuv:
        import re
        m = re.match(r'^(\d+)x(\d+)$', args.size or '')
        if not m or int(m.group(1)) <= 0 or int(m.group(2)) <= 0:
            ap.error('--yuv needs --size WxH (got %r)' % (args.size,))
        args.yuv_size = (int(m.group(1)), int(m.group(2)))
        w, h = args.yuv_size
        if not os.path.isfile(args.yuv):
            ap.error('--yuv: no such file: %s' % args.yuv)
        frame_bytes, size, frames = yuv_file_frames(args.yuv, w, h, fmt=args.yuv_format)
        if frames is None:
            ap.error('--yuv: %s holds %d bytes, not a whole number of %dx%d frames of %d bytes' % (args.yuv, size, w, h, frame_bytes))
    elif args.size:
        ap.error('--size belongs to --yuv')
    if args.estimate_mv and (not (args.frames or args.yuv) or args.mv):
        ap.error('--estimate-mv needs --frames or --yuv and excludes --mv')
    if args.dump_mv and not args.estimate_mv:
        ap.error('--dump-mv needs --estimate-mv')
    args.estimate = motion_options.estimate_of(ap, args)
    return args


def class_names(path, ncls):
    """the lines of a --classes file as Overlay's `names`: ncls - 1 foreground names, or ncls with the background's first"""
    with open(path) as f:
        lines = [ln.strip() for ln in f if ln.strip()]
    if len(lines) == ncls - 1:
        return ['background'] + lines
    if len(lines) != ncls:
        raise ValueError('%s names %d classes; the network has %d and the background' % (path, len(lines), ncls - 1))
    return lines


class _Drawer(object):
    """--draw / --draw-yuv / --draw-raw: one overlay.Overlay for the clip, made at the first frame from the detection buffers' shape"""

    def __init__(self, args, clip):
        self.args, self.clip, self.ov, self.yuv_out, self.raw_out = args, clip, None, None, None
        if args.draw:
            os.makedirs(args.draw, exist_ok=True)
        if args.draw_yuv:
            self.yuv_out = open(args.draw_yuv, 'wb')
        if args.draw_raw:
            self.raw_out = open(args.draw_raw, 'wb')

    def frame(self, idx, dets, counts, ids=None):
        """draws frame idx's detections (the device buffers fg.*_frame returned; ids: --track's, one colour and one number per object) and
        writes the frame"""
        args, clip = self.args, self.clip
        if self.ov is None:
            ncls, R = int(dets.shape[0]), int(dets.shape[1])
            names = class_names(args.classes, ncls) if args.classes else None
            self.ov = overlay.Overlay(ncls, R, max_boxes=min(overlay.MAX_BOXES, max(1, (ncls - 1) * R)), thickness=args.draw_thickness,
                                      label_scale=args.draw_scale, names=names, device=dets.device)
        if args.draw:
            from PIL import Image
            bgr = self.ov.draw_bgr(clip.bgr_u8(idx), dets, counts, args.score, ids=ids)
            stem = os.path.splitext(os.path.basename(clip.names[idx]))[0]
            Image.fromarray(np.ascontiguousarray(bgr.cpu().numpy()[:, :, ::-1])).save(os.path.join(args.draw, stem + '.png'))
        if self.yuv_out is not None:
            buf, planes = clip.planes_copy(idx)
            self.ov.draw_yuv420(planes.pop('y'), dets, counts, args.score, matrix=clip.matrix, ids=ids, **planes)
            self.yuv_out.write(buf.cpu().numpy().tobytes())
        if self.raw_out is not None:
            buf, planes = clip.planes_copy(idx)
            self.ov.draw_yuv(clip.fmt, planes.pop('y'), dets, counts, args.score, matrix=clip.matrix, ids=ids, width=clip.src_w, **planes)
            self.raw_out.write(buf.cpu().numpy().tobytes())

    def close(self):
        for f in (self.yuv_out, self.raw_out):
            if f is not None:
                f.close()


def main(argv=None):
    args = parse_args(argv)
    if args.cfg:
        cfg = update_config(args.cfg, config)
        update_network_config(cfg)
    else:
        cfg = lsfa_test_config()
    cfg.TEST.KEY_FRAME_INTERVAL = args.interval
    dev = 'cuda:0'
    if args.yuv:
        clip = YuvFileClip(args.yuv, args.yuv_size[0], args.yuv_size[1], cfg, args.yuv_format, args.yuv_matrix, args.estimate, dev, args.dump_mv)
    else:
        clip = FrameDirClip(args.frames, args.mv, cfg, args.estimate, dev, args.dump_mv) if args.frames else _Synthetic(args.num, 600, 1000)
    if args.prefix:
        arg_params, aux_params = load_param(args.prefix, args.epoch, process=True)
    else:
        arg_params, aux_params = P.init_params(cfg, seed=0)
    net = resnet_v1_101_flownet_rfcn(cfg)
    key = net.get_key_test_symbol(cfg).bind(arg_params, aux_params, dev)
    cur = net.get_cur_test_symbol(cfg).bind(arg_params, aux_params, dev)
    fg = FrameGraphs(key, cur, cfg, clip.height, clip.width, dev, thresh=args.score, use_graphs=not args.no_graph,
                     prefetch=False)
    fg.scale = float(clip.im_scale)
    fg.im_info[0, 2] = fg.scale
    classes = None       # class names live in the dataset (imdb.classes); ids are reported without one
    drawer = _Drawer(args, clip) if args.draw or args.draw_yuv or args.draw_raw else None
    tracker = None       # --track: made at the first frame from the detection buffers' shape

    results, total, count = [], 0.0, 0
    key_idx = 0          # the running key frame: every `interval` frames behind the last one - or, with --scene-cut / --stale-key, where a scene starts or the key frame is stale
    for idx in range(clip.num_frames):
        data = clip.frame(idx).to(dev)
        is_key = idx == 0 or idx - key_idx == args.interval
        mv_res = None if is_key else clip.mv_res(idx, key_idx)
        if mv_res is None:       # --scene-cut / --stale-key: the estimator's next_frame* found a cut or a stale key frame; the clip starts its chain over at this frame (key_frame*)
            is_key, key_idx = True, idx
        mv, res = (None, None) if is_key else [t.to(dev) for t in mv_res]
        torch.cuda.synchronize()
        t0 = time.time()
        if idx == 0:
            dets, counts, _ = fg.first_frame(data)
            torch.cuda.synchronize()
            dets_h, counts_h = dets.cpu().numpy(), counts.cpu().numpy()
            fg.capture()                                   # the reference's "warm up" (:104-116)
            print('warmup done')
        else:
            dets, counts, _ = fg.key_frame(data) if is_key else fg.cur_frame(data, mv, res)
            dets_h, counts_h = dets.cpu().numpy(), counts.cpu().numpy()    # .cpu() is the per-frame sync
            total += time.time() - t0
            count += 1
            print('testing {} {:.4f}s'.format(clip.names[idx], total / count))
        ids, ids_h = None, None
        if args.track:               # after the frame's time is taken, like the drawing; one launch, on the device buffers
            if tracker is None:
                tracker = tracks.Tracker(int(dets.shape[0]), int(dets.shape[1]), max_tracks=args.track_slots, score_thresh=args.score, iou_thresh=args.track_iou,
                                         max_age=args.track_max_age, min_hits=args.track_min_hits, device=dets.device)
            # prediction from the estimator's rows of this frame's pair; a key frame restarts the chain and has none
            rows = clip.last_rows() if args.estimate is not None and not is_key else None
            ids = tracker.step(dets, counts, rows)
            if drawer is None:
                ids_h = ids.cpu().numpy()
        frame_dets = []
        for j in range(1, dets_h.shape[0]):
            for r, (x1, y1, x2, y2, s) in enumerate(dets_h[j, :counts_h[j]]):
                frame_dets.append({'class': classes[j] if classes else j, 'score': float(s),
                                   'box': [float(x1), float(y1), float(x2), float(y2)]})
                if ids_h is not None:
                    frame_dets[-1]['track'] = int(ids_h[j, r])
        results.append({'frame': clip.names[idx], 'key': is_key, 'dets': frame_dets})
        if drawer is not None:       # after the frame's time is taken, on the device buffers: the reference's tic/toc excludes draw_boxes too
            drawer.frame(idx, dets, counts, ids)
    if drawer is not None:
        drawer.close()
    print('done: {} frames, {} detections above {:.2f}'.format(len(results), sum(len(r['dets']) for r in results),
                                                                args.score))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(results, f)
    return results


if __name__ == '__main__':
    main()
