#!/usr/bin/env python
"""Counterpart of dff_rfcn/demo.py (:63-158): run the key / non-key frame loop over one clip, print
the running mean time per frame like the reference's tic/toc loop, and report the detections that
score above 0.7 after per-class NMS.

    python -m lsfa_amd.demo                         # synthetic 1000x600 clip, random-init weights
    python -m lsfa_amd.demo --frames DIR [--mv DIR] [--prefix P --epoch E] [--out dets.json]
    python -m lsfa_amd.demo --frames DIR --estimate-mv [--search 16 --mv-lambda 4] [--dump-mv DIR]

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
Drawing boxes into images (draw_boxes, :150-156) is left to the caller: the output is JSON.
"""
import argparse
import glob
import json
import os
import time

import numpy as np
import torch

from lsfa_amd.config.config import config, lsfa_test_config, update_config, update_network_config
from lsfa_amd.core.graphs import FrameGraphs
from lsfa_amd.symbols import params as P
from lsfa_amd.symbols.resnet_v1_101_flownet_rfcn import resnet_v1_101_flownet_rfcn
from lsfa_amd.utils.image import resize, transform, transform_mv_res
from lsfa_amd.utils.load_model import load_param
from lsfa_amd.utils.synthetic import SyntheticClip


class FrameDirClip(object):
    """Frames of one clip from a directory, preprocessed like the reference's demo (:73-82).  estimate: None, or a dict of
    hip.MotionEstimator's parameters (search, lam, max_sad) - motion vectors and residuals are then estimated from the frames on
    `device`; dump_mv: a directory that receives them as the .npz files `mv_dir` is read from."""

    def __init__(self, frame_dir, mv_dir, cfg, estimate=None, device='cuda:0', dump_mv=None):
        from PIL import Image
        names = sorted(sum((glob.glob(os.path.join(frame_dir, e)) for e in ('*.JPEG', '*.jpg', '*.jpeg', '*.png')), []))
        if not names:
            raise FileNotFoundError('no frames under %s' % frame_dir)
        if estimate is not None and mv_dir is not None:
            raise ValueError('either read motion vectors (mv_dir) or estimate them, not both')
        if dump_mv is not None and estimate is None:
            raise ValueError('dump_mv writes the ESTIMATED motion vectors: it needs estimate')
        self.names, self.mv_dir, self.cfg = names, mv_dir, cfg
        self._open = Image.open
        self.num_frames = len(names)
        f0, self.im_scale = self._load(0)
        self.height, self.width = f0.shape[2], f0.shape[3]
        self.estimate, self.device, self.dump_mv = estimate, device, dump_mv
        self._me, self._me_key, self._me_last, self._u8 = None, None, None, {}
        if dump_mv is not None:
            os.makedirs(dump_mv, exist_ok=True)

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

    def _estimated(self, i, key_i):
        from lsfa_amd import hip
        if self._me is None:
            k = self._frame_u8(key_i)
            self._me = hip.MotionEstimator(int(k.shape[1]), int(k.shape[0]), self.device, **self.estimate)
        me = self._me
        if self._me_key != key_i or i < self._me_last:        # a new interval (or a step back): start from the key frame again
            self._u8 = {f: t for f, t in self._u8.items() if key_i <= f <= i}
            me.key_frame(self._frame_u8(key_i))
            self._me_key, self._me_last = key_i, key_i
        for f in range(self._me_last + 1, i + 1):             # the P-frame chain: every frame against the one before it
            me.next_frame(self._frame_u8(f))
        self._me_last = i
        cfg = self.cfg
        cur, key = self._frame_u8(i), self._frame_u8(key_i)
        if self.dump_mv is not None:
            stem = os.path.splitext(os.path.basename(self.names[i]))[0]
            np.savez(os.path.join(self.dump_mv, stem + '.npz'), mv=(-me.acc.motion_vectors()).cpu().numpy(),
                     res=me.acc.residual(cur, key).cpu().numpy())
        mv, res = me.network_inputs(cur, key, self.im_scale, cfg.network.PIXEL_MEANS, cfg.network.PIXEL_SCALE)
        return mv.clone(), res.clone()                        # the estimator reuses its output buffers

    def mv_res(self, i, key_i):
        if self.estimate is not None:
            return self._estimated(i, key_i)
        fh, fw = -(-self.height // 16), -(-self.width // 16)
        if self.mv_dir is None:
            return torch.zeros(1, 2, fh, fw), torch.zeros(1, 3, fh, fw)
        stem = os.path.splitext(os.path.basename(self.names[i]))[0]
        z = np.load(os.path.join(self.mv_dir, stem + '.npz'))
        cfg = self.cfg
        return transform_mv_res(z['mv'], z['res'], self.im_scale, cfg.network.PIXEL_MEANS, cfg.network.PIXEL_SCALE)


class _Synthetic(object):
    def __init__(self, n, h, w):
        self.c = SyntheticClip(0, n, h, w)
        self.num_frames, self.height, self.width, self.im_scale = n, h, w, 1.0
        self.names = ['synthetic/%06d' % i for i in range(n)]

    def frame(self, i):
        return self.c.frame(i)

    def mv_res(self, i, key_i):
        return self.c.motion_vector(i, key_i), self.c.res_diff(i)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='LSFA demo: key / non-key frame loop over one clip')
    ap.add_argument('--cfg', default=None)
    ap.add_argument('--frames', default=None, help='directory of frames (default: a synthetic clip)')
    ap.add_argument('--mv', default=None, help='directory of per-frame .npz with mv / res arrays')
    ap.add_argument('--estimate-mv', action='store_true', help='estimate block motion vectors from the frames on the GPU (needs --frames)')
    ap.add_argument('--search', type=int, default=16, help='--estimate-mv: search range in pixels, 1..32 (a parameter, not a tuned value)')
    ap.add_argument('--mv-lambda', type=int, default=4, help='--estimate-mv: cost per pixel of vector length (a parameter, not a tuned value)')
    ap.add_argument('--dump-mv', default=None, help='--estimate-mv: write the estimated mv / res as the .npz files --mv reads')
    ap.add_argument('--num', type=int, default=30, help='frames of the synthetic clip')
    ap.add_argument('--interval', type=int, default=10, help='key frame interval (demo.py:68)')
    ap.add_argument('--prefix', default=None)
    ap.add_argument('--epoch', type=int, default=0)
    ap.add_argument('--score', type=float, default=0.7, help='report threshold (demo.py:147)')
    ap.add_argument('--out', default=None, help='write the detections as JSON here')
    ap.add_argument('--no-graph', action='store_true')
    args = ap.parse_args(argv)
    if args.estimate_mv and (not args.frames or args.mv):
        ap.error('--estimate-mv needs --frames and excludes --mv')
    if args.dump_mv and not args.estimate_mv:
        ap.error('--dump-mv needs --estimate-mv')
    return args


def main(argv=None):
    args = parse_args(argv)
    if args.cfg:
        cfg = update_config(args.cfg, config)
        update_network_config(cfg)
    else:
        cfg = lsfa_test_config()
    cfg.TEST.KEY_FRAME_INTERVAL = args.interval
    dev = 'cuda:0'
    estimate = dict(search=args.search, lam=args.mv_lambda) if args.estimate_mv else None
    clip = FrameDirClip(args.frames, args.mv, cfg, estimate, dev, args.dump_mv) if args.frames else _Synthetic(args.num, 600, 1000)
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

    results, total, count = [], 0.0, 0
    for idx in range(clip.num_frames):
        data = clip.frame(idx).to(dev)
        mv, res = (None, None) if idx % args.interval == 0 else [t.to(dev) for t in clip.mv_res(idx, idx - idx % args.interval)]
        torch.cuda.synchronize()
        t0 = time.time()
        if idx == 0:
            dets, counts, _ = fg.first_frame(data)
            torch.cuda.synchronize()
            dets_h, counts_h = dets.cpu().numpy(), counts.cpu().numpy()
            fg.capture()                                   # the reference's "warm up" (:104-116)
            print('warmup done')
        else:
            dets, counts, _ = fg.key_frame(data) if idx % args.interval == 0 else fg.cur_frame(data, mv, res)
            dets_h, counts_h = dets.cpu().numpy(), counts.cpu().numpy()    # .cpu() is the per-frame sync
            total += time.time() - t0
            count += 1
            print('testing {} {:.4f}s'.format(clip.names[idx], total / count))
        frame_dets = []
        for j in range(1, dets_h.shape[0]):
            for x1, y1, x2, y2, s in dets_h[j, :counts_h[j]]:
                frame_dets.append({'class': classes[j] if classes else j, 'score': float(s),
                                   'box': [float(x1), float(y1), float(x2), float(y2)]})
        results.append({'frame': clip.names[idx], 'key': idx % args.interval == 0, 'dets': frame_dets})
    print('done: {} frames, {} detections above {:.2f}'.format(len(results), sum(len(r['dets']) for r in results),
                                                                args.score))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(results, f)
    return results


if __name__ == '__main__':
    main()
