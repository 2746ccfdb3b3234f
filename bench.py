#!/usr/bin/env python
"""LSFA per-frame inference benchmark on MI355X.

    python bench.py --gpus N --steps K --warmup W                      # BASELINE configs[1] (the headline)
    python bench.py --dtype bf16 --clips 4                             # configs[2]: bf16 contractions, 4 clips in lock-step
    python bench.py --interval 1 --maps-per-launch 32 --full           # configs[4]: every frame a key frame; warp /
                                                                       #   aggregate roofline on 32 maps per launch (HBM-resident)

Metric (BASELINE.json): frames/sec at 1000x600, key_interval = 10, synthetic VID-shaped clips,
random-init weights of the trained LSFA architecture (ResNet-101 + DCN + FlowNet + Nq + small net
+ R-FCN head), fp32.  Default workload = BASELINE.json configs[1] ("dff_rfcn ResNet-101 LSFA, 1 clip
key_interval=10 on 1xMI355X, fp32").

A STEP is one key-frame interval of the clip(s) of this GPU: 1 key frame (ResNet-101 + FlowNet + flow
warp x scale map + Nq aggregation + heads + Proposal + PSROI + detection NMS) followed by
key_interval-1 non-key frames (small net + MV warp + residual + heads + Proposal + PSROI +
detection NMS).  Frames, motion vectors and residuals are resident in HBM before the timed
region (the bench contract: `value` never includes PCIe; the same pipeline with the inputs starting in
pinned host memory and uploaded inside the region is the extra figure `value_uploaded_inputs`, or
`value` itself under --host-inputs); every frame's detections are copied to pinned host memory inside it.

N > 1: launched by torch.distributed.run, one rank per GPU; rank r runs clip(s) r (clips are
independent: "scaling": "weak", no data-path collective); the only collective is the final
all_gather of per-frame detection counts over RCCL, outside the per-frame path.

A plain run sets up, warms up, times the --steps steps and prints the line.  With --full, rank 0 adds after
the timed region, untimed: `value_spread` (the region twice more), the extra regions (`value_uploaded_inputs`,
`value_exact_fp32`, `value_frame_by_frame`), `roofline` (HIP events around every launch of the hand-written ops,
the same frames re-issued eagerly; a captured graph carries no per-launch events; --maps-per-launch), `parity`
(the first frames of the clip against oracle/graph_ref.py: end to end, and stage by stage on the GPU's own inputs)
and `cpu_baseline` (the oracle graph timed on the host cores).

--dump-outputs DIR writes what the last timed step delivered to the host (rank 0's clips) as DIR/<name>.npy:
`detections` (K, B, classes, R, 5) float64 [x1, y1, x2, y2, score], rows past a class's count zeroed, and `counts`
(K, B, classes) float64.  The inputs are seeded: the same arguments give the same inputs in every run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_SPLIT_PEAK_TFLOPS = round(2500.0 / 6, 1)           # dense bf16 MFMA peak / the six partial products of an fp32 product
MFMA_BF16_PEAK_TFLOPS = 2500.0                           # dense bf16 / fp16 MFMA peak (MI355X_MICROARCH.md)
HBM_PEAK_GBS = 8000.0                                   # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
TRAFFIC_FILE = os.path.join(ROOT, 'profiles', 'traffic.json')   # HBM bytes per launch from rocprofv3 PMC passes, keyed by shape


def warp_bytes(N, C, HW):
    """feat + (scale map | small-net feature) + out, + flow, each touched once."""
    return N * (3 * C * HW + 2 * HW) * 4


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--interval', type=int, default=10)
    ap.add_argument('--height', type=int, default=600)
    ap.add_argument('--width', type=int, default=1000)
    ap.add_argument('--dtype', default='f32', choices=['f32', 'bf16'])
    ap.add_argument('--clips', type=int, default=1,
                    help='clips per GPU advancing in lock-step, one image of each per frame on the batch axis (configs[2]: 4)')
    ap.add_argument('--maps-per-launch', type=int, default=0,
                    help='--full: roofline leg on this many feature maps per launch of the warp / aggregate kernels (configs[4]: 32, '
                         '942 MB per launch, HBM-resident); 0 = the frame loop\'s own single-map launches')
    ap.add_argument('--settle-s', type=float, default=2.5,
                    help='setup: after graph capture, replay untimed intervals for this long before the W warm-up steps (a fresh '
                         'device needs 1-3 s of load to reach its steady clocks; W = 5 intervals is 30 ms)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-parity', action='store_true')
    ap.add_argument('--no-spread', action='store_true', help='skip the two extra repeats of the timed region behind `value_spread`')
    ap.add_argument('--host-inputs', action='store_true',
                    help='`value` = the PCIe-inclusive rate: uint8 frames + fp32 motion vectors / residuals start in pinned HOST memory, are uploaded per interval '
                         'inside the timed region and transformed on the GPU (lib/utils/image.py:296-308).  Default: `value` is measured with every input already '
                         'resident in HBM when the timed region starts (the bench contract) and the PCIe-inclusive rate is an extra region of the same line '
                         '(`value_uploaded_inputs`)')
    ap.add_argument('--resident-inputs', action='store_true',
                    help='do not build the host-side input blocks at all: no `value_uploaded_inputs` region (r1-r4)')
    ap.add_argument('--eager-loop', type=int, default=0,
                    help='profiling aid (tools/profile_round.sh): no timed region - re-issue the roofline leg (eager_profile_batched: key_group intervals the way the '
                         'pipeline batches them, serially on one stream) this many times and print its per-kernel FLOP table; run it under rocprofv3')
    ap.add_argument('--no-frame-by-frame', action='store_true', help='skip the extra frame-by-frame region behind `value_frame_by_frame`')
    ap.add_argument('--no-graph', action='store_true', help='issue every launch eagerly instead of replaying hipGraphs')
    ap.add_argument('--no-prefetch', action='store_true', help='do not overlap the next frame\'s small net with this frame\'s tail')
    ap.add_argument('--lanes', type=int, default=2,
                    help='non-key frames of a segment alternate over this many streams while the next key frame runs on '
                         'its own stream (lsfa_amd.core.graphs.FramePipeline); 0 = strictly serial frames')
    ap.add_argument('--segment', type=int, default=-1,
                    help='non-key frames of a segment that go through the network in ONE pass, batch axis = frames (the reference\'s batch test '
                         'symbol, resnet_v1_101_flownet_rfcn.py:661-751); -1 = interval - 1 when one clip runs pipelined, else 0 = frame by frame')
    ap.add_argument('--key-group', type=int, default=12,
                    help='key frames whose image-only half (backbone, FlowNet) is computed in one pass (FramePipeline key_group); 1 = one by one.  '
                         '12 since r6 (profiles/r6/key_group_sweep.txt: 6 -> 3664, 12 -> 3784, 18 -> 3810, 24 -> 3854 frames/s over 120 intervals; '
                         'sizes that are not multiples of 6 lose)')
    ap.add_argument('--ramp', default='',
                    help='sizes of the first passes of key fronts after the pipeline ran empty, e.g. "1,2" (FramePipeline ramp); default: full groups at once')
    ap.add_argument('--lookahead', action='store_true',
                    help='queue each key frame ahead of the non-key frames that precede it in display order')
    ap.add_argument('--no-flow-stream', action='store_true', help='FlowNet after the backbone on the key stream instead of beside it')
    ap.add_argument('--cpu-budget-s', type=float, default=20.0)
    ap.add_argument('--max-unique-steps', type=int, default=16, help='distinct intervals of frames kept in HBM')
    ap.add_argument('--full', action='store_true',
                    help='everything beyond the headline figure: the repeats behind `value_spread`, the uploaded-input, exact-fp32 and frame-by-frame '
                         'regions, the roofline legs (--maps-per-launch included), parity against the oracle and the CPU baseline.  Off: set up, '
                         'warm up, time the --steps steps, print the line')
    ap.add_argument('--dump-outputs', default='', metavar='DIR',
                    help='write what the last timed step delivered (detections and per-class counts of its frames) as DIR/<name>.npy')
    return ap.parse_args()


class Runner(object):
    """The clip stream(s) of one GPU: the pred_eval frame loop (dff_rfcn/core/tester.py:237-281)."""

    def __init__(self, args, rank, device):
        from lsfa_amd import hip
        from lsfa_amd.config.config import lsfa_test_config
        from lsfa_amd.symbols import params as P
        from lsfa_amd.symbols.resnet_v1_101_flownet_rfcn import resnet_v1_101_flownet_rfcn
        from lsfa_amd.utils.synthetic import SyntheticClip
        self.hip, self.args, self.device = hip, args, device
        self.cfg = cfg = lsfa_test_config(key_frame_interval=args.interval)
        self.arg, self.aux = P.init_params(cfg, seed=0)
        dt = torch.float32 if args.dtype == 'f32' else torch.bfloat16
        net = resnet_v1_101_flownet_rfcn(cfg)
        self.key = net.get_key_test_symbol(cfg).bind(self.arg, self.aux, device, dt)
        self.cur = net.get_cur_test_symbol(cfg).bind(self.arg, self.aux, device, dt)
        self.K, self.B = args.interval, args.clips
        self.nsteps_unique = min(args.max_unique_steps, args.steps + args.warmup)
        nframes = self.nsteps_unique * self.K + 1
        self.clips = [SyntheticClip(rank * self.B + b, nframes, args.height, args.width, self.K) for b in range(self.B)]
        cat = lambda fn: torch.cat([fn(c) for c in self.clips], 0)
        # frames resident in HBM: frame 0 primes the recurrence, then nsteps_unique intervals
        self.frames = [cat(lambda c: c.frame(f, device)) for f in range(nframes)]
        self.mv, self.res = {}, {}
        for s in range(self.nsteps_unique):
            kf = 1 + s * self.K
            for i in range(1, self.K):
                self.mv[kf + i] = cat(lambda c: c.motion_vector(kf + i, kf, device))
                self.res[kf + i] = cat(lambda c: c.res_diff(kf + i, device))
        # r5: the inputs as a loader hands them over (dff_rfcn/core/loader.py:131-141: HOST arrays per frame).  Per interval two pinned blocks:
        # the key frame (uint8 HWC BGR, what a decoder returns) - uploaded `key_group - 1` intervals ahead, because a pass of key fronts needs the
        # images of its whole group - and [the K-1 non-key frames uint8 | their motion vectors fp32 | their residuals fp32], uploaded with the
        # interval.  One copy per block on a copy stream, transform (lib/utils/image.py:296-308) on the GPU behind it, into preallocated rings.
        # (they feed `value` under --host-inputs, else only the uploaded-input region of --full)
        self.host_inputs = (not args.resident_inputs) and args.lanes > 0 and (getattr(args, 'full', False) or getattr(args, 'host_inputs', False))
        self._inputs_resident_now = not (self.host_inputs and getattr(args, 'host_inputs', False))
        if self.host_inputs:
            K, B, H, W = self.K, self.B, args.height, args.width
            fh, fw = self.clips[0].fh, self.clips[0].fw
            self._nb_rest_frames = (K - 1) * B * H * W * 3
            self._nb_mv, self._nb_res = (K - 1) * B * 2 * fh * fw * 4, (K - 1) * B * 3 * fh * fw * 4
            assert self._nb_rest_frames % 16 == 0 and self._nb_mv % 16 == 0, "input block offsets must stay 16-byte aligned"
            self.host_key, self.host_rest = [], []
            # the decoder's view of the RESIDENT frames (integer-valued RGB planes -> uint8 HWC BGR): the two input modes then see the same images bit
            # for bit.  (SyntheticClip.frame_u8 renders on the host; its sines differ from the device's in the last ulp and a few dozen pixels per frame
            # round the other way - enough to move the mAP-agreement figure in its fourth digit between the modes.)
            u8_of = lambda t: t.detach().cpu().flip(0).permute(1, 2, 0).to(torch.uint8)
            for s_ in range(self.nsteps_unique):
                kf = 1 + s_ * K
                hk = torch.empty((B, H, W, 3), dtype=torch.uint8).pin_memory()
                for b in range(B):
                    hk[b] = u8_of(self.frames[kf][b])
                blk = torch.empty(self._nb_rest_frames + self._nb_mv + self._nb_res, dtype=torch.uint8).pin_memory()
                fr = blk[:self._nb_rest_frames].view(K - 1, B, H, W, 3)
                mvv = blk[self._nb_rest_frames:self._nb_rest_frames + self._nb_mv].view(torch.float32).view(K - 1, B, 2, fh, fw)
                rsv = blk[self._nb_rest_frames + self._nb_mv:].view(torch.float32).view(K - 1, B, 3, fh, fw)
                for i in range(1, K):
                    for b in range(B):
                        fr[i - 1, b] = u8_of(self.frames[kf + i][b])
                    mvv[i - 1] = self.mv[kf + i].cpu()
                    rsv[i - 1] = self.res[kf + i].cpu()
                self.host_key.append(hk)
                self.host_rest.append(blk)
            G = max(1, args.key_group)
            self._rk, self._rr = 2 * G + 4, 6        # ring depths: a key image lives until the NEXT key frame's pass has read it as `data_key_old`
            self.dkey_u8 = [torch.empty((B, H, W, 3), dtype=torch.uint8, device=device) for _ in range(self._rk)]
            self.dkey_f32 = [torch.empty((B, 3, H, W), dtype=torch.float32, device=device) for _ in range(self._rk)]
            self.drest_blk = [torch.empty(self.host_rest[0].numel(), dtype=torch.uint8, device=device) for _ in range(self._rr)]
            self.drest_f32 = [torch.empty(((K - 1) * B, 3, H, W), dtype=torch.float32, device=device) for _ in range(self._rr)]
            self._seq = 0                            # intervals queued so far (ring slots and the events below are keyed by it)
            self._up_key, self._up_rest, self._done, self._done_key = {}, {}, {}, {}
            self._pixel_means = [float(v) for v in cfg.network.PIXEL_MEANS]
            self._pixel_scale = float(cfg.network.PIXEL_SCALE)
        R, ncls = cfg.TEST.RPN_POST_NMS_TOP_N, cfg.dataset.NUM_CLASSES
        # one pinned slot per frame of an interval; dets and counts back to back like the device side keeps them
        # (lsfa_amd/core/graphs.py _alloc_post), so a frame's results leave the device with ONE copy
        n_d, n_c = self.B * ncls * R * 5, (self.B * ncls * 4 + 7) // 8
        self.host_flat = torch.empty((self.K, n_d + n_c), dtype=torch.float64).pin_memory()
        self.host_dets = self.host_flat[:, :n_d].view(self.K, self.B, ncls, R, 5)
        self._n_d, self.ncls, self._R = n_d, ncls, R
        from lsfa_amd.core.graphs import FrameGraphs, FramePipeline
        pipelined = args.lanes > 0
        self.segment = (self.K - 1 if (pipelined and self.K > 2) else 0) if args.segment < 0 else (args.segment if pipelined else 0)
        self.key_group = max(1, args.key_group) if pipelined else 1
        F = self.segment
        nimg = max(F, 1) * self.B                   # images of a batched segment, frame-major
        self.host_seg = torch.empty(nimg * ncls * R * 5 + (nimg * ncls * 4 + 7) // 8, dtype=torch.float64).pin_memory()
        if args.lanes > 0:
            self.fg = FramePipeline(self.key, self.cur, cfg, args.height, args.width, device,
                                    use_graphs=not args.no_graph, lanes=max(args.lanes, 2 if F else 1),
                                    flow_stream=not args.no_flow_stream, lookahead=args.lookahead, batch=self.B,
                                    segment=F, key_group=self.key_group, ramp=tuple(int(v) for v in args.ramp.split(',') if v.strip()))
        else:
            self.fg = FrameGraphs(self.key, self.cur, cfg, args.height, args.width, device, use_graphs=not args.no_graph,
                                  prefetch=not args.no_prefetch, batch=self.B)

    @property
    def feat(self):
        return self.fg.feat

    def prime(self):
        """Frame 0 of the clip (flag 0: no aggregation) sets up feat_key / data_key; then the per-frame
        launch sequences are captured into hipGraphs (untimed)."""
        self.fg.first_frame(self.frames[0])
        self.fg.capture()

    def _in_segment(self, slot):
        """frame `slot` of the interval came back with its whole segment (one copy per segment, host_seg) rather than on its own"""
        return self.segment > 0 and slot >= 1 and self.segment == self.K - 1

    def host_counts_of(self, slot):
        if self._in_segment(slot):
            F, n, B = self.segment, self.ncls, self.B
            return self.host_seg[F * B * n * self._R * 5:].view(torch.int32)[:F * B * n].view(F, B, n)[slot - 1]
        return self.host_flat[slot, self._n_d:].view(torch.int32)[:self.B * self.ncls].view(self.B, self.ncls)

    def host_dets_of(self, slot):
        if self._in_segment(slot):
            F, n, B = self.segment, self.ncls, self.B
            return self.host_seg[:F * B * n * self._R * 5].view(F, B, n, self._R, 5)[slot - 1]
        return self.host_dets[slot]

    @property
    def host_counts(self):
        """(K, B, ncls) int32: the per-class detection counts of the last interval's frames (a copy)."""
        return torch.stack([self.host_counts_of(k) for k in range(self.K)])

    def last_interval_rows(self):
        """The last interval's detections as the rows the reference's result file holds (lib/dataset/imagenet_vid.py:260-268):
        [frame, class, score, x1, y1, x2, y2] float64, frames numbered (clip of this rank, frame of the interval)."""
        counts, rows = self.host_counts, []
        for k in range(self.K):
            for b in range(self.B):
                for j in range(1, self.ncls):
                    n = int(counts[k, b, j])
                    if n:
                        d = self.host_dets_of(k)[b, j, :n].numpy()
                        r = np.empty((n, 7), np.float64)
                        r[:, 0], r[:, 1], r[:, 2], r[:, 3:] = k * self.B + b, j, d[:, 4], d[:, :4]
                        rows.append(r)
        return np.vstack(rows) if rows else np.zeros((0, 7), np.float64)

    def last_step_outputs(self):
        """What the last step delivered to the host, once the pipeline is drained: per frame of the interval and clip, every class's
        detections [x1, y1, x2, y2, score] (rows past the class's count zeroed: those slots hold whatever an earlier frame left) and the
        per-class counts.  -> {name: float64 array}"""
        counts = self.host_counts.numpy().astype(np.int64)                                 # (K, B, ncls)
        dets = np.stack([self.host_dets_of(k).numpy() for k in range(self.K)])            # (K, B, ncls, R, 5)
        valid = np.arange(self._R) < counts[..., None]
        return {"detections": np.where(valid[..., None], dets, 0.0).astype(np.float64), "counts": counts.astype(np.float64)}

    def _deliver(self, bufs, slot):
        seg = getattr(bufs[0], 'lsfa_segment', None)
        if seg is not None:          # a frame of a batched segment: the whole segment's results leave the device with its last frame, in one copy
            flat, f, F = seg
            if f == F - 1 and flat.numel() == self.host_seg.numel():
                self.host_seg.copy_(flat, non_blocking=True)
            elif flat.numel() != self.host_seg.numel():
                self.host_dets[slot].copy_(bufs[0].view(self.host_dets[slot].shape), non_blocking=True)
                self.host_counts_of(slot).copy_(bufs[1].view(self.B, self.ncls), non_blocking=True)
            return
        flat = getattr(bufs[0], 'lsfa_flat', None)
        if flat is not None and flat.numel() == self.host_flat.shape[1]:
            self.host_flat[slot].copy_(flat, non_blocking=True)
        else:
            self.host_dets[slot].copy_(bufs[0].view(self.host_dets[slot].shape), non_blocking=True)
            self.host_counts_of(slot).copy_(bufs[1].view(self.B, self.ncls), non_blocking=True)

    def step(self, s, fg=None, end=None, key_group=None):
        """One key-frame interval: key frame (flag 1) + K-1 non-key frames (flag 2).  end: one past the last step of the run of consecutive
        steps this one belongs to (key_group: only key frames of the same run are looked ahead at)."""
        fg = fg or self.fg
        key_group = self.key_group if key_group is None else key_group
        kf = 1 + (s % self.nsteps_unique) * self.K
        if hasattr(fg, 'lanes'):      # pipelined: frames are queued in order, copies ride on each frame's stream
            ahead = range(s + 1, s + key_group if end is None else min(s + key_group, end))
            if self.host_inputs and not self._inputs_resident_now:
                # this interval's key image and non-key block, and the key images of the intervals its key group looks ahead at
                q = self._seq
                # WHERE the uploads are queued matters more than what they cost: ROCm multiplexes HIP streams onto 4 hardware queues and the
                # pipeline's four streams have one each (lsfa_amd/core/streams.py), so a fifth stream shares a queue - behind the key stream's
                # 10 ms passes an interval's 16 MB block arrived late and the lanes starved (2580 frames/s against 3460 with resident inputs).
                # The non-key block goes onto a lane's stream, the key images onto the FlowNet / tail stream: queues with slack.
                lanes = list(fg.s_lane)
                # (interval 1: no non-key frames, the lanes are idle and the FlowNet / tail stream carries every frame's back half: the lanes' queue then)
                ks = lanes[0] if self.K == 1 or fg.s_flow is None else fg.s_flow
                keys = [self._upload_key(q + j, s + j, ks) for j in range(1 + len(ahead))]
                # (the lane this interval's segment will be queued on - not this loop's own parity: the pipeline's count may be ahead of it)
                rest_stream = fg.stream_of_next_segment() if hasattr(fg, 'stream_of_next_segment') else lanes[q % len(lanes)]
                fr, mvs, rss, ev_rest = self._upload_rest(q, s, rest_stream) if self.K > 1 else (None, None, None, None)      # (interval 1: every frame is a key frame)
                ev_keys = keys[-1][1]                # one stream, in order: the last upload's event covers the earlier ones
                B = self.B
                fg.key_frame(keys[0][0], deliver=lambda b: self._deliver(b, 0), ready=ev_keys,
                             upcoming=[k[0] for k in keys[1:]] if key_group > 1 else None)
                for i in range(1, self.K):
                    fg.cur_frame(fr[(i - 1) * B:i * B], mvs[i - 1], rss[i - 1], deliver=lambda b, i=i: self._deliver(b, i), ready=ev_rest)
                # everything that reads interval q - 1's inputs has been queued by now (its segment goes out with this key frame): their ring slots
                # may be refilled once these events have passed
                # (key images are read on the key and FlowNet / tail streams, the non-key blocks on the lanes: each ring waits for its readers only -
                # the key stream runs whole passes ahead, and a lane's upload must not wait for those)
                for ring, sts in ((self._done_key, [fg.s_key] + ([fg.s_flow] if fg.s_flow is not None else [])), (self._done, list(fg.s_lane))):
                    evs = []
                    for st in sts:
                        e = torch.cuda.Event()
                        e.record(st)
                        evs.append(e)
                    ring[q] = evs
                    ring.pop(q - 4 * self._rk, None)
                self._up_key.pop(q, None)
                self._up_rest.pop(q, None)
                self._seq = q + 1
                return
            fg.key_frame(self.frames[kf], deliver=lambda b: self._deliver(b, 0),
                         upcoming=[self.frames[1 + (j % self.nsteps_unique) * self.K] for j in ahead] if key_group > 1 else None)
            for i in range(1, self.K):
                fg.cur_frame(self.frames[kf + i], self.mv[kf + i], self.res[kf + i],
                             deliver=lambda b, i=i: self._deliver(b, i))
            return
        nxt = lambda i: self.frames[kf + i + 1] if i + 1 < self.K else None   # the frame after a non-key frame, if non-key too
        self._deliver(fg.key_frame(self.frames[kf], nxt(0)), 0)
        for i in range(1, self.K):
            self._deliver(fg.cur_frame(self.frames[kf + i], self.mv[kf + i], self.res[kf + i], nxt(i)), i)

    _inputs_resident_now = True         # the timed region: inputs already in HBM (the bench contract); False: uploaded inside the region (--host-inputs, and the extra region)

    def _wait_free(self, q, depth, done, stream):
        """ring slot q % depth was last filled for interval q - depth: its readers are all queued once interval q - depth + 1 has been (see step)"""
        for e in done.get(q - depth + 1, ()):
            stream.wait_event(e)

    def _upload_key(self, q, step, stream):
        """Interval `step`'s key image (queue position q): pinned host -> device ring slot, transform behind it.  -> ((B, 3, H, W) fp32, event)"""
        u = self._up_key.get(q)
        if u is None:
            i = q % self._rk
            with torch.cuda.stream(stream):
                self._wait_free(q, self._rk, self._done_key, stream)
                self.dkey_u8[i].copy_(self.host_key[step % self.nsteps_unique], non_blocking=True)
                self.hip.image_transform_u8(self.dkey_u8[i], self._pixel_means, self._pixel_scale, out=self.dkey_f32[i])
                ev = torch.cuda.Event()
                ev.record(stream)
            u = self._up_key[q] = (self.dkey_f32[i], ev)
        return u

    def _upload_rest(self, q, step, stream):
        """Interval `step`'s non-key frames, motion vectors and residuals: ONE copy of the pinned block.  -> (frames ((K-1)*B, 3, H, W) fp32,
        mv (K-1, B, 2, fh, fw), res (K-1, B, 3, fh, fw), event)"""
        u = self._up_rest.get(q)
        if u is None:
            a, i = self.args, q % self._rr
            fh, fw = self.clips[0].fh, self.clips[0].fw
            with torch.cuda.stream(stream):
                self._wait_free(q, self._rr, self._done, stream)
                blk = self.drest_blk[i]
                blk.copy_(self.host_rest[step % self.nsteps_unique], non_blocking=True)
                self.hip.image_transform_u8(blk[:self._nb_rest_frames].view((self.K - 1) * self.B, a.height, a.width, 3), self._pixel_means,
                                            self._pixel_scale, out=self.drest_f32[i])
                mv = blk[self._nb_rest_frames:self._nb_rest_frames + self._nb_mv].view(torch.float32).view(self.K - 1, self.B, 2, fh, fw)
                rs = blk[self._nb_rest_frames + self._nb_mv:].view(torch.float32).view(self.K - 1, self.B, 3, fh, fw)
                ev = torch.cuda.Event()
                ev.record(stream)
            u = self._up_rest[q] = (self.drest_f32[i], mv, rs, ev)
        return u

    def other_inputs_region(self, steps, warmup, settle_s=0.75):
        """r5: the main pipeline fed the OTHER way - uploads inside the region when `value` was measured with resident inputs (the default), resident
        inputs under --host-inputs - for `steps` timed intervals -> frames/s"""
        main = self._inputs_resident_now
        self._inputs_resident_now = not main
        try:
            # its own settle, like the main region's: the first passes over the pinned blocks and the device rings (and the clocks after the
            # eager roofline leg) are not the steady state - without it this region read 10 % low against the same mode measured as `value`
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < settle_s:
                for s in range(32):
                    self.step(s, end=32)
                self.fg.flush()
                torch.cuda.synchronize()
            rates = []
            for _ in range(2):            # the region twice, like the main region's repeats: the second is reported (the first still carries one-time costs)
                for s in range(warmup):
                    self.step(s, end=warmup)
                self.fg.flush()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for s in range(warmup, warmup + steps):
                    self.step(s, end=warmup + steps)
                self.fg.flush()
                torch.cuda.synchronize()
                rates.append(self.B * steps * self.K / (time.perf_counter() - t1))
                self._up_key.clear()
                self._up_rest.clear()
            self.other_inputs_rates = [round(v, 3) for v in rates]
            return rates[-1]
        finally:
            self._inputs_resident_now = main
            self._up_key.clear()
            self._up_rest.clear()

    def exact_fp32_region(self, steps=3):
        """r5: the same clip with EVERY product an fp32 product (executors bound with pieces = 0: lsfa_conv_nhwc_fused_fwd on
        v_mfma_f32_32x32x2_f32 - a reference evaluation, see Executor) through the frame-by-frame pipeline, `steps` timed intervals.
        -> frames/s, or None in the bf16 mode."""
        if self.args.dtype != 'f32':
            return None
        from lsfa_amd.core.graphs import FramePipeline
        from lsfa_amd.symbols.resnet_v1_101_flownet_rfcn import resnet_v1_101_flownet_rfcn
        a, cfg = self.args, self.cfg
        net = resnet_v1_101_flownet_rfcn(cfg)
        key = net.get_key_test_symbol(cfg).bind(self.arg, self.aux, self.device, torch.float32, pieces=0)
        cur = net.get_cur_test_symbol(cfg).bind(self.arg, self.aux, self.device, torch.float32, pieces=0)
        fg = FramePipeline(key, cur, cfg, a.height, a.width, self.device, use_graphs=not a.no_graph, lanes=max(a.lanes, 1),
                           flow_stream=not a.no_flow_stream, batch=self.B, segment=0, key_group=1)
        seg, self.segment = self.segment, 0
        try:
            fg.first_frame(self.frames[0])
            fg.capture()
            self.step(0, fg, key_group=1)
            fg.flush()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for s in range(1, 1 + steps):
                self.step(s, fg, key_group=1)
            fg.flush()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t1
            key.check_status()
            cur.check_status()
        finally:
            self.segment = seg
            if hasattr(fg, 'close'):
                fg.close()
        return self.B * steps * self.K / dt

    def frame_by_frame_region(self, steps, warmup, settle_s=0.5):
        """r5: the SAME clip through the frame-by-frame pipeline (segment 0, key_group 1: one frame per pass, no look-ahead - the streaming
        case) for `steps` timed intervals after its own capture, a short settle and `warmup` intervals.  -> frames/s of this rank"""
        from lsfa_amd.core.graphs import FramePipeline
        a = self.args
        fg = FramePipeline(self.key, self.cur, self.cfg, a.height, a.width, self.device, use_graphs=not a.no_graph, lanes=max(a.lanes, 1),
                           flow_stream=not a.no_flow_stream, lookahead=a.lookahead, batch=self.B, segment=0, key_group=1)
        seg, self.segment = self.segment, 0          # (_deliver / host_counts_of: every frame comes back on its own)
        try:
            fg.first_frame(self.frames[0])
            fg.capture()
            t0, n = time.perf_counter(), 0
            while time.perf_counter() - t0 < settle_s:
                self.step(n, fg, key_group=1)
                n += 1
            for s in range(warmup):
                self.step(s, fg, key_group=1)
            fg.flush()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for s in range(warmup, warmup + steps):
                self.step(s, fg, key_group=1)
            fg.flush()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t1
        finally:
            self.segment = seg
            if hasattr(fg, 'close'):
                fg.close()
        return self.B * steps * self.K / dt

    # ---- untimed legs (rank 0) ----------------------------------------------------------------
    OPS = ['warp_bilinear', 'aggregate', 'rfcn_head', 'proposal', 'det_postprocess', 'conv_nhwc']

    def eager_profile_step(self, s):
        """The same interval issued eagerly with the per-kernel event hooks on (a captured graph has no
        per-launch events): the roofline leg.  -> {op: (total_ms, launches)}"""
        from lsfa_amd.core.graphs import FrameGraphs
        eg = FrameGraphs(self.key, self.cur, self.cfg, self.args.height, self.args.width, self.device, use_graphs=False,
                         prefetch=False, batch=self.B)
        eg.feat_old.copy_(self.fg.feat_old)
        eg.data_key_old.copy_(self.fg.data_key_old)
        eg.feat = self.fg.feat.clone()
        self.step(s, eg)     # warm
        torch.cuda.synchronize()
        self.hip.prof_enable(True, ops=self.OPS)
        self.hip.prof_read()
        self.hip.conv_flops_reset(True)
        self.step(s, eg)
        torch.cuda.synchronize()
        prof = self.hip.prof_read()
        self.conv_flops = self.hip.conv_flops_read()
        self.conv_flops3 = self.hip.conv_flops_three_products()
        self.conv_flops1 = self.hip.conv_flops_one_product()
        self.conv_bytes, self.conv_by_kernel = self.hip.conv_bytes_read(), self.hip.conv_by_kernel()
        self.hip.conv_flops_reset(False)
        self.hip.prof_enable(False)
        return prof

    def eager_profile_batched(self, s):
        """The roofline leg of the batched pipeline: G consecutive intervals the way FramePipeline(segment, key_group) computes them - one pass
        for the G key fronts, per key frame aggregation + heads + detections, one pass per segment - issued eagerly on ONE stream with the
        per-kernel event hooks on (nothing overlaps: the durations are the kernels' own).  -> {op: (total_ms, launches)} over the G intervals."""
        from lsfa_amd.core import graphs
        G, F, K, cfg, hip = self.key_group, self.segment, self.K, self.cfg, self.hip
        key, cur, fg = self.key, self.cur, self.fg
        H, W = self.args.height, self.args.width
        kfs = [1 + ((s + j) % self.nsteps_unique) * K for j in range(G)]
        imgs = torch.cat([self.frames[k] for k in kfs], 0)
        olds = torch.cat([fg.data_key_old] + [self.frames[k] for k in kfs[:-1]], 0)
        feat0 = fg.feat.clone()
        im1 = fg.klanes[0].im_info
        R, ncls = cfg.TEST.RPN_POST_NMS_TOP_N, cfg.dataset.NUM_CLASSES
        B = self.B
        post1, _ = graphs._alloc_post(B, ncls, R, self.device)
        postF, _ = graphs._alloc_post(max(F, 1) * B, ncls, R, self.device)
        imF = im1.repeat(max(F, 1), 1)
        segs = []
        for kf in kfs:
            idx = list(range(kf + 1, kf + K))
            segs.append((torch.cat([self.frames[i] for i in idx], 0), torch.cat([self.mv[i] for i in idx], 0), torch.cat([self.res[i] for i in idx], 0)) if idx else None)

        def run():
            conv = key.key_backbone(imgs)
            flow, scale = key.key_flow(imgs, olds)
            f = feat0
            for i in range(G):
                sl = slice(i * B, (i + 1) * B)
                f = key.key_aggregate(conv[sl], flow[sl], scale[sl], f)
                graphs._post_all(key.key_heads(f, im1), post1, cfg, H, W, 1.0, fg.thresh)
                if segs[i] is None:
                    continue
                d, m, r_ = segs[i]
                if F == K - 1:
                    graphs._post_all(cur.forward(data=d, im_info=imF, feat_key=f, motion_vector=m, res_diff=r_), postF, cfg, H, W, 1.0, fg.thresh)
                else:
                    for j in range(K - 1):
                        sj = slice(j * B, (j + 1) * B)
                        graphs._post_all(cur.forward(data=d[sj], im_info=im1, feat_key=f, motion_vector=m[sj], res_diff=r_[sj]),
                                         post1, cfg, H, W, 1.0, fg.thresh)
        run()                # warm
        torch.cuda.synchronize()
        hip.prof_enable(True, ops=self.OPS)
        hip.prof_read()
        hip.conv_flops_reset(True)
        run()
        torch.cuda.synchronize()
        prof = hip.prof_read()
        self.conv_flops = hip.conv_flops_read()
        self.conv_flops3 = hip.conv_flops_three_products()
        self.conv_flops1 = hip.conv_flops_one_product()
        self.conv_bytes, self.conv_by_kernel = hip.conv_bytes_read(), hip.conv_by_kernel()
        hip.conv_flops_reset(False)
        hip.prof_enable(False)
        C, hw = cfg.network.DFF_FEAT_DIM, (-(-H // 16)) * (-(-W // 16))
        per_seg = ((1 + 2 * F) * C * hw + 2 * F * hw) * 4 * B if F == K - 1 else (K - 1) * warp_bytes(B, C, hw)
        self.warp_bytes_total = G * (warp_bytes(B, C, hw) + (per_seg if K > 1 else 0))
        self.profiled_intervals = G
        return prof

    def many_maps_leg(self, M, iters=10):
        """configs[4]'s HBM-resident regime: M feature maps per launch through lsfa_warp_bilinear (key-path
        epilogue: x scale map; cur-path epilogue: + rnet_conv0(res) + small-net feature) and
        lsfa_aggregate_softmax2_batched, timed by the same event hooks.  3 x M x 9.8 MB per launch."""
        hip, dev = self.hip, self.device
        C = self.cfg.network.DFF_FEAT_DIM
        fh, fw = -(-self.args.height // 16), -(-self.args.width // 16)
        g = torch.Generator(device=dev).manual_seed(5)
        feat = torch.randn((M, C, fh, fw), device=dev, generator=g)
        other = torch.randn((M, C, fh, fw), device=dev, generator=g)
        out = torch.empty_like(feat)
        flow = torch.cat([self.clips[0].motion_vector(4, 1, dev)] * M, 0) + 0.05 * torch.randn((M, 2, fh, fw), device=dev, generator=g)
        res = torch.randn((M, 3, fh, fw), device=dev, generator=g)
        logits = torch.randn((2 * M, 1, fh, fw), device=dev, generator=g)
        rnet_w, rnet_b = self.cur.rnet_w, self.cur.rnet_b
        legs = {'warp_bilinear (x scale map)': lambda: hip.warp_bilinear(feat, flow, mul=other, out=out),
                'warp_bilinear (+res +small-net)': lambda: hip.warp_bilinear(feat, flow, add=other, res=res, res_w=rnet_w,
                                                                             res_b=rnet_b, out=out),
                'aggregate_softmax2_batched': lambda: hip.aggregate_softmax2(feat, other, logits, out=out)}
        result = {}
        for name, fn in legs.items():
            op = 'aggregate' if name.startswith('aggregate') else 'warp_bilinear'
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            hip.prof_enable(True, ops=[op])
            hip.prof_read()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            ms, n = hip.prof_read()[op]
            hip.prof_enable(False)
            nbytes = warp_bytes(M, C, fh * fw)
            result[name] = {"avg_us": round(ms * 1e3 / n, 2), "launches": n, "algorithmic_bytes_per_launch": nbytes,
                            "achieved_GBps": round(nbytes * n / (ms * 1e-3) / 1e9, 1)}
        # what a plain streaming kernel moving the same three tensors gets on this box (torch.mul, 16-byte accesses)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.mul(feat, other, out=out)
        a.record()
        for _ in range(iters):
            torch.mul(feat, other, out=out)
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / iters
        result["reference: torch.mul of the same three tensors"] = {"avg_us": round(us, 2), "achieved_GBps": round(3 * feat.numel() * 4 / us / 1e3, 1)}
        return result

    def _gpu_frames_batched(self, im_info):
        """Frames 1 (key) .. K of clip 0 computed the way the batched pipeline computes them (FramePipeline segment / key_group: the key
        frame's front in one pass with the next key frames', the non-key frames in one pass), eagerly with taps on, each frame cut out of
        its batch: what the parity leg judges is the arithmetic the timed region ran."""
        from oracle import e2e as e2e_mod
        from lsfa_amd.core import graphs
        cfg, K, H, W, key, cur, hip = self.cfg, self.K, self.args.height, self.args.width, self.key, self.cur, self.hip
        one = lambda t: t[:1]
        R, ncls = cfg.TEST.RPN_POST_NMS_TOP_N, cfg.dataset.NUM_CLASSES
        im1 = torch.from_numpy(im_info).to(self.device)
        with torch.no_grad():
            out0 = key.forward(data=one(self.frames[0]), im_info=im1, data_key_old=one(self.frames[0]),
                               feat_key_old=torch.zeros((1, cfg.network.DFF_FEAT_DIM, 1, 1), device=self.device))
            feat0 = out0['choose_feat_output'].clone()
            G = max(1, min(self.key_group, self.nsteps_unique))
            kfs = [1 + j * K for j in range(G)]
            imgs = torch.cat([one(self.frames[k]) for k in kfs], 0)
            olds = torch.cat([one(self.frames[0])] + [one(self.frames[k]) for k in kfs[:-1]], 0)
            conv = key.key_backbone(imgs)
            flow, scale = key.key_flow(imgs, olds)
            key.taps = {}
            feat1 = key.key_aggregate(conv[0:1], flow[0:1], scale[0:1], feat0)
            out1 = key.key_heads(feat1, im1)
            taps1 = dict(key.taps, backbone_feat=conv[0:1])
            key.taps = None
            post1, _ = graphs._alloc_post(1, ncls, R, self.device)
            graphs._post_all(out1, post1, cfg, H, W, 1.0, self.fg.thresh)
            gpu = {1: dict(taps=taps1, out=out1, dets=post1[0][0].cpu().numpy().copy(), counts=post1[1][0].cpu().numpy().copy(), prev=feat0)}
            idx = list(range(2, K + 1))
            F = len(idx)
            if F and self.segment == F:
                cur.taps = {}
                outF = cur.forward(data=torch.cat([one(self.frames[i]) for i in idx], 0), im_info=im1.expand(F, -1).contiguous(), feat_key=feat1,
                                   motion_vector=torch.cat([one(self.mv[i]) for i in idx], 0), res_diff=torch.cat([one(self.res[i]) for i in idx], 0))
                tapsF = dict(cur.taps)
                cur.taps = None
                postF, _ = graphs._alloc_post(F, ncls, R, self.device)
                graphs._post_all(outF, postF, cfg, H, W, 1.0, self.fg.thresh)
                for j, i in enumerate(idx):
                    t, o = e2e_mod.image_of_batch(tapsF, outF, j, F)
                    gpu[i] = dict(taps=t, out=o, dets=postF[0][j].cpu().numpy().copy(), counts=postF[1][j].cpu().numpy().copy(),
                                  key_feat=feat1, mv=one(self.mv[i]), res=one(self.res[i]))
            else:
                for i in idx:
                    cur.taps = {}
                    o = cur.forward(data=one(self.frames[i]), im_info=im1, feat_key=feat1, motion_vector=one(self.mv[i]), res_diff=one(self.res[i]))
                    t = dict(cur.taps)
                    cur.taps = None
                    graphs._post_all(o, post1, cfg, H, W, 1.0, self.fg.thresh)
                    gpu[i] = dict(taps=t, out=o, dets=post1[0][0].cpu().numpy().copy(), counts=post1[1][0].cpu().numpy().copy(),
                                  key_feat=feat1, mv=one(self.mv[i]), res=one(self.res[i]))
        torch.cuda.synchronize()
        return gpu

    def parity_and_cpu_baseline(self, budget_s, want_parity):
        """The oracle's statement of the clip's first frames (torch-CPU convs + C kernels), timed on the
        host (`cpu_baseline`, kind "port") and compared with the GPU's eager run of the same frames (`parity`).
        Clip 0 of this rank, frames 0 (first), 1 (key), 2.. (non-key)."""
        import oracle
        from oracle import graph_ref
        from lsfa_amd.core.graphs import FrameGraphs
        cfg, K, H, W = self.cfg, self.K, self.args.height, self.args.width
        im_info = self.clips[0].im_info()
        npf = lambda t: t.detach().float().cpu().numpy()
        one = lambda t: t[:1]
        f = [npf(one(self.frames[i])) for i in range(0, K + 1)]
        # ---- GPU, eager, taps on, each frame on its own intermediate values -------------------------
        gpu = {}
        batched = hasattr(self.fg, 'lanes') and (self.segment > 0 or self.key_group > 1)
        if want_parity and batched:
            gpu = self._gpu_frames_batched(im_info)
        elif want_parity:
            eg = FrameGraphs(self.key, self.cur, cfg, H, W, self.device, use_graphs=False, prefetch=False, taps=True, batch=1)
            eg.first_frame(one(self.frames[0]))
            eg.capture()
            feat0_gpu = eg.feat.clone()
            d, c, _ = eg.key_frame(one(self.frames[1]))
            gpu[1] = dict(taps=dict(eg.key_taps), out=dict(eg.key_out), dets=d.cpu().numpy().copy(), counts=c.cpu().numpy().copy(),
                          prev=feat0_gpu)
            for i in range(2, K + 1):
                d, c, _ = eg.cur_frame(one(self.frames[i]), one(self.mv[i]), one(self.res[i]))
                gpu[i] = dict(taps=dict(eg.cur_taps), out=dict(eg.cur_out), dets=d.cpu().numpy().copy(),
                              counts=c.cpu().numpy().copy(), key_feat=eg.feat, mv=one(self.mv[i]), res=one(self.res[i]))
            torch.cuda.synchronize()
        # ---- CPU oracle ---------------------------------------------------------------------------
        ref = {}
        ref[0] = graph_ref.key_forward(cfg, self.arg, self.aux, f[0], f[0], np.zeros((1, 1024, 1, 1), np.float32), im_info)
        t0 = time.time()
        ref[1] = graph_ref.key_forward(cfg, self.arg, self.aux, f[1], f[0], ref[0]['choose_feat_output'], im_info)
        oracle.det_postprocess(ref[1]['rois_output'], ref[1]['bbox_pred_reshape_output'][0], ref[1]['cls_prob_reshape_output'][0], H, W, 1.0)
        key_s = time.time() - t0
        nonkey_s, n_nonkey = 0.0, 0
        for i in range(2, K + 1):
            t1 = time.time()
            ref[i] = graph_ref.cur_forward(cfg, self.arg, self.aux, f[i], ref[1]['choose_feat_output'], npf(one(self.mv[i])),
                                           npf(one(self.res[i])), im_info)
            oracle.det_postprocess(ref[i]['rois_output'], ref[i]['bbox_pred_reshape_output'][0], ref[i]['cls_prob_reshape_output'][0], H, W, 1.0)
            nonkey_s += time.time() - t1
            n_nonkey += 1
            if time.time() - t0 > budget_s:
                break
        per_nonkey = nonkey_s / max(n_nonkey, 1)
        per_step = key_s + per_nonkey * (K - 1)
        cpu = {"value": round(K / per_step, 3), "unit": "frames/s", "cores": int(torch.get_num_threads()), "kind": "port",
               "sample": "1 key frame + %d non-key frame(s) of the same clip at %dx%d through oracle/graph_ref.py "
                         "(torch-CPU fp32 convs, C oracle for warp/aggregate/proposal/psroi/nms); %.1f s key, %.2f s per "
                         "non-key frame, extrapolated to one %d-frame interval" % (n_nonkey, W, H, key_s, per_nonkey, K)}
        if not want_parity:
            return cpu, None
        # ---- parity: end to end (each side on its own values), and stage by stage on the GPU's inputs ------
        frames = sorted(i for i in gpu if i in ref and i >= 1)
        # the float64 statement of the same frames: the yardstick both fp32 evaluations are measured against (oracle/e2e.py)
        from oracle import e2e as e2e_mod
        F64 = torch.float64
        d = {0: graph_ref.key_forward(cfg, self.arg, self.aux, f[0], f[0], np.zeros((1, 1024, 1, 1), np.float32), im_info, dtype=F64)}
        d[1] = graph_ref.key_forward(cfg, self.arg, self.aux, f[1], f[0], d[0]['choose_feat_output'], im_info, dtype=F64)
        for i in frames:
            if i >= 2:
                d[i] = graph_ref.cur_forward(cfg, self.arg, self.aux, f[i], d[1]['choose_feat_output'], npf(one(self.mv[i])),
                                             npf(one(self.res[i])), im_info, dtype=F64)
        e2e = []
        for i in frames:
            try:
                e2e.append(e2e_mod.frame_gap(cfg, e2e_mod.gpu_side(cfg, gpu[i]['taps'], gpu[i]['out'], im_info), ref[i], d[i], im_info, H, W))
            except AssertionError as ex:       # Proposal itself differs from the oracle on the GPU's maps: counted below as a failure
                e2e.append({'failures': [str(ex)]})
        forced = 0
        for i in frames[:3]:
            forced += forced_mismatches(cfg, self.arg, gpu[i], im_info, H, W)
        agg = lambda k: max((e[k] for e in e2e if e.get(k) is not None), default=None)
        tot = lambda k: int(sum(e.get(k, 0) for e in e2e))
        worst = {}
        for q in ('rpn_score', 'rpn_delta', 'roi_px', 'box_px', 'cls_prob'):
            rows = [e['err_vs_f64_' + q] for e in e2e if 'err_vs_f64_' + q in e]
            if rows:
                w = max(rows, key=lambda r: r['gpu'])
                worst[q] = {"gpu": w['gpu'], "oracle_fp32": max(r['oracle_fp32'] for r in rows),
                            "worst_frame_ratio": max((r['ratio'] for r in rows if r['ratio'] is not None), default=None),
                            "worst_frame_ratio_beyond_one_ulp": max((r['ratio_beyond_one_ulp'] for r in rows if r.get('ratio_beyond_one_ulp') is not None), default=None),
                            "ulp": rows[0].get('ulp')}
        feat64 = d[1]['choose_feat_output']
        parity = {"frames_compared": frames,
                  "vs": "oracle/graph_ref.py in fp32 AND in float64, un-forced: GPU and oracles each on their own intermediate values; "
                        "criterion oracle/e2e.py: GPU error vs float64 <= %.1f x the fp32 oracle's (+ 1 ulp), ROIs identified by anchor index, "
                        "every pair of proposals the fp32 sides order differently must tie in float64" % e2e_mod.RATIO,
                  "criterion_failures": [x for e in e2e for x in e['failures']][:8],
                  "error_vs_float64": worst,
                  "max_abs_dbox": agg('max_abs_dbox'), "max_abs_dscore": agg('max_abs_dscore'),
                  "roi_rows_in_a_different_order": tot('roi_displaced'), "of_which_float64_ties": tot('roi_displaced_ties'),
                  "roi_kept_on_one_side_only": tot('roi_only_one_side'), "of_which_iou_threshold_ties": tot('roi_iou_ties'),
                  "rois_on_a_psroi_rounding_boundary": tot('unstable_rois'),
                  "rois_compared": tot('rois_compared'),
                  "survivor_mismatch": tot('survivor_mismatch'), "survivors": tot('survivors'),
                  "feature_rel_err_key_frame": rel_err(npf(gpu[1]['out']['choose_feat_output']), ref[1]['choose_feat_output']),
                  "feature_rel_err_key_frame_vs_float64": {"gpu": rel_err(npf(gpu[1]['out']['choose_feat_output']), feat64),
                                                           "oracle_fp32": rel_err(ref[1]['choose_feat_output'], feat64)},
                  "contractions": self.args.dtype,
                  "note": ("dense contractions in bf16 on the GPU vs the fp32 / float64 oracle graphs: outputs differ by bf16 round-off "
                           "(feature_rel_err_key_frame), so the fp32 criterion is expected to fail; the bit-exactness claim "
                           "in this mode is the hand-written-stage line below") if self.args.dtype != 'f32' else
                          "fp32 in / fp32 accumulate on both sides; the GPU's convolutions form every fp32 product from split operands on the "
                          "matrix pipe (two fp16 pieces + a power-of-two scale, three products; or three bf16 pieces, six products) and sum "
                          "in MFMA tile order, the oracle in the CPU library's order",
                  "handwritten_stage_mismatches_on_gpu_inputs": int(forced),
                  "handwritten_stages_checked": "warp, aggregate, proposal, psroi+avg+softmax, det_postprocess of frames %s "
                                                "(bit-exact = 0 mismatching elements)" % frames[:3]}
        # r5: mAP agreement over three intervals (30 frames), the GPU's rows from the timed region's own path (hipGraph pipeline, batched passes)
        try:
            parity["map_vs_oracle"] = self.map_vs_oracle(ref, intervals=min(3, self.nsteps_unique))
        except Exception as e:       # a reported extra
            parity["map_vs_oracle"] = "failed: %r" % (e,)
        return cpu, parity

    def map_vs_oracle(self, known, intervals=3):
        """north_star's "mAP within 0.1 of the reference", in the only form available without trained weights (oracle/map_check.py): VID mAP@0.5
        of this GPU's detections of frames 1 .. intervals*K against the fp32 oracle's most confident detections of the same frames.  The GPU's
        rows are produced by the pipeline the timed region runs (re-primed on frame 0, hipGraph replay, batched passes, this run's dtype)."""
        from oracle import map_check
        K, cfg = self.K, self.cfg
        npf = lambda t: t[:1].detach().float().cpu().numpy()
        im_info = self.clips[0].im_info()
        rows_ref = map_check.oracle_rows(cfg, self.arg, self.aux, lambda f: npf(self.frames[f]), lambda f: npf(self.mv[f]), lambda f: npf(self.res[f]),
                                         im_info, K, intervals, known={i: known[i] for i in known})
        self.fg.first_frame(self.frames[0])
        rows = []
        for s in range(intervals):
            self.step(s, end=intervals)
            if hasattr(self.fg, 'flush'):
                self.fg.flush()
            torch.cuda.synchronize()
            counts = self.host_counts
            for k in range(K):
                for j in range(1, self.ncls):
                    n = int(counts[k, 0, j])
                    if n:
                        d = self.host_dets_of(k)[0, j, :n].numpy()
                        r = np.empty((n, 7), np.float64)
                        r[:, 0], r[:, 1], r[:, 2], r[:, 3:] = 1 + s * K + k, j, d[:, 4], d[:, :4]
                        rows.append(r)
        rows_gpu = np.vstack(rows) if rows else np.zeros((0, 7), np.float64)
        out = map_check.map_vs_oracle(rows_gpu, rows_ref, range(1, intervals * K + 1), self.ncls)
        out["contractions"] = self.args.dtype
        return out


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def forced_mismatches(cfg, arg, g, im_info, h, w):
    """Elements of one GPU frame's hand-written stages that differ from the oracle run on the GPU's own inputs to
    that stage (0 = every stage bit-exact)."""
    import oracle
    npf = lambda t: t.detach().float().cpu().numpy()
    taps, out = g['taps'], g['out']
    bad = 0
    if 'prev' in g:      # key frame
        warp = oracle.warp_bilinear(npf(g['prev']), npf(taps['flow']), mul=npf(taps['scale_map']))
        bad += int((warp != npf(taps['warp'])).sum())
        agg = oracle.aggregate_softmax2(warp, npf(taps['backbone_feat']), npf(taps['nq_logits']))
        bad += int((agg != npf(out['choose_feat_output'])).sum())
    else:
        want = oracle.warp_bilinear(npf(g['key_feat']), npf(g['mv']), add=npf(taps['small_feat']), res=npf(g['res']),
                                    res_w=arg['rnet_conv0_weight'], res_b=arg['rnet_conv0_bias'])
        bad += int((want != npf(out['conv_feat'])).sum())
    rois, _ = oracle.proposal(npf(taps['rpn_cls_prob']), npf(taps['rpn_bbox_pred']), im_info, cfg.network.RPN_FEAT_STRIDE,
                              cfg.network.ANCHOR_SCALES, cfg.network.ANCHOR_RATIOS, cfg.TEST.RPN_PRE_NMS_TOP_N,
                              cfg.TEST.RPN_POST_NMS_TOP_N, cfg.TEST.RPN_NMS_THRESH, cfg.TEST.RPN_MIN_SIZE)
    bad += int((rois != npf(out['rois_output'])).sum())
    cls_prob, _, bbox = oracle.rfcn_head(npf(taps['cls_map']), npf(taps['box_map']), rois)
    bad += int((cls_prob != npf(out['cls_prob_reshape_output'])[0]).sum()) + int((bbox != npf(out['bbox_pred_reshape_output'])[0]).sum())
    wd, wc, _ = oracle.det_postprocess(npf(out['rois_output']), npf(out['bbox_pred_reshape_output'])[0],
                                       npf(out['cls_prob_reshape_output'])[0], h, w, 1.0, nms_thresh=cfg.TEST.NMS,
                                       max_per_image=cfg.TEST.max_per_image, class_agnostic=cfg.CLASS_AGNOSTIC)
    bad += int((wc != g['counts']).sum())
    for j in range(1, len(wc)):
        bad += int((wd[j, :wc[j]] != g['dets'][j, :wc[j]]).sum()) if wc[j] == g['counts'][j] else 0
    return bad


def load_traffic(key):
    try:
        with open(TRAFFIC_FILE) as f:
            return json.load(f).get(key, {}).get('hbm_bytes_per_launch')
    except (OSError, ValueError):
        return None


def load_launch_counts(args):
    """Kernel launches per key / non-key frame, counted from the rocprofv3 kernel trace of this configuration
    (tools/summarize_prof.py writes profiles/launch_counts.json); None when no trace of it is committed."""
    try:
        with open(os.path.join(ROOT, 'profiles', 'launch_counts.json')) as f:
            d = json.load(f)
        return d.get("%dx%d,interval=%d,clips=%d,%s" % (args.width, args.height, args.interval, args.clips, args.dtype))
    except (OSError, ValueError):
        return None


DUMP_LIMIT_BYTES = 64 * 10 ** 6


def dump_outputs(d, outputs):
    """--dump-outputs: every array as d/<name>.npy.  Above DUMP_LIMIT_BYTES in all, each array is cut to a fixed, seeded sample of its
    rows (the last axis kept whole), in their order, its share of the limit in proportion to its size."""
    os.makedirs(d, exist_ok=True)
    total = sum(a.nbytes for a in outputs.values())
    budget = DUMP_LIMIT_BYTES - 1024 * len(outputs)          # (room for the .npy headers)
    for name, a in outputs.items():
        if total > budget:
            rows = a.reshape(-1, a.shape[-1])
            n = max(1, len(rows) * budget // total)
            a = rows[np.sort(np.random.default_rng(0).choice(len(rows), n, replace=False))]
        np.save(os.path.join(d, name + '.npy'), a)


def main():
    args = parse()
    parity_failed = False
    from lsfa_amd import hip as _hip
    if os.environ.get('LSFA_PROPOSAL_PLAN'):      # lab: 'chip' | 'chip-box-sweep' | 'single' (process-wide; identical results)
        _hip.proposal_set_plan(os.environ['LSFA_PROPOSAL_PLAN'])
    if _hip.LAB_SKIP:
        # ablation (tools/lab/tail_ablation.sh): launches are dropped, detections are garbage - the line says so and carries no parity and no
        # CPU baseline
        if _hip.LAB_SKIP_NMS:
            _hip.proposal_set_plan('lab-no-nms')
        args.no_parity = args.no_cpu_baseline = True
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    # LSFA_BENCH_FORCE_DIST=1 (tests/test_multirank_gpu.py): take the distributed branch at world size 1 too, so that a one-GPU box executes
    # every line the N-GPU run will - RCCL initialisation, device barriers, all_reduce / all_gather on device tensors - except N > 1 itself
    distributed = world > 1 or (os.environ.get('LSFA_BENCH_FORCE_DIST') == '1' and 'RANK' in os.environ)
    # test hook (one-GPU boxes): LSFA_BENCH_BACKEND=gloo LSFA_BENCH_ONE_DEVICE=1 runs every rank on cuda:0 and
    # the collectives on CPU tensors, to exercise the N>1 control flow without N GPUs
    backend = os.environ.get('LSFA_BENCH_BACKEND', 'nccl')
    if os.environ.get('LSFA_BENCH_ONE_DEVICE') == '1':
        local_rank = 0
    if distributed:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        torch.cuda.set_device(local_rank)
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=torch.device('cuda', local_rank))
        else:
            dist.init_process_group(backend)
    coll_dev = ('cuda:%d' % local_rank) if backend == 'nccl' else 'cpu'
    device = 'cuda:%d' % local_rank
    torch.cuda.set_device(local_rank)
    r = Runner(args, rank, device)
    r.prime()

    if args.eager_loop > 0:
        # profiling aid: the serial eager loop alone (rocprofv3 --kernel-trace / --pmc around it give per-kernel durations and MFMA-busy of the
        # SAME launches the `roofline` object is computed from)
        prof = None
        for _ in range(args.eager_loop):
            prof = r.eager_profile_batched(args.warmup) if (hasattr(r.fg, 'lanes') and (r.segment > 0 or r.key_group > 1)) else r.eager_profile_step(args.warmup)
        conv_ms, conv_n = prof.get('conv_nhwc', (0.0, 0))
        conv_fl, _ = r.conv_flops
        print(json.dumps({"config": {"workload": "eager loop x%d: %d interval(s) per pass, key fronts x%d, segments of %d" % (args.eager_loop, getattr(r, 'profiled_intervals', 1), r.key_group, r.segment)},
                          "roofline": {"achieved": round(conv_fl / (conv_ms * 1e-3) / 1e12, 1) if conv_ms else None, "launches": conv_n,
                                       "avg_us": round(conv_ms * 1e3 / max(conv_n, 1), 2), "by_kernel": r.conv_by_kernel}}))
        return

    def drain():
        if hasattr(r.fg, 'flush'):
            r.fg.flush()             # the pipeline queues a segment when the next key frame arrives: queue the last one
        torch.cuda.synchronize()     # device-wide: drains every stream of the frame pipeline
        if getattr(r, 'host_inputs', False):
            r._up_key.clear()        # (uploads issued ahead for a look-ahead that the end of the run cut short)
            r._up_rest.clear()

    # setup, untimed and not part of the W warm-up steps: keep the device under the workload's load until its clocks have settled
    settle_steps, t_settle = 0, time.perf_counter()
    # bursts of 32 intervals (~0.19 s) between drains: with bursts of 8 (46 ms) the device never reached its sustained state during setup
    # and went through the transition - three to six intervals of 7.5-9.7 ms instead of 5.6 - inside the first timed region in half of
    # the runs (profiles/r3/ab_experiments.txt section 9, tools/trace_regions.py)
    # ... and never shorter than the timed region itself: the first run of K consecutive intervals without a drain lets the host queue deeper than
    # any burst before it, and the runtime grows its command / signal pools ONCE, inside that run (r5: the first 100-interval region read 6 % under
    # its two repeats - 18 ms - while 20-interval regions and the throttled upload mode did not)
    settle_drain = int(os.environ.get('LSFA_BENCH_SETTLE_DRAIN', str(max(32, args.steps))))
    burst = settle_drain or max(32, args.steps)
    while time.perf_counter() - t_settle < args.settle_s:
        r.step(settle_steps, end=(settle_steps // burst + 1) * burst)        # a burst is one run of consecutive steps
        settle_steps += 1
        if settle_drain and settle_steps % settle_drain == 0:
            drain()
    if settle_steps % burst:
        # the time limit cut the last burst short: the fronts it computed ahead are dropped (FramePipeline.first_frame-style reset)
        if hasattr(r.fg, 'drop_fronts'):
            r.fg.drop_fronts()
    if settle_drain:
        drain()
    # the clip starts over from its first frame: the key features are recurrent, and the W + N steps below then depend on nothing the
    # time-limited settle left behind - the same arguments give the same outputs in every run (--dump-outputs)
    r.fg.first_frame(r.frames[0])
    for s in range(args.warmup):
        r.step(s, end=args.warmup)
    drain()

    def barrier():
        if distributed:
            dist.barrier(device_ids=[local_rank]) if backend == 'nccl' else dist.barrier()

    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(args.warmup, args.warmup + args.steps):
        r.step(s, end=args.warmup + args.steps)
    drain()
    barrier()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:          # before anything else runs the pipeline again
        dump_outputs(args.dump_outputs, r.last_step_outputs())
    # --full, run-to-run spread: the same K steps twice more, each bracketed like the timed region above (`value` stays the FIRST
    # region's; the driver's fresh-box figure and a builder's warm-box one have differed by ~10 %: this makes that visible)
    repeats = [elapsed]
    host_enqueue = []            # how long the host loop of a repeat took to QUEUE its K steps (the rest of the region is waiting for the GPU)
    for _ in range(2 if args.full and not args.no_spread else 0):
        barrier()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for s in range(args.warmup, args.warmup + args.steps):
            r.step(s, end=args.warmup + args.steps)
        host_enqueue.append(time.perf_counter() - t1)
        drain()
        barrier()
        repeats.append(time.perf_counter() - t1)
    batched = hasattr(r.fg, 'lanes') and (r.segment > 0 or r.key_group > 1)
    extras = args.full and rank == 0             # the untimed legs of --full
    prof = (r.eager_profile_batched(args.warmup) if batched else r.eager_profile_step(args.warmup)) if extras else None
    # r5: the streaming figure beside the headline: the same clip frame by frame (one extra short region; rank 0, untimed by the driver)
    other_inputs = None
    if getattr(r, 'host_inputs', False) and extras and not args.no_frame_by_frame:
        try:
            other_inputs = r.other_inputs_region(args.steps, args.warmup)
        except Exception as e:
            other_inputs = "failed: %r" % (e,)
    exact = None
    if extras and not args.no_frame_by_frame and args.lanes > 0:
        try:
            exact = r.exact_fp32_region()
        except Exception as e:
            exact = "failed: %r" % (e,)
    fbf = None
    if batched and extras and not args.no_frame_by_frame:
        try:
            fbf = r.frame_by_frame_region(args.steps, args.warmup)
        except Exception as e:          # a reported extra: never lose the bench line to it
            fbf = "failed: %r" % (e,)

    uploads_extra = bool(getattr(r, 'host_inputs', False)) and not getattr(args, 'host_inputs', False)      # `value`: resident inputs; the extra region: uploads
    # an overflow of the fp16 form's scale anywhere in the run is an error, not a number (outside the timed regions: it synchronises)
    r.key.check_status()
    r.cur.check_status()
    multi = None
    if distributed:
        own = [float(v) for v in repeats]
        tt = torch.tensor(repeats, device=coll_dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        repeats = [float(v) for v in tt.tolist()]
        elapsed = repeats[0]
        # what every rank saw: its own time for the first region (-> per-rank frames/s) and which device it ran on
        mine = torch.tensor([own[0], float(local_rank), float(rank)], device=coll_dev, dtype=torch.float64)
        seen = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(seen, mine)
        # the final gather of detections - the one data-path collective (RCCL over xGMI): the benchmarked clip's detection rows of the
        # last interval, [frame, class, score, x1, y1, x2, y2] per row, ragged per rank (lsfa_amd/core/parallel.py gather_rows)
        from lsfa_amd.core.parallel import gather_rows
        rows = r.last_interval_rows()
        if backend == 'nccl':
            torch.cuda.synchronize()
        dist.barrier(device_ids=[local_rank]) if backend == 'nccl' else dist.barrier()
        tg = time.perf_counter()
        all_rows = gather_rows(rows, torch.device(coll_dev))
        if backend == 'nccl':
            torch.cuda.synchronize()
        gather_s = time.perf_counter() - tg
        total_dets = int(all_rows.shape[0])
        per_rank_frames = args.clips * args.steps * args.interval
        multi = {"backend": "rccl (torch.distributed 'nccl')" if backend == 'nccl' else backend,
                 "rccl_ranks_seen": world if backend == 'nccl' else 0, "ranks_seen": world,
                 "per_rank": [{"rank": int(v[2].item()), "device": int(v[1].item()), "seconds": round(float(v[0].item()), 6),
                               "frames_per_s": round(per_rank_frames / float(v[0].item()), 2)} for v in seen],
                 "final_gather": {"rows": total_dets, "bytes": int(all_rows.nbytes), "seconds": round(gather_s, 6),
                                  "what": "detection rows of every rank's last interval, counts first then one padded all_gather"},
                 "collectives_in_timed_region": 0}
    else:
        total_dets = int(r.host_counts.sum().item())

    if rank == 0:
        K, B = args.interval, args.clips
        frames = world * B * args.steps * K
        fh, fw = int(np.ceil(args.height / 16.0)), int(np.ceil(args.width / 16.0))
        C = r.cfg.network.DFF_FEAT_DIM
        if args.full:
            # ---- roofline: the HBM-bound hand-written kernel (warp), live from HIP events ---------------------
            warp_ms, warp_n = prof['warp_bilinear']
            bytes_per_launch = warp_bytes(B, C, fh * fw)
            if getattr(r, 'warp_bytes_total', None):       # batched pipeline: launches of one map (key frames) and of a segment's maps (one shared key feature)
                bytes_per_launch = r.warp_bytes_total // max(warp_n, 1)
            achieved = bytes_per_launch * warp_n / (warp_ms * 1e-3) / 1e9 if warp_ms > 0 else 0.0
            ops = {k: {"avg_us": round(v[0] * 1e3 / v[1], 2), "launches": v[1], "total_us": round(v[0] * 1e3, 1)}
                   for k, v in prof.items() if v[1]}
            hand_total = sum(o["total_us"] for o in ops.values()) or 1.0
            dom = max(ops, key=lambda k: ops[k]["total_us"]) if ops else None
            # which kernel lsfa_warp_bilinear runs for this shape (warp.hip's predicate: planes of 1,024-4,096 even pixels go through LDS)
            staged = (fh * fw) % 2 == 0 and 1024 <= fh * fw <= 4096 and os.environ.get('LSFA_WARP_VARIANT', 'auto') != 'gather'
            warp_kernel = ("warp_staged_kernel (lsfa_warp_bilinear: MV/flow warp + fused epilogue; planes staged in LDS by DMA)" if staged else
                           "warp_kernel (lsfa_warp_bilinear: MV/flow warp + fused epilogue; gather form: plane size outside the LDS-staged kernel's range)")
            mixed = bool(getattr(r, 'warp_bytes_total', None))
            maps_label = ("a MIX of launches: %d map(s) per key-frame launch (flow warp) and %d maps per segment launch (MV warp, one shared key feature); "
                          "algorithmic_bytes_per_launch is the mean over both kinds" % (B, B * r.segment)) if mixed and getattr(r, 'segment', 0) > 0 \
                else "%d map(s) per launch" % B
            roof_hbm = {"bound": "hbm", "kernel": "%s, %s" % (warp_kernel, maps_label),
                    "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(achieved / HBM_PEAK_GBS, 4),
                    "traffic": load_traffic("warp_bilinear:N=%d,C=%d,H=%d,W=%d" % (B, C, fh, fw)),
                    "launches": warp_n, "avg_us": round(warp_ms * 1e3 / max(warp_n, 1), 2),
                    "algorithmic_bytes_per_launch": bytes_per_launch,
                    "measured": "HIP events around each launch on its stream, same frames re-issued eagerly right after the "
                                "timed region (graph replays carry no per-launch events); traffic = FETCH_SIZE x2 + WRITE_SIZE "
                                "from the rocprofv3 PMC passes under profiles/ for this shape, null if none was taken",
                    "note": "%.0f MB per launch: resident in the 256 MiB Infinity Cache, so this is cache bandwidth against "
                            "the HBM peak; --maps-per-launch 32 gives the HBM-resident figure" % (bytes_per_launch / 1e6)}
            # ---- roofline of the dominant hand-written kernel: the split-bf16 convolution (matrix pipe) -----------------
            conv_ms, conv_n = prof.get('conv_nhwc', (0.0, 0))
            conv_fl, conv_calls = getattr(r, 'conv_flops', (0.0, 0))
            if conv_n and conv_fl > 0:
                tf = conv_fl / (conv_ms * 1e-3) / 1e12
                # matrix-pipe peak for this mix of calls: six bf16 products per fp32 product (2500 / 6), three fp16 ones on the calls
                # that ran the two-piece form (2500 / 3): harmonic mix by FLOPs
                fl3 = float(getattr(r, 'conv_flops3', 0.0))
                fl1 = float(getattr(r, 'conv_flops1', 0.0))
                fl6 = conv_fl - fl3 - fl1
                mfma_work = 6 * fl6 + 3 * fl3 + fl1          # matrix-instruction FLOPs actually issued
                mix_peak = conv_fl / (mfma_work / MFMA_BF16_PEAK_TFLOPS)
                roof = {"bound": "mfma", "kernel": "the split-operand convolution family behind lsfa_conv_fwd (ring / direct kernels + their reduce passes): "
                        "every convolution of ResNet-101 + DCN, feat_conv_3x3, the small net, fuse_reduce_add, FlowNet, the Nq net; %d calls of %d interval(s)%s" %
                        (conv_n, getattr(r, 'profiled_intervals', 1), " computed the way the pipeline batches them (key fronts x%d, segments of %d frames)" % (r.key_group, r.segment) if batched else ""),
                        "achieved": round(tf, 1), "peak": round(mix_peak, 1), "unit": "TFLOP/s",
                        "frac": round(tf / mix_peak, 4),
                        "flops_share_by_products_per_fp32_product": {"six (three bf16 pieces)": round(fl6 / conv_fl, 3), "three (two fp16 pieces)": round(fl3 / conv_fl, 3),
                                                                      "one (bf16 mode)": round(fl1 / conv_fl, 3)},
                        "frac_of_six_product_peak": round(tf / MFMA_SPLIT_PEAK_TFLOPS, 4),     # what rounds 1-2 quoted as `frac` (every call on six products)
                        "traffic": load_traffic("conv_split:%dx%d,interval=%d,%s%s" % (args.width, args.height, args.interval, args.dtype,
                                                                                      "" if args.clips == 1 else ",clips=%d" % args.clips)),
                        "launches": conv_n, "avg_us": round(conv_ms * 1e3 / conv_n, 2),
                        "algorithmic_flops_per_launch": round(conv_fl / max(conv_n, 1)),       # x launches / (avg_us x launches) = achieved
                        "algorithmic_bytes_per_launch": round(float(getattr(r, 'conv_bytes', 0.0)) / max(conv_n, 1)),
                        "flop_counted_calls": conv_calls,      # == launches: FLOPs and time cover the same lsfa_conv_fwd / lsfa_deconv4x4s2_crop_fwd calls (FlowNet included)
                        "by_kernel": getattr(r, 'conv_by_kernel', None),
                        "mfma_work": {"achieved": round(mfma_work / (conv_ms * 1e-3) / 1e12, 1), "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s"},
                        "fp32_mfma_pipe_peak": 157.3,
                        "measured": "HIP events around each lsfa_conv_fwd / lsfa_deconv4x4s2_crop_fwd call (convolution kernel + its reduce pass) re-issued "
                                    "eagerly after the timed region; algorithmic FLOPs = 2*M*N*K and algorithmic bytes = every operand once (input channels read, "
                                    "packed weights, output, residual, stored second output) summed over the SAME calls; by_kernel = the same calls by the kernel "
                                    "instantiation the launch plan picks (lsfa_conv_plan_query; tools/conv_family_roofline.py joins it with the rocprofv3 "
                                    "kernel trace and MFMA-busy counters -> profiles/r5/conv_family_roofline.csv); traffic = HBM bytes "
                                    "per call of the kernel family (FETCH_SIZE x2 + WRITE_SIZE, separate rocprofv3 PMC passes over the eager loop, "
                                    "profiles/traffic.json), null if no profile of this configuration is committed",
                        "note": "fp32 in / fp32 accumulate; an fp32 product costs three fp16 matrix instructions' worth (two-piece form: the fp32 "
                                "path's default, peak for fp32-equivalent FLOPs 2500 / 3 = 833.3), six bf16 ones (three-piece form: FlowNet, 416.7) "
                                "or one (bf16 mode, 2500); `peak` is the dense bf16 / fp16 matrix peak divided by the FLOP-weighted products per "
                                "fp32 product of this mix; the fp32 matrix instructions peak at 157.3"}
            else:
                roof = roof_hbm
        line = {
            "metric": "frames/sec/GPU at 1000x600 key_interval=10 (whole-job frames/s)",
            "value": round(frames / elapsed, 3), "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "settle_s": args.settle_s, "settle_steps": settle_steps,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": ("ABLATION, NOT A RESULT (LSFA_LAB_SKIP=%s: launches dropped): " % ",".join(sorted(_hip.LAB_SKIP)) if _hip.LAB_SKIP else "") +
                                   "dff_rfcn ResNet-101 LSFA (DCN + FlowNet + Nq + small net + R-FCN), %d clip%s per GPU%s, "
                                   "key_interval=%d, %dx%d, %s; step = 1 key + %d non-key frames per clip" %
                                   (B, "" if B == 1 else "s", "" if B == 1 else " in lock-step (batch axis)", K, args.width,
                                    args.height, args.dtype, K - 1),
                       "frames_per_step": K * B, "ms_per_frame": round(elapsed / (args.steps * K * B) * 1e3, 3),
                       "parallelism": "clip-parallel x%d" % world, "detections_last_interval": total_dets,
                       "launch": "eager" if args.no_graph else "hipGraph replay per frame",
                       "setup_before_warmup": "graph capture + %d untimed interval(s) over %.1f s (clock settle), then the %d warm-up steps"
                                              % (settle_steps, args.settle_s, args.warmup),
                       "gemm_solutions": "not applicable: no library GEMM or convolution is left in the frame path (r4)",
                       "pipeline": ("key stream%s + %d non-key lanes%s" % (
                           "" if args.no_flow_stream else " + FlowNet/tail stream", args.lanes,
                           ", next key frame queued ahead of the segment before it" if args.lookahead else ""))
                       if args.lanes > 0 else "serial",
                       "batching": ("one clip, frames in display order; the %d non-key frames of a segment go through the network in one pass (batch axis = "
                                    "frames, like the reference's batch test symbol) and the image-only half (backbone, FlowNet) of %d consecutive key "
                                    "frames in one pass (look-ahead of %d frames%s); "
                                    "--segment 0 --key-group 1 = frame by frame" %
                                    (r.segment, r.key_group, (r.key_group - 1) * K,
                                     "; after the pipeline ran empty the first passes are %s key frames" % args.ramp if args.ramp.strip() else "")) if batched else "none: one frame per pass"},
            "inputs": (("resident in HBM as fp32 when the timed region starts (the bench contract: `value` never includes PCIe); `value_uploaded_inputs` is the "
                        "PCIe-inclusive rate of the same pipeline" if uploads_extra else
                        "host-pinned, uploaded in region (--host-inputs): per interval one pinned block (uint8 BGR frames as a decoder hands them over + fp32 motion "
                        "vectors / residuals, dff_rfcn/core/loader.py:131-141) -> one H2D copy -> transform (lib/utils/image.py:296-308) on the GPU; uploads run "
                        "ahead of the frames by the key group's look-ahead; `value_resident_inputs` is the contract's figure")
                       if getattr(r, 'host_inputs', False)
                       else "resident in HBM as fp32 before the timed region (no --full nor --host-inputs, --resident-inputs, or a serial / "
                            "non-pipelined run)"),
            "multi_gpu": multi,
        }
        if args.full:
            line.update({
                "value_spread": {"min": round(frames / max(repeats), 3), "max": round(frames / min(repeats), 3), "repeats": len(repeats),
                                 "values": [round(frames / t, 3) for t in repeats],
                                 "note": "the timed region run %d times back to back; `value` is the first" % len(repeats),
                                 "host_enqueue_share_of_repeats": [round(h / t, 3) for h, t in zip(host_enqueue, repeats[1:])]},
                "value_resident_inputs": (round(frames / elapsed, 3) if uploads_extra or not getattr(r, 'host_inputs', False)
                                          else (round(other_inputs, 3) if isinstance(other_inputs, float) else other_inputs)),
                "value_uploaded_inputs": ((round(other_inputs, 3) if isinstance(other_inputs, float) else other_inputs) if uploads_extra
                                          else (round(frames / elapsed, 3) if getattr(r, 'host_inputs', False) else None)),
                "value_other_inputs_regions": getattr(r, 'other_inputs_rates', None),
                "value_uploaded_inputs_note": "frames/s of this GPU with the inputs starting in pinned HOST memory: per interval one pinned block (uint8 BGR frames as a "
                                              "decoder hands them over + fp32 motion vectors / residuals, dff_rfcn/core/loader.py:131-141) -> one H2D copy inside the "
                                              "region -> transform (lib/utils/image.py:296-308) on the GPU, uploads ahead of the frames by the key group's look-ahead; "
                                              "the extra region (rank 0: its own 0.75 s settle, then the region twice - `value_other_inputs_regions` - the second reported), or `value` itself under --host-inputs",
                "value_exact_fp32": (round(exact, 3) if isinstance(exact, float) else exact),
                "value_exact_fp32_note": "frames/s, frame by frame, with every convolution on the EXACT fp32 matrix instructions (v_mfma_f32_32x32x2_f32, "
                                         "157 TFLOP/s peak; Executor pieces = 0, a reference evaluation): what the two-fp16-piece form is compared with in "
                                         "tests/test_parity_fullres_gpu.py::test_two_fp16_pieces_against_exact_fp32_products_at_1000x600; compare with value_frame_by_frame",
                "value_frame_by_frame": (round(fbf, 3) if isinstance(fbf, float) else fbf),
                "value_frame_by_frame_note": "frames/s of this GPU for the same clip with one frame per pass (--segment 0 --key-group 1: no look-ahead, the "
                                             "streaming case; inputs as for `value`), %d timed intervals after its own graph capture + 0.5 s settle + %d warm-up intervals; null when the "
                                             "headline configuration is itself unbatched" % (args.steps, args.warmup),
                "roofline": roof,
                "roofline_hbm_kernel": roof_hbm,
                "roofline_handwritten_ops": {
                    "per_op": ops, "dominant_by_time": dom,
                    "dominant_share_of_handwritten_time": round(ops[dom]["total_us"] / hand_total, 3) if dom else None,
                    "note": "one eager interval; proposal / det_postprocess / rfcn_head are latency-bound by construction "
                            "(0.5 MB, 53 KB, 18 MB of algorithmic bytes): judged in us, not as a fraction of HBM peak"},
            })
            if args.maps_per_launch > 0:
                M = args.maps_per_launch
                mm = r.many_maps_leg(M)
                w = mm['warp_bilinear (x scale map)']
                line["roofline_single_map"] = roof_hbm
                line["roofline_mfma_kernel"] = roof
                del line["roofline_hbm_kernel"]
                line["roofline"] = {"bound": "hbm", "kernel": "%s, %d maps per launch (x scale map epilogue)" % (warp_kernel, M),
                                    "achieved": w["achieved_GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                    "frac": round(w["achieved_GBps"] / HBM_PEAK_GBS, 4),
                                    "traffic": load_traffic("warp_bilinear:N=%d,C=%d,H=%d,W=%d" % (M, C, fh, fw)),
                                    "launches": w["launches"], "avg_us": w["avg_us"],
                                    "algorithmic_bytes_per_launch": w["algorithmic_bytes_per_launch"],
                                    "measured": "HIP events around each launch, untimed leg after the frame loop; %d MB per launch "
                                                "(> 256 MiB Infinity Cache: HBM-resident)" % (w["algorithmic_bytes_per_launch"] // 1000000),
                                    "other_kernels_same_size": {k: v for k, v in mm.items() if k != 'warp_bilinear (x scale map)'}}
        if (args.height, args.width) == (600, 1000):
            # algorithmic FLOPs of the dense contractions, key frame 392.0 G, non-key frame 17.3 G
            gflop = (392.0 + 17.3 * (K - 1)) * B
            peak = round(MFMA_BF16_PEAK_TFLOPS / 3.0, 1) if args.dtype == 'f32' else MFMA_BF16_PEAK_TFLOPS
            tf = gflop / (elapsed / args.steps) / 1e3
            line["roofline_dense"] = {"bound": "mfma", "scope": "SURVEY.md 8(d)'s algorithmic FLOPs of one interval's dense contractions / the timed region's step "
                                      "time (whole pipeline, everything overlapped), against the same peak as `roofline`: the dense 16-bit matrix peak / 3 "
                                      "products per fp32 product (f32) or / 1 (bf16)", "achieved": round(tf, 1), "peak": peak,
                                      "unit": "TFLOP/s", "frac": round(tf / peak, 4), "gflop_per_step": round(gflop, 1)}
        if args.full and not (args.no_cpu_baseline and args.no_parity):
            try:
                cpu, parity = r.parity_and_cpu_baseline(args.cpu_budget_s, not args.no_parity)
                if not args.no_cpu_baseline:
                    line["cpu_baseline"] = cpu
                if parity is not None:
                    line["parity"] = parity
            except Exception as e:  # the checker legs are reported extras; never lose the bench line to them
                line["cpu_baseline"] = {"value": None, "unit": "frames/s", "cores": int(torch.get_num_threads()),
                                        "kind": "port", "sample": "failed: %r" % (e,)}
        launches = load_launch_counts(args)
        if launches is not None:
            line["kernel_launches"] = launches
        print(json.dumps(line))
        bad = (line.get("parity") or {}).get("handwritten_stage_mismatches_on_gpu_inputs")
        if bad:
            sys.stderr.write("bench.py: %d elements of the hand-written stages differ from the oracle on the GPU's own inputs\n" % bad)
            parity_failed = True
    if distributed:
        dist.barrier(device_ids=[local_rank]) if backend == 'nccl' else dist.barrier()
        dist.destroy_process_group()
    if parity_failed:
        sys.exit(3)


if __name__ == '__main__':
    main()
