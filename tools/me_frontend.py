#!/usr/bin/env python
"""Time of the motion-estimation front end for one 1000x600 frame next to the non-key frame it feeds (device events, same process):

    luma_u8, mv_estimate at R = 16 and 32          back to back on one stream, eager and as a replayed graph of `iters` calls
    next_frame + network_inputs                    hip.MotionEstimator: luma, search, accumulation, field, residual, transform_mv_res
    one non-key frame                              tools/curframe_only.py's loop body (small net + MV warp + heads + detection post-processing)

The condition to read off: the front end for one frame costs less than the non-key frame.  --kernels-only runs just the front-end
launches a few times (for `rocprofv3 --kernel-trace --stats -- python tools/me_frontend.py --kernels-only`).  Prints one JSON object.

--segment runs the segment leg instead (profiles/r7/me_segment.txt), under a time limit of its own (--time-limit seconds, enforced in
this process): a key frame + nine frames at R = 16 and 32, one clip,

    per-frame graph        MotionEstimator.key_frame, then next_frame + network_inputs nine times, captured as ONE graph
    segment graph          SegmentMotionEstimator.segment of the same ten frames: luma of the stack, chain search, inputs
    each new kernel alone  mv_estimate_chain (against nine mv_estimate launches) and mv_segment_inputs

The two forms are replayed alternately, round by round, in one process; the condition to read off is that the segment form is not
slower than the per-frame graph beyond the min-to-max spread the same run shows.

--segment --levels L [--size WxH] runs the pyramid leg instead (profiles/r8/me_pyramid.txt): the segment form with the full search at
R = 16 and R = 32 and with the pyramid search (L = 1: R = 16; L = 2: R = 8 and R = 16; --refine r, default 2) in the same alternating
rounds, then each new launch alone: luma_pyramid, the top-level search, every refinement level.  The condition to read off: a pyramid
configuration whose reach is at least 32 takes no longer per segment than the full search at R = 32 beyond the run's min-to-max spread.

--segment --cut [--size WxH] runs the scene-cut leg instead (profiles/r10/me_cut.txt): the segment form without and with cut= (DESIGN.md
"Scene cuts") at L = 0 / R = 16 and L = 2 / R = 8 in the same alternating rounds, then lsfa_mv_cut_score alone (both its launches) next to
the luma launch of the same stack.  With --kernels-only the cut form is run a few times without timing (for a kernel trace that splits the
two launches).  Nothing is gated: the figures to read off are the difference of the medians against the spreads, and the cut launches
against the luma launch.

--segment --stale [--levels 2] [--size WxH] runs the stale-key leg instead (profiles/r11/me_stale.txt): the segment form without and with
stale= (DESIGN.md "Stale key frames") at L = 0 / R = 16, or with --levels 2 at L = 2 / R = 8, in the same alternating rounds, then alone: the
level-0 search launch of that configuration (mv_estimate_chain, or the level-0 mv_refine_chain), lsfa_mv_key_sad, the mode's three
launches together, and lsfa_mv_key_sad on the same planes as five chains of one frame (no table walk: what the walk costs per pair).  The expectation to read off - not gated: what the mode adds per segment stays below that level-0 search launch,
beyond the spread.  With --kernels-only the stale form is run a few times without timing (for a kernel trace)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from lsfa_amd import hip
from lsfa_amd.utils.synthetic import SyntheticClip

DEV = 'cuda:0'
W, H = 1000, 600


def timed(fn, iters, warmup=5):
    """microseconds per call: `iters` calls between two events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def graphed(fn, iters, rounds=5):
    """microseconds per call with `iters` calls captured in one graph (no host enqueue between the launches): min and median over rounds"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / iters)
    return dict(min=round(min(us), 2), median=round(float(np.median(us)), 2))


def alternating(fns, reps, rounds=9):
    """{name: microseconds per call, min / median / max over rounds}: every fn captured `reps` times in a graph of its own, the graphs
    replayed in turn, round by round"""
    graphs = {}
    for name, fn in fns:
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(reps):
                fn()
        g.replay()
        graphs[name] = g
    torch.cuda.synchronize()
    us = {name: [] for name, _ in fns}
    for _ in range(rounds):
        for name, _ in fns:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graphs[name].replay()
            b.record()
            torch.cuda.synchronize()
            us[name].append(a.elapsed_time(b) * 1e3 / reps)
    return {name: dict(min=round(min(v), 2), median=round(float(np.median(v)), 2), max=round(max(v), 2)) for name, v in us.items()}


def segment_leg(reps, time_limit):
    import signal

    def too_long(signum, frame):
        raise SystemExit('the segment leg ran into its time limit of %d s' % time_limit)

    signal.signal(signal.SIGALRM, too_long)
    signal.alarm(time_limit)
    F = 9
    clip = SyntheticClip(0, F + 1, H, W)
    stack = torch.stack([clip.frame_u8(f) for f in range(F + 1)]).unsqueeze(0).to(DEV)
    out = dict(device=torch.cuda.get_device_name(0), frame='%dx%d' % (W, H), frames=F, clips=1, segments_per_graph=reps)
    for R in (16, 32):
        me = hip.MotionEstimator(W, H, DEV, search=R)
        sme = hip.SegmentMotionEstimator(W, H, frames=F, clips=1, device=DEV, search=R)
        per_frame_out = []

        def per_frame():
            del per_frame_out[:]
            me.key_frame(stack[0, 0])
            for f in range(1, F + 1):
                me.next_frame(stack[0, f])
                per_frame_out.append(me.network_inputs(stack[0, f], stack[0, 0], 1.0, (0.0, 0.0, 0.0), 1.0))

        def segment():
            return sme.segment(stack, 1.0, (0.0, 0.0, 0.0), 1.0)

        # the two forms agree on the last frame (every frame: tests/test_me_segment_gpu.py) before anything is timed
        per_frame()
        mv, res = segment()
        torch.cuda.synchronize()
        assert torch.equal(mv[F - 1], per_frame_out[-1][0]) and torch.equal(res[F - 1], per_frame_out[-1][1])
        luma = sme._luma[:(F + 1) * H * W].view(1, F + 1, H, W)
        rows, sad = sme.rows, sme.sad
        pair_rows, pair_sad = torch.empty_like(rows[0, 0]), torch.empty_like(sad[0, 0])

        def nine_pairs():
            for f in range(1, F + 1):
                hip.mv_estimate(luma[0, f], luma[0, f - 1], R, 4, 0, out=pair_rows, sad_out=pair_sad)

        r = alternating([('per_frame_graph', per_frame), ('segment_graph', segment)], reps)
        r.update(alternating([('nine_mv_estimate', nine_pairs), ('mv_estimate_chain', lambda: hip.mv_estimate_chain(luma, R, 4, 0, out=rows, sad_out=sad)),
                              ('mv_segment_inputs', lambda: hip.mv_segment_inputs(rows, stack, 1.0, out=(mv, res))),
                              ('luma_u8_stack', lambda: hip.luma_u8(stack.view((F + 1) * H, W, 3), out=luma.view((F + 1) * H, W)))], reps))
        a, b = r['per_frame_graph'], r['segment_graph']
        spread = max(a['max'] - a['min'], b['max'] - b['min'])
        r['spread_us'] = round(spread, 2)
        r['segment_not_slower_beyond_spread'] = bool(b['median'] <= a['median'] + spread)
        r['launches'] = dict(per_frame_graph=2 + 8 * F, segment_graph=3)
        out['R%d' % R] = r
    signal.alarm(0)
    print(json.dumps(out))


def pyramid_leg(reps, time_limit, levels, refine):
    import signal

    def too_long(signum, frame):
        raise SystemExit('the pyramid leg ran into its time limit of %d s' % time_limit)

    signal.signal(signal.SIGALRM, too_long)
    signal.alarm(time_limit)
    F = 9
    clip = SyntheticClip(0, F + 1, H, W)
    stack = torch.stack([clip.frame_u8(f) for f in range(F + 1)]).unsqueeze(0).to(DEV)
    out = dict(device=torch.cuda.get_device_name(0), frame='%dx%d' % (W, H), frames=F, clips=1, segments_per_graph=reps, levels=levels, refine=refine)
    forms = [('full_R16', hip.SegmentMotionEstimator(W, H, frames=F, device=DEV, search=16)),
             ('full_R32', hip.SegmentMotionEstimator(W, H, frames=F, device=DEV, search=32))]
    pyramids = [('pyramid_L%d_R%d_r%d' % (levels, R, refine), hip.SegmentMotionEstimator(W, H, frames=F, device=DEV, search=R, levels=levels, refine=refine))
                for R in ((16,) if levels == 1 else (8, 16))]
    for name, sme in forms + pyramids:
        sme.segment(stack, 1.0, (0.0, 0.0, 0.0), 1.0)        # the outputs are allocated at the first call
    torch.cuda.synchronize()
    r = alternating([(name, (lambda e: lambda: e.segment(stack, 1.0, (0.0, 0.0, 0.0), 1.0))(sme)) for name, sme in forms + pyramids], reps)
    full = r['full_R32']
    for name, sme in pyramids:
        p = r[name]
        spread = max(full['max'] - full['min'], p['max'] - p['min'])
        p.update(reach=sme.reach, launches=sme.levels + 4, spread_us=round(spread, 2))
        if sme.reach >= 32:
            p['not_slower_than_full_R32_beyond_spread'] = bool(p['median'] <= full['median'] + spread)
        s = sme._search          # the buffers of the segment, level by level: the planes, the same as (1, F + 1, h_k, w_k) stacks, the rows
        planes = [s.planes(k, 0, F + 1) for k in range(levels + 1)]
        stacks = [p.unsqueeze(0) for p in planes]
        rows = [s.rows[k][:F * s.blocks[k] * 7].view(1, F, s.blocks[k], 7) for k in range(levels + 1)]
        alone = [('luma_pyramid', lambda planes=planes: hip.luma_pyramid(planes[0], levels, out=planes[1:])),
                 ('top_search_level%d' % levels, lambda sme=sme, stacks=stacks, rows=rows: hip.mv_estimate_chain(stacks[levels], sme.search, 4, 0, out=rows[levels]))]
        for k in range(levels - 1, -1, -1):
            alone.append(('refine_level%d' % k, lambda k=k, stacks=stacks, rows=rows: hip.mv_refine_chain(stacks[k], rows[k + 1], refine, 4, 0, out=rows[k])))
        p['alone'] = alternating(alone, reps)
    out.update(r)
    signal.alarm(0)
    print(json.dumps(out))


def cut_leg(reps, time_limit, kernels_only):
    import signal

    def too_long(signum, frame):
        raise SystemExit('the scene-cut leg ran into its time limit of %d s' % time_limit)

    signal.signal(signal.SIGALRM, too_long)
    signal.alarm(time_limit)
    F = 9
    clip = SyntheticClip(0, F + 1, H, W)
    stack = torch.stack([clip.frame_u8(f) for f in range(F + 1)]).unsqueeze(0).to(DEV)
    out = dict(device=torch.cuda.get_device_name(0), frame='%dx%d' % (W, H), frames=F, clips=1, segments_per_graph=reps)
    for levels, R in ((0, 16), (2, 8)):
        plain = hip.SegmentMotionEstimator(W, H, frames=F, device=DEV, search=R, levels=levels)
        cut = hip.SegmentMotionEstimator(W, H, frames=F, device=DEV, search=R, levels=levels, cut=dict())
        want = [x.clone() for x in plain.segment(stack, 1.0, (0.0, 0.0, 0.0), 1.0)]
        got = cut.segment(stack, 1.0, (0.0, 0.0, 0.0), 1.0)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(cut.rows, plain.rows)
        if kernels_only:
            for _ in range(20):
                cut.segment(stack, 1.0, (0.0, 0.0, 0.0), 1.0)
            torch.cuda.synchronize()
            continue
        r = alternating([('segment', lambda: plain.segment(stack, 1.0, (0.0, 0.0, 0.0), 1.0)),
                         ('segment_cut', lambda: cut.segment(stack, 1.0, (0.0, 0.0, 0.0), 1.0))], reps)
        a, b = r['segment'], r['segment_cut']
        r['cut_costs_us'] = round(b['median'] - a['median'], 2)
        r['spread_us'] = round(max(a['max'] - a['min'], b['max'] - b['min']), 2)
        r['launches'] = dict(segment=levels + (4 if levels else 3), segment_cut=levels + (4 if levels else 3) + 2)
        r['unmatched'] = cut.unmatched.cpu().tolist()
        luma = cut._search.planes(0, 0, F + 1).unsqueeze(0)
        r['alone'] = alternating([('mv_cut_score', lambda: hip.mv_cut_score(luma, cut.sad, out=(cut.intra, cut.unmatched))),
                                  ('luma_u8_stack', lambda: hip.luma_u8(stack.view((F + 1) * H, W, 3), out=luma.view((F + 1) * H, W)))], reps)
        out['L%d_R%d' % (levels, R)] = r
    signal.alarm(0)
    print(json.dumps(out))


def stale_leg(reps, time_limit, levels, refine, kernels_only):
    import signal

    def too_long(signum, frame):
        raise SystemExit('the stale-key leg ran into its time limit of %d s' % time_limit)

    signal.signal(signal.SIGALRM, too_long)
    signal.alarm(time_limit)
    F, R = 9, 8 if levels else 16
    clip = SyntheticClip(0, F + 1, H, W)
    stack = torch.stack([clip.frame_u8(f) for f in range(F + 1)]).unsqueeze(0).to(DEV)
    out = dict(device=torch.cuda.get_device_name(0), frame='%dx%d' % (W, H), frames=F, clips=1, segments_per_graph=reps, levels=levels, search=R)
    kw = dict(frames=F, device=DEV, search=R, levels=levels, refine=refine)
    plain, stale = hip.SegmentMotionEstimator(W, H, **kw), hip.SegmentMotionEstimator(W, H, stale=dict(), **kw)
    want = [x.clone() for x in plain.segment(stack, 1.0, (0.0, 0.0, 0.0), 1.0)]
    got = stale.segment(stack, 1.0, (0.0, 0.0, 0.0), 1.0)
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(stale.rows, plain.rows)
    if kernels_only:
        for _ in range(20):
            stale.segment(stack, 1.0, (0.0, 0.0, 0.0), 1.0)
        torch.cuda.synchronize()
        signal.alarm(0)
        return
    r = alternating([('segment', lambda: plain.segment(stack, 1.0, (0.0, 0.0, 0.0), 1.0)),
                     ('segment_stale', lambda: stale.segment(stack, 1.0, (0.0, 0.0, 0.0), 1.0))], reps)
    a, b = r['segment'], r['segment_stale']
    r['stale_costs_us'] = round(b['median'] - a['median'], 2)
    r['spread_us'] = round(max(a['max'] - a['min'], b['max'] - b['min']), 2)
    r['launches'] = dict(segment=levels + (4 if levels else 3), segment_stale=levels + (4 if levels else 3) + 3)
    r['key_unmatched'] = stale.key_unmatched.cpu().tolist()
    s = stale._search
    luma = s.planes(0, 0, F + 1).unsqueeze(0)
    rows0 = s.rows[0][:F * s.blocks[0] * 7].view(1, F, s.blocks[0], 7)
    if levels:
        rows1 = s.rows[1][:F * s.blocks[1] * 7].view(1, F, s.blocks[1], 7)
        search = ('mv_refine_chain_level0', lambda: hip.mv_refine_chain(luma, rows1, refine, 4, 0, out=rows0))
    else:
        search = ('mv_estimate_chain', lambda: hip.mv_estimate_chain(luma, R, 4, 0, out=rows0))

    def key_sad():
        hip._check(hip.lib().lsfa_mv_key_sad(luma.data_ptr(), s.plane[0], 1, F, W, H, rows0.data_ptr(), s.keysad.data_ptr(), hip._stream()), 'lsfa_mv_key_sad')

    def key_sad_no_walk():
        # the same ten planes as five chains of ONE frame: five pairs whose only step is the block's own row (scalar loads), no table gather
        hip._check(hip.lib().lsfa_mv_key_sad(luma.data_ptr(), s.plane[0], 5, 1, W, H, rows0.data_ptr(), s.keysad.data_ptr(), hip._stream()), 'lsfa_mv_key_sad')

    r['alone'] = alternating([search, ('mv_key_sad', key_sad), ('key_score(three launches)', lambda: s.key_score(1, F)),
                              ('mv_key_sad_five_pairs_of_one_step', key_sad_no_walk)], reps)
    # per pair: nine pairs that walk 0..8 table steps against five that walk none - what the walk's table loads cost
    r['key_sad_us_per_pair'] = dict(walking=round(r['alone']['mv_key_sad']['median'] / F, 2),
                                    one_step=round(r['alone']['mv_key_sad_five_pairs_of_one_step']['median'] / 5, 2))
    r['level0_search_us'] = r['alone'][search[0]]['median']
    r['adds_less_than_the_level0_search_beyond_spread'] = bool(r['stale_costs_us'] + r['spread_us'] < r['level0_search_us'])
    out['L%d_R%d' % (levels, R)] = r
    signal.alarm(0)
    print(json.dumps(out))


def non_key_frame(iters):
    from lsfa_amd.config.config import lsfa_test_config
    from lsfa_amd.symbols import params as P
    from lsfa_amd.symbols.resnet_v1_101_flownet_rfcn import resnet_v1_101_flownet_rfcn
    cfg = lsfa_test_config(key_frame_interval=10)
    arg, aux = P.init_params(cfg, seed=0)
    cur = resnet_v1_101_flownet_rfcn(cfg).get_cur_test_symbol(cfg).bind(arg, aux, DEV)
    data = torch.rand(1, 3, H, W, device=DEV) * 255
    im_info = torch.tensor([[H, W, 1.0]], device=DEV)
    feat = torch.randn(1, 1024, 38, 63, device=DEV)
    mv, res = torch.randn(1, 2, 38, 63, device=DEV) * 0.5, torch.randn(1, 3, 38, 63, device=DEV)
    R, ncls = cfg.TEST.RPN_POST_NMS_TOP_N, cfg.dataset.NUM_CLASSES
    bufs = (torch.zeros((1, ncls, R, 5), dtype=torch.float64, device=DEV), torch.zeros((1, ncls), dtype=torch.int32, device=DEV),
            torch.full((1, ncls, R), -1, dtype=torch.int32, device=DEV))

    def frame():
        out = cur.forward(data=data, im_info=im_info, feat_key=feat, motion_vector=mv, res_diff=res)
        hip.det_postprocess_batch(out['rois_output'], out['bbox_pred_reshape_output'].reshape(R, -1), out['cls_prob_reshape_output'].reshape(R, -1),
                                  1, H, W, 1.0, bufs, nms_thresh=cfg.TEST.NMS, max_per_image=cfg.TEST.max_per_image, class_agnostic=cfg.CLASS_AGNOSTIC)

    with torch.no_grad():
        return dict(eager_us=round(timed(frame, iters), 1))


def main():
    global W, H
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--skip-non-key', action='store_true')
    ap.add_argument('--segment', action='store_true', help='the segment leg: nine frames per-frame against the three-launch segment form')
    ap.add_argument('--segment-reps', type=int, default=20, help='--segment: segments captured per graph')
    ap.add_argument('--time-limit', type=int, default=240, help='--segment: seconds after which the leg gives up')
    ap.add_argument('--levels', type=int, default=0, choices=(0, 1, 2), help='--segment: the pyramid leg with this many extra levels (0: the segment leg)')
    ap.add_argument('--refine', type=int, default=2, choices=(1, 2, 3), help='--levels: the refinement radius')
    ap.add_argument('--cut', action='store_true', help='--segment: the scene-cut leg (the segment form without and with cut=)')
    ap.add_argument('--stale', action='store_true', help='--segment: the stale-key leg (the segment form without and with stale=), at --levels 0 or 2')
    ap.add_argument('--size', default=None, help='--segment: the frame size as WxH (default 1000x600)')
    args = ap.parse_args()
    if args.size:
        if not args.segment:
            ap.error('--size belongs to --segment')
        W, H = (int(v) for v in args.size.split('x'))
    if args.cut:
        if not args.segment:
            ap.error('--cut belongs to --segment')
        return cut_leg(args.segment_reps, args.time_limit, args.kernels_only)
    if args.stale:
        if not args.segment:
            ap.error('--stale belongs to --segment')
        return stale_leg(args.segment_reps, args.time_limit, args.levels, args.refine, args.kernels_only)
    if args.segment and args.levels:
        return pyramid_leg(args.segment_reps, args.time_limit, args.levels, args.refine)
    if args.segment:
        return segment_leg(args.segment_reps, args.time_limit)
    clip = SyntheticClip(0, 4, H, W)
    frames = [clip.frame_u8(f).to(DEV) for f in range(3)]
    y = [hip.luma_u8(f) for f in frames]
    rows = torch.empty((38 * 63, 7), dtype=torch.int32, device=DEV)
    sad = torch.empty((38, 63), dtype=torch.int32, device=DEV)
    me = hip.MotionEstimator(W, H, DEV)
    me.key_frame(frames[0])

    def front_end():
        me.next_frame(frames[1])
        me.network_inputs(frames[1], frames[0], 1.0, (0.0, 0.0, 0.0), 1.0)

    if args.kernels_only:
        for _ in range(20):
            hip.luma_u8(frames[1], out=y[1])
            hip.mv_estimate(y[1], y[0], 16, 4, 0, out=rows, sad_out=sad)
            hip.mv_estimate(y[2], y[1], 32, 4, 0, out=rows, sad_out=sad)
            front_end()
        torch.cuda.synchronize()
        return
    out = dict(device=torch.cuda.get_device_name(0), frame='%dx%d' % (W, H), iters=args.iters)
    blocks = 38 * 63
    for name, fn, work in (('luma_u8', lambda: hip.luma_u8(frames[1], out=y[1]), None),
                           ('mv_estimate_R16', lambda: hip.mv_estimate(y[1], y[0], 16, 4, 0, out=rows, sad_out=sad), blocks * 33 * 33 * 64),
                           ('mv_estimate_R32', lambda: hip.mv_estimate(y[2], y[1], 32, 4, 0, out=rows, sad_out=sad), blocks * 65 * 65 * 64),
                           ('front_end(next_frame+network_inputs)', front_end, None)):
        r = dict(eager_us=round(timed(fn, args.iters), 2), graph_us=graphed(fn, args.iters))
        if work:
            # the search's arithmetic: one dword SAD (4 pixels) per block dword, row and candidate
            r['dword_sads'] = work
            r['dword_sads_per_s'] = round(work / (r['graph_us']['min'] * 1e-6), -9)
        out[name] = r
    hip.prof_enable(True, ops=['mv_estimate'])
    for _ in range(50):
        hip.mv_estimate(y[1], y[0], 16, 4, 0, out=rows, sad_out=sad)
    ms, n = hip.prof_read()['mv_estimate']
    hip.prof_enable(False)
    out['mv_estimate_R16_prof_read_us'] = round(ms * 1e3 / n, 2)
    if not args.skip_non_key:
        out['non_key_frame'] = non_key_frame(30)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
