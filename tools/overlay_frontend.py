#!/usr/bin/env python
"""Time of the detection overlay (lsfa_amd/overlay.py: lsfa_overlay_plan + one paint launch) next to the frame it decorates (device
events, same process; profiles/r16/overlay_frontend.txt):

    plan + paint                   for BGR and NV12 at 1000x600 and 1920x1080 with 0, 30 and 300 recorded detections of 30 classes,
                                   launched eagerly and as a replayed graph of `reps` calls
    plan + paint, other surfaces   Overlay.draw_yuv (lsfa_overlay_paint_yuv) for p010, yuyv422 and yuv444p - and for nv12, the same surface
                                   through the new export - with the same detections, beside draw_yuv420's NV12 of the same run
    yuv420_to_bgr_u8               the shipped conversion at the same size: one full-frame pass to hold the overlay against
    one non-key frame              tools/me_frontend.py's non_key_frame at 1000x600, eager

Every form of one size is timed in turn, round by round, so that whatever else the machine does falls on all of them; min, median and max
over the rounds are printed, in microseconds per call.  The conditions to read off (reported, not gated):
  - plan + paint with 30 detections at 1000x600 costs less than a tenth of the non-key frame the same run measures;
  - with no detection - every tile leaves after the sift - it costs no more than the full-frame pass, beyond the min-to-max spread.
--kernels-only runs the launches a few times without timing (for `rocprofv3 --kernel-trace --stats -- python tools/overlay_frontend.py
--kernels-only`).  Prints one JSON object."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lsfa_amd import hip, overlay, yuvfmt

DEV = 'cuda:0'
NCLS, ROWS = 31, 300
SIZES = ((1000, 600), (1920, 1080))
DETECTIONS = (0, 30, 300)
OTHER_SURFACES = ('nv12', 'p010', 'yuyv422', 'yuv444p')          # through Overlay.draw_yuv


def detections(n, W, H, seed=0):
    """dets (NCLS, ROWS, 5), counts with n boxes of the sizes a detector reports, dealt to the classes in turn"""
    rs = np.random.RandomState(seed + n)
    dets, counts = np.zeros((NCLS, ROWS, 5)), np.zeros(NCLS, np.int32)
    for k in range(n):
        j = 1 + k % (NCLS - 1)
        w, h = rs.uniform(0.04, 0.3) * W, rs.uniform(0.06, 0.4) * H
        x1, y1 = rs.uniform(0, W - w), rs.uniform(0, H - h)
        dets[j, counts[j]] = (x1, y1, x1 + w, y1 + h, rs.uniform(0.7, 1.0))
        counts[j] += 1
    return torch.from_numpy(dets).to(DEV), torch.from_numpy(counts).to(DEV)


def surface(fmt, W, H):
    """the planes of one frame of format fmt as draw_yuv's keyword arguments, random samples"""
    _, _, layout, sample = yuvfmt.fields(fmt)
    ch, cw = yuvfmt.chroma_shape(fmt, H, W)

    def plane(rows, cols):
        if sample == yuvfmt.U8:
            return torch.randint(0, 256, (rows, cols), dtype=torch.uint8, device=DEV)
        return (torch.randint(0, 1024, (rows, cols), dtype=torch.int16, device=DEV) << (6 if sample == yuvfmt.HI10 else 0))
    if layout >= yuvfmt.YUYV:
        return dict(y=plane(H, 4 * cw), width=W)
    if layout == yuvfmt.PLANAR:
        return dict(y=plane(H, W), u=plane(ch, cw), v=plane(ch, cw))
    return dict(y=plane(H, W), uv=plane(ch, 2 * cw))


def forms(W, H):
    """[(name, fn)] of one size: the overlay per surface and detection count, and the conversion"""
    ch, cw = -(-H // 2), -(-W // 2)
    y = torch.randint(0, 256, (H, W), dtype=torch.uint8, device=DEV)
    uv = torch.randint(0, 256, (ch, 2 * cw), dtype=torch.uint8, device=DEV)
    bgr = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=DEV)
    converted = torch.empty((H, W, 3), dtype=torch.uint8, device=DEV)
    out = [('yuv420_to_bgr_u8', lambda: hip.yuv420_to_bgr_u8(y, uv=uv, out=converted))]
    others = {fmt: surface(fmt, W, H) for fmt in OTHER_SURFACES}
    for n in DETECTIONS:
        ov = overlay.Overlay(NCLS, ROWS, max_boxes=512, device=DEV)
        dets, counts = detections(n, W, H)
        out.append(('bgr_%d' % n, lambda ov=ov, dets=dets, counts=counts: ov.draw_bgr(bgr, dets, counts, 0.7)))
        out.append(('nv12_%d' % n, lambda ov=ov, dets=dets, counts=counts: ov.draw_yuv420(y, dets, counts, 0.7, uv=uv)))
        out[-1][1]()
        assert int(ov.drawn()[0, 0]) == n, (n, ov.drawn())
        for fmt in OTHER_SURFACES:
            out.append(('%s_yuv_%d' % (fmt, n), lambda ov=ov, dets=dets, counts=counts, fmt=fmt, kw=others[fmt]: ov.draw_yuv(fmt, kw['y'], dets, counts, 0.7, **{
                k: v for k, v in kw.items() if k != 'y'})))
    return out


def stats(v):
    return dict(min=round(min(v), 2), median=round(float(np.median(v)), 2), max=round(max(v), 2))


def alternating(fns, reps, rounds):
    """{name: {graph, eager: microseconds per call, min / median / max over rounds}}: every fn captured `reps` times in a graph of its own;
    in every round each graph is replayed once and each fn launched `reps` times eagerly, in turn"""
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
    us = {name: dict(graph=[], eager=[]) for name, _ in fns}
    for _ in range(rounds):
        for name, fn in fns:
            for how in ('graph', 'eager'):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                if how == 'graph':
                    graphs[name].replay()
                else:
                    for _ in range(reps):
                        fn()
                b.record()
                torch.cuda.synchronize()
                us[name][how].append(a.elapsed_time(b) * 1e3 / reps)
    return {name: {how: stats(v) for how, v in d.items()} for name, d in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50, help='calls per graph and per eager window')
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--skip-non-key', action='store_true')
    args = ap.parse_args()
    if args.kernels_only:
        for W, H in SIZES:
            for _, fn in forms(W, H):
                for _ in range(5):
                    fn()
        torch.cuda.synchronize()
        return
    out = dict(device=torch.cuda.get_device_name(0), classes=NCLS - 1, rows=ROWS, calls_per_window=args.reps, rounds=args.rounds, unit='us per call')
    for W, H in SIZES:
        out['%dx%d' % (W, H)] = alternating(forms(W, H), args.reps, args.rounds)
    small = out['%dx%d' % SIZES[0]]
    if not args.skip_non_key:
        from me_frontend import non_key_frame
        out['non_key_frame_1000x600'] = non_key_frame(30)
        cur = out['non_key_frame_1000x600']['eager_us']
        out['goal_30_detections_below_a_tenth_of_the_non_key_frame'] = {
            k: dict(eager_us=small[k]['eager']['median'], graph_us=small[k]['graph']['median'], tenth_us=round(cur / 10, 1),
                    met=bool(small[k]['eager']['median'] < cur / 10)) for k in ('bgr_30', 'nv12_30')}
    goal = {}
    for size in ('%dx%d' % s for s in SIZES):
        r = out[size]
        full = r['yuv420_to_bgr_u8']
        for k in ('bgr_0', 'nv12_0'):
            for how in ('graph', 'eager'):
                spread = max(full[how]['max'] - full[how]['min'], r[k][how]['max'] - r[k][how]['min'])
                goal['%s %s %s' % (size, k, how)] = dict(us=r[k][how]['median'], full_pass_us=full[how]['median'], spread_us=round(spread, 2),
                                                         met=bool(r[k][how]['median'] <= full[how]['median'] + spread))
    out['goal_no_detections_not_above_the_full_frame_pass_beyond_spread'] = goal
    # every other surface over draw_yuv420's NV12 of this run (the paint kernel of lsfa_overlay_paint_yuv420 is untouched by the new export)
    out['other_surfaces_over_nv12'] = {
        size: {'%s_yuv_%d' % (fmt, n): {how: round(out[size]['%s_yuv_%d' % (fmt, n)][how]['median'] / out[size]['nv12_%d' % n][how]['median'], 3)
                                        for how in ('graph', 'eager')} for fmt in OTHER_SURFACES for n in DETECTIONS}
        for size in ('%dx%d' % s for s in SIZES)}
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main()
