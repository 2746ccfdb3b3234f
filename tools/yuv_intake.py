#!/usr/bin/env python
"""Frame intake at 1000 x 600, packed BGR against NV12 and against 10-bit planes (P010 and planar 16-bit words), N = 1, 9, 12 frames per call, in ONE process on one device (device events,
`--iters` calls per figure after a warm-up, `--rounds` rounds with the two paths alternating; every figure is printed as min / median / max
over the rounds, which IS the run-to-run spread to judge a difference by):

    upload + intake      pinned host memory -> device copy -> `data`:  3 B/pixel + lsfa_image_transform_u8  against
                         1.5 B/pixel + lsfa_image_transform_yuv420  and  3 B/pixel (16-bit words) + lsfa_image_transform_yuv420p10
    kernels alone        each intake kernel as a replayed graph of `--iters` launches (no host enqueue between them), with the bytes the
                         algorithm reads and writes over that time: lsfa_image_transform_u8, lsfa_image_transform_yuv420 (NV12, I420),
                         lsfa_yuv420_to_bgr_u8 (NV12 with and without y_packed, I420), lsfa_luma_u8 (what y_packed saves), and the resize
                         forms lsfa_image_resize_transform (uint8) / lsfa_image_resize_transform_yuv420 (NV12, I420) at scale 1, stride 16; and
                         the 10-bit legs, semi-planar (P010) and planar (yuv420p10le): lsfa_image_transform_yuv420p10, lsfa_yuv420p10_to_bgr_u8
                         (with and without y_packed) and lsfa_image_resize_transform_yuv420p10

The expectations: the NV12 transform kernel is not slower than the u8 one beyond the spread - it writes the same bytes and reads half - and
neither is the 10-bit transform kernel (either layout), which reads the u8 kernel's 3 B and writes its 12 B per pixel.

--formats: instead of the above, the other chroma formats (lsfa_amd/csrc/yuvfmt.hip) at 1000 x 600 and 1920 x 1080: the nv16, yuyv422,
yuv444p and p210 legs of lsfa_yuv_to_bgr_u8, lsfa_image_transform_yuv and lsfa_image_resize_transform_yuv (scale 1, stride 16) as replayed
graphs, each beside the shipped NV12 (for p210: P010) leg of the same kernel measured in the same run.  The expectation printed per leg:
its median is at most 1.10 x the yardstick's median scaled by the ratio of the algorithmic bytes per pixel (image_transform: NV16 reads 2
and writes 12 B, NV12 1.5 and 12 B, so 14 / 13.5); `ratio` is the measured time over that scaled time and `holds` says ratio <= 1.10.
Prints one JSON object per line.  Ends itself after --time-limit seconds."""
import argparse
import ctypes
import json
import os
import signal
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from lsfa_amd import hip, yuv10, yuvfmt

DEV = 'cuda:0'
W, H = 1000, 600
MEANS, SCALE = (102.9801, 115.9465, 122.7717), 0.0125


def stats(us):
    return dict(min=round(min(us), 2), median=round(float(np.median(us)), 2), max=round(max(us), 2))


def eager_rounds(fns, iters, rounds, warmup=10):
    """microseconds per call of each fn in `fns`: `iters` calls between two events, the fns alternating within every round"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3 / iters)
    return {k: stats(v) for k, v in us.items()}


def graph_rounds(fns, iters, rounds):
    """the same with `iters` calls of a fn captured in one graph: kernel time without the host's enqueue"""
    graphs = {}
    for k, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(iters):
                fn()
        g.replay()
        graphs[k] = g
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for k, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            torch.cuda.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3 / iters)
    return {k: stats(v) for k, v in us.items()}


def format_legs(args):
    """the --formats section: see the module docstring"""
    rs = np.random.RandomState(1)
    margin = 1.10
    for w, h in ((1000, 600), (1920, 1080)):
        px, ph, pw = h * w, -(-h // 16) * 16, -(-w // 16) * 16
        for N in args.frames:
            def planes(rows, cols, words=False):
                a = rs.randint(0, 1 << 16, (N, rows, cols)).astype(np.uint16).view(np.int16) if words else rs.randint(0, 256, (N, rows, cols)).astype(np.uint8)
                return torch.from_numpy(a).to(DEV)
            # name: (format of yuvfmt or None for the shipped export, plane arguments, bytes read per pixel)
            nv12, p010 = planes(h * 3 // 2, w), planes(h * 3 // 2, w, True)
            nv16, p210 = planes(2 * h, w), planes(2 * h, w, True)
            i444 = planes(3 * h, w)
            legs = {
                'nv12': (None, dict(y=nv12[:, :h], uv=nv12[:, h:]), 1.5),
                'p010': (None, dict(y=p010[:, :h], uv=p010[:, h:]), 3.0),
                'nv16': ('nv16', dict(y=nv16[:, :h], uv=nv16[:, h:]), 2.0),
                'yuyv422': ('yuyv422', dict(y=planes(h, 2 * w)), 2.0),
                'yuv444p': ('yuv444p', dict(y=i444[:, :h], u=i444[:, h:2 * h], v=i444[:, 2 * h:]), 3.0),
                'p210': ('p210', dict(y=p210[:, :h], uv=p210[:, h:]), 4.0),
            }
            data = torch.empty((N, 3, h, w), dtype=torch.float32, device=DEV)
            rdata = torch.empty((N, 3, ph, pw), dtype=torch.float32, device=DEV)
            bgr_out = torch.empty((N, h, w, 3), dtype=torch.uint8, device=DEV)
            tf = dict(pixel_means=MEANS, pixel_scale=SCALE)
            kernels, nbytes = {}, {}
            for name, (fmt, kw, read) in legs.items():
                if fmt is None:
                    to_bgr, transform, resize = ((hip.yuv420_to_bgr_u8, hip.image_transform_yuv420, hip.image_resize_transform_yuv420) if name == 'nv12' else
                                                 (yuv10.yuv420p10_to_bgr_u8, yuv10.image_transform_yuv420p10, yuv10.image_resize_transform_yuv420p10))
                    kernels['to_bgr_' + name] = lambda f=to_bgr, kw=kw: f(out=bgr_out, **kw)
                    kernels['transform_' + name] = lambda f=transform, kw=kw: f(out=data, **tf, **kw)
                    kernels['resize_' + name] = lambda f=resize, kw=kw: f(im_scale=1.0, stride=16, out=rdata, **tf, **kw)
                else:
                    assert torch.equal(yuvfmt.image_transform_yuv(fmt, **tf, **kw), hip.image_transform_u8(yuvfmt.yuv_to_bgr_u8(fmt, **kw), MEANS, SCALE))
                    kernels['to_bgr_' + name] = lambda fmt=fmt, kw=kw: yuvfmt.yuv_to_bgr_u8(fmt, out=bgr_out, **kw)
                    kernels['transform_' + name] = lambda fmt=fmt, kw=kw: yuvfmt.image_transform_yuv(fmt, out=data, **tf, **kw)
                    kernels['resize_' + name] = lambda fmt=fmt, kw=kw: yuvfmt.image_resize_transform_yuv(fmt, im_scale=1.0, stride=16, out=rdata, **tf, **kw)
                nbytes['to_bgr_' + name] = (read + 3) * px * N
                nbytes['transform_' + name] = (read + 12) * px * N
                nbytes['resize_' + name] = (read * px + 12 * ph * pw) * N
            r = graph_rounds(kernels, args.iters, args.rounds)
            for k in kernels:
                r[k]['bytes'] = int(nbytes[k])
                r[k]['GB_per_s_at_median'] = round(nbytes[k] / (r[k]['median'] * 1e-6) / 1e9, 1)
            print(json.dumps(dict(frame='%dx%d' % (w, h), N=N, what='kernels alone, replayed graph', us=r)), flush=True)
            for kernel in ('to_bgr', 'transform', 'resize'):
                for name in ('nv16', 'yuyv422', 'yuv444p', 'p210'):
                    yard = 'p010' if name == 'p210' else 'nv12'
                    a, b = r['%s_%s' % (kernel, yard)], r['%s_%s' % (kernel, name)]
                    scaled = a['median'] * nbytes['%s_%s' % (kernel, name)] / nbytes['%s_%s' % (kernel, yard)]
                    print(json.dumps(dict(frame='%dx%d' % (w, h), N=N, what='expectation: %s %s within %.2f x the %s leg scaled by bytes' % (kernel, name, margin, yard),
                                          us=b['median'], yardstick_us=a['median'], scaled_us=round(scaled, 2), ratio=round(b['median'] / scaled, 3),
                                          spread=round(b['max'] - b['min'], 2), yardstick_spread=round(a['max'] - a['min'], 2),
                                          holds=bool(b['median'] <= margin * scaled))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--formats', action='store_true', help='the other chroma formats at 1000x600 and 1920x1080 in place of the 4:2:0 report')
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--frames', type=int, nargs='*', default=[1, 9, 12])
    ap.add_argument('--time-limit', type=int, default=420, help='seconds after which the process ends itself')
    args = ap.parse_args()
    signal.alarm(args.time_limit)
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: nothing to measure')
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), frame='1000x600 and 1920x1080' if args.formats else '%dx%d' % (W, H), iters=args.iters, rounds=args.rounds,
                          unit='microseconds per call: min / median / max over the rounds')), flush=True)
    if args.formats:
        return format_legs(args)
    rs = np.random.RandomState(0)
    px = H * W
    means_c = (ctypes.c_double * 3)(*MEANS)
    for N in args.frames:
        # host side: what a decoder (NV12: Y rows, then interleaved chroma rows, one surface per frame) or a host colour conversion (BGR) leaves
        h_bgr = torch.from_numpy(rs.randint(0, 256, (N, H, W, 3)).astype(np.uint8)).pin_memory()
        h_nv12 = torch.from_numpy(rs.randint(0, 256, (N, H * 3 // 2, W)).astype(np.uint8)).pin_memory()
        d_bgr = torch.empty((N, H, W, 3), dtype=torch.uint8, device=DEV)
        d_nv12 = torch.empty((N, H * 3 // 2, W), dtype=torch.uint8, device=DEV)
        d_bgr.copy_(h_bgr)
        d_nv12.copy_(h_nv12)
        y, uv = d_nv12[:, :H], d_nv12[:, H:]
        d_i420 = d_nv12.clone()
        u = d_i420[:, H:].reshape(N, 2, H // 2, W // 2)[:, 0]
        v = d_i420[:, H:].reshape(N, 2, H // 2, W // 2)[:, 1]
        yi = d_i420[:, :H]
        data = torch.empty((N, 3, H, W), dtype=torch.float32, device=DEV)
        rdata = torch.empty((N, 3, 608, 1008), dtype=torch.float32, device=DEV)
        bgr_out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=DEV)
        y_packed = torch.empty((N, H, W), dtype=torch.uint8, device=DEV)
        luma = torch.empty((H, W), dtype=torch.uint8, device=DEV)
        # 10-bit: the same surfaces in 16-bit words, the sample in the high ten bits (P010) - every word is defined input
        h_p010 = torch.from_numpy(rs.randint(0, 1 << 16, (N, H * 3 // 2, W)).astype(np.uint16).view(np.int16)).pin_memory()
        d_p010 = torch.empty((N, H * 3 // 2, W), dtype=torch.int16, device=DEV)
        d_p010.copy_(h_p010)
        y10, uv10 = d_p010[:, :H], d_p010[:, H:]
        d_pl10 = d_p010.clone()
        u10 = d_pl10[:, H:].reshape(N, 2, H // 2, W // 2)[:, 0]
        v10 = d_pl10[:, H:].reshape(N, 2, H // 2, W // 2)[:, 1]
        y10p = d_pl10[:, :H]
        assert torch.equal(yuv10.image_transform_yuv420p10(y10, uv10, pixel_means=MEANS, pixel_scale=SCALE),
                           hip.image_transform_u8(yuv10.yuv420p10_to_bgr_u8(y10, uv10), MEANS, SCALE))
        assert torch.equal(hip.image_transform_yuv420(y, uv, pixel_means=MEANS, pixel_scale=SCALE),
                           hip.image_transform_u8(hip.yuv420_to_bgr_u8(y, uv), MEANS, SCALE))

        def up_bgr():
            d_bgr.copy_(h_bgr, non_blocking=True)
            hip.image_transform_u8(d_bgr, MEANS, SCALE, out=data)

        def up_nv12():
            d_nv12.copy_(h_nv12, non_blocking=True)
            hip.image_transform_yuv420(y, uv, pixel_means=MEANS, pixel_scale=SCALE, out=data)

        def up_p010():
            d_p010.copy_(h_p010, non_blocking=True)
            yuv10.image_transform_yuv420p10(y10, uv10, pixel_means=MEANS, pixel_scale=SCALE, out=data)

        r = eager_rounds(dict(bgr_upload_transform_u8=up_bgr, nv12_upload_transform_yuv420=up_nv12, p010_upload_transform_yuv420p10=up_p010,
                              p010_upload_only=lambda: d_p010.copy_(h_p010, non_blocking=True),
                              bgr_upload_only=lambda: d_bgr.copy_(h_bgr, non_blocking=True),
                              nv12_upload_only=lambda: d_nv12.copy_(h_nv12, non_blocking=True)), args.iters, args.rounds)
        print(json.dumps(dict(N=N, what='upload + intake, eager', upload_bytes=dict(bgr=3 * px * N, nv12=px * N * 3 // 2, p010=3 * px * N), us=r)), flush=True)

        def resize_u8():          # the C entry point itself: hip.image_resize_transform allocates its output at every call
            hip._check(hip.lib().lsfa_image_resize_transform(hip._ptr(d_bgr), 1, N, H, W, ctypes.c_double(1.0), H, W, 16, means_c, ctypes.c_double(SCALE),
                                                             hip._ptr(rdata), 608, 1008, hip._stream()), 'lsfa_image_resize_transform')

        kernels = {
            # name: (fn, bytes read + written by the algorithm)
            'image_transform_u8': (lambda: hip.image_transform_u8(d_bgr, MEANS, SCALE, out=data), (3 + 12) * px * N),
            'image_transform_yuv420_nv12': (lambda: hip.image_transform_yuv420(y, uv, pixel_means=MEANS, pixel_scale=SCALE, out=data), (1.5 + 12) * px * N),
            'image_transform_yuv420_i420': (lambda: hip.image_transform_yuv420(yi, u=u, v=v, pixel_means=MEANS, pixel_scale=SCALE, out=data), (1.5 + 12) * px * N),
            'yuv420_to_bgr_u8': (lambda: hip.yuv420_to_bgr_u8(y, uv, out=bgr_out), (1.5 + 3) * px * N),
            'yuv420_to_bgr_u8+y_packed': (lambda: hip.yuv420_to_bgr_u8(y, uv, out=bgr_out, y_packed=y_packed), (1.5 + 4) * px * N),
            'yuv420_to_bgr_u8_i420': (lambda: hip.yuv420_to_bgr_u8(yi, u=u, v=v, out=bgr_out), (1.5 + 3) * px * N),
            'luma_u8(one frame)': (lambda: hip.luma_u8(d_bgr[0], out=luma), (3 + 1) * px),
            'image_resize_transform_u8': (resize_u8, (3 * px + 12 * 608 * 1008) * N),
            'image_resize_transform_yuv420': (lambda: hip.image_resize_transform_yuv420(y, uv, im_scale=1.0, pixel_means=MEANS, pixel_scale=SCALE, stride=16,
                                                                                       out=rdata), (1.5 * px + 12 * 608 * 1008) * N),
            'image_resize_transform_yuv420_i420': (lambda: hip.image_resize_transform_yuv420(yi, u=u, v=v, im_scale=1.0, pixel_means=MEANS, pixel_scale=SCALE,
                                                                                            stride=16, out=rdata), (1.5 * px + 12 * 608 * 1008) * N),
            'image_transform_yuv420p10_semi': (lambda: yuv10.image_transform_yuv420p10(y10, uv10, pixel_means=MEANS, pixel_scale=SCALE, out=data),
                                               (3 + 12) * px * N),
            'image_transform_yuv420p10_planar': (lambda: yuv10.image_transform_yuv420p10(y10p, u=u10, v=v10, msb_aligned=False, pixel_means=MEANS, pixel_scale=SCALE, out=data),
                                                 (3 + 12) * px * N),
            'yuv420p10_to_bgr_u8_semi': (lambda: yuv10.yuv420p10_to_bgr_u8(y10, uv10, out=bgr_out), (3 + 3) * px * N),
            'yuv420p10_to_bgr_u8_semi+y_packed': (lambda: yuv10.yuv420p10_to_bgr_u8(y10, uv10, out=bgr_out, y_packed=y_packed), (3 + 4) * px * N),
            'yuv420p10_to_bgr_u8_planar': (lambda: yuv10.yuv420p10_to_bgr_u8(y10p, u=u10, v=v10, msb_aligned=False, out=bgr_out), (3 + 3) * px * N),
            'yuv420p10_to_bgr_u8_planar+y_packed': (lambda: yuv10.yuv420p10_to_bgr_u8(y10p, u=u10, v=v10, msb_aligned=False, out=bgr_out, y_packed=y_packed), (3 + 4) * px * N),
            'image_resize_transform_yuv420p10_semi': (lambda: yuv10.image_resize_transform_yuv420p10(y10, uv10, im_scale=1.0, pixel_means=MEANS,
                                                                                                     pixel_scale=SCALE, stride=16, out=rdata),
                                                      (3 * px + 12 * 608 * 1008) * N),
            'image_resize_transform_yuv420p10_planar': (lambda: yuv10.image_resize_transform_yuv420p10(y10p, u=u10, v=v10, msb_aligned=False, im_scale=1.0, pixel_means=MEANS,
                                                                                                       pixel_scale=SCALE, stride=16, out=rdata),
                                                        (3 * px + 12 * 608 * 1008) * N),
        }
        r = graph_rounds({k: f for k, (f, _) in kernels.items()}, args.iters, args.rounds)
        for k, (_, nbytes) in kernels.items():
            r[k]['bytes'] = int(nbytes)
            r[k]['GB_per_s_at_median'] = round(nbytes / (r[k]['median'] * 1e-6) / 1e9, 1)
        print(json.dumps(dict(N=N, what='kernels alone, replayed graph', us=r)), flush=True)
        a, b = r['image_transform_u8'], r['image_transform_yuv420_nv12']
        print(json.dumps(dict(N=N, what='expectation: NV12 transform not slower than u8 beyond the spread',
                              u8=a['median'], nv12=b['median'], u8_spread=round(a['max'] - a['min'], 2), nv12_spread=round(b['max'] - b['min'], 2),
                              holds=bool(b['median'] <= a['median'] + max(a['max'] - a['min'], b['max'] - b['min'])))), flush=True)
        for layout in ('semi', 'planar'):
            b = r['image_transform_yuv420p10_' + layout]
            print(json.dumps(dict(N=N, what='expectation: 10-bit transform (%s) not slower than u8 beyond the spread' % layout,
                                  u8=a['median'], p10=b['median'], u8_spread=round(a['max'] - a['min'], 2), p10_spread=round(b['max'] - b['min'], 2),
                                  holds=bool(b['median'] <= a['median'] + max(a['max'] - a['min'], b['max'] - b['min'])))), flush=True)


if __name__ == '__main__':
    main()
