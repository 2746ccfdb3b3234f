#!/usr/bin/env python
"""Writes the cases tools/san_yuvfmt_host.cpp runs: for every geometry of tests/test_yuvfmt_gpu.py, every one of the 29 formats and all three
matrices, the planes EXACTLY as long as their last sample (no padding behind it) and what tests/ref_yuvfmt.py says they convert to: the BGR
frame, y_packed, `data` (ref_yuv.transform) and the resized `data` (oracle/np_ref.py's cv2_resize_linear of the converted frame, padded and
transformed as lsfa_image_resize_transform with is_u8 = 1 states it), with the kernel the launch must pick.  No GPU, no library.

    python tools/san_yuvfmt_cases.py cases.bin

A case: 21 int64 (H, W, N, format, chroma planes, matrix, y_pitch, y_fs, c_pitch, c_fs, y_off, y_bytes, c_off, c_bytes, out_off, stride, h1,
w1, ph, pw, expect_quad), 5 float64 (im_scale, the three means, pixel_scale), then the blobs: y, u_or_uv (unless packed), v (planar only),
bgr, y_packed, data, resized."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import ref_yuvfmt as ref          # noqa: E402
from oracle import np_ref          # noqa: E402

MEANS, PS = (102.9801, 115.9465, 122.7717), 0.0125
# (H, W, extra pitch: bytes or 's' for one sample, frames, extra bytes between frames, base offset in samples, output offset in bytes)
GEOMETRIES = [(1, 1, 0, 1, 0, 0, 0), (1, 2, 0, 1, 0, 0, 0), (3, 5, 0, 1, 0, 0, 0), (2, 4, 0, 1, 0, 0, 0), (4, 8, 4, 1, 0, 0, 0), (4, 8, 16, 1, 0, 0, 0),
              (4, 8, 's', 1, 0, 0, 0), (4, 8, 0, 1, 0, 1, 0), (6, 12, 0, 3, 2, 0, 0), (6, 12, 16, 3, 32, 0, 0), (23, 37, 0, 1, 0, 0, 0),
              (4, 8, 0, 1, 0, 0, 1)]
FULL = (600, 1000, 0, 1, 0, 0, 0)
RESIZES = [(0.5, 0), (0.6, 16), (1.25, 16), (1.25, 0)]


def laid_out(plane, pitch, fs):
    """(N, rows, cols) samples -> bytes: rows `pitch` bytes apart, frames `fs` apart, 0xA5 between, nothing behind the last sample"""
    n, rows, cols = plane.shape
    b = plane.dtype.itemsize
    buf = np.full((n - 1) * fs + (rows - 1) * pitch + b * cols, 0xA5, np.uint8)
    for i in range(n):
        for r in range(rows):
            at = i * fs + r * pitch
            buf[at:at + b * cols] = np.frombuffer(plane[i, r].astype('<u2' if b == 2 else np.uint8).tobytes(), np.uint8)
    return buf


def resized(bgr, scale, stride):
    out = []
    for frame in bgr:
        im = np_ref.cv2_resize_linear(frame.astype(np.float32), scale, scale)
        h1, w1 = im.shape[:2]
        if stride:
            ph, pw = -(-h1 // stride) * stride, -(-w1 // stride) * stride
            pad = np.zeros((ph, pw, 3))
            pad[:h1, :w1] = im
            out.append(np.stack([(pad[:, :, 2 - i] - MEANS[2 - i]) * PS for i in range(3)]).astype(np.float32))
        else:
            ph, pw = h1, w1
            out.append(np.stack([(im[:, :, 2 - i] - np.float32(MEANS[2 - i])).astype(np.float32).astype(np.float64) * PS
                                 for i in range(3)]).astype(np.float32))
    return np.stack(out), (h1, w1, ph, pw)


def expect_quad(c, H, W, y_off, y_pitch, y_fs, c_pitch, c_fs, out_off):
    """the header's rule: W % 4 == 0, for 4:2:0 an even H, every base, pitch and frame stride a multiple of the load it feeds"""
    sub, layout, sample = ref.fields(c)
    sx, sy = ref.SHIFTS[sub]
    b = 1 if sample == 0 else 2
    y_load = 8 if layout >= ref.YUYV else 4 * b
    c_load = (1 if layout == ref.PLANAR else 2) * (4 >> sx) * b
    ok = W % 4 == 0 and (sy == 0 or H % 2 == 0) and out_off == 0 and (y_off | y_pitch | y_fs) % y_load == 0
    return int(ok and (layout >= ref.YUYV or (c_pitch | c_fs) % c_load == 0))


def main(path):
    rs = np.random.RandomState(2015)
    count = 0
    with open(path, 'wb') as f:
        for gi, (H, W, extra, N, gap, off, out_off) in enumerate(GEOMETRIES + [FULL]):
            for c in ref.ALL if (H, W) != FULL[:2] else [ref.NAMES['nv16']]:
                _, layout, sample = ref.fields(c)
                b = 1 if sample == 0 else 2
                for matrix in (0, 1, 2) if (H, W) != FULL[:2] else (1,):
                    Y, U, V = ref.random_samples(c, rs, H, W, N)
                    planes = ref.lay_out(c, Y, U, V)
                    ex = b if extra == 's' else extra
                    y = planes['y']
                    y_pitch = y.dtype.itemsize * y.shape[-1] + ex
                    y_fs = H * y_pitch + gap if N > 1 else 0
                    yb = laid_out(y, y_pitch, y_fs)
                    chroma = [planes[k] for k in ('uv', 'u', 'v') if k in planes]
                    c_pitch = c_fs = 0
                    cbs = []
                    if chroma:
                        c_pitch = b * chroma[0].shape[-1] + ex
                        c_fs = chroma[0].shape[-2] * c_pitch + gap if N > 1 else 0
                        cbs = [laid_out(p, c_pitch, c_fs) for p in chroma]
                    bgr = ref.to_bgr(c, matrix=matrix, width=W, **planes)
                    scale, stride = RESIZES[(gi + count) % len(RESIZES)]
                    rdata, (h1, w1, ph, pw) = resized(bgr, scale, stride)
                    if min(h1, w1) < 1:
                        scale, stride = 1.25, 16
                        rdata, (h1, w1, ph, pw) = resized(bgr, scale, stride)
                    y_off = off * (b if layout < ref.YUYV else 1)
                    quad = expect_quad(c, H, W, y_off, y_pitch, y_fs, c_pitch, c_fs, out_off)
                    np.array([H, W, N, c, len(chroma), matrix, y_pitch, y_fs, c_pitch, c_fs, y_off, yb.size, 0, cbs[0].size if cbs else 0, out_off, stride,
                              h1, w1, ph, pw, quad], '<i8').tofile(f)
                    np.array([scale] + list(MEANS) + [PS], '<f8').tofile(f)
                    for blob in [yb] + cbs + [bgr, ref.y_packed(c, planes['y'], W), ref.transform(bgr, MEANS, PS).astype('<f4'), rdata.astype('<f4')]:
                        np.ascontiguousarray(blob).tofile(f)
                    count += 1
    print('%d cases -> %s' % (count, path))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else 'san_yuvfmt_cases.bin')
