#!/usr/bin/env python
"""Writes the cases tools/san_yuv10_host.cpp runs: for every geometry of tests/test_yuv10_gpu.py, both chroma layouts, both alignments and
all three matrices, the planes EXACTLY as long as their last sample (no padding behind it) and what tests/ref_yuv10.py says they convert to:
the BGR frame, y_packed, `data` (ref_yuv.transform) and the resized `data` (oracle/np_ref.py's cv2_resize_linear of the converted frame,
padded and transformed as lsfa_image_resize_transform with is_u8 = 1 states it).  No GPU, no library.

    python tools/san_yuv10_cases.py cases.bin

A case: 21 int64 (H, W, N, semi, shift, matrix, y_pitch, y_fs, c_pitch, c_fs, y_off, y_bytes, c_off, c_bytes, out_off, stride, h1, w1, ph, pw,
expect_quad), 5 float64 (im_scale, the three means, pixel_scale), then the blobs: y, u_or_uv, v (planar only), bgr, y_packed, data, resized."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import ref_yuv10          # noqa: E402
from oracle import np_ref          # noqa: E402

MEANS, PS = (102.9801, 115.9465, 122.7717), 0.0125
# (H, W, extra pitch bytes, frames, extra bytes between frames, base offset in bytes, output offset in bytes)
GEOMETRIES = [(2, 4, 0, 1, 0, 0, 0), (6, 8, 0, 1, 0, 0, 0), (16, 32, 0, 1, 0, 0, 0), (1, 1, 0, 1, 0, 0, 0), (7, 9, 0, 1, 0, 0, 0), (5, 4, 0, 1, 0, 0, 0),
              (6, 10, 0, 1, 0, 0, 0), (6, 8, 8, 1, 0, 0, 0), (6, 8, 2, 1, 0, 0, 0), (6, 8, 0, 1, 0, 2, 0), (6, 8, 8, 3, 48, 0, 0), (7, 9, 6, 3, 10, 0, 0),
              (6, 8, 0, 1, 0, 0, 1)]
RESIZES = [(0.5, 0), (0.6, 16), (1.25, 16), (1.25, 0)]


def laid_out(plane, pitch, fs):
    """(N, rows, cols) words -> bytes: rows `pitch` bytes apart, frames `fs` apart, 0xA5 between, nothing behind the last sample"""
    n, rows, cols = plane.shape
    buf = np.full((n - 1) * fs + (rows - 1) * pitch + 2 * cols, 0xA5, np.uint8)
    for i in range(n):
        for r in range(rows):
            at = i * fs + r * pitch
            buf[at:at + 2 * cols] = np.frombuffer(plane[i, r].astype('<u2').tobytes(), np.uint8)
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


def main(path):
    rs = np.random.RandomState(2010)
    count = 0
    with open(path, 'wb') as f:
        for gi, (H, W, extra, N, gap, off, out_off) in enumerate(GEOMETRIES):
            ch, cw = ref_yuv10.chroma_shape(H, W)
            for semi in (1, 0):
                for shift in (6, 0):
                    for matrix in (0, 1, 2):
                        y, u, v = (ref_yuv10.random_words(rs, s) for s in ((N, H, W), (N, ch, cw), (N, ch, cw)))
                        c = ref_yuv10.interleave(u, v) if semi else u
                        y_pitch, c_pitch = 2 * W + extra, 2 * c.shape[-1] + extra
                        y_fs, c_fs = (H * y_pitch + gap, ch * c_pitch + gap) if N > 1 else (0, 0)
                        yb, cb = laid_out(y, y_pitch, y_fs), laid_out(c, c_pitch, c_fs)
                        vb = None if semi else laid_out(v, c_pitch, c_fs)
                        bgr = ref_yuv10.to_bgr(y, u=u, v=v, matrix=matrix, shift=shift)
                        scale, stride = RESIZES[(gi + count) % len(RESIZES)]
                        rdata, (h1, w1, ph, pw) = resized(bgr, scale, stride)
                        if min(h1, w1) < 1:
                            scale, stride = 1.25, 16
                            rdata, (h1, w1, ph, pw) = resized(bgr, scale, stride)
                        aligned = lambda m: (off | y_pitch | y_fs) % m == 0          # noqa: E731
                        c_ok = (c_pitch | c_fs) % (8 if semi else 4) == 0
                        quad = int(W % 4 == 0 and H % 2 == 0 and aligned(8) and c_ok and out_off == 0)
                        np.array([H, W, N, semi, shift, matrix, y_pitch, y_fs, c_pitch, c_fs, off, yb.size, 0, cb.size, out_off, stride, h1, w1, ph, pw,
                                  quad], '<i8').tofile(f)
                        np.array([scale] + list(MEANS) + [PS], '<f8').tofile(f)
                        for blob in [yb, cb] + ([] if semi else [vb]) + [bgr, ref_yuv10.y_packed(y, shift), ref_yuv10.transform(bgr, MEANS, PS).astype('<f4'),
                                                                        rdata.astype('<f4')]:
                            np.ascontiguousarray(blob).tofile(f)
                        count += 1
    print('%d cases -> %s' % (count, path))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else 'san_yuv10_cases.bin')
