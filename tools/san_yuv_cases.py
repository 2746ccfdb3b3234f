#!/usr/bin/env python
"""Writes the cases tools/san_yuv_host.cpp runs through the nine intake exports of lsfa_amd/csrc/yuvfmt.hip, the planes EXACTLY as long as
their last sample (no padding behind it), with what the numpy references say they convert to - the BGR frame, y_packed, `data`
(ref_yuv.transform) and the resized `data` (oracle/np_ref.py's cv2_resize_linear of the converted frame, padded and transformed as
lsfa_image_resize_transform with is_u8 = 1 states it) - and the kernel the launch must pick:

    entry 0  lsfa_*_yuv           every geometry of tests/test_yuvfmt_gpu.py, all 29 formats, all three matrices      tests/ref_yuvfmt.py
    entry 1  lsfa_*yuv420*        every geometry of tests/test_yuv_gpu.py and a few more, NV12 and I420, three matrices  tests/ref_yuv.py
    entry 2  lsfa_*yuv420p10*     every geometry of tests/test_yuv10_gpu.py, both layouts, both alignments, three matrices  tests/ref_yuv10.py

No GPU, no library.

    python tools/san_yuv_cases.py cases.bin

A case: 22 int64 (H, W, N, format, chroma planes, matrix, y_pitch, y_fs, c_pitch, c_fs, y_off, y_bytes, c_off, c_bytes, out_off, stride, h1,
w1, ph, pw, expect_quad, entry), 5 float64 (im_scale, the three means, pixel_scale), then the blobs: y, u_or_uv (unless packed), v (planar
only), bgr, y_packed, data, resized.  The 4:2:0 entries take their layout from the chroma planes and their shift from the format's sample."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import ref_yuv          # noqa: E402
import ref_yuv10          # noqa: E402
import ref_yuvfmt as ref          # noqa: E402
from oracle import np_ref          # noqa: E402

MEANS, PS = (102.9801, 115.9465, 122.7717), 0.0125
# (H, W, extra pitch: bytes or 's' for one sample, frames, extra bytes between frames, base offset in samples, output offset in bytes)
GEOMETRIES = [(1, 1, 0, 1, 0, 0, 0), (1, 2, 0, 1, 0, 0, 0), (3, 5, 0, 1, 0, 0, 0), (2, 4, 0, 1, 0, 0, 0), (4, 8, 4, 1, 0, 0, 0), (4, 8, 16, 1, 0, 0, 0),
              (4, 8, 's', 1, 0, 0, 0), (4, 8, 0, 1, 0, 1, 0), (6, 12, 0, 3, 2, 0, 0), (6, 12, 16, 3, 32, 0, 0), (23, 37, 0, 1, 0, 0, 0),
              (4, 8, 0, 1, 0, 0, 1)]
FULL = (600, 1000, 0, 1, 0, 0, 0)
# the same for the 8-bit 4:2:0 exports: the quad path, W % 4, odd sizes, pitches that keep and that break the load alignment, batches, bases
GEOMETRIES_420 = [(2, 2, 0, 1, 0, 0, 0), (4, 6, 0, 1, 0, 0, 0), (5, 7, 0, 1, 0, 0, 0), (16, 16, 0, 1, 0, 0, 0), (34, 50, 14, 1, 0, 0, 0), (16, 24, 8, 3, 100, 0, 0),
                  (16, 16, 0, 1, 0, 1, 0), (6, 8, 4, 3, 36, 0, 0), (4, 8, 2, 1, 0, 0, 0), (6, 8, 4, 3, 34, 0, 0), (6, 8, 0, 1, 0, 0, 1), (1, 1, 0, 1, 0, 0, 0)]
# ... and for the 10-bit ones (offsets in bytes there)
GEOMETRIES_420P10 = [(2, 4, 0, 1, 0, 0, 0), (6, 8, 0, 1, 0, 0, 0), (16, 32, 0, 1, 0, 0, 0), (1, 1, 0, 1, 0, 0, 0), (7, 9, 0, 1, 0, 0, 0), (5, 4, 0, 1, 0, 0, 0),
                     (6, 10, 0, 1, 0, 0, 0), (6, 8, 8, 1, 0, 0, 0), (6, 8, 2, 1, 0, 0, 0), (6, 8, 0, 1, 0, 2, 0), (6, 8, 8, 3, 48, 0, 0), (7, 9, 6, 3, 10, 0, 0),
                     (6, 8, 0, 1, 0, 0, 1)]
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


class Writer(object):
    def __init__(self, f):
        self.f, self.count = f, 0

    def case(self, entry, c, geometry, matrix, planes, bgr, y_packed, quad=None):
        """one case of format c on `planes` (y and uv | u, v as (N, rows, cols) samples); quad: the entry's own statement of the kernel it
        picks, which must be the header's rule"""
        H, W, extra, N, gap, off, out_off = geometry
        _, layout, sample = ref.fields(c)
        b = 1 if sample == 0 else 2
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
        scale, stride = RESIZES[(geometry[0] + self.count) % len(RESIZES)]
        rdata, (h1, w1, ph, pw) = resized(bgr, scale, stride)
        if min(h1, w1) < 1:
            scale, stride = 1.25, 16
            rdata, (h1, w1, ph, pw) = resized(bgr, scale, stride)
        want_quad = expect_quad(c, H, W, off, y_pitch, y_fs, c_pitch, c_fs, out_off)
        assert quad is None or quad(off, y_pitch, y_fs, c_pitch, c_fs) == want_quad, (entry, hex(c), geometry)
        np.array([H, W, N, c, len(chroma), matrix, y_pitch, y_fs, c_pitch, c_fs, off, yb.size, 0, cbs[0].size if cbs else 0, out_off, stride,
                  h1, w1, ph, pw, want_quad, entry], '<i8').tofile(self.f)
        np.array([scale] + list(MEANS) + [PS], '<f8').tofile(self.f)
        for blob in [yb] + cbs + [bgr, y_packed, ref.transform(bgr, MEANS, PS).astype('<f4'), rdata.astype('<f4')]:
            np.ascontiguousarray(blob).tofile(self.f)
        self.count += 1


def format_cases(w, rs):
    for geometry in GEOMETRIES + [FULL]:
        H, W, _, N, _, off, _ = geometry
        for c in ref.ALL if geometry != FULL else [ref.NAMES['nv16']]:
            _, layout, sample = ref.fields(c)
            for matrix in (0, 1, 2) if geometry != FULL else (1,):
                planes = ref.lay_out(c, *ref.random_samples(c, rs, H, W, N))
                g = geometry[:5] + (off * (2 if sample and layout < ref.YUYV else 1),) + geometry[6:]          # the base offset in bytes
                w.case(0, c, g, matrix, planes, ref.to_bgr(c, matrix=matrix, width=W, **planes), ref.y_packed(c, planes['y'], W))


def cases_420(w, rs):
    """the shipped 8-bit exports: the four-pixel kernel where W % 4 == 0, H is even, Y and NV12 chroma dword aligned, I420 chroma half-word aligned"""
    for geometry in GEOMETRIES_420:
        H, W, _, N, _, _, out_off = geometry
        ch, cw = ref_yuv.chroma_shape(H, W)
        for semi in (1, 0):
            for matrix in (0, 1, 2):
                y, u, v = (rs.randint(0, 256, s).astype(np.uint8) for s in ((N, H, W), (N, ch, cw), (N, ch, cw)))
                planes = dict(y=y, uv=ref_yuv.interleave(u, v)) if semi else dict(y=y, u=u, v=v)

                def quad(off, y_pitch, y_fs, c_pitch, c_fs):
                    return int(W % 4 == 0 and H % 2 == 0 and (off | y_pitch | y_fs) % 4 == 0 and (c_pitch | c_fs) % (4 if semi else 2) == 0 and out_off == 0)
                w.case(1, ref.code(0, ref.UV if semi else ref.PLANAR, 0), geometry, matrix, planes, ref_yuv.to_bgr(y, u=u, v=v, matrix=matrix), y, quad)


def cases_420p10(w, rs):
    """the shipped 10-bit exports: the four-pixel kernel where W % 4 == 0, H is even, Y and interleaved chroma 8-byte, planar chroma 4-byte aligned"""
    for geometry in GEOMETRIES_420P10:
        H, W, _, N, _, _, out_off = geometry
        ch, cw = ref_yuv10.chroma_shape(H, W)
        for semi in (1, 0):
            for shift in (6, 0):
                for matrix in (0, 1, 2):
                    y, u, v = (ref_yuv10.random_words(rs, s) for s in ((N, H, W), (N, ch, cw), (N, ch, cw)))
                    planes = dict(y=y, uv=ref_yuv10.interleave(u, v)) if semi else dict(y=y, u=u, v=v)

                    def quad(off, y_pitch, y_fs, c_pitch, c_fs):
                        return int(W % 4 == 0 and H % 2 == 0 and (off | y_pitch | y_fs) % 8 == 0 and (c_pitch | c_fs) % (8 if semi else 4) == 0 and out_off == 0)
                    w.case(2, ref.code(0, ref.UV if semi else ref.PLANAR, 2 if shift else 1), geometry, matrix, planes,
                           ref_yuv10.to_bgr(y, u=u, v=v, matrix=matrix, shift=shift), ref_yuv10.y_packed(y, shift), quad)


def main(path):
    with open(path, 'wb') as f:
        w = Writer(f)
        format_cases(w, np.random.RandomState(2015))
        cases_420(w, np.random.RandomState(2014))
        cases_420p10(w, np.random.RandomState(2010))
    print('%d cases -> %s' % (w.count, path))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else 'san_yuv_cases.bin')
