"""The detection overlay on every YUV surface of the intake (include/lsfa_hip.h "Detection overlay", lsfa_overlay_paint_yuv; DESIGN.md
"Detection overlay", "Every YUV surface") stated in numpy: only the mapping from a pixel's result to the samples of a surface.  The result
itself - the index map - is tests/ref_overlay.py's `plan` and `cover`, the format's fields are tests/ref_yuvfmt.py's.  It is what the device
kernel is compared with bit for bit; tests/test_overlay_fmt_cpu.py pins it by derived answers.

  sample value of a colour component c: the byte c; the 16-bit word c << 2 (sample 1, the low ten bits); the word c << 8 (sample 2)
  luma: Y[y][x] takes component 0 of pixel (x, y)'s result
  chroma: the sample (cx, cy) takes components 1 and 2 of the result of pixel (cx << sx, cy << sy)
  a sample whose pixel is uncovered is not assigned"""
import numpy as np

import ref_overlay
import ref_yuvfmt

SHL = {0: 0, 1: 2, 2: 8}


def code_of(fmt):
    return ref_yuvfmt.NAMES[fmt] if isinstance(fmt, str) else int(fmt)


def paint(fmt, index, colors, y, uv=None, u=None, v=None, width=None):
    """the planes of format `fmt` (a name of ref_yuvfmt.NAMES or a code) as ref_yuvfmt.lay_out gives them, changed in place: uint8, or
    uint16 words; a packed format's one plane is y, `width` its W where that is odd.  index (H, W): ref_overlay.cover's map."""
    c = code_of(fmt)
    assert ref_yuvfmt.valid(c), c
    sub, layout, sample = ref_yuvfmt.fields(c)
    sx, sy = ref_yuvfmt.SHIFTS[sub]
    H, W = index.shape
    dt = ref_yuvfmt.dtype(c)
    value = (np.asarray(colors, np.uint8).astype(np.uint32) << SHL[sample]).astype(dt)          # (ncls + 1, 3) sample values
    planes = [p for p in (y, uv, u, v) if p is not None]
    assert all(p.dtype == dt and p.ndim == 2 for p in planes), [p.dtype for p in planes]
    sub_index = index[::1 << sy, ::1 << sx]          # the result of pixel (cx << sx, cy << sy) at [cy, cx]
    hit, chit = index >= 0, sub_index >= 0
    ch, cw = ref_yuvfmt.chroma_shape(c, H, W)
    assert sub_index.shape == (ch, cw)
    if layout >= ref_yuvfmt.YUYV:
        assert uv is None and u is None and v is None and y.shape == (H, 4 * cw) and width in (None, W)
        yo, uo = (0, 1) if layout == ref_yuvfmt.YUYV else (1, 0)
        Y, U, V = y[:, yo::2][:, :W], y[:, uo::4], y[:, uo + 2::4]          # views: with odd W the last group's second Y is outside Y
    else:
        assert y.shape == (H, W) and width in (None, W)
        Y = y
        if layout == ref_yuvfmt.PLANAR:
            assert uv is None and u.shape == (ch, cw) == v.shape
            U, V = u, v
        else:
            assert u is None and v is None and uv.shape == (ch, 2 * cw)
            first, second = uv[:, 0::2], uv[:, 1::2]
            U, V = (first, second) if layout == ref_yuvfmt.UV else (second, first)
    Y[hit] = value[index[hit], 0]
    U[chit] = value[sub_index[chit], 1]
    V[chit] = value[sub_index[chit], 2]
    return y


def draw(fmt, y, dets, counts, thresh, font, colors, uv=None, u=None, v=None, width=None, **kw):
    """plan + cover + paint of one frame, like ref_overlay.draw_yuv420; kw: thickness, label_scale, with_score, names, max_boxes
    -> (y, records, n)"""
    packed = ref_yuvfmt.fields(code_of(fmt))[1] >= ref_yuvfmt.YUYV
    H = y.shape[0]
    W = y.shape[1] if not packed else (y.shape[1] // 2 if width is None else width)
    recs, n = ref_overlay.plan(dets, counts, thresh, H, W, **kw)
    index = ref_overlay.cover(recs, H, W, np.asarray(dets).shape[0], font, kw.get("thickness", 3), kw.get("label_scale", 2))
    paint(fmt, index, colors, y, uv=uv, u=u, v=v, width=width)
    return y, recs, n
