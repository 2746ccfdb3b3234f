"""The detection overlay's integer specification (include/lsfa_hip.h "Detection overlay"; DESIGN.md "Detection overlay") stated once in numpy.
It is what the device kernels are compared with bit for bit; tests/test_overlay_cpu.py pins it by cases with known answers.  Nothing here
is cv2's rasteriser: the specification is this project's own.

`plan` turns one image's dets / counts into the ordered records (the device's layout, int for int), `cover` turns records into the colour
index of every pixel (-1: no record covers it), `paint_bgr` / `paint_yuv420` store the covered samples of a surface and leave every other
byte alone.  The glyph table and the colour rows are arguments: lsfa_amd/overlay.py owns the drawings and the palette."""
import math

import numpy as np

REC_INTS, NAME_LEN, MAX_CHARS = 16, 12, 18
SPACE, ZERO, DOT, UNKNOWN, GLYPHS = 0, 1, 39, 41, 42
LIMIT = float(2 ** 30)


def ring(thickness):
    """(o, i): the outline reaches o pixels outwards and i - 1 inwards from the edge"""
    o = (thickness - 1) // 2
    return o, thickness - o


def score_digits(score):
    """m = clamp(floor(score * 1000 + 0.5), 0, 9999); the product is a float64 of its own before the addition"""
    prod = np.float64(score) * np.float64(1000.0)
    return int(min(max(math.floor(prod + np.float64(0.5)), 0), 9999)) if math.isfinite(prod) else (9999 if prod > 0 else 0)


def characters(j, score, label_scale, with_score, names):
    """the glyph indices of a record's label"""
    if label_scale == 0:
        return []
    if names is None:
        ch = [ZERO + int(d) for d in str(j)]
    else:
        ch = []
        for g in np.asarray(names)[j][:NAME_LEN]:
            if g == 0xFF:
                break
            ch.append(int(g) if g < GLYPHS else UNKNOWN)
    if with_score:
        m = score_digits(score)
        ch += [SPACE, ZERO + m // 1000, DOT, ZERO + m // 100 % 10, ZERO + m // 10 % 10, ZERO + m % 10]
    return ch


def plan(dets, counts, thresh, H, W, thickness=3, label_scale=2, with_score=True, names=None, max_boxes=256):
    """one image: dets (ncls, R, 5) float64, counts (ncls) -> (records (k, REC_INTS) int32 in draw order, (recorded, eligible and not skipped))"""
    dets, counts = np.asarray(dets, np.float64), np.asarray(counts)
    ncls, R = dets.shape[:2]
    o, i = ring(thickness)
    recs, kept = [], 0
    for j in range(1, ncls):
        for r in range(min(max(int(counts[j]), 0), R)):
            row = dets[j, r]
            if not np.isfinite(row).all() or not row[4] >= thresh:
                continue
            x1, y1, x2, y2 = (int(min(max(float(v), -LIMIT), LIMIT)) for v in row[:4])          # int() truncates
            if x2 < x1 or y2 < y1 or x2 < 0 or y2 < 0 or x1 > W - 1 or y1 > H - 1:
                continue
            kept += 1
            if kept > max_boxes:
                continue
            ch = characters(j, row[4], label_scale, with_score, names)
            L = len(ch)
            lx = ly = w = h = 0
            if L:
                w, h = label_scale * (6 * L + 1), 9 * label_scale
                lx, ly = x1 - o, y1 - o - h
                if ly < 0:
                    ly = y1 + i
                if lx + w > W:
                    lx = W - w
                if lx < 0:
                    lx = 0
            packed = [0] * (REC_INTS - 10)
            for k, g in enumerate(ch):
                packed[k // 4] |= g << (8 * (k % 4))
            recs.append([x1, y1, x2, y2, lx, ly, w, h, j, L] + packed)
    return np.array(recs, np.int64).reshape(-1, REC_INTS).astype(np.int32), (min(kept, max_boxes), kept)


def _clip(lo, hi, size):
    """the inclusive range [lo, hi] cut to [0, size - 1] as a slice (possibly empty)"""
    lo, hi = max(int(lo), 0), min(int(hi), size - 1)
    return slice(lo, max(hi + 1, lo))


def cover(records, H, W, ncls, font, thickness=3, label_scale=2):
    """(H, W) int32: the colour index of every pixel - class j, ncls for a text pixel, -1 where no record covers it.  Records are painted in
    draw order, each over what is there: the last record that contains a pixel gives its result."""
    font = np.asarray(font).reshape(GLYPHS, 8)
    o, i = ring(thickness)
    z = label_scale
    out = np.full((H, W), -1, np.int32)
    for rec in np.asarray(records).reshape(-1, REC_INTS).tolist():
        x1, y1, x2, y2, lx, ly, w, h, j, L = rec[:10]
        ys, xs = _clip(y1 - o, y2 + o, H), _clip(x1 - o, x2 + o, W)
        mask = np.ones((ys.stop - ys.start, xs.stop - xs.start), bool)
        if x1 + i <= x2 - i and y1 + i <= y2 - i:
            iy, ix = _clip(y1 + i, y2 - i, H), _clip(x1 + i, x2 - i, W)
            if iy.stop > iy.start and ix.stop > ix.start:
                mask[iy.start - ys.start:iy.stop - ys.start, ix.start - xs.start:ix.stop - xs.start] = False
        view = out[ys, xs]
        view[mask] = j
        if L == 0 or w == 0:
            continue
        ch = [(rec[10 + k // 4] >> (8 * (k % 4))) & 255 for k in range(L)]
        ys, xs = _clip(ly, ly + h - 1, H), _clip(lx, lx + w - 1, W)
        yy, xx = np.meshgrid(np.arange(ys.start, ys.stop), np.arange(xs.start, xs.stop), indexing="ij")
        dx, dy = xx - lx - z, yy - ly - z
        u, v = dx // z, dy // z
        inside = (dx >= 0) & (dy >= 0) & (u < 6 * L) & (u % 6 < 5) & (v < 7)
        g = np.asarray(ch + [0])[np.where(inside, u // 6, L)]
        bits = font[g, np.where(inside, v, 7)] >> np.where(inside, 4 - u % 6, 0) & 1
        out[ys, xs] = np.where(inside & (bits == 1), ncls, j)
    return out


def paint_bgr(frame, index, colors):
    """frame (H, W, 3) uint8 changed in place: covered pixels take their colour row, every other byte stays"""
    colors = np.asarray(colors, np.uint8)
    hit = index >= 0
    frame[hit] = colors[index[hit]]
    return frame


def paint_yuv420(y, index, colors, uv=None, u=None, v=None):
    """y (H, W) and uv (ceil(H/2), 2 ceil(W/2)) or u, v (ceil(H/2), ceil(W/2)) uint8, changed in place: Y[y][x] takes component 0 of pixel
    (x, y)'s result, the chroma sample (cx, cy) components 1 and 2 of pixel (2cx, 2cy)'s; an uncovered pixel's samples stay"""
    colors = np.asarray(colors, np.uint8)
    hit = index >= 0
    y[hit] = colors[index[hit], 0]
    sub = index[::2, ::2]
    chit = sub >= 0
    if uv is not None:
        uv[:, 0::2][chit] = colors[sub[chit], 1]
        uv[:, 1::2][chit] = colors[sub[chit], 2]
    else:
        u[chit] = colors[sub[chit], 1]
        v[chit] = colors[sub[chit], 2]
    return y


def draw_bgr(frame, dets, counts, thresh, font, colors, **kw):
    """plan + cover + paint_bgr of one frame; kw: thickness, label_scale, with_score, names, max_boxes -> (frame, records, n)"""
    H, W = frame.shape[:2]
    recs, n = plan(dets, counts, thresh, H, W, **kw)
    index = cover(recs, H, W, np.asarray(dets).shape[0], font, kw.get("thickness", 3), kw.get("label_scale", 2))
    return paint_bgr(frame, index, colors), recs, n


def draw_yuv420(y, dets, counts, thresh, font, colors, uv=None, u=None, v=None, **kw):
    H, W = y.shape
    recs, n = plan(dets, counts, thresh, H, W, **kw)
    index = cover(recs, H, W, np.asarray(dets).shape[0], font, kw.get("thickness", 3), kw.get("label_scale", 2))
    paint_yuv420(y, index, colors, uv=uv, u=u, v=v)
    return y, recs, n
