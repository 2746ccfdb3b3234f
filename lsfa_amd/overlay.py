"""Detection overlay on torch tensors: the ctypes wrappers of lsfa_overlay_plan, lsfa_overlay_paint_bgr, lsfa_overlay_paint_yuv420 and
lsfa_overlay_paint_yuv (lsfa_amd/csrc/overlay.hip; include/lsfa_hip.h, "Detection overlay"), the glyphs they draw with, the palette and
the YUV colour rows.  Built on lsfa_amd/hip.py's binding and checkers and under its rule: every tensor is validated before its pointer is taken, and there is no
fallback - a missing library or a refused call is an LsfaError.

The detections stay where lsfa_det_postprocess(_batch) left them - dets (ncls, R, 5) float64 and counts (ncls) int32, or (N, ..) of a
batch - and are burnt into a frame that is on the device already: packed BGR (H, W, 3) / (N, H, W, 3) uint8, or the 8-bit 4:2:0 planes
the YUV intake takes (y and uv of NV12, or y, u and v of I420), or - draw_yuv - the planes of any format of lsfa_amd/yuvfmt.py: 4:2:2,
4:4:4, V before U, packed YUYV / UYVY, ten-bit words.  Row views of pitched surfaces are taken as they are: pitch and frame
stride come from .stride().  Nothing is read back and nothing is allocated by a draw call, so the two launches can be captured in a graph.
With ids=, the track ids lsfa_amd/tracks.py assigns, the plan is lsfa_overlay_plan_ids: one colour and one number per object.

This is the project's own integer specification (the header; DESIGN.md "Detection overlay"; tests/ref_overlay.py in numpy), not cv2's
rasteriser: no Hershey fonts, no anti-aliasing, and a fixed palette where the reference's draw_boxes picks random colours."""
import numpy as np
import torch

from lsfa_amd import hip, yuvfmt
from lsfa_amd.hip import LsfaError, _check, _ptr, _tensor

REC_INTS = 16               # LSFA_OVERLAY_REC_INTS
NAME_LEN = 12               # LSFA_OVERLAY_NAME_LEN
GLYPH_BYTES = 336           # LSFA_OVERLAY_GLYPH_BYTES
MAX_BOXES = 4096            # LSFA_OVERLAY_MAX_BOXES
MAX_CLASSES = 4096          # LSFA_OVERLAY_MAX_CLASSES
NAME_END = 0xFF

# The glyphs: 5 x 7 in a 6 x 8 cell, this project's own drawings, stated once.  CHARSET[k] is drawn by the k-th block of seven rows.
CHARSET = " 0123456789abcdefghijklmnopqrstuvwxyz_-.%?"
GLYPH_ART = """
.....  .###.  ..#..  .###.  ####.  ...#.  #####  ..##.  #####  .###.  .###.
.....  #...#  .##..  #...#  ....#  ..##.  #....  .#...  ....#  #...#  #...#
.....  #..##  ..#..  ....#  ....#  .#.#.  ####.  #....  ...#.  #...#  #...#
.....  #.#.#  ..#..  ..##.  .###.  #..#.  ....#  ####.  ..#..  .###.  .####
.....  ##..#  ..#..  .#...  ....#  #####  ....#  #...#  .#...  #...#  ....#
.....  #...#  ..#..  #....  ....#  ...#.  #...#  #...#  .#...  #...#  ...#.
.....  .###.  .###.  #####  ####.  ...#.  .###.  .###.  .#...  .###.  .##..

.....  #....  .....  ....#  .....  ..##.  .....  #....  ..#..  ...#.  #....  .##..  .....
.....  #....  .....  ....#  .....  .#..#  .####  #....  .....  .....  #....  ..#..  .....
.###.  ####.  .###.  .####  .###.  .#...  #...#  #.##.  .##..  ..##.  #..#.  ..#..  ##.#.
....#  #...#  #....  #...#  #...#  ###..  #...#  ##..#  ..#..  ...#.  #.#..  ..#..  #.#.#
.####  #...#  #....  #...#  #####  .#...  .####  #...#  ..#..  ...#.  ##...  ..#..  #.#.#
#...#  #...#  #...#  #...#  #....  .#...  ....#  #...#  ..#..  #..#.  #.#..  ..#..  #.#.#
.####  ####.  .###.  .####  .###.  .#...  .###.  #...#  .###.  .##..  #..#.  .###.  #...#

.....  .....  .....  .....  .....  .....  .#...  .....  .....  .....  .....  .....  .....
.....  .....  .....  .....  .....  .....  .#...  .....  .....  .....  .....  .....  .....
#.##.  .###.  ####.  .####  #.##.  .####  ###..  #...#  #...#  #...#  #...#  #...#  #####
##..#  #...#  #...#  #...#  ##..#  #....  .#...  #...#  #...#  #.#.#  .#.#.  #...#  ...#.
#...#  #...#  ####.  .####  #....  .###.  .#...  #...#  #...#  #.#.#  ..#..  .####  ..#..
#...#  #...#  #....  ....#  #....  ....#  .#..#  #..##  .#.#.  #.#.#  .#.#.  ....#  .#...
#...#  .###.  #....  ....#  #....  ####.  ..##.  .##.#  ..#..  .#.#.  #...#  .###.  #####

.....  .....  .....  ##..#  .###.
.....  .....  .....  ##.#.  #...#
.....  .....  .....  ...#.  ....#
.....  #####  .....  ..#..  ...#.
.....  .....  .....  .#...  ..#..
.....  .....  .##..  .#.##  .....
#####  .....  .##..  #..##  ..#..
"""


def _glyph_rows():
    """GLYPH_ART -> 42 tuples of seven five-character rows, in CHARSET's order"""
    glyphs = []
    for block in GLYPH_ART.strip("\n").split("\n\n"):
        rows = [line.split() for line in block.split("\n")]
        if len(rows) != 7 or len(set(len(r) for r in rows)) != 1:
            raise AssertionError("a block of GLYPH_ART is seven rows of equally many glyphs")
        glyphs += [tuple(r[k] for r in rows) for k in range(len(rows[0]))]
    if len(glyphs) != len(CHARSET) or any(len(row) != 5 or set(row) - set("#.") for g in glyphs for row in g):
        raise AssertionError("GLYPH_ART draws %d glyphs of 5 x 7 for the %d characters" % (len(glyphs), len(CHARSET)))
    return glyphs


GLYPHS = _glyph_rows()


def font_table():
    """the `font` argument: (42, 8) uint8, glyph g's row v at [g, v] with bit 4 its left column; row 7 is the cell's empty line"""
    t = np.zeros((len(GLYPHS), 8), np.uint8)
    for g, rows in enumerate(GLYPHS):
        for v, row in enumerate(rows):
            t[g, v] = sum(1 << (4 - c) for c in range(5) if row[c] == "#")
    return t


def glyph_indices(text):
    """the glyph index of every character of `text`: upper case folds to lower case, a character outside CHARSET becomes '?'"""
    return [CHARSET.index(c) if c in CHARSET else CHARSET.index("?") for c in str(text).lower()]


def name_table(names, ncls):
    """(ncls, NAME_LEN) uint8 for the `names` argument: row j holds the first NAME_LEN glyph indices of names[j], ended by 0xFF"""
    if len(names) != ncls:
        raise LsfaError("overlay: %d names for %d classes (class 0, the background, has a row too)" % (len(names), ncls))
    t = np.full((ncls, NAME_LEN), NAME_END, np.uint8)
    for j, name in enumerate(names):
        idx = glyph_indices(name)[:NAME_LEN]
        t[j, :len(idx)] = idx
    return t


def palette(ncls):
    """(ncls + 1, 3) uint8 B, G, R: class j's colour deals the bits of j to R, G, B from bit 7 down; row ncls, the text colour, is white"""
    t = np.zeros((ncls + 1, 3), np.uint8)
    for j in range(ncls):
        r = g = b = 0
        c = j
        for k in range(8):
            r |= (c & 1) << (7 - k)
            g |= (c >> 1 & 1) << (7 - k)
            b |= (c >> 2 & 1) << (7 - k)
            c >>= 3
        t[j] = (b, g, r)
    t[ncls] = 255
    return t


# (Y row, U row, V row) over (R, G, B), the offset of Y: the mirrors of the three intake matrices; the chroma rows sum to zero
_TO_YUV = {
    'bt601': ((66, 129, 25), (-38, -74, 112), (112, -94, -18), 16),
    'bt709': ((47, 157, 16), (-26, -86, 112), (112, -102, -10), 16),
    'jpeg': ((77, 150, 29), (-43, -85, 128), (128, -107, -21), 0),
}


def bgr_to_yuv(colors, matrix='bt601'):
    """(.., 3) uint8 B, G, R -> (.., 3) uint8 Y, U, V by the integer matrix that mirrors the intake's: ((row . RGB + 128) >> 8) + offset,
    clipped to 0..255"""
    if matrix not in _TO_YUV:
        raise LsfaError("bgr_to_yuv: matrix %r is not one of %s" % (matrix, sorted(_TO_YUV)))
    c = np.asarray(colors).astype(np.int64)
    b, g, r = c[..., 0], c[..., 1], c[..., 2]
    ry, ru, rv, off = _TO_YUV[matrix]
    planes = [((k[0] * r + k[1] * g + k[2] * b + 128) >> 8) + o for k, o in ((ry, off), (ru, 128), (rv, 128))]
    return np.clip(np.stack(planes, -1), 0, 255).astype(np.uint8)


def _upload(a, device):
    t = torch.empty(a.shape, dtype=torch.uint8, device=device)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


class Overlay(object):
    """Draws the detections of up to `batch` images of `ncls` classes x `R` rows.  The font, the names and the colours (B, G, R and the
    three Y, U, V forms) are uploaded once and the record buffers (batch, max_boxes, REC_INTS) and n (batch, 2) are made here; a draw call
    is lsfa_overlay_plan and one paint launch and allocates nothing.
      names: ncls strings (class 0 too), drawn by their first NAME_LEN characters; None: the class id in decimal
      colors: (ncls + 1, 3) B, G, R with the text colour last; None: palette(ncls)
      thickness 1..8, label_scale 0..4 (0: no label), with_score: ' d.ddd' behind the name"""

    def __init__(self, ncls, R, max_boxes=256, thickness=3, label_scale=2, names=None, with_score=True, colors=None, device='cuda:0', batch=1):
        for what, v, lo, hi in (("ncls", ncls, 1, MAX_CLASSES), ("R", R, 1, 1 << 24), ("max_boxes", max_boxes, 1, MAX_BOXES), ("thickness", thickness, 1, 8),
                                ("label_scale", label_scale, 0, 4), ("batch", batch, 1, 65535)):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise LsfaError("Overlay: %s %r is not an int in %d..%d" % (what, v, lo, hi))
        self.ncls, self.R, self.max_boxes, self.thickness, self.label_scale, self.batch = ncls, R, max_boxes, thickness, label_scale, batch
        self.with_score = bool(with_score)
        self.device = torch.device(device)
        bgr = palette(ncls) if colors is None else np.asarray(colors)
        if bgr.shape != (ncls + 1, 3) or bgr.dtype != np.uint8:
            raise LsfaError("Overlay: colors must be (%d, 3) uint8 B, G, R with the text colour last, got %s %s" % (ncls + 1, bgr.shape, bgr.dtype))
        self._font = _upload(font_table(), self.device)
        self._names = None if names is None else _upload(name_table(list(names), ncls), self.device)
        self._bgr = _upload(bgr, self.device)
        self._yuv = {m: _upload(bgr_to_yuv(bgr, m), self.device) for m in sorted(_TO_YUV)}
        self.records = torch.zeros((batch, max_boxes, REC_INTS), dtype=torch.int32, device=self.device)
        self.n = torch.zeros((batch, 2), dtype=torch.int32, device=self.device)

    def _plan(self, who, N, batched, H, W, dets, counts, thresh, ids=None):
        """validates dets / counts (and ids) against the frames' N and launches lsfa_overlay_plan, or lsfa_overlay_plan_ids with ids"""
        lead = (N,) if batched else ()
        if N > self.batch:
            raise LsfaError("%s: %d frames, this Overlay was made for a batch of %d" % (who, N, self.batch))
        _tensor(who, "dets", dets, torch.float64, lead + (self.ncls, self.R, 5), self.device)
        _tensor(who, "counts", counts, torch.int32, lead + (self.ncls,), self.device)
        if ids is not None:
            if self.ncls < 2:
                raise LsfaError("%s: ids need at least 2 classes: a track's colour is one of the classes 1..ncls-1" % who)
            _tensor(who, "ids", ids, torch.int32, lead + (self.ncls, self.R), self.device)
            _check(hip.lib().lsfa_overlay_plan_ids(_ptr(dets), _ptr(counts), _ptr(ids), N, self.ncls, self.R, float(thresh), H, W, self.thickness,
                                                   self.label_scale, 1 if self.with_score else 0, _ptr(self._names), self.max_boxes,
                                                   _ptr(self.records), _ptr(self.n), hip._stream()), "lsfa_overlay_plan_ids")
            return
        _check(hip.lib().lsfa_overlay_plan(_ptr(dets), _ptr(counts), N, self.ncls, self.R, float(thresh), H, W, self.thickness, self.label_scale,
                                           1 if self.with_score else 0, _ptr(self._names), self.max_boxes, _ptr(self.records), _ptr(self.n),
                                           hip._stream()), "lsfa_overlay_plan")

    @hip._on_tensor_device
    def draw_bgr(self, frames, dets, counts, thresh, ids=None):
        """frames (H, W, 3) or (N, H, W, 3) uint8, drawn into in place; pixels are packed (strides 3 and 1), rows and frames may be pitched.
        dets (ncls, R, 5) float64 and counts (ncls) int32 of one frame, (N, ..) of a batch.  ids (ncls, R) / (N, ncls, R) int32, a Tracker's:
        only rows with an id above 0 are drawn, in the track's colour, labelled name-id.  Returns frames."""
        who = "Overlay.draw_bgr"
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.device != self.device or frames.dim() not in (3, 4) or \
                int(frames.shape[-1]) != 3 or frames.stride(-1) != 1 or frames.stride(-2) != 3 or min(frames.shape) < 1:
            raise LsfaError("%s: frames must be a (H, W, 3) or (N, H, W, 3) uint8 tensor on %s with packed pixels, got %s strides %s" %
                            (who, self.device, hip._arrived(frames), tuple(frames.stride()) if isinstance(frames, torch.Tensor) else None))
        batched = frames.dim() == 4
        N, H, W = int(frames.shape[0]) if batched else 1, int(frames.shape[-3]), int(frames.shape[-2])
        pitch = int(frames.stride(-3)) if H > 1 else max(int(frames.stride(-3)), 3 * W)
        fs = int(frames.stride(0)) if batched and N > 1 else 0
        if pitch < 3 * W or fs < 0:
            raise LsfaError("%s: a row pitch is below its row: %s strides %s" % (who, tuple(frames.shape), tuple(frames.stride())))
        self._plan(who, N, batched, H, W, dets, counts, thresh, ids)
        _check(hip.lib().lsfa_overlay_paint_bgr(_ptr(frames), pitch, fs, N, H, W, _ptr(self.records), _ptr(self.n), self.max_boxes, self.thickness,
                                                self.label_scale, _ptr(self._font), _ptr(self._bgr), self.ncls, hip._stream()),
               "lsfa_overlay_paint_bgr")
        return frames

    @hip._on_tensor_device
    def draw_yuv420(self, y, dets, counts, thresh, uv=None, u=None, v=None, matrix='bt601', ids=None):
        """the planes of hip.yuv420_to_bgr_u8 - y and uv (NV12) or y, u and v (I420), one frame or (N, ..) - drawn into in place with the
        colours converted by `matrix`, the matrix the stream is decoded with.  dets / counts / ids as draw_bgr."""
        who = "Overlay.draw_yuv420"
        args, N, H, W, batched = hip._yuv_planes(who, y, uv, u, v, matrix)
        if y.device != self.device:
            raise LsfaError("%s: the planes are on %s, this Overlay on %s" % (who, y.device, self.device))
        self._plan(who, N, batched, H, W, dets, counts, thresh, ids)
        _check(hip.lib().lsfa_overlay_paint_yuv420(*(args[:10] + (_ptr(self.records), _ptr(self.n), self.max_boxes, self.thickness, self.label_scale,
                                                                  _ptr(self._font), _ptr(self._yuv[matrix]), self.ncls, hip._stream()))),
               "lsfa_overlay_paint_yuv420")
        return y

    @hip._on_tensor_device
    def draw_yuv(self, fmt, y, dets, counts, thresh, uv=None, u=None, v=None, matrix='bt601', ids=None, width=None):
        """the planes of yuvfmt.yuv_to_bgr_u8 in any of its formats - `fmt` a name of yuvfmt.FORMATS or a code; uint8 planes, or int16 /
        uint16 words of ten bits; a packed format's one plane as y, with `width` where W is odd - drawn into in place with the colours
        converted by `matrix`.  A ten-bit surface takes the 8-bit colour as c << 2 (low ten bits) or c << 8 (high ten), the whole word
        stored, so it reads back through the intake as the same BGR.  dets / counts / ids as draw_bgr.  Returns y."""
        who = "Overlay.draw_yuv"
        args, N, H, W, batched = yuvfmt._planes(who, fmt, y, uv, u, v, matrix, width)
        if y.device != self.device:
            raise LsfaError("%s: the planes are on %s, this Overlay on %s" % (who, y.device, self.device))
        self._plan(who, N, batched, H, W, dets, counts, thresh, ids)
        _check(hip.lib().lsfa_overlay_paint_yuv(*(args[:10] + (args[11], _ptr(self.records), _ptr(self.n), self.max_boxes, self.thickness,
                                                               self.label_scale, _ptr(self._font), _ptr(self._yuv[matrix]), self.ncls,
                                                               hip._stream()))),
               "lsfa_overlay_paint_yuv")
        return y

    def drawn(self):
        """n of the last draw call, read back: (batch, 2) int32 numpy, per image {records drawn, eligible rows that were not skipped}; the
        one synchronising call of this class"""
        return self.n.cpu().numpy()
