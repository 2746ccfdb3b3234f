"""YUV intake for the other chroma formats on torch tensors: the ctypes wrappers of lsfa_yuv_to_bgr_u8, lsfa_image_transform_yuv and
lsfa_image_resize_transform_yuv (lsfa_amd/csrc/yuvfmt.hip; include/lsfa_hip.h, "YUV intake, other chroma formats") and the two motion
estimators on such frames.  Built on lsfa_amd/hip.py's binding and checkers and under its rule: every tensor is validated before its pointer
is taken, and there is no fallback - a missing library or a refused call is an LsfaError.

A format is a name of FORMATS (libav's pix_fmt names where there is one) or a code sub | layout << 4 | sample << 8 of the header.  Planes are
CUDA tensors of torch.uint8 (bytes) or torch.int16 / torch.uint16 (16-bit words; the bits count, not the sign): y (H, W) or (N, H, W) and
either u, v (.., ch, cw) - two planes - or uv (.., ch, 2 cw) - one interleaved plane, U first or V first as the format says - with
ch = ceil(H / 2^sy), cw = ceil(W / 2^sx).  A packed format (yuyv422, uyvy422) has one plane: y is the (.., H, 4 ceil(W / 2)) plane of
four-byte groups and `width` says W where it is odd (the default is the even 2 * groups).  Row views of pitched surfaces (`y[:, :W]`) are
taken as they are: pitch and frame stride come from .stride()."""
import torch

from lsfa_amd import hip
from lsfa_amd.hip import LsfaError, _check, _means, _ptr

SUB_420, SUB_422, SUB_444 = 0, 1, 2
PLANAR, UV, VU, YUYV, UYVY = 0, 1, 2, 3, 4
U8, LO10, HI10 = 0, 1, 2
_SHIFTS = {SUB_420: (1, 1), SUB_422: (1, 0), SUB_444: (0, 0)}


def code(sub, layout, sample):
    """LSFA_YUV_FORMAT of the header"""
    return sub | layout << 4 | sample << 8


FORMATS = {
    'nv12': code(SUB_420, UV, U8), 'i420': code(SUB_420, PLANAR, U8), 'nv21': code(SUB_420, VU, U8),
    'yuv422p': code(SUB_422, PLANAR, U8), 'nv16': code(SUB_422, UV, U8), 'nv61': code(SUB_422, VU, U8),
    'yuyv422': code(SUB_422, YUYV, U8), 'yuy2': code(SUB_422, YUYV, U8), 'uyvy422': code(SUB_422, UYVY, U8),
    'yuv444p': code(SUB_444, PLANAR, U8), 'nv24': code(SUB_444, UV, U8), 'nv42': code(SUB_444, VU, U8),
    'p010': code(SUB_420, UV, HI10), 'yuv420p10le': code(SUB_420, PLANAR, LO10),
    'yuv422p10le': code(SUB_422, PLANAR, LO10), 'p210': code(SUB_422, UV, HI10),
    'yuv444p10le': code(SUB_444, PLANAR, LO10), 'p410': code(SUB_444, UV, HI10),
}


def fields(fmt):
    """a name of FORMATS or a code -> (code, sub, layout, sample), checked: 27 + 2 codes are formats"""
    c = FORMATS.get(fmt, fmt) if isinstance(fmt, str) else fmt
    if isinstance(c, bool) or not isinstance(c, int):
        raise LsfaError("yuvfmt: format %r is not one of %s or a code sub | layout << 4 | sample << 8" % (fmt, ", ".join(sorted(FORMATS))))
    sub, layout, sample = c & 15, (c >> 4) & 15, (c >> 8) & 15
    if c < 0 or c >> 12 or sub > SUB_444 or layout > UYVY or sample > HI10 or (layout >= YUYV and (sub != SUB_422 or sample != U8)):
        raise LsfaError("yuvfmt: format %r is not a valid code: sub 0..2 | layout 0..4 << 4 | sample 0..2 << 8, packed layouts only as 4:2:2 of "
                        "bytes" % (fmt,))
    return c, sub, layout, sample


def chroma_shape(fmt, height, width):
    """(rows, columns) of a chroma plane in chroma samples"""
    sx, sy = _SHIFTS[fields(fmt)[1]]
    return -(-height // (1 << sy)), -(-width // (1 << sx))


def frame_bytes(fmt, width, height):
    """the bytes of one frame as `ffmpeg -f rawvideo -pix_fmt X` writes it: planes back to back, no pitch"""
    _, _, layout, sample = fields(fmt)
    b = 1 if sample == U8 else 2
    if layout >= YUYV:
        return height * 4 * -(-width // 2)
    ch, cw = chroma_shape(fmt, height, width)
    return b * (height * width + 2 * ch * cw)


def _planes(who, fmt, y, uv, u, v, matrix, width):
    """The plane arguments of the lsfa_*_yuv exports: hip._yuv_planes at the format's fields, then `format`"""
    try:
        c, sub, layout, sample = fields(fmt)
    except LsfaError as e:
        raise LsfaError("%s: %s" % (who, e))
    args, N, H, W, batched = hip._yuv_planes(who, y, uv, u, v, matrix, sub, layout, sample != U8, width, fmt)
    return args + (c,), N, H, W, batched


@hip._on_tensor_device
def yuv_to_bgr_u8(fmt, y, uv=None, u=None, v=None, matrix='bt601', out=None, y_packed=None, width=None):
    """lsfa_yuv_to_bgr_u8: a frame of format `fmt` on the device (see the module docstring) to packed uint8 BGR (H, W, 3) / (N, H, W, 3), the
    layout lsfa_mv_residual, luma_u8 and image_transform_u8 take.  matrix as hip.yuv420_to_bgr_u8; nearest-neighbour chroma, integer
    arithmetic (include/lsfa_hip.h - this project's own specification, not swscale's).  y_packed: an optional (.., H, W) uint8 tensor that
    receives the luma as 8 bits (Y of bytes; min(255, (Y + 2) >> 2) of ten-bit samples): what mv_estimate searches.  One launch."""
    who = "yuv_to_bgr_u8"
    args, N, H, W, batched = _planes(who, fmt, y, uv, u, v, matrix, width)
    out = hip._yuv_bgr_out(who, N, H, W, batched, y.device, out, y_packed)
    _check(hip.lib().lsfa_yuv_to_bgr_u8(*(args + (_ptr(out), _ptr(y_packed), hip._stream()))), "lsfa_yuv_to_bgr_u8")
    return out


@hip._on_tensor_device
def image_transform_yuv(fmt, y, uv=None, u=None, v=None, matrix='bt601', pixel_means=(0.0, 0.0, 0.0), pixel_scale=1.0, out=None, width=None):
    """lsfa_image_transform_yuv: the planes of yuv_to_bgr_u8 -> `data` (N, 3, H, W) float32: bit-identical to
    hip.image_transform_u8(yuv_to_bgr_u8(...)) without storing the BGR frame, and without its H*W % 4 condition.  One launch."""
    who = "image_transform_yuv"
    args, N, H, W, _ = _planes(who, fmt, y, uv, u, v, matrix, width)
    out = hip._yuv_out(who, out, (N, 3, H, W), torch.float32, y.device)
    _check(hip.lib().lsfa_image_transform_yuv(*(args + (_means(pixel_means), float(pixel_scale), _ptr(out), hip._stream()))),
           "lsfa_image_transform_yuv")
    return out


@hip._on_tensor_device
def image_resize_transform_yuv(fmt, y, uv=None, u=None, v=None, im_scale=1.0, matrix='bt601', pixel_means=(0.0, 0.0, 0.0), pixel_scale=1.0,
                               stride=0, out=None, width=None):
    """lsfa_image_resize_transform_yuv: the planes of yuv_to_bgr_u8 -> `data` (N, 3, h, w) float32: hip.image_resize_transform of the
    converted uint8 frame, bit-identical to it, reading the taps from the planes.  One launch."""
    who = "image_resize_transform_yuv"
    args, N, H, W, _ = _planes(who, fmt, y, uv, u, v, matrix, width)
    stride, h1, w1, ph, pw, out = hip._yuv_resized_out(who, N, H, W, im_scale, stride, y.device, out)
    _check(hip.lib().lsfa_image_resize_transform_yuv(*(args + (float(im_scale), h1, w1, stride, _means(pixel_means), float(pixel_scale), _ptr(out),
                                                               ph, pw, hip._stream()))),
           "lsfa_image_resize_transform_yuv")
    return out


class _Formatted(object):
    """the two hooks of hip._SearchFront for a frame of self.fmt: the conversion, and the shape of the `y` argument (a packed row is
    4 ceil(W / 2) bytes wide)"""

    def _set_format(self, who, fmt):
        try:
            self._packed = fields(fmt)[2] >= YUYV
        except LsfaError as e:
            raise LsfaError("%s: %s" % (who, e))
        self.fmt = fmt

    def _to_bgr(self, y, uv, u, v, matrix, out=None, y_packed=None):
        return yuv_to_bgr_u8(self.fmt, y, uv, u, v, matrix, out=out, y_packed=y_packed, width=self.width)

    def _y_plane(self):
        return (self.height, 4 * -(-self.width // 2)) if self._packed else (self.height, self.width)


class MotionEstimatorYuv(_Formatted, hip.MotionEstimator):
    """hip.MotionEstimator whose key_frame_yuv / next_frame_yuv take frames of format `fmt` (yuv_to_bgr_u8's planes; a packed format's one
    plane as y).  Everything behind the conversion is the shipped estimator's: luma_from='bgr' searches lsfa_luma_u8 of the converted frame,
    luma_from='y' the frame's own luma as 8 bits (the conversion's y_packed, no luma launch).  Nothing is allocated after the first *_yuv call."""

    def __init__(self, width, height, device='cuda:0', fmt='nv12', **kw):
        self._set_format("MotionEstimatorYuv", fmt)
        hip.MotionEstimator.__init__(self, width, height, device, **kw)


class SegmentMotionEstimatorYuv(_Formatted, hip.SegmentMotionEstimator):
    """hip.SegmentMotionEstimator whose segment_yuv takes frames of format `fmt`: y (C * (n + 1), ..) and uv | u, v, one conversion launch"""

    def __init__(self, width, height, frames=9, clips=1, device='cuda:0', fmt='nv12', **kw):
        self._set_format("SegmentMotionEstimatorYuv", fmt)
        hip.SegmentMotionEstimator.__init__(self, width, height, frames, clips, device, **kw)
