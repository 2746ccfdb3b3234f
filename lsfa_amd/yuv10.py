"""10-bit YUV 4:2:0 intake on torch tensors: the ctypes wrappers of lsfa_yuv420p10_to_bgr_u8, lsfa_image_transform_yuv420p10 and
lsfa_image_resize_transform_yuv420p10 (lsfa_amd/csrc/yuvfmt.hip; include/lsfa_hip.h, "10-bit YUV 4:2:0 intake") and the two motion
estimators on such planes.  Built on lsfa_amd/hip.py's binding and checkers and under its rule: every tensor is validated before its pointer
is taken, and there is no fallback - a missing library or a refused call is an LsfaError.

Planes are torch.int16 or torch.uint16 CUDA tensors of 16-bit words (the bits count, not the sign): y (H, W) or (N, H, W) and either uv
(.., ceil(H/2), 2 ceil(W/2)) - interleaved U, V words, P010's layout - or u, v (.., ceil(H/2), ceil(W/2)).  msb_aligned=True reads the
sample from the high ten bits of a word (P010 / P016 surfaces), False from the low ten (yuv420p10le / I010); either goes with either layout.
Row views of pitched surfaces (`y[:, :W]`) are taken as they are: pitch and frame stride come from .stride(), times two bytes."""
import torch

from lsfa_amd import hip
from lsfa_amd.hip import LsfaError, _check, _means, _ptr


def _planes(who, y, uv, u, v, matrix, msb_aligned):
    """The plane arguments of the lsfa_*yuv420p10* exports: hip._yuv_planes on 16-bit words, then `shift`"""
    if not isinstance(msb_aligned, bool):
        raise LsfaError("%s: msb_aligned must be True (P010: the sample in the high ten bits) or False (yuv420p10le), got %r" % (who, msb_aligned))
    args, N, H, W, batched = hip._yuv_planes(who, y, uv, u, v, matrix, words=True)
    return args + (6 if msb_aligned else 0,), N, H, W, batched


@hip._on_tensor_device
def yuv420p10_to_bgr_u8(y, uv=None, u=None, v=None, matrix='bt601', msb_aligned=True, out=None, y_packed=None):
    """lsfa_yuv420p10_to_bgr_u8: a decoder's 10-bit YUV 4:2:0 planes on the device (see the module docstring) to packed uint8 BGR (H, W, 3) /
    (N, H, W, 3), the layout lsfa_mv_residual, luma_u8 and image_transform_u8 take.  matrix as hip.yuv420_to_bgr_u8; the conversion is done
    in ten bits and rounded once (include/lsfa_hip.h - this project's own specification, not swscale's).  y_packed: an optional (.., H, W)
    uint8 tensor that receives the luma reduced to 8 bits, min(255, (Y + 2) >> 2): what mv_estimate searches.  One launch."""
    who = "yuv420p10_to_bgr_u8"
    args, N, H, W, batched = _planes(who, y, uv, u, v, matrix, msb_aligned)
    out = hip._yuv_bgr_out(who, N, H, W, batched, y.device, out, y_packed)
    _check(hip.lib().lsfa_yuv420p10_to_bgr_u8(*(args + (_ptr(out), _ptr(y_packed), hip._stream()))), "lsfa_yuv420p10_to_bgr_u8")
    return out


@hip._on_tensor_device
def image_transform_yuv420p10(y, uv=None, u=None, v=None, matrix='bt601', msb_aligned=True, pixel_means=(0.0, 0.0, 0.0), pixel_scale=1.0, out=None):
    """lsfa_image_transform_yuv420p10: the planes of yuv420p10_to_bgr_u8 -> `data` (N, 3, H, W) float32: bit-identical to
    hip.image_transform_u8(yuv420p10_to_bgr_u8(...)) without storing the BGR frame, and without its H*W % 4 condition.  One launch."""
    who = "image_transform_yuv420p10"
    args, N, H, W, _ = _planes(who, y, uv, u, v, matrix, msb_aligned)
    out = hip._yuv_out(who, out, (N, 3, H, W), torch.float32, y.device)
    _check(hip.lib().lsfa_image_transform_yuv420p10(*(args + (_means(pixel_means), float(pixel_scale), _ptr(out), hip._stream()))),
           "lsfa_image_transform_yuv420p10")
    return out


@hip._on_tensor_device
def image_resize_transform_yuv420p10(y, uv=None, u=None, v=None, im_scale=1.0, matrix='bt601', msb_aligned=True, pixel_means=(0.0, 0.0, 0.0),
                                     pixel_scale=1.0, stride=0, out=None):
    """lsfa_image_resize_transform_yuv420p10: the planes of yuv420p10_to_bgr_u8 -> `data` (N, 3, h, w) float32: hip.image_resize_transform of
    the converted uint8 frame, bit-identical to it, reading the taps from the planes.  One launch."""
    who = "image_resize_transform_yuv420p10"
    args, N, H, W, _ = _planes(who, y, uv, u, v, matrix, msb_aligned)
    stride, h1, w1, ph, pw, out = hip._yuv_resized_out(who, N, H, W, im_scale, stride, y.device, out)
    _check(hip.lib().lsfa_image_resize_transform_yuv420p10(*(args + (float(im_scale), h1, w1, stride, _means(pixel_means), float(pixel_scale),
                                                                     _ptr(out), ph, pw, hip._stream()))),
           "lsfa_image_resize_transform_yuv420p10")
    return out


class _Words10(object):
    """the conversion hook of hip._SearchFront for 10-bit planes: self.msb_aligned picks the alignment"""

    def _to_bgr(self, y, uv, u, v, matrix, out=None, y_packed=None):
        return yuv420p10_to_bgr_u8(y, uv, u, v, matrix, self.msb_aligned, out=out, y_packed=y_packed)


class MotionEstimator10(_Words10, hip.MotionEstimator):
    """hip.MotionEstimator whose key_frame_yuv / next_frame_yuv take 10-bit planes (yuv420p10_to_bgr_u8's; msb_aligned as there).  Everything
    behind the conversion is the 8-bit estimator's: luma_from='bgr' searches lsfa_luma_u8 of the converted frame, luma_from='y' the luma
    reduced to 8 bits (the conversion's y_packed, no luma launch).  Nothing is allocated after the first *_yuv call."""

    def __init__(self, width, height, device='cuda:0', msb_aligned=True, **kw):
        if not isinstance(msb_aligned, bool):
            raise LsfaError("MotionEstimator10: msb_aligned must be True or False, got %r" % (msb_aligned,))
        self.msb_aligned = msb_aligned
        hip.MotionEstimator.__init__(self, width, height, device, **kw)


class SegmentMotionEstimator10(_Words10, hip.SegmentMotionEstimator):
    """hip.SegmentMotionEstimator whose segment_yuv takes 10-bit planes: y (C * (n + 1), H, W) words and uv | u, v, one conversion launch"""

    def __init__(self, width, height, frames=9, clips=1, device='cuda:0', msb_aligned=True, **kw):
        if not isinstance(msb_aligned, bool):
            raise LsfaError("SegmentMotionEstimator10: msb_aligned must be True or False, got %r" % (msb_aligned,))
        self.msb_aligned = msb_aligned
        hip.SegmentMotionEstimator.__init__(self, width, height, frames, clips, device, **kw)
