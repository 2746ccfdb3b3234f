"""The six 4:2:0 intake exports (lsfa_*yuv420*, lsfa_*yuv420p10*; lsfa_amd/csrc/yuvfmt.hip) on the frames the v_ashr_pk_u8_i32 finding is
about (DESIGN.md "Other chroma formats"): a blue or a red clipped to 0 beside channels that are not, inside one group of four pixels that
the four-pixel kernel packs into three dwords.  Shift-then-saturate there compiled to a half-register pack that left 0xFF in the bytes
behind a clipped blue; the one conversion clamps before it shifts.  Everything is compared with `==` against tests/ref_yuv.py and
tests/ref_yuv10.py: NV12, I420, P010 and yuv420p10le, all three matrices, both kernels."""
import numpy as np
import pytest
import torch

import ref_yuv
import ref_yuv10

DEV = "cuda:0"
MATRICES = ("bt601", "bt709", "jpeg")
FORMATS = ("nv12", "i420", "p010", "yuv420p10le")
PS = 0.0125
# (N, H, W): aligned dense planes with W % 4 == 0 and an even H take the four-pixel kernel, 3 x 5 the element-wise one
QUAD, ELEMS = (2, 4, 8), (1, 3, 5)
# a group of four pixels is one of two kinds, alternating along x, down the chroma rows and from frame to frame.  Its two chroma samples
# (U, V) differ, and so do its Y over the two rows that share them: Y walks over {0, 16, 128, 235, 255}, U and V over {0, 16, 128, 240, 255}
CHROMA = (((0, 0), (255, 240)), ((128, 128), (16, 240)))
LUMA = (((128, 255, 16, 235), (0, 255, 235, 16)), ((0, 128, 235, 255), (0, 128, 255, 235)))


def clipping_planes(N, H, W):
    """y (N, H, W), u, v (N, ceil(H / 2), ceil(W / 2)) uint8 of the groups above"""
    ch, cw = ref_yuv.chroma_shape(H, W)
    n, y, x = np.meshgrid(np.arange(N), np.arange(H), np.arange(W), indexing="ij")
    Y = np.asarray(LUMA, np.uint8)[(x // 4 + y // 2 + n) % 2, y % 2, x % 4]
    n, cy, cx = np.meshgrid(np.arange(N), np.arange(ch), np.arange(cw), indexing="ij")
    UV = np.asarray(CHROMA, np.uint8)[(cx // 2 + cy + n) % 2, cx % 2]
    return Y, np.ascontiguousarray(UV[..., 0]), np.ascontiguousarray(UV[..., 1])


_WANT = {}


def want(shape, matrix):
    """the planes of a shape and ref_yuv's frame of them, once per (shape, matrix)"""
    if (shape, matrix) not in _WANT:
        y, u, v = clipping_planes(*shape)
        _WANT[(shape, matrix)] = (y, u, v, ref_yuv.to_bgr(y, u=u, v=v, matrix=matrix))
    return _WANT[(shape, matrix)]


def t(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)


def calls(hip, fmt, y, u, v):
    """-> ((to_bgr, transform, resize_transform) of the format, the device planes as their keyword arguments).  10-bit planes are 4 x the
    8-bit ones with junk in the six bits the alignment ignores."""
    from lsfa_amd import yuv10
    if fmt in ("nv12", "i420"):
        fns, extra, il = (hip.yuv420_to_bgr_u8, hip.image_transform_yuv420, hip.image_resize_transform_yuv420), {}, ref_yuv.interleave
    else:
        shift = ref_yuv10.SHIFTS[fmt]
        y, u, v = (ref_yuv10.widen(p, shift, low_bits=junk) for p, junk in ((y, 0x2b), (u, 0x15), (v, 0x3f)))
        fns = (yuv10.yuv420p10_to_bgr_u8, yuv10.image_transform_yuv420p10, yuv10.image_resize_transform_yuv420p10)
        extra, il = dict(msb_aligned=shift == 6), ref_yuv10.interleave
    planes = dict(y=t(y), uv=t(il(u, v))) if fmt in ("nv12", "p010") else dict(y=t(y), u=t(u), v=t(v))
    planes.update(extra)
    return fns, planes


@pytest.mark.parametrize("matrix", MATRICES)
def test_the_frames_clip_inside_every_group_of_four(matrix):
    """the numpy reference alone: every group of four pixels of the 8-wide frame holds a blue equal to 0 and a blue in 1..254, and the same
    of red; some group holds a blue of 0, one of 255 and one between them.  The 10-bit reference of the widened planes is the 8-bit frame."""
    y, u, v, bgr = want(QUAD, matrix)
    groups = bgr.reshape(-1, 4, 3)
    for ch in (0, 2):
        g = groups[:, :, ch]
        assert ((g == 0).any(axis=1) & ((g > 0) & (g < 255)).any(axis=1)).all(), ch
    b = groups[:, :, 0]
    assert ((b == 0).any(axis=1) & (b == 255).any(axis=1) & ((b > 0) & (b < 255)).any(axis=1)).any()
    assert (np.diff(u.astype(int), axis=-1) != 0).all() and (np.diff(v.astype(int), axis=-1) != 0).all()          # neighbouring chroma differs
    for shift in (6, 0):
        wide = [ref_yuv10.widen(p, shift, low_bits=junk) for p, junk in ((y, 0x2b), (u, 0x15), (v, 0x3f))]
        assert all(((w >> (0 if shift == 6 else 10)) & 63).all() for w in wide)          # the junk is there
        np.testing.assert_array_equal(ref_yuv10.to_bgr(wide[0], u=wide[1], v=wide[2], matrix=matrix, shift=shift), bgr)
        np.testing.assert_array_equal(ref_yuv10.y_packed(wide[0], shift), y)
    assert (want(ELEMS, matrix)[3][..., 0] == 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", [QUAD, ELEMS], ids=["four_pixel", "element_wise"])
def test_the_420_exports_on_clipped_channels(hip, shape, fmt, matrix):
    """BGR with y_packed == the reference; image_transform_* == image_transform_u8 of the reference's frame - as ref_yuv.transform states it
    in numpy, and as the device runs it where it runs (it refuses the 15 pixels of 3 x 5: H * W % 4); the resize form at im_scale=1.25,
    stride=16 == image_resize_transform of the reference's frame"""
    from lsfa_amd.config.config import lsfa_test_config
    mn = tuple(float(m) for m in lsfa_test_config().network.PIXEL_MEANS)
    y, u, v, bgr = want(shape, matrix)
    (to_bgr, transform, resize), planes = calls(hip, fmt, y, u, v)
    yp = torch.full(y.shape, 0x5A, dtype=torch.uint8, device=DEV)
    got = to_bgr(matrix=matrix, y_packed=yp, **planes)
    np.testing.assert_array_equal(got.cpu().numpy(), bgr)
    np.testing.assert_array_equal(yp.cpu().numpy(), y)
    ref_frame = t(bgr)
    data = transform(matrix=matrix, pixel_means=mn, pixel_scale=PS, **planes)
    np.testing.assert_array_equal(data.cpu().numpy(), ref_yuv.transform(bgr, mn, PS))
    if y[0].size % 4 == 0:
        assert torch.equal(data, hip.image_transform_u8(ref_frame, mn, PS))
    assert torch.equal(resize(im_scale=1.25, matrix=matrix, pixel_means=mn, pixel_scale=PS, stride=16, **planes),
                       hip.image_resize_transform(ref_frame, 1.25, mn, PS, stride=16))
