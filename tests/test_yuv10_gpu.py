"""lsfa_yuv420p10_to_bgr_u8, lsfa_image_transform_yuv420p10 and lsfa_image_resize_transform_yuv420p10 (lsfa_amd/csrc/yuvfmt.hip) on the GPU
against tests/ref_yuv10.py, against the shipped 8-bit kernels on planes that are 4 x an 8-bit plane and against the packed-BGR entry points
they fuse, bit for bit (`==` everywhere); yuv10.MotionEstimator10 / SegmentMotionEstimator10 against the 8-bit estimators on the converted
frames; graph capture; every error path of the C ABI; the demo's 10-bit --yuv input.  tests/test_yuv10_cpu.py pins the reference.

The sizes are the point of the cases: (2, 4) is the smallest launch of the four-pixel kernel, (6, 8) and (16, 32) run it, (1, 1), (7, 9),
(5, 4) and (6, 10) must take the element-wise one (odd sizes, odd H with W % 4 == 0, W % 4 != 0), as must a pitch of the row + 2 bytes and a
base 2 bytes in; a pitch of the row + 8 bytes and three frames with a gap between them stay with the four-pixel kernel."""
import ctypes
import json

import numpy as np
import pytest
import torch

import guarded_arena
import ref_me
import ref_yuv
import ref_yuv10

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LAYOUTS = ("semi", "planar")
SHIFTS = (6, 0)
MATRICES = ("bt601", "bt709", "jpeg")
PS = 0.0125
FILL = 0xA5A5 - 0x10000           # the int16 reading of the words around every plane


@pytest.fixture(scope="module")
def yuv10(hip):
    from lsfa_amd import yuv10 as module
    return module


def means():
    from lsfa_amd.config.config import lsfa_test_config
    return tuple(float(m) for m in lsfa_test_config().network.PIXEL_MEANS)


def t(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)


class Surface(object):
    """numpy (rows, cols) or (N, rows, cols) uint16 words -> .view, a device int16 VIEW of that shape with rows `pitch` BYTES apart, frames
    `gap` bytes further apart than a frame and the base `offset` bytes into its allocation; every other word holds 0xA5A5, and intact()
    says that the whole allocation is still what it was"""

    def __init__(self, a, pitch=None, gap=0, offset=0):
        batched = a.ndim == 3
        n = a.shape[0] if batched else 1
        rows, cols = a.shape[-2:]
        pitch = 2 * cols if pitch is None else pitch
        assert pitch % 2 == 0 and gap % 2 == 0 and offset % 2 == 0
        fs = rows * pitch + gap
        self.buf = torch.full(((offset + n * fs) // 2 + 8,), FILL, dtype=torch.int16, device=DEV)
        view = torch.as_strided(self.buf, (n, rows, cols), (fs // 2, pitch // 2, 1), offset // 2)
        view.copy_(t(a.reshape(n, rows, cols)))
        self.view = view if batched else view[0]
        self.before = self.buf.clone()

    def intact(self):
        return torch.equal(self.buf, self.before)


def surfaces(y, u, v, layout, extra=0, gap=0, y_offset=0):
    """-> (keyword arguments of the yuv10.*yuv420p10* functions for the numpy planes, the Surfaces behind them); extra: pitch bytes beyond the row"""
    c = {"uv": ref_yuv10.interleave(u, v)} if layout == "semi" else {"u": u, "v": v}
    s = {"y": Surface(y, 2 * y.shape[-1] + extra, gap, y_offset)}
    s.update({k: Surface(p, 2 * p.shape[-1] + extra, gap) for k, p in c.items()})
    return {k: x.view for k, x in s.items()}, list(s.values())


# (H, W, pitch bytes beyond the row, frames, extra bytes between frames, Y base offset in bytes)
GEOMETRIES = [(2, 4, 0, None, 0, 0), (6, 8, 0, None, 0, 0), (16, 32, 0, None, 0, 0), (1, 1, 0, None, 0, 0), (7, 9, 0, None, 0, 0), (5, 4, 0, None, 0, 0),
              (6, 10, 0, None, 0, 0), (6, 8, 8, None, 0, 0), (6, 8, 2, None, 0, 0), (6, 8, 0, None, 0, 2), (6, 8, 8, 3, 48, 0), (7, 9, 6, 3, 10, 0)]
_WANT = {}


def random_planes(H, W, seed, n=None):
    rs = np.random.RandomState(seed)
    ch, cw = ref_yuv10.chroma_shape(H, W)
    lead = () if n is None else (n,)
    return tuple(ref_yuv10.random_words(rs, lead + s) for s in ((H, W), (ch, cw), (ch, cw)))


def want(geo, shift, matrix):
    """a geometry's planes and ref_yuv10's frame and packed luma of them, computed once per (geometry, shift, matrix) and shared"""
    key = (geo, shift, matrix)
    if key not in _WANT:
        H, W, _, n, _, _ = geo
        y, u, v = random_planes(H, W, seed=H * 100 + W + len(_WANT), n=n)
        _WANT[key] = (y, u, v, ref_yuv10.to_bgr(y, u=u, v=v, matrix=matrix, shift=shift), ref_yuv10.y_packed(y, shift))
    return _WANT[key]


@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_yuv420p10_to_bgr_u8_equals_the_reference(yuv10, layout, shift, matrix):
    """lsfa_yuv420p10_to_bgr_u8 == ref_yuv10 at every geometry, with y_packed; the outputs lie in guarded_arena's bands, which keep their
    pattern, and the planes' allocations - pitch padding, gaps, the words around them - keep every bit"""
    arena = guarded_arena.Arena(0xFF)
    for geo in GEOMETRIES:
        H, W, extra, n, gap, off = geo
        y, u, v, bgr, yp = want(geo, shift, matrix)
        planes, surf = surfaces(y, u, v, layout, extra, gap, off)
        got = yuv10.yuv420p10_to_bgr_u8(matrix=matrix, msb_aligned=shift == 6, **planes)
        assert got.dtype == torch.uint8 and tuple(got.shape) == bgr.shape, geo
        np.testing.assert_array_equal(got.cpu().numpy(), bgr, err_msg=str(geo))
        out, luma = arena.place(bgr.shape, torch.uint8, "out %s" % (geo,)), arena.place(yp.shape, torch.uint8, "y_packed %s" % (geo,))
        assert yuv10.yuv420p10_to_bgr_u8(matrix=matrix, msb_aligned=shift == 6, out=out, y_packed=luma, **planes) is out
        np.testing.assert_array_equal(out.cpu().numpy(), bgr, err_msg=str(geo))
        np.testing.assert_array_equal(luma.cpu().numpy(), yp, err_msg=str(geo))
        assert all(s.intact() for s in surf), geo
    arena.check()


def test_yuv420p10_to_bgr_u8_full_size(yuv10):
    """... and two frames of 1280 x 720 in one launch: P010 under BT.709, planar low-aligned words under BT.601"""
    geo = (720, 1280, 0, 2, 0, 0)
    for layout, shift, matrix in (("semi", 6, "bt709"), ("planar", 0, "bt601")):
        y, u, v, bgr, yp = want(geo, shift, matrix)
        planes, _ = surfaces(y, u, v, layout)
        luma = torch.zeros((2, 720, 1280), dtype=torch.uint8, device=DEV)
        got = yuv10.yuv420p10_to_bgr_u8(matrix=matrix, msb_aligned=shift == 6, y_packed=luma, **planes)
        np.testing.assert_array_equal(got.cpu().numpy(), bgr)
        np.testing.assert_array_equal(luma.cpu().numpy(), yp)
        assert bgr.min() == 0 and bgr.max() == 255


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_four_times_an_8_bit_plane_gives_the_shipped_8_bit_kernels(hip, yuv10, layout, shift):
    """planes = 8-bit planes << 2 << shift (the ignored bits filled at random): all three entry points == hip.yuv420_to_bgr_u8 /
    image_transform_yuv420 / image_resize_transform_yuv420 on the 8-bit planes, and y_packed gives the 8-bit Y back"""
    mn = means()
    rs = np.random.RandomState(80 + shift)
    for H, W, n in ((16, 32, 2), (7, 9, None)):
        ch, cw = ref_yuv.chroma_shape(H, W)
        lead = () if n is None else (n,)
        p8 = [rs.randint(0, 256, lead + s).astype(np.uint8) for s in ((H, W), (ch, cw), (ch, cw))]
        p10 = [ref_yuv10.widen(p, shift) | (rs.randint(0, 64, p.shape).astype(np.uint16) << (0 if shift == 6 else 10)) for p in p8]
        k8 = dict(y=t(p8[0]), uv=t(ref_yuv.interleave(p8[1], p8[2]))) if layout == "semi" else dict(y=t(p8[0]), u=t(p8[1]), v=t(p8[2]))
        k10, _ = surfaces(p10[0], p10[1], p10[2], layout)
        for matrix in MATRICES:
            luma = torch.zeros(p8[0].shape, dtype=torch.uint8, device=DEV)
            got = yuv10.yuv420p10_to_bgr_u8(matrix=matrix, msb_aligned=shift == 6, y_packed=luma, **k10)
            assert torch.equal(got, hip.yuv420_to_bgr_u8(matrix=matrix, **k8)) and torch.equal(luma, k8["y"]), (H, W, matrix)
            assert torch.equal(yuv10.image_transform_yuv420p10(matrix=matrix, msb_aligned=shift == 6, pixel_means=mn, pixel_scale=PS, **k10),
                               hip.image_transform_yuv420(matrix=matrix, pixel_means=mn, pixel_scale=PS, **k8)), (H, W, matrix)
            for scale, stride in ((0.6, 16), (1.25, 0)):
                assert torch.equal(yuv10.image_resize_transform_yuv420p10(im_scale=scale, matrix=matrix, msb_aligned=shift == 6, pixel_means=mn, pixel_scale=PS,
                                                                          stride=stride, **k10),
                                   hip.image_resize_transform_yuv420(im_scale=scale, matrix=matrix, pixel_means=mn, pixel_scale=PS, stride=stride, **k8))


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_image_transform_yuv420p10_is_the_two_step_path(hip, yuv10, layout, shift):
    """lsfa_image_transform_yuv420p10 == image_transform_u8(yuv420p10_to_bgr_u8(...)) wherever the u8 form runs (H*W % 4 == 0), and == ref_yuv10 +
    the float64 formula at every geometry; `data` lies in guarded bands"""
    mn = means()
    arena = guarded_arena.Arena(0x7F)
    for gi, geo in enumerate(GEOMETRIES):
        H, W, extra, n, gap, off = geo
        matrix = MATRICES[gi % 3]
        y, u, v, bgr, _ = want(geo, shift, matrix)
        planes, surf = surfaces(y, u, v, layout, extra, gap, off)
        kw = dict(matrix=matrix, msb_aligned=shift == 6, **planes)
        got = yuv10.image_transform_yuv420p10(pixel_means=mn, pixel_scale=PS, **kw)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n or 1, 3, H, W)
        np.testing.assert_array_equal(got.cpu().numpy(), ref_yuv10.transform(bgr if n else bgr[None], mn, PS), err_msg=str(geo))
        if (H * W) % 4 == 0:
            frame = yuv10.yuv420p10_to_bgr_u8(**kw)
            assert torch.equal(got, hip.image_transform_u8(frame if n else frame.unsqueeze(0), mn, PS)), geo
        out = arena.place(got.shape, torch.float32, "data %s" % (geo,))
        assert yuv10.image_transform_yuv420p10(pixel_means=mn, pixel_scale=PS, out=out, **kw) is out and torch.equal(out, got)
        assert all(s.intact() for s in surf), geo
    arena.check()


@pytest.mark.parametrize("stride", [0, 16])
@pytest.mark.parametrize("scale", [0.5, 0.6, 1.25])
def test_image_resize_transform_yuv420p10_is_the_two_step_path(hip, yuv10, scale, stride):
    """lsfa_image_resize_transform_yuv420p10 == image_resize_transform (uint8 frames, float interpolation) of the converted frame: both
    subtraction rules, two pitched frames per launch, an odd size, both layouts and alignments"""
    mn = means()
    arena = guarded_arena.Arena(0x7F)
    for H, W, n, extra, layout, shift, matrix in ((36, 52, 2, 24, "semi", 6, "bt601"), (37, 53, None, 0, "planar", 0, "bt709"),
                                                 (36, 52, None, 2, "planar", 6, "jpeg"), (6, 10, None, 0, "semi", 0, "bt601")):
        y, u, v = random_planes(H, W, seed=H + W, n=n)
        planes, surf = surfaces(y, u, v, layout, extra, 40 if n else 0)
        kw = dict(matrix=matrix, msb_aligned=shift == 6, **planes)
        frame = yuv10.yuv420p10_to_bgr_u8(**kw)
        np.testing.assert_array_equal(frame.cpu().numpy(), ref_yuv10.to_bgr(y, u=u, v=v, matrix=matrix, shift=shift))
        expect = hip.image_resize_transform(frame, scale, mn, PS, stride=stride)
        out = arena.place(expect.shape, torch.float32, "resized data %dx%d" % (W, H))
        got = yuv10.image_resize_transform_yuv420p10(im_scale=scale, pixel_means=mn, pixel_scale=PS, stride=stride, out=out, **kw)
        assert got is out and torch.equal(got, expect), (H, W, layout, shift)
        assert torch.equal(yuv10.image_resize_transform_yuv420p10(im_scale=scale, pixel_means=mn, pixel_scale=PS, stride=stride, **kw), expect)
        assert float(got.abs().max()) > 0 and all(s.intact() for s in surf)
    arena.check()


# ---- the estimators -----------------------------------------------------------------------------------------------------------------------
def clip10(n, width, height, m, seed, shift):
    """n frames of a translating texture as 10-bit (y, u, v) words - an 8-bit conversion times four plus two random low bits, the ignored
    bits random - with ref_yuv10's BGR frames and packed luma of them"""
    rs = np.random.RandomState(seed)
    planes = []
    for f in ref_me.translated_clip(n, width, height, m, seed=seed, sigma=2.0):
        p8 = ref_yuv.forward(f)
        ten = [(p.astype(np.uint16) << 2) | rs.randint(0, 4, p.shape).astype(np.uint16) for p in p8]
        planes.append(tuple((s << 6) | rs.randint(0, 64, s.shape).astype(np.uint16) if shift == 6 else s | (rs.randint(0, 64, s.shape).astype(np.uint16) << 10)
                            for s in ten))
    return planes, [ref_yuv10.to_bgr(y, u=u, v=v, shift=shift) for y, u, v in planes], [ref_yuv10.y_packed(y, shift) for y, _, _ in planes]


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_motion_estimator10_chain(hip, yuv10, layout, shift):
    """48 x 64, search 4, three frames.  luma_from='bgr': rows, SAD, accumulated field and network_inputs are hip.MotionEstimator's fed the
    converted BGR frames.  luma_from='y': rows and SAD are hip.mv_estimate's on the reduced Y planes."""
    height, width = 48, 64
    planes, frames, lumas = clip10(3, width, height, (2, -1), seed=48 + shift, shift=shift)
    mn = means()
    a = yuv10.MotionEstimator10(width, height, DEV, msb_aligned=shift == 6, search=4, lam=4)
    b = hip.MotionEstimator(width, height, DEV, search=4, lam=4)
    c = yuv10.MotionEstimator10(width, height, DEV, msb_aligned=shift == 6, search=4, lam=4, luma_from='y')
    assert a.bgr_key is None and a.bgr_cur is None
    dp = [surfaces(y, u, v, layout, extra=16)[0] for y, u, v in planes]
    df, dl = [t(f) for f in frames], [t(p) for p in lumas]
    key = a.key_frame_yuv(**dp[0])
    assert key is a.bgr_key and torch.equal(key, df[0])
    b.key_frame(df[0])
    c.key_frame_yuv(**dp[0])
    for f in (1, 2):
        cur = a.next_frame_yuv(**dp[f])
        assert cur is a.bgr_cur and cur is not a.bgr_key and torch.equal(cur, df[f]), f
        rows = b.next_frame(df[f])
        assert torch.equal(a.rows, rows) and torch.equal(a.sad, b.sad) and torch.equal(a.acc.accu, b.acc.accu), f
        a_mv, a_res = a.network_inputs(a.bgr_cur, a.bgr_key, 1.25, mn, PS)
        b_mv, b_res = b.network_inputs(df[f], df[0], 1.25, mn, PS)
        assert torch.equal(a_mv, b_mv) and torch.equal(a_res, b_res), f
        c.next_frame_yuv(**dp[f])
        want_rows, want_sad = hip.mv_estimate(dl[f], dl[f - 1], 4, 4, c.max_sad, return_sad=True)
        assert torch.equal(c.rows, want_rows) and torch.equal(c.sad, want_sad), f
        assert torch.equal(c.bgr_cur, df[f])
    assert float(a_mv.abs().max()) > 0


def test_segment_motion_estimator10_equals_segment_on_the_converted_stack(hip, yuv10):
    """2 clips of a key frame + 2 frames, 32 x 48: segment_yuv == SegmentMotionEstimator.segment on ref_yuv10's frames; with luma_from='y'
    the rows are hip.mv_estimate_chain's on the reduced Y planes"""
    H, W, C, n = 32, 48, 2, 2
    mn = means()
    for layout, shift in (("semi", 6), ("planar", 0)):
        clips = [clip10(n + 1, W, H, m, seed=s, shift=shift) for m, s in (((2, -1), 5), ((-1, 2), 6))]
        y, u, v = (np.stack([p[i] for planes, _, _ in clips for p in planes]) for i in range(3))
        bgr = np.stack([np.stack(frames) for _, frames, _ in clips])
        luma = np.stack([np.stack(l) for _, _, l in clips])
        kw, _ = surfaces(y, u, v, layout, extra=8, gap=32)
        a = yuv10.SegmentMotionEstimator10(W, H, frames=n, clips=C, device=DEV, msb_aligned=shift == 6, search=4, lam=4)
        b = hip.SegmentMotionEstimator(W, H, frames=n, clips=C, device=DEV, search=4, lam=4)
        a_mv, a_res = a.segment_yuv(im_scale=1.25, pixel_means=mn, pixel_scale=PS, **kw)
        b_mv, b_res = b.segment(t(bgr), 1.25, mn, PS)
        assert torch.equal(a.bgr, t(bgr)) and torch.equal(a.rows, b.rows) and torch.equal(a.sad, b.sad)
        assert torch.equal(a_mv, b_mv) and torch.equal(a_res, b_res) and float(a_mv.abs().max()) > 0
        c = yuv10.SegmentMotionEstimator10(W, H, frames=n, clips=C, device=DEV, msb_aligned=shift == 6, search=4, lam=4, luma_from='y')
        c.segment_yuv(im_scale=1.25, pixel_means=mn, pixel_scale=PS, **kw)
        want_rows = hip.mv_estimate_chain(t(luma), 4, 4, c.max_sad)
        assert torch.equal(c.rows, want_rows.view_as(c.rows)) and torch.equal(c.bgr, t(bgr))


def test_motion_estimator10_graph_capture(yuv10):
    """key_frame_yuv + two next_frame_yuv + network_inputs captured with torch.cuda.graph on one stream, replayed on NEW plane contents
    written into the same tensors == the eager run on those contents"""
    width, height = 64, 48
    mn = means()
    clips = [clip10(3, width, height, (2, -1), seed=1, shift=6)[0], clip10(3, width, height, (-3, 2), seed=2, shift=6)[0]]
    bufs = [surfaces(y, u, v, "semi", extra=16)[0] for y, u, v in clips[0]]
    me = yuv10.MotionEstimator10(width, height, DEV, search=16, lam=4)

    def step(m, planes):
        m.key_frame_yuv(**planes[0])
        m.next_frame_yuv(**planes[1])
        m.next_frame_yuv(**planes[2])
        return m.network_inputs(m.bgr_cur, m.bgr_key, 1.0, mn, 1.0)

    step(me, bufs)                           # warm-up: the BGR buffers and network_inputs' outputs are allocated at the first call
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_mv, out_res = step(me, bufs)
    for k, clip in enumerate(clips[::-1] + clips):
        for buf, (y, u, v) in zip(bufs, clip):
            buf["y"].copy_(t(y))
            buf["uv"].copy_(t(ref_yuv10.interleave(u, v)))
        g.replay()
        torch.cuda.synchronize()
        eager = yuv10.MotionEstimator10(width, height, DEV, search=16, lam=4)
        e_mv, e_res = step(eager, [surfaces(y, u, v, "semi")[0] for y, u, v in clip])
        assert torch.equal(me.rows, eager.rows) and torch.equal(me.sad, eager.sad), k
        assert torch.equal(out_mv, e_mv) and torch.equal(out_res, e_res), k
    assert float(out_mv.abs().max()) > 0


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_every_error_path_of_the_c_abi_returns_einval_and_launches_nothing(hip, yuv10):
    """NULL planes and outputs, N / H / W below 1, a matrix outside 0..2, a shift other than 0 or 6, an odd base, pitch or frame stride, a
    pitch below its row: LSFA_EINVAL from all three exports with the export's name in the message, the outputs untouched; then the same
    buffers through a valid call are correct.  Every refused call is refused on its arguments alone: no pointer is followed."""
    H, W = 6, 8
    y, u, v = random_planes(H, W, seed=7)
    semi, _ = surfaces(y, u, v, "semi", extra=8)
    planar, _ = surfaces(y, u, v, "planar", extra=8)
    mn = means()
    bgr = torch.full((H, W, 3), 7, dtype=torch.uint8, device=DEV)
    data = torch.full((1, 3, H, W), 7.0, device=DEV)
    rdata = torch.full((1, 3, 16, 16), 7.0, device=DEV)          # scale 1.25: 8 x 10, padded to 16
    L = hip.lib()
    mean_arr = (ctypes.c_double * 3)(*mn)

    def args(planes, **over):
        yy = planes["y"]
        c = planes["uv"] if "uv" in planes else planes["u"]
        a = dict(y=yy.data_ptr(), y_pitch=2 * yy.stride(-2), y_fs=0, c=c.data_ptr(), v=planes["v"].data_ptr() if "v" in planes else None,
                 c_pitch=2 * c.stride(-2), c_fs=0, N=1, H=H, W=W, matrix=0, shift=6)
        a.update(over)
        return [a[k] for k in ("y", "y_pitch", "y_fs", "c", "v", "c_pitch", "c_fs", "N", "H", "W", "matrix", "shift")]

    def calls(planes, bgr_ptr, data_ptr, rdata_ptr, mean_ptr=mean_arr, **over):
        a = args(planes, **over)
        return (("lsfa_yuv420p10_to_bgr_u8", a + [bgr_ptr, None, None]),
                ("lsfa_image_transform_yuv420p10", a + [mean_ptr, PS, data_ptr, None]),
                ("lsfa_image_resize_transform_yuv420p10", a + [1.25, 8, 10, 16, mean_ptr, PS, rdata_ptr, 16, 16, None]))

    y_ptr, c_ptr = semi["y"].data_ptr(), semi["uv"].data_ptr()
    bad = [dict(y=None), dict(c=None), dict(N=0), dict(N=-1), dict(H=0), dict(H=-3), dict(W=0), dict(W=-8), dict(matrix=3), dict(matrix=-1), dict(shift=2),
           dict(shift=10), dict(shift=-6), dict(shift=16), dict(y=y_ptr + 1), dict(c=c_ptr + 1), dict(y_pitch=2 * W + 1), dict(c_pitch=2 * W + 1),
           dict(y_fs=101), dict(c_fs=-3), dict(y_pitch=2 * W - 2), dict(c_pitch=2 * W - 2), dict(y_pitch=0), dict(y_pitch=-32)]
    for over in bad:
        for name, a in calls(semi, bgr.data_ptr(), data.data_ptr(), rdata.data_ptr(), **over):
            assert getattr(L, name)(*a) == -1, (name, over)                          # LSFA_EINVAL
            assert name.encode() in L.lsfa_last_error(), (name, over)
    planar_bad = [dict(v=planar["v"].data_ptr() + 1), dict(c_pitch=W - 2), dict(c_pitch=W + 1)]
    for over in planar_bad:
        for name, a in calls(planar, bgr.data_ptr(), data.data_ptr(), rdata.data_ptr(), **over):
            assert getattr(L, name)(*a) == -1, (name, over)
    # a planar chroma row is half an interleaved one: W bytes... is enough for two planes and too narrow for interleaved words
    assert L.lsfa_yuv420p10_to_bgr_u8(*(args(planar, c_pitch=W) + [bgr.data_ptr(), None, None])) == 0
    assert L.lsfa_yuv420p10_to_bgr_u8(*(args(semi, c_pitch=W) + [bgr.data_ptr(), None, None])) == -1
    assert b"interleaved" in L.lsfa_last_error()
    bgr.fill_(7)
    # NULL outputs and means
    for name, a in calls(semi, None, None, None):
        assert getattr(L, name)(*a) == -1, name
    for name, a in calls(semi, bgr.data_ptr(), data.data_ptr(), rdata.data_ptr(), mean_ptr=None)[1:]:
        assert getattr(L, name)(*a) == -1, name
    # an output shape that does not follow from h1 / w1 / stride, a scale of zero
    a = args(semi)
    assert L.lsfa_image_resize_transform_yuv420p10(*(a + [1.25, 8, 10, 16, mean_arr, PS, rdata.data_ptr(), 16, 32, None])) == -1
    assert b"padded to 16 gives 16 x 16" in L.lsfa_last_error()
    assert L.lsfa_image_resize_transform_yuv420p10(*(a + [0.0, 8, 10, 16, mean_arr, PS, rdata.data_ptr(), 16, 16, None])) == -1
    torch.cuda.synchronize()
    assert bool((bgr == 7).all()) and bool((data == 7.0).all()) and bool((rdata == 7.0).all())
    # ... and the same buffers are written by the good calls
    want_bgr = ref_yuv10.to_bgr(y, u=u, v=v, shift=6)
    for planes in (semi, planar):
        bgr.fill_(7)
        for name, a in calls(planes, bgr.data_ptr(), data.data_ptr(), rdata.data_ptr()):
            assert getattr(L, name)(*a) == 0, name
        np.testing.assert_array_equal(bgr.cpu().numpy(), want_bgr)
        np.testing.assert_array_equal(data.cpu().numpy(), ref_yuv10.transform(want_bgr[None], mn, PS))
        assert torch.equal(rdata, hip.image_resize_transform(bgr, 1.25, mn, PS, stride=16))


def test_prof_scope_counts_one_launch_per_call(hip, yuv10):
    quad, _ = surfaces(*random_planes(16, 16, seed=8), layout="semi")
    odd, _ = surfaces(*random_planes(5, 7, seed=8), layout="planar")
    hip.prof_enable(True, ops=["stem"])
    try:
        hip.prof_read()
        for planes in (quad, odd):              # the four-pixel and the element-wise kernel
            yuv10.yuv420p10_to_bgr_u8(**planes)
            yuv10.image_transform_yuv420p10(**planes)
            yuv10.image_resize_transform_yuv420p10(im_scale=1.5, stride=16, **planes)
        ms, n = hip.prof_read()["stem"]
    finally:
        hip.prof_enable(False)
    assert n == 6 and ms > 0.0


# ---- the demo -------------------------------------------------------------------------------------------------------------------------------
def test_demo_runs_nv12_p010_and_yuv420p10le_of_one_clip_to_the_same_detections(hip, tmp_path):
    """a 12-frame 160 x 96 clip three ways from one set of 8-bit planes - NV12, P010 (<< 8) and yuv420p10le (<< 2) - through
    lsfa_amd.demo --yuv --estimate-mv --dump-mv: identical detections, identical dumps"""
    from lsfa_amd import demo
    planes = [ref_yuv.forward(f) for f in ref_me.translated_clip(12, 160, 96, (3, -2), seed=6, sigma=2.0)]
    with open(str(tmp_path / "clip.nv12"), "wb") as f:
        for y, u, v in planes:
            f.write(ref_yuv.raw_frame_bytes(y, u, v, "nv12"))
    for fmt, up in (("p010", 8), ("yuv420p10le", 2)):
        with open(str(tmp_path / ("clip." + fmt)), "wb") as f:
            for p in planes:
                f.write(ref_yuv10.raw_frame_bytes(*[a.astype(np.uint16) << up for a in p], fmt))
    assert (tmp_path / "clip.p010").stat().st_size == 2 * (tmp_path / "clip.nv12").stat().st_size == 12 * 160 * 96 * 3
    outs = {}
    common = ["--size", "160x96", "--estimate-mv", "--interval", "4", "--score", "0.05"]
    for fmt in ("nv12", "p010", "yuv420p10le"):
        out = tmp_path / (fmt + ".json")
        demo.main(["--yuv", str(tmp_path / ("clip." + fmt)), "--yuv-format", fmt, "--dump-mv", str(tmp_path / ("mv_" + fmt)), "--out", str(out)] + common)
        outs[fmt] = [(r["key"], r["dets"]) for r in json.loads(out.read_text())]          # (the frame names carry the file's name)
    assert outs["nv12"] == outs["p010"] == outs["yuv420p10le"]
    assert [k for k, _ in outs["p010"]] == [i % 4 == 0 for i in range(12)] and sum(len(d) for _, d in outs["p010"]) > 0
    non_key = [i for i in range(12) if i % 4]
    for fmt in ("p010", "yuv420p10le"):
        assert sorted(p.name for p in (tmp_path / ("mv_" + fmt)).iterdir()) == ["%06d.npz" % i for i in non_key]
        for i in non_key:
            a, b = np.load(str(tmp_path / "mv_nv12" / ("%06d.npz" % i))), np.load(str(tmp_path / ("mv_" + fmt) / ("%06d.npz" % i)))
            assert (a["mv"] == b["mv"]).all() and (a["res"] == b["res"]).all(), (fmt, i)
    assert np.abs(a["mv"]).max() > 0
    from lsfa_amd.config.config import lsfa_test_config
    clip = demo.YuvFileClip(str(tmp_path / "clip.p010"), 160, 96, lsfa_test_config(), "p010")
    assert clip.num_frames == 12 and clip.frame_bytes == 160 * 96 * 3 and clip.planes(0)["y"].dtype == torch.int16
