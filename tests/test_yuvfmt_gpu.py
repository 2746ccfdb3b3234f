"""lsfa_yuv_to_bgr_u8, lsfa_image_transform_yuv and lsfa_image_resize_transform_yuv (lsfa_amd/csrc/yuvfmt.hip) on the GPU against
tests/ref_yuvfmt.py over all 29 formats, against the shipped 4:2:0 kernels and against the packed-BGR entry points they fuse, bit for bit
(`==` everywhere); yuvfmt.MotionEstimatorYuv / SegmentMotionEstimatorYuv against the shipped estimators on the converted frames; graph
capture; every refusal of the C ABI; memory ownership; the demo's --yuv input in four formats.  tests/test_yuvfmt_cpu.py pins the reference.

The sizes are the point of the cases: (1, 1), (1, 2), (3, 5) and (23, 37) must take the element-wise kernel, (2, 4) is one thread of the
four-pixel kernel, (4, 8) runs it with a pitch of the row + 4 or + 16 bytes where the format's loads divide that, and must fall to the
element-wise one with a pitch of the row + one sample, with the base one sample in and - (6, 12), three frames - with a frame stride that
is no multiple of 4 bytes; three pitched frames 32 bytes apart stay with the four-pixel kernel.  Every plane is an allocation of exactly
its promised size: nothing lies behind its last sample."""
import ctypes
import json

import numpy as np
import pytest
import torch

import guarded_arena
import ref_me
import ref_yuv
import ref_yuv10
import ref_yuvfmt as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MATRICES = ("bt601", "bt709", "jpeg")
PS = 0.0125
NAME_OF = {c: n for n, c in sorted(ref.NAMES.items(), reverse=True)}          # yuyv422, not yuy2


def fmt_id(c):
    return NAME_OF.get(c, "0x%03x" % c)


@pytest.fixture(scope="module")
def yuvfmt(hip):
    from lsfa_amd import yuvfmt as module
    return module


def means():
    from lsfa_amd.config.config import lsfa_test_config
    return tuple(float(m) for m in lsfa_test_config().network.PIXEL_MEANS)


def t(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)


class Surface(object):
    """numpy (rows, cols) or (N, rows, cols) bytes or uint16 words -> .view, a device VIEW (uint8 / int16) of that shape with rows `pitch`
    BYTES apart, frames `gap` bytes further apart than a frame and the base `offset` bytes into an allocation that ends with the last
    sample; every other byte holds 0xA5, and intact() says that the whole allocation is still what it was"""

    def __init__(self, a, pitch=None, gap=0, offset=0):
        batched = a.ndim == 3
        n = a.shape[0] if batched else 1
        rows, cols = a.shape[-2:]
        b = a.dtype.itemsize
        pitch = b * cols if pitch is None else pitch
        assert pitch % b == 0 and gap % b == 0 and offset % b == 0 and pitch >= b * cols
        fs = rows * pitch + gap
        used = (n - 1) * fs + (rows - 1) * pitch + b * cols
        self.buf = torch.full((offset + used,), 0xA5, dtype=torch.uint8, device=DEV)
        body = self.buf[offset:] if b == 1 else self.buf[offset:].view(torch.int16)
        view = torch.as_strided(body, (n, rows, cols), (fs // b, pitch // b, 1))
        view.copy_(t(a.reshape(n, rows, cols)))
        self.view = view if batched else view[0]
        self.before = self.buf.clone()

    def intact(self):
        return torch.equal(self.buf, self.before)


def surfaces(planes, extra=0, gap=0, y_offset=0):
    """ref.lay_out's numpy planes -> (the same keyword arguments as device views, the Surfaces behind them); extra: pitch bytes beyond the row"""
    s = {k: Surface(p, p.dtype.itemsize * p.shape[-1] + extra, gap, y_offset if k == "y" else 0) for k, p in planes.items()}
    return {k: x.view for k, x in s.items()}, list(s.values())


# (H, W, pitch beyond the row: bytes, or 's' for one sample, frames, extra bytes between frames, Y base offset in samples)
GEOMETRIES = [(1, 1, 0, None, 0, 0), (1, 2, 0, None, 0, 0), (3, 5, 0, None, 0, 0), (2, 4, 0, None, 0, 0), (4, 8, 4, None, 0, 0), (4, 8, 16, None, 0, 0),
              (4, 8, 's', None, 0, 0), (4, 8, 0, None, 0, 1), (6, 12, 0, 3, 2, 0), (6, 12, 16, 3, 32, 0), (23, 37, 0, None, 0, 0)]
RAGGED = [g for g in GEOMETRIES if g[:2] in ((1, 1), (1, 2), (3, 5), (23, 37)) or g[2] == 's' or g[5] or g[4] == 2]
OWNED = ("nv21", "yuv422p", "nv16", "yuyv422", "uyvy422", "yuv444p", "nv42", "yuv422p10le", "p210", "yuv444p10le", "p410")
_WANT = {}


def want(c, geo, matrix):
    """a geometry's planes in format c and ref_yuvfmt's frame and packed luma of them, computed once per (format, geometry, matrix)"""
    key = (c, geo, matrix)
    if key not in _WANT:
        H, W, _, n, _, _ = geo
        Y, U, V = ref.random_samples(c, np.random.RandomState(c + H * 100 + W + 7 * len(_WANT)), H, W, n)
        planes = ref.lay_out(c, Y, U, V)
        _WANT[key] = (planes, ref.to_bgr(c, matrix=matrix, width=W, **planes), ref.y_packed(c, planes["y"], W))
    return _WANT[key]


def placed(c, geo, matrix):
    H, W, extra, n, gap, off = geo
    b = 1 if ref.fields(c)[2] == 0 else 2
    planes, bgr, yp = want(c, geo, matrix)
    dev, surf = surfaces(planes, b if extra == 's' else extra, gap, off * b)
    return dict(width=W, matrix=matrix, **dev), surf, bgr, yp


# ---- 1: the reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ref.ALL, ids=fmt_id)
def test_yuv_to_bgr_u8_equals_the_reference(yuvfmt, c):
    """lsfa_yuv_to_bgr_u8 == ref_yuvfmt at every geometry under every matrix, in bgr and in y_packed; the planes' allocations keep every bit"""
    for geo in GEOMETRIES:
        for matrix in MATRICES:
            kw, surf, bgr, yp = placed(c, geo, matrix)
            got = yuvfmt.yuv_to_bgr_u8(c, **kw)
            assert got.dtype == torch.uint8 and tuple(got.shape) == bgr.shape, (geo, matrix)
            np.testing.assert_array_equal(got.cpu().numpy(), bgr, err_msg=str((geo, matrix)))
            luma = torch.full(yp.shape, 9, dtype=torch.uint8, device=DEV)
            out = torch.empty_like(got)
            assert yuvfmt.yuv_to_bgr_u8(c, out=out, y_packed=luma, **kw) is out
            np.testing.assert_array_equal(out.cpu().numpy(), bgr, err_msg=str((geo, matrix)))
            np.testing.assert_array_equal(luma.cpu().numpy(), yp, err_msg=str((geo, matrix)))
            assert all(s.intact() for s in surf), geo


def test_full_size(yuvfmt):
    """one frame of 1000 x 600: NV16 under BT.709 through all three exports' plane kernels"""
    c, geo = ref.NAMES["nv16"], (600, 1000, 0, None, 0, 0)
    kw, _, bgr, yp = placed(c, geo, "bt709")
    luma = torch.zeros((600, 1000), dtype=torch.uint8, device=DEV)
    got = yuvfmt.yuv_to_bgr_u8(c, y_packed=luma, **kw)
    np.testing.assert_array_equal(got.cpu().numpy(), bgr)
    np.testing.assert_array_equal(luma.cpu().numpy(), yp)
    assert bgr.min() == 0 and bgr.max() == 255
    np.testing.assert_array_equal(yuvfmt.image_transform_yuv(c, pixel_means=means(), pixel_scale=PS, **kw).cpu().numpy(), ref.transform(bgr[None], means(), PS))


# ---- 2: the shipped kernels ---------------------------------------------------------------------------------------------------------------
def test_the_shipped_4_2_0_formats_give_the_shipped_kernels_bytes(hip, yuvfmt):
    """nv12, i420, p010, yuv420p10le through the new exports == hip.yuv420_to_bgr_u8 / yuv10.yuv420p10_to_bgr_u8 and their fused forms; nv21
    == nv12 of swapped chroma"""
    from lsfa_amd import yuv10
    mn = means()
    for geo in GEOMETRIES:
        for name, matrix in (("nv12", "bt601"), ("i420", "bt709"), ("p010", "jpeg"), ("yuv420p10le", "bt601")):
            kw, _, _, _ = placed(ref.NAMES[name], geo, matrix)
            kw.pop("width")
            shipped = dict(kw, msb_aligned=name == "p010") if "10" in name else kw
            a, b, c3 = ((yuv10.yuv420p10_to_bgr_u8, yuv10.image_transform_yuv420p10, yuv10.image_resize_transform_yuv420p10) if "10" in name else
                        (hip.yuv420_to_bgr_u8, hip.image_transform_yuv420, hip.image_resize_transform_yuv420))
            l1, l2 = (torch.zeros(kw["y"].shape, dtype=torch.uint8, device=DEV) for _ in range(2))
            assert torch.equal(yuvfmt.yuv_to_bgr_u8(name, y_packed=l1, **kw), a(y_packed=l2, **shipped)) and torch.equal(l1, l2), (name, geo)
            assert torch.equal(yuvfmt.image_transform_yuv(name, pixel_means=mn, pixel_scale=PS, **kw), b(pixel_means=mn, pixel_scale=PS, **shipped)), (name, geo)
            assert torch.equal(yuvfmt.image_resize_transform_yuv(name, im_scale=1.25, stride=16, pixel_means=mn, pixel_scale=PS, **kw),
                               c3(im_scale=1.25, stride=16, pixel_means=mn, pixel_scale=PS, **shipped)), (name, geo)
        planes, _, _ = want(ref.NAMES["nv12"], geo, "bt601")
        vu = np.ascontiguousarray(planes["uv"].reshape(planes["uv"].shape[:-1] + (-1, 2))[..., ::-1]).reshape(planes["uv"].shape)
        assert torch.equal(yuvfmt.yuv_to_bgr_u8("nv21", t(planes["y"]), uv=t(vu)), hip.yuv420_to_bgr_u8(t(planes["y"]), uv=t(planes["uv"]))), geo


@pytest.mark.parametrize("sub", (1, 2))
def test_doubled_chroma_gives_the_shipped_4_2_0_result(hip, yuvfmt, sub):
    """4:2:2 planes made by writing each 4:2:0 chroma row twice and 4:4:4 planes doubled both ways, in every layout of bytes == hip.yuv420_to_bgr_u8"""
    for H, W in ((3, 5), (4, 8), (6, 12), (23, 37)):
        Y, U, V = ref.random_samples(ref.code(0, 0, 0), np.random.RandomState(H + W), H, W)
        for matrix in MATRICES:
            shipped = hip.yuv420_to_bgr_u8(t(Y), u=t(U), v=t(V), matrix=matrix)
            u2, v2 = ref.upsample(U, V, sub, H, W)
            for layout in (0, 1, 2) + ((3, 4) if sub == 1 else ()):
                c = ref.code(sub, layout, 0)
                kw = {k: t(p) for k, p in ref.lay_out(c, Y, u2, v2).items()}
                assert torch.equal(yuvfmt.yuv_to_bgr_u8(c, matrix=matrix, width=W, **kw), shipped), (H, W, matrix, layout)


# ---- 3, 4: the fused forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ref.ALL, ids=fmt_id)
def test_image_transform_yuv_is_the_two_step_path(hip, yuvfmt, c):
    """lsfa_image_transform_yuv == image_transform_u8(yuv_to_bgr_u8(...)) wherever the u8 form runs (H*W % 4 == 0), and == ref_yuvfmt + the
    float64 formula at every geometry"""
    mn = means()
    for gi, geo in enumerate(GEOMETRIES):
        H, W, _, n, _, _ = geo
        kw, surf, bgr, _ = placed(c, geo, MATRICES[gi % 3])
        got = yuvfmt.image_transform_yuv(c, pixel_means=mn, pixel_scale=PS, **kw)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n or 1, 3, H, W)
        np.testing.assert_array_equal(got.cpu().numpy(), ref.transform(bgr if n else bgr[None], mn, PS), err_msg=str(geo))
        if (H * W) % 4 == 0:
            frame = yuvfmt.yuv_to_bgr_u8(c, **kw)
            assert torch.equal(got, hip.image_transform_u8(frame if n else frame.unsqueeze(0), mn, PS)), geo
        assert all(s.intact() for s in surf), geo


@pytest.mark.parametrize("stride", [0, 16])
@pytest.mark.parametrize("scale", [0.5, 0.6, 1.25])
def test_image_resize_transform_yuv_is_the_two_step_path(hip, yuvfmt, scale, stride):
    """lsfa_image_resize_transform_yuv == image_resize_transform (uint8 frames, float interpolation) of the converted frame: every format at
    an odd size and three pitched frames, both subtraction rules"""
    mn = means()
    for c in ref.ALL:
        for geo in ((23, 37, 0, None, 0, 0), (6, 12, 16, 3, 32, 0)):
            kw, surf, bgr, _ = placed(c, geo, MATRICES[c % 3])
            frame = yuvfmt.yuv_to_bgr_u8(c, **kw)
            np.testing.assert_array_equal(frame.cpu().numpy(), bgr)
            expect = hip.image_resize_transform(frame, scale, mn, PS, stride=stride)
            out = torch.full_like(expect, 7.0)
            got = yuvfmt.image_resize_transform_yuv(c, im_scale=scale, pixel_means=mn, pixel_scale=PS, stride=stride, out=out, **kw)
            assert got is out and torch.equal(got, expect), (fmt_id(c), geo)
            assert float(got.abs().max()) > 0 and all(s.intact() for s in surf)


# ---- 5: the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_c_abi_returns_einval_and_launches_nothing(hip, yuvfmt):
    """the header's list, through all three exports: LSFA_EINVAL with the export's name in the message, no launch counted under LSFA_OP_STEM,
    the outputs untouched; then the same buffers through well-formed calls: one launch each, and correct"""
    H, W = 4, 8
    mn = means()
    L = hip.lib()
    mean_arr = (ctypes.c_double * 3)(*mn)
    F = yuvfmt.code
    geo = (H, W, 16, None, 0, 0)
    dev = {name: placed(ref.NAMES[name], geo, "bt601") for name in ("nv16", "yuv422p", "yuyv422", "p210", "yuv422p10le", "nv24")}
    bgr = torch.full((H, W, 3), 7, dtype=torch.uint8, device=DEV)
    data = torch.full((1, 3, H, W), 7.0, device=DEV)
    rdata = torch.full((1, 3, 16, 16), 7.0, device=DEV)          # scale 1.25: 5 x 10, padded to 16

    def args(name, **over):
        kw = dev[name][0]
        b = kw["y"].element_size()
        cp = kw.get("uv", kw.get("u"))
        a = dict(y=kw["y"].data_ptr(), y_pitch=b * kw["y"].stride(-2), y_fs=0, c=cp.data_ptr() if cp is not None else None,
                 v=kw["v"].data_ptr() if "v" in kw else None, c_pitch=b * cp.stride(-2) if cp is not None else 0, c_fs=0, N=1, H=H, W=W, matrix=0,
                 format=ref.NAMES[name])
        a.update(over)
        return [a[k] for k in ("y", "y_pitch", "y_fs", "c", "v", "c_pitch", "c_fs", "N", "H", "W", "matrix", "format")]

    def calls(name, bgr_ptr, data_ptr, rdata_ptr, mean_ptr=mean_arr, **over):
        a = args(name, **over)
        return (("lsfa_yuv_to_bgr_u8", a + [bgr_ptr, None, None]),
                ("lsfa_image_transform_yuv", a + [mean_ptr, PS, data_ptr, None]),
                ("lsfa_image_resize_transform_yuv", a + [1.25, 5, 10, 16, mean_ptr, PS, rdata_ptr, 16, 16, None]))

    some = dev["nv16"][0]["y"].data_ptr()
    bad = [("nv16", over) for over in (
        dict(y=None), dict(c=None), dict(N=0), dict(N=-1), dict(H=0), dict(H=-3), dict(W=0), dict(W=-8), dict(matrix=3), dict(matrix=-1),
        dict(y_pitch=W - 1), dict(c_pitch=W - 1), dict(y_pitch=0), dict(y_pitch=-32), dict(v=some),
        dict(format=3), dict(format=15), dict(format=F(1, 5, 0)), dict(format=F(1, 1, 3)), dict(format=1 << 12 | F(1, 1, 0)), dict(format=-1),
        dict(format=F(1, 0, 0)),                                                   # planar without v
        dict(format=F(2, 1, 0), c_pitch=2 * W - 1), dict(format=F(2, 2, 0), c_pitch=2 * W - 2),          # 4:4:4 interleaved: the chroma row is 2 W
        dict(format=F(1, 3, 0)), dict(format=F(1, 4, 0)))]                          # packed with chroma planes
    bad += [("yuyv422", over) for over in (
        dict(format=F(0, 3, 0)), dict(format=F(2, 4, 0)), dict(format=F(1, 3, 1)), dict(format=F(1, 4, 2)), dict(y=None), dict(c=some), dict(v=some),
        dict(c_pitch=16), dict(c_fs=64), dict(y_pitch=2 * W - 1), dict(y_pitch=2 * W - 4), dict(W=17))]          # nine groups: 36 bytes
    bad += [("yuv422p", over) for over in (dict(v=None), dict(c_pitch=W // 2 - 1), dict(format=F(2, 0, 0), c_pitch=W - 1))]
    bad += [("p210", over) for over in (
        dict(y=dev["p210"][0]["y"].data_ptr() + 1), dict(c=dev["p210"][0]["uv"].data_ptr() + 1), dict(y_pitch=2 * W + 17), dict(c_pitch=2 * W + 17),
        dict(y_fs=101), dict(c_fs=-3), dict(y_pitch=2 * W - 2), dict(c_pitch=2 * W - 2))]
    bad += [("yuv422p10le", dict(v=dev["yuv422p10le"][0]["v"].data_ptr() + 1)), ("yuv422p10le", dict(c_pitch=W - 2))]
    hip.prof_enable(True, ops=["stem"])
    try:
        hip.prof_read()
        for name, over in bad:
            for export, a in calls(name, bgr.data_ptr(), data.data_ptr(), rdata.data_ptr(), **over):
                assert getattr(L, export)(*a) == -1, (export, name, over)                          # LSFA_EINVAL
                assert export.encode() in L.lsfa_last_error(), (export, name, over)
        # NULL outputs and means
        for export, a in calls("nv16", None, None, None):
            assert getattr(L, export)(*a) == -1, export
        for export, a in calls("nv16", bgr.data_ptr(), data.data_ptr(), rdata.data_ptr(), mean_ptr=None)[1:]:
            assert getattr(L, export)(*a) == -1, export
        # an output shape that does not follow from h1 / w1 / stride, a scale of zero
        a = args("nv16")
        assert L.lsfa_image_resize_transform_yuv(*(a + [1.25, 5, 10, 16, mean_arr, PS, rdata.data_ptr(), 16, 32, None])) == -1
        assert b"padded to 16 gives 16 x 16" in L.lsfa_last_error()
        assert L.lsfa_image_resize_transform_yuv(*(a + [0.0, 5, 10, 16, mean_arr, PS, rdata.data_ptr(), 16, 16, None])) == -1
        assert hip.prof_read()["stem"][1] == 0                 # nothing was launched
        torch.cuda.synchronize()
        assert bool((bgr == 7).all()) and bool((data == 7.0).all()) and bool((rdata == 7.0).all())
        # ... and the same buffers are written by the good calls, one launch each
        for name in sorted(dev):
            bgr.fill_(7)
            for export, a in calls(name, bgr.data_ptr(), data.data_ptr(), rdata.data_ptr()):
                assert getattr(L, export)(*a) == 0, (export, name, L.lsfa_last_error())
            ms, n = hip.prof_read()["stem"]
            assert n == 3 and ms > 0.0, name
            want_bgr = dev[name][2]
            np.testing.assert_array_equal(bgr.cpu().numpy(), want_bgr)
            np.testing.assert_array_equal(data.cpu().numpy(), ref.transform(want_bgr[None], mn, PS))
            hip.prof_enable(False)
            assert torch.equal(rdata, hip.image_resize_transform(bgr, 1.25, mn, PS, stride=16))
            hip.prof_enable(True, ops=["stem"])
    finally:
        hip.prof_enable(False)


def test_one_launch_per_call_of_either_kernel(hip, yuvfmt):
    """the wrappers, through the four-pixel and the element-wise kernel: one launch each under LSFA_OP_STEM"""
    hip.prof_enable(True, ops=["stem"])
    try:
        hip.prof_read()
        calls = 0
        for c in (ref.NAMES["nv16"], ref.NAMES["uyvy422"], ref.NAMES["p410"], ref.NAMES["nv21"]):
            for geo in ((4, 8, 16, None, 0, 0), (3, 5, 0, None, 0, 0)):
                kw = placed(c, geo, "bt601")[0]
                yuvfmt.yuv_to_bgr_u8(c, **kw)
                yuvfmt.image_transform_yuv(c, **kw)
                yuvfmt.image_resize_transform_yuv(c, im_scale=1.5, stride=16, **kw)
                calls += 3
        ms, n = hip.prof_read()["stem"]
    finally:
        hip.prof_enable(False)
    assert n == calls == 24 and ms > 0.0


# ---- 6: the estimators --------------------------------------------------------------------------------------------------------------------
def clip_of(c, n, width, height, m, seed):
    """n frames of a translating texture in format c - ref_yuv.forward's 4:2:0 planes, the chroma doubled to the format's subsampling, for
    words times four plus two random low bits with the ignored bits random - with ref_yuvfmt's BGR frames and packed luma of them"""
    rs = np.random.RandomState(seed)
    sub, _, sample = ref.fields(c)
    planes, frames, lumas = [], [], []
    for f in ref_me.translated_clip(n, width, height, m, seed=seed, sigma=2.0):
        Y, U, V = ref_yuv.forward(f)
        U, V = ref.upsample(U, V, sub, height, width)
        if sample:
            Y, U, V = (ref_yuv10.widen(p, 0 if sample == 1 else 6, low_bits=0) for p in (Y, U, V))
            junk = [rs.randint(0, 4, p.shape).astype(np.uint16) << (0 if sample == 1 else 6) for p in (Y, U, V)]
            wild = [rs.randint(0, 64, p.shape).astype(np.uint16) << (10 if sample == 1 else 0) for p in (Y, U, V)]
            Y, U, V = (p | j | w for p, j, w in zip((Y, U, V), junk, wild))
        laid = ref.lay_out(c, Y, U, V)
        planes.append(laid)
        frames.append(ref.to_bgr(c, width=width, **laid))
        lumas.append(ref.y_packed(c, laid["y"], width))
    return planes, frames, lumas


ESTIMATED = ("nv21", "nv16", "yuv444p", "yuyv422", "p210")          # one of each sub, one packed, one of words


@pytest.mark.parametrize("name", ESTIMATED)
def test_motion_estimator_yuv_chain(hip, yuvfmt, name):
    """48 x 64, search 4, a key frame and three frames.  luma_from='bgr': rows, SAD, accumulated field and network_inputs are hip.MotionEstimator's
    fed the converted BGR frames.  luma_from='y': rows and SAD are hip.mv_estimate's on the frames' own luma."""
    height, width = 48, 64
    planes, frames, lumas = clip_of(ref.NAMES[name], 4, width, height, (2, -1), seed=48)
    mn = means()
    a = yuvfmt.MotionEstimatorYuv(width, height, DEV, fmt=name, search=4, lam=4)
    b = hip.MotionEstimator(width, height, DEV, search=4, lam=4)
    c = yuvfmt.MotionEstimatorYuv(width, height, DEV, fmt=name, search=4, lam=4, luma_from='y')
    assert a.bgr_key is None and a.bgr_cur is None
    dp = [surfaces(p, extra=16)[0] for p in planes]
    df, dl = [t(f) for f in frames], [t(p) for p in lumas]
    key = a.key_frame_yuv(**dp[0])
    assert key is a.bgr_key and torch.equal(key, df[0])
    b.key_frame(df[0])
    c.key_frame_yuv(**dp[0])
    for f in (1, 2, 3):
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


def test_segment_motion_estimator_yuv_equals_segment_on_the_converted_stack(hip, yuvfmt):
    """2 clips of a key frame + 2 frames, 32 x 48: segment_yuv == SegmentMotionEstimator.segment on ref_yuvfmt's frames; with luma_from='y'
    the rows are hip.mv_estimate_chain's on the frames' own luma"""
    H, W, C, n = 32, 48, 2, 2
    mn = means()
    for name in ("uyvy422", "yuv422p10le", "nv42"):
        clips = [clip_of(ref.NAMES[name], n + 1, W, H, m, seed=s) for m, s in (((2, -1), 5), ((-1, 2), 6))]
        stack = {k: np.stack([p[k] for planes, _, _ in clips for p in planes]) for k in clips[0][0][0]}
        bgr = np.stack([np.stack(frames) for _, frames, _ in clips])
        luma = np.stack([np.stack(l) for _, _, l in clips])
        kw, _ = surfaces(stack, extra=8, gap=32)
        a = yuvfmt.SegmentMotionEstimatorYuv(W, H, frames=n, clips=C, device=DEV, fmt=name, search=4, lam=4)
        b = hip.SegmentMotionEstimator(W, H, frames=n, clips=C, device=DEV, search=4, lam=4)
        a_mv, a_res = a.segment_yuv(im_scale=1.25, pixel_means=mn, pixel_scale=PS, **kw)
        b_mv, b_res = b.segment(t(bgr), 1.25, mn, PS)
        assert torch.equal(a.bgr, t(bgr)) and torch.equal(a.rows, b.rows) and torch.equal(a.sad, b.sad), name
        assert torch.equal(a_mv, b_mv) and torch.equal(a_res, b_res) and float(a_mv.abs().max()) > 0, name
        c = yuvfmt.SegmentMotionEstimatorYuv(W, H, frames=n, clips=C, device=DEV, fmt=name, search=4, lam=4, luma_from='y')
        c.segment_yuv(im_scale=1.25, pixel_means=mn, pixel_scale=PS, **kw)
        want_rows = hip.mv_estimate_chain(t(luma), 4, 4, c.max_sad)
        assert torch.equal(c.rows, want_rows.view_as(c.rows)) and torch.equal(c.bgr, t(bgr)), name


def test_motion_estimator_yuv_graph_capture_and_no_allocation_after_the_first_call(yuvfmt):
    """key_frame_yuv + two next_frame_yuv + network_inputs of packed YUYV frames: nothing is allocated after the first pass; captured with
    torch.cuda.graph on one stream and replayed on NEW contents written into the same tensors == the eager run on those contents"""
    width, height = 64, 48
    mn = means()
    c = ref.NAMES["yuyv422"]
    clips = [clip_of(c, 3, width, height, (2, -1), seed=1)[0], clip_of(c, 3, width, height, (-3, 2), seed=2)[0]]
    bufs = [surfaces(p, extra=16)[0] for p in clips[0]]
    me = yuvfmt.MotionEstimatorYuv(width, height, DEV, fmt="yuyv422", search=16, lam=4)

    def step(m, planes):
        m.key_frame_yuv(**planes[0])
        m.next_frame_yuv(**planes[1])
        m.next_frame_yuv(**planes[2])
        return m.network_inputs(m.bgr_cur, m.bgr_key, 1.0, mn, 1.0)

    step(me, bufs)                           # the first pass: the BGR buffers and network_inputs' outputs are allocated here
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    me.key_frame_yuv(**bufs[0])
    me.next_frame_yuv(**bufs[1])
    me.next_frame_yuv(**bufs[2])
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] == before          # nothing is allocated after the first *_yuv call
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_mv, out_res = step(me, bufs)
    for k, clip in enumerate(clips[::-1] + clips):
        for buf, p in zip(bufs, clip):
            buf["y"].copy_(t(p["y"]))
        g.replay()
        torch.cuda.synchronize()
        eager = yuvfmt.MotionEstimatorYuv(width, height, DEV, fmt="yuyv422", search=16, lam=4)
        e_mv, e_res = step(eager, [surfaces(p)[0] for p in clip])
        assert torch.equal(me.rows, eager.rows) and torch.equal(me.sad, eager.sad), k
        assert torch.equal(out_mv, e_mv) and torch.equal(out_res, e_res), k
    assert float(out_mv.abs().max()) > 0


# ---- 7: memory ownership ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", guarded_arena.PATTERNS, ids=["0xFF", "0x7F"])
def test_no_result_depends_on_memory_a_call_does_not_own(yuvfmt, pattern):
    """the three wrappers at the ragged geometries, in eleven formats (every layout, subsampling and sample size): the outputs the wrappers allocate themselves lie between bands of
    `pattern`, which stay intact; the results equal those on ordinary tensors; every input plane is an allocation of exactly its size and
    keeps every bit"""
    mn = means()
    for c in (ref.NAMES[name] for name in OWNED):
        for gi, geo in enumerate(RAGGED):
            kw, surf, bgr, yp = placed(c, geo, MATRICES[(c + gi) % 3])
            plain = (yuvfmt.yuv_to_bgr_u8(c, **kw), yuvfmt.image_transform_yuv(c, pixel_means=mn, pixel_scale=PS, **kw),
                     yuvfmt.image_resize_transform_yuv(c, im_scale=1.25, stride=16, pixel_means=mn, pixel_scale=PS, **kw))
            arena = guarded_arena.Arena(pattern)
            with pytest.MonkeyPatch.context() as mp, guarded_arena.guarded_allocations(mp, arena):
                luma = arena.place(yp.shape, torch.uint8, "y_packed")
                guarded = (yuvfmt.yuv_to_bgr_u8(c, y_packed=luma, **kw), yuvfmt.image_transform_yuv(c, pixel_means=mn, pixel_scale=PS, **kw),
                           yuvfmt.image_resize_transform_yuv(c, im_scale=1.25, stride=16, pixel_means=mn, pixel_scale=PS, **kw))
            assert all(arena.record(g) is not None for g in guarded), (fmt_id(c), geo)
            arena.check()
            torch.cuda.synchronize()          # the status is clear: nothing faulted
            assert guarded_arena.same(guarded_arena.host(plain), guarded_arena.host(guarded)), (fmt_id(c), geo)
            np.testing.assert_array_equal(luma.cpu().numpy(), yp)
            np.testing.assert_array_equal(guarded[0].cpu().numpy(), bgr)
            assert all(s.intact() for s in surf), (fmt_id(c), geo)


# ---- 8: the demo --------------------------------------------------------------------------------------------------------------------------
def test_demo_runs_nv12_yuv422p_yuyv422_and_yuv444p_of_one_clip_to_the_same_detections(hip, yuvfmt, tmp_path):
    """an 8-frame 160 x 96 clip four ways from one set of 4:2:0 planes - NV12, yuv422p (chroma rows doubled), yuyv422 and yuv444p (doubled both
    ways) - through lsfa_amd.demo --yuv --estimate-mv --dump-mv: identical detections, identical dumps"""
    from lsfa_amd import demo
    W, H, n = 160, 96, 8
    planes = [ref_yuv.forward(f) for f in ref_me.translated_clip(n, W, H, (3, -2), seed=6, sigma=2.0)]
    formats = ("nv12", "yuv422p", "yuyv422", "yuv444p")
    for name in formats:
        c = ref.NAMES[name]
        with open(str(tmp_path / ("clip." + name)), "wb") as f:
            for Y, U, V in planes:
                f.write(ref.raw_frame_bytes(c, Y, *ref.upsample(U, V, ref.fields(c)[0], H, W)))
        assert (tmp_path / ("clip." + name)).stat().st_size == n * yuvfmt.frame_bytes(name, W, H)
    outs = {}
    common = ["--size", "%dx%d" % (W, H), "--estimate-mv", "--interval", "4", "--score", "0.05"]
    for name in formats:
        out = tmp_path / (name + ".json")
        demo.main(["--yuv", str(tmp_path / ("clip." + name)), "--yuv-format", name, "--dump-mv", str(tmp_path / ("mv_" + name)), "--out", str(out)] + common)
        outs[name] = [(r["key"], r["dets"]) for r in json.loads(out.read_text())]          # (the frame names carry the file's name)
    assert outs["nv12"] == outs["yuv422p"] == outs["yuyv422"] == outs["yuv444p"]
    assert [k for k, _ in outs["nv12"]] == [i % 4 == 0 for i in range(n)] and sum(len(d) for _, d in outs["nv12"]) > 0
    non_key = [i for i in range(n) if i % 4]
    for name in formats[1:]:
        assert sorted(p.name for p in (tmp_path / ("mv_" + name)).iterdir()) == ["%06d.npz" % i for i in non_key]
        for i in non_key:
            a, b = np.load(str(tmp_path / "mv_nv12" / ("%06d.npz" % i))), np.load(str(tmp_path / ("mv_" + name) / ("%06d.npz" % i)))
            assert (a["mv"] == b["mv"]).all() and (a["res"] == b["res"]).all(), (name, i)
    assert np.abs(a["mv"]).max() > 0
    from lsfa_amd.config.config import lsfa_test_config
    clip = demo.YuvFileClip(str(tmp_path / "clip.yuyv422"), W, H, lsfa_test_config(), "yuyv422")
    assert clip.num_frames == n and clip.frame_bytes == 2 * W * H and tuple(clip.planes(0)["y"].shape) == (H, 2 * W)
