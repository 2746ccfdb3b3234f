"""tests/ref_overlay_fmt.py (the numpy statement of the overlay on every YUV surface of the intake) pinned without a GPU by derived answers;
the refusals of overlay.Overlay.draw_yuv under the spy of tests/binding_contract.py and the demo's --draw-raw arguments: nothing here
launches a kernel."""
import numpy as np
import pytest
import torch

import binding_contract as bc
import ref_overlay
import ref_overlay_fmt as ref
import ref_yuv
import ref_yuvfmt
from lsfa_amd import demo, hip, overlay, yuvfmt

FONT = overlay.font_table()
NCLS = 5
BGR = overlay.palette(NCLS)
COLORS = overlay.bgr_to_yuv(BGR, "bt601")
SENTINEL = 0x5A


def random_index(rs, H, W):
    """the index map of random thin boxes on an H x W frame, with one-character labels where the frame has room for them: covered and
    uncovered pixels in every neighbourhood"""
    rows = 2
    dets = np.zeros((NCLS, rows, 5))
    counts = np.full(NCLS, rows, np.int32)
    dets[..., 0], dets[..., 1] = rs.uniform(-2, W - 1, (NCLS, rows)), rs.uniform(-2, H - 1, (NCLS, rows))
    dets[..., 2], dets[..., 3] = dets[..., 0] + rs.uniform(0, 0.6 * W + 1, (NCLS, rows)), dets[..., 1] + rs.uniform(0, 0.6 * H + 1, (NCLS, rows))
    dets[..., 4] = rs.uniform(0.3, 1.0, (NCLS, rows))
    kw = dict(thickness=1, label_scale=1 if H >= 20 else 0, with_score=False)
    recs, n = ref_overlay.plan(dets, counts, 0.5, H, W, **kw)
    index = ref_overlay.cover(recs, H, W, NCLS, FONT, kw["thickness"], kw["label_scale"])
    assert H * W < 30 or ((index >= 0).any() and (index < 0).any())
    return index


def index_of_boxes(rows, H, W):
    """thickness 1, no label: rows [(class, x1, y1, x2, y2)]"""
    dets, counts = np.zeros((NCLS, 4, 5)), np.zeros(NCLS, np.int32)
    for j, *box in rows:
        dets[j, counts[j]] = box + [0.9]
        counts[j] += 1
    recs, _ = ref_overlay.plan(dets, counts, 0.5, H, W, thickness=1, label_scale=0)
    return ref_overlay.cover(recs, H, W, NCLS, FONT, 1, 0)


def surface(c, rs, H, W, fill=None):
    """the planes of one frame of format c as keyword arguments: random samples, or every byte / word `fill`"""
    Y, U, V = ref_yuvfmt.random_samples(c, rs, H, W)
    if fill is not None:
        Y, U, V = (np.full_like(a, fill) for a in (Y, U, V))
    p = ref_yuvfmt.lay_out(c, Y, U, V)
    if fill is not None:
        p["y"][...] = fill
    return p


def copy(p):
    return {k: a.copy() for k, a in p.items()}


SIZES = [(1, 1), (5, 7), (8, 12), (9, 16), (21, 31)]


@pytest.mark.parametrize("H,W", SIZES)
def test_the_420_codes_equal_ref_overlay_byte_for_byte(H, W):
    rs = np.random.RandomState(H * 100 + W)
    index = random_index(rs, H, W)
    for name in ("nv12", "i420"):
        c = ref_yuvfmt.NAMES[name]
        p = surface(c, rs, H, W)
        want = copy(p)
        ref_overlay.paint_yuv420(want["y"], index, COLORS, **{k: a for k, a in want.items() if k != "y"})
        assert ref.paint(name, index, COLORS, **p) is p["y"]
        for k in p:
            np.testing.assert_array_equal(p[k], want[k], err_msg="%s %s" % (name, k))
        q = copy(want)
        ref.paint(c, index, COLORS, **q)           # a code as well as a name; painting twice changes nothing
        assert all((q[k] == want[k]).all() for k in q)


@pytest.mark.parametrize("H,W", SIZES)
def test_yuv444p_planes_are_the_index_map_looked_up(H, W):
    rs = np.random.RandomState(H + W)
    index = random_index(rs, H, W)
    p = surface(ref_yuvfmt.NAMES["yuv444p"], rs, H, W)
    before = copy(p)
    ref.paint("yuv444p", index, COLORS, **p)
    for col, k in enumerate(("y", "u", "v")):
        np.testing.assert_array_equal(p[k], np.where(index >= 0, COLORS[np.maximum(index, 0), col], before[k]))


def test_edges_on_odd_columns_and_rows_reach_chroma_as_the_subsampling_says():
    H, W = 12, 16
    index = index_of_boxes([(1, 3, 2, 9, 8)], H, W)         # left edge at x = 3, right at 9: odd; top at y = 2, bottom at 8: even
    assert (index[3:8, 3] == 1).all() and (index[3:8, 4] == -1).all()
    planes = {}
    for name in ("i420", "yuv422p", "yuv444p"):
        p = surface(ref_yuvfmt.NAMES[name], np.random.RandomState(1), H, W, fill=SENTINEL)
        ref.paint(name, index, COLORS, **p)
        assert (p["y"][3:8, 3] == COLORS[1, 0]).all()          # luma is drawn everywhere
        planes[name] = p
    # the vertical edge (rows strictly between the horizontal ones): untouched in 4:2:0 and 4:2:2, written in 4:4:4
    assert (planes["i420"]["u"][2:4, 1] == SENTINEL).all() and (planes["i420"]["v"][2:4, 4] == SENTINEL).all()
    assert (planes["yuv422p"]["u"][3:8, 1] == SENTINEL).all() and (planes["yuv422p"]["v"][3:8, 4] == SENTINEL).all()
    assert (planes["yuv444p"]["u"][3:8, 3] == COLORS[1, 1]).all() and (planes["yuv444p"]["v"][3:8, 9] == COLORS[1, 2]).all()
    # the horizontal edges on even rows reach the chroma of even columns in all three
    assert (planes["i420"]["u"][1, 2:5] == COLORS[1, 1]).all() and (planes["yuv422p"]["u"][2, 2:5] == COLORS[1, 1]).all()
    # an edge on an odd row: untouched in 4:2:0 only
    index = index_of_boxes([(2, 2, 3, 10, 7)], H, W)        # top at y = 3, bottom at 7; left at 2, right at 10
    for name, rows, written in (("i420", (1, 3), False), ("yuv422p", (3, 7), True), ("yuv444p", (3, 7), True)):
        p = surface(ref_yuvfmt.NAMES[name], np.random.RandomState(2), H, W, fill=SENTINEL)
        ref.paint(name, index, COLORS, **p)
        sx = 0 if name == "yuv444p" else 1
        inner = slice((4 >> sx), (8 >> sx) + 1)            # chroma columns of pixels 4 .. 8, strictly inside the vertical edges
        for r in rows:
            assert (p["u"][r, inner] == (COLORS[2, 1] if written else SENTINEL)).all(), (name, r)
            assert (p["v"][r, inner] == (COLORS[2, 2] if written else SENTINEL)).all(), (name, r)
        if name == "i420":                                   # ... while the vertical edges on even columns still reach its even rows
            assert p["u"][2, 1] == COLORS[2, 1] and p["u"][2, 5] == COLORS[2, 1] and (p["u"][2, 2:5] == SENTINEL).all()


@pytest.mark.parametrize("sub", [0, 1, 2])
@pytest.mark.parametrize("sample", [0, 1, 2])
def test_vu_layouts_equal_uv_with_the_chroma_columns_swapped(sub, sample):
    H, W = 7, 9
    rs = np.random.RandomState(10 * sub + sample)
    index = random_index(rs, H, W)
    uv_code, vu_code = ref_yuvfmt.code(sub, ref_yuvfmt.UV, sample), ref_yuvfmt.code(sub, ref_yuvfmt.VU, sample)
    p = surface(uv_code, rs, H, W)
    q = copy(p)
    ref.paint(uv_code, index, COLORS, **p)
    ref.paint(vu_code, index, COLORS[:, [0, 2, 1]], **q)
    assert (p["y"] == q["y"]).all() and (p["uv"] == q["uv"]).all() and COLORS[1, 1] != COLORS[1, 2]


@pytest.mark.parametrize("W", [12, 13, 1])
@pytest.mark.parametrize("name", ["yuyv422", "uyvy422"])
def test_packing_the_painted_planes_equals_painting_the_packed_planes(name, W):
    H = 6
    rs = np.random.RandomState(W)
    index = random_index(rs, H, W)
    c = ref_yuvfmt.NAMES[name]
    Y, U, V = ref_yuvfmt.random_samples(c, rs, H, W)
    packed = ref_yuvfmt.lay_out(c, Y, U, V)["y"]              # with odd W the spare Y byte holds 0x5A
    ref.paint("yuv422p", index, COLORS, y=Y, u=U, v=V)
    ref.paint(name, index, COLORS, y=packed, width=W)
    np.testing.assert_array_equal(packed, ref_yuvfmt.lay_out(c, Y, U, V)["y"])
    if W % 2:
        index[:] = 1                                          # even with every pixel covered
        ref.paint(name, index, COLORS, y=packed, width=W)
        spare = packed.reshape(H, -1, 4)[:, -1, 2 if name == "yuyv422" else 3]
        assert (spare == 0x5A).all() and COLORS[1, 0] != 0x5A


@pytest.mark.parametrize("sub", [0, 1, 2])
@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("sample", [1, 2])
def test_words_are_the_bytes_shifted_and_uncovered_words_keep_all_their_bits(sub, layout, sample):
    H, W = 7, 10
    rs = np.random.RandomState(sub + 3 * layout + 9 * sample)
    index = random_index(rs, H, W)
    shl = 2 if sample == 1 else 8
    c8, c16 = ref_yuvfmt.code(sub, layout, 0), ref_yuvfmt.code(sub, layout, sample)
    p8 = surface(c8, rs, H, W)
    p16 = {k: (a.astype(np.uint16) << shl).astype(np.uint16) for k, a in p8.items()}
    before = copy(p8)
    ref.paint(c8, index, COLORS, **p8)
    ref.paint(c16, index, COLORS, **p16)
    for k in p8:
        np.testing.assert_array_equal(p16[k], p8[k].astype(np.uint16) << shl)          # covered samples (and here the others too)
        assert (p8[k] != before[k]).any()
    ones = surface(c16, rs, H, W, fill=0xFFFF)
    ref.paint(c16, index, COLORS, **ones)
    ignored = 0xFFFF ^ (0x3FF << (0 if sample == 1 else 6))
    sx, sy = ref_yuvfmt.SHIFTS[sub]
    Y, U, V, _ = ref_yuvfmt.split(c16, **ones)
    for plane, hit in ((Y, index >= 0), (U, index[::1 << sy, ::1 << sx] >= 0), (V, index[::1 << sy, ::1 << sx] >= 0)):
        assert (plane[~hit] == 0xFFFF).all() and (plane[hit] & ignored == 0).all() and hit.any() and (~hit).any()


@pytest.mark.parametrize("sample", [0, 1, 2])
@pytest.mark.parametrize("matrix", ["bt601", "bt709", "jpeg"])
def test_a_drawn_colour_reads_back_through_the_intake_as_its_bgr(matrix, sample):
    """every pixel whose own result and the result of its chroma's source pixel are one colour index converts to ref_yuv.convert of that
    colour's Y, U, V - whatever the sample width"""
    H, W = 9, 14
    m = ref_yuv.MATRICES[matrix]
    colors = overlay.bgr_to_yuv(BGR, matrix)
    want_bgr = ref_yuv.convert(colors[:, 0], colors[:, 1], colors[:, 2], m)          # (ncls + 1, 3)
    checked = 0
    for c in [k for k in ref_yuvfmt.ALL if ref_yuvfmt.fields(k)[2] == sample]:
        rs = np.random.RandomState(c)
        index = random_index(rs, H, W)
        sub = ref_yuvfmt.fields(c)[0]
        sx, sy = ref_yuvfmt.SHIFTS[sub]
        p = surface(c, rs, H, W)
        ref.paint(c, index, colors, **p)
        bgr = ref_yuvfmt.to_bgr(c, matrix=m, **p)
        yy, xx = np.arange(H)[:, None], np.arange(W)[None, :]
        source = index[(yy >> sy) << sy, (xx >> sx) << sx]
        same = (index >= 0) & (source == index)
        assert same.any()
        np.testing.assert_array_equal(bgr[same], want_bgr[index[same]], err_msg="format 0x%x %s" % (c, matrix))
        checked += 1
    assert checked == (11 if sample == 0 else 9)


def test_draw_is_plan_cover_and_paint():
    H, W = 9, 13
    rs = np.random.RandomState(4)
    dets = np.zeros((NCLS, 2, 5))
    dets[1, 0], dets[3, 0] = (2, 3, 8, 7, 0.9), (5.5, 1, 12, 6, 0.7)
    counts = np.array([0, 1, 0, 1, 0], np.int32)
    p = surface(ref_yuvfmt.NAMES["uyvy422"], rs, H, W)
    q = copy(p)
    y, recs, n = ref.draw("uyvy422", p["y"], dets, counts, 0.5, FONT, COLORS, width=W, thickness=1, label_scale=1)
    assert y is p["y"] and n == (2, 2)
    ref.paint("uyvy422", ref_overlay.cover(recs, H, W, NCLS, FONT, 1, 1), COLORS, y=q["y"], width=W)
    assert (p["y"] == q["y"]).all()


# ---- Overlay.draw_yuv under the spy ---------------------------------------------------------------------------------------------------------
H, W, R = 6, 10, 5


@pytest.fixture()
def spied(monkeypatch):
    spy = bc.Spy(hip.lib())
    monkeypatch.setattr(hip, "lib", lambda: spy)
    with bc.fake_cuda(monkeypatch):
        yield spy


def z(*shape, dtype=torch.uint8):
    return torch.zeros(shape, dtype=dtype).as_subclass(bc.FakeCuda)


def dz(*lead):
    return z(*(lead + (NCLS, R, 5)), dtype=torch.float64), z(*(lead + (NCLS,)), dtype=torch.int32)


def refused(spy, fn, *a, **kw):
    del spy.calls[:]
    with pytest.raises(hip.LsfaError) as e:
        fn(*a, **kw)
    assert "Overlay.draw_yuv" in str(e.value)
    assert not spy.calls, "%s launched %s before refusing" % (fn.__name__, spy.launched())


def test_a_well_formed_call_reaches_exactly_its_two_exports(spied):
    ov = overlay.Overlay(NCLS, R, max_boxes=7, thickness=2, label_scale=1, device=bc.CUDA0, batch=2)
    dets, counts = dz()
    y, uv = z(H, W + 6, dtype=torch.int16)[:, :W], z(3, 10, dtype=torch.int16)
    assert ov.draw_yuv("p010", y, dets, counts, 0.25, uv=uv, matrix="bt709") is y
    assert spied.launched() == ["lsfa_overlay_plan", "lsfa_overlay_paint_yuv"]
    got = spied.values("lsfa_overlay_paint_yuv")
    assert (got["y_pitch"], got["c_pitch"], got["y_frame_stride"], got["c_frame_stride"], got["N"], got["H"], got["W"], got["v"]) == \
        (2 * (W + 6), 20, 0, 0, 1, H, W, None)
    assert (got["format"], got["max_boxes"], got["thickness"], got["label_scale"], got["ncls"]) == (yuvfmt.FORMATS["p010"], 7, 2, 1, NCLS)
    assert got["colors"] == ov._yuv["bt709"].data_ptr() and got["font"] == ov._font.data_ptr() and got["y"] == y.data_ptr()
    assert got["records"] == ov.records.data_ptr() and got["n"] == ov.n.data_ptr() and got["u_or_uv"] == uv.data_ptr()
    del spied.calls[:]
    packed = z(2, H, 12)
    ov.draw_yuv(yuvfmt.FORMATS["uyvy422"], packed, *dz(2), 0.5, width=5)
    got = spied.values("lsfa_overlay_paint_yuv")
    assert spied.launched() == ["lsfa_overlay_plan", "lsfa_overlay_paint_yuv"] and spied.values("lsfa_overlay_plan")["W"] == 5
    assert (got["N"], got["W"], got["y_pitch"], got["y_frame_stride"], got["u_or_uv"], got["v"], got["c_pitch"], got["c_frame_stride"]) == \
        (2, 5, 12, 12 * H, None, None, 0, 0)
    del spied.calls[:]
    ov.draw_yuv("yuv444p", z(H, W), dets, counts, 0.5, u=z(H, W), v=z(H, W), ids=z(NCLS, R, dtype=torch.int32))
    assert spied.launched() == ["lsfa_overlay_plan_ids", "lsfa_overlay_paint_yuv"] and spied.values("lsfa_overlay_paint_yuv")["v"] is not None


def test_bad_calls_are_refused_before_anything_is_launched(spied):
    ov = overlay.Overlay(NCLS, R, device=bc.CUDA0, batch=2)
    dets, counts = dz()
    fn = ov.draw_yuv
    w16 = lambda *s: z(*s, dtype=torch.int16)          # noqa: E731
    y, uv, u, v = z(H, W), z(3, 10), z(3, 5), z(3, 5)
    refused(spied, fn, "nv12", bc.plain(y).clone(), dets, counts, 0.5, uv=uv)                     # a host tensor, in every position
    refused(spied, fn, "nv12", y, dets, counts, 0.5, uv=bc.plain(uv).clone())
    refused(spied, fn, "i420", y, dets, counts, 0.5, u=u, v=bc.plain(v).clone())
    refused(spied, fn, "nv12", y, bc.plain(dets).clone(), counts, 0.5, uv=uv)
    refused(spied, fn, "nv12", y, dets, bc.plain(counts).clone(), 0.5, uv=uv)
    refused(spied, fn, "p010", y, dets, counts, 0.5, uv=uv)                                        # the dtype of the sample width
    refused(spied, fn, "p010", w16(H, W), dets, counts, 0.5, uv=uv)
    refused(spied, fn, "nv12", w16(H, W), dets, counts, 0.5, uv=w16(3, 10))
    refused(spied, fn, "yuv444p10le", w16(H, W), dets, counts, 0.5, u=w16(H, W), v=z(H, W, dtype=torch.float32))
    refused(spied, fn, "nv16", y, dets, counts, 0.5, uv=uv)                                        # the chroma shape of the subsampling
    refused(spied, fn, "nv24", y, dets, counts, 0.5, uv=z(H, W))
    refused(spied, fn, "yuv422p", y, dets, counts, 0.5, u=u, v=v)
    refused(spied, fn, "yuv444p", y, dets, counts, 0.5, u=z(H, 5), v=z(H, 5))
    refused(spied, fn, "i420", y, dets, counts, 0.5, u=u, v=z(3, 4))
    refused(spied, fn, "nv12", y, dets, counts, 0.5, uv=uv, v=v)                                   # v with an interleaved layout
    refused(spied, fn, "nv21", y, dets, counts, 0.5, uv=uv, u=u, v=v)
    refused(spied, fn, "i420", y, dets, counts, 0.5, uv=uv)                                        # ... and one plane for two
    refused(spied, fn, "i420", y, dets, counts, 0.5, u=u)
    refused(spied, fn, "yuyv422", z(H, 20), dets, counts, 0.5, uv=uv)                              # chroma with a packed layout
    refused(spied, fn, "uyvy422", z(H, 20), dets, counts, 0.5, u=u, v=v)
    refused(spied, fn, "yuyv422", z(H, 18), dets, counts, 0.5)                                     # a packed row that is no whole groups
    refused(spied, fn, "yuyv422", z(H, 20), dets, counts, 0.5, width=8)                            # a width that is not the groups'
    refused(spied, fn, "nv12", y, dets, counts, 0.5, uv=uv, width=W + 1)
    for bad in ("yv12", 0x33, yuvfmt.code(0, yuvfmt.YUYV, 0), yuvfmt.code(1, yuvfmt.UYVY, 1), 1 << 12, -1, 1.0, None, True):
        refused(spied, fn, bad, y, dets, counts, 0.5, uv=uv)                                       # a bad format
    refused(spied, fn, "nv12", y, dets, counts, 0.5, uv=uv, matrix="bt2020")                       # a bad matrix
    refused(spied, fn, "nv12", y, dets, counts, 0.5, uv=uv, matrix=0)
    refused(spied, fn, "nv12", z(H, 2 * W)[:, ::2], dets, counts, 0.5, uv=uv)                      # a last dimension that is not dense
    refused(spied, fn, "nv12", y, dets, counts, 0.5, uv=z(3, 20)[:, ::2])
    refused(spied, fn, "nv12", torch.as_strided(z(H * W), (H, W), (W - 2, 1)), dets, counts, 0.5, uv=uv)          # a pitch below its row
    refused(spied, fn, "nv12", y, dets, counts, 0.5, uv=torch.as_strided(z(30), (3, 10), (8, 1)))
    refused(spied, fn, "i420", y, dets, counts, 0.5, u=u, v=z(3, 8)[:, :5])                        # u and v of different pitch
    refused(spied, fn, "nv12", z(2, H, W), dets, counts, 0.5, uv=z(2, 3, 10))                      # a batch of frames for one frame's detections
    refused(spied, fn, "nv12", z(3, H, W), *dz(3), 0.5, uv=z(3, 3, 10))                            # more frames than the Overlay was made for
    refused(spied, fn, "nv12", y, dets, counts, 0.5, uv=uv, ids=z(NCLS, R, dtype=torch.int64))
    del spied.calls[:]
    fn("nv21", y, dets, counts, 0.5, uv=uv)
    assert spied.launched() == ["lsfa_overlay_plan", "lsfa_overlay_paint_yuv"]


# ---- the demo's arguments -------------------------------------------------------------------------------------------------------------------
def test_the_demo_takes_draw_raw_with_every_format_and_refuses_wrong_combinations(tmp_path, capsys):
    w, h = 8, 4
    for fmt in ("p010", "yuyv422", "nv21", "yuv444p10le", "nv12"):
        src = tmp_path / ("clip." + fmt)
        src.write_bytes(bytes(2 * yuvfmt.frame_bytes(fmt, w, h)))
        a = demo.parse_args(["--yuv", str(src), "--size", "%dx%d" % (w, h), "--yuv-format", fmt, "--draw-raw", str(tmp_path / "out.raw"), "--track",
                             "--draw-thickness", "2", "--draw-scale", "1"])
        assert (a.draw_raw, a.yuv_format, a.draw_thickness, a.draw_scale, a.draw, a.draw_yuv) == (str(tmp_path / "out.raw"), fmt, 2, 1, None, None)
    names = tmp_path / "classes.txt"
    names.write_text("cat\ndog\n")
    yuv = ["--yuv", str(src), "--size", "%dx%d" % (w, h)]
    a = demo.parse_args(yuv + ["--draw-raw", "o.raw", "--draw-yuv", "o.nv12", "--draw", "d", "--classes", str(names)])
    assert (a.draw_raw, a.draw_yuv, a.draw, a.classes) == ("o.raw", "o.nv12", "d", str(names))
    bad = [["--draw-raw", "out.raw"],                                                     # no --yuv
           ["--frames", "dir", "--draw-raw", "out.raw"],
           yuv + ["--draw-raw", str(src)],                                                # onto its input
           yuv + ["--draw-raw", "same.yuv", "--draw-yuv", "same.yuv"],
           yuv + ["--yuv-format", "nv21", "--draw-raw", "o.raw", "--draw-yuv", "o.yuv"],  # --draw-yuv keeps its nv12 | i420 check
           yuv + ["--draw-raw", "o.raw", "--draw-scale", "5"]]
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            demo.parse_args(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
    assert "--draw-raw FILE" in demo.__doc__
