"""tests/ref_overlay.py (the numpy statement of the detection overlay) pinned without a GPU by cases with known answers; the glyph table, the
palette and the YUV colour rows of lsfa_amd/overlay.py; and the refusals of overlay.Overlay's methods and of the demo's arguments under the
spy of tests/binding_contract.py: nothing here launches a kernel."""
import numpy as np
import pytest
import torch

import binding_contract as bc
import ref_overlay as ref
from lsfa_amd import demo, hip, overlay

FONT = overlay.font_table()
NCLS = 4
COLORS = overlay.palette(NCLS)


def dets_of(rows, ncls=NCLS, R=4):
    """rows: [(class, x1, y1, x2, y2, score)] in the order they fill their class -> dets (ncls, R, 5), counts (ncls)"""
    dets, counts = np.zeros((ncls, R, 5)), np.zeros(ncls, np.int32)
    for j, *row in rows:
        dets[j, counts[j]] = row
        counts[j] += 1
    return dets, counts


def index_of(rows, H, W, thresh=0.5, **kw):
    dets, counts = dets_of(rows)
    recs, n = ref.plan(dets, counts, thresh, H, W, **kw)
    return ref.cover(recs, H, W, NCLS, FONT, kw.get("thickness", 3), kw.get("label_scale", 2)), recs, n


def picture(index):
    return ["".join("." if c < 0 else "T" if c == NCLS else str(c) for c in row) for row in index]


# ---- the outline --------------------------------------------------------------------------------------------------------------------------
def test_one_thin_box_without_a_label_by_hand():
    index, recs, n = index_of([(2, 1.9, 2.2, 5.99, 6.0, 0.9)], 8, 8, thickness=1, label_scale=0)
    assert picture(index) == ["........",
                              "........",
                              ".22222..",
                              ".2...2..",
                              ".2...2..",
                              ".2...2..",
                              ".22222..",
                              "........"]
    assert n == (1, 1) and recs[0, :10].tolist() == [1, 2, 5, 6, 0, 0, 0, 0, 2, 0]
    frame = np.full((8, 8, 3), 7, np.uint8)
    ref.paint_bgr(frame, index, COLORS)
    assert (frame[index < 0] == 7).all() and (frame[index == 2] == COLORS[2]).all() and COLORS[2].tolist() == [0, 128, 0]


@pytest.mark.parametrize("t,columns", [(1, [10]), (2, [10, 11]), (3, [9, 10, 11]), (8, [7, 8, 9, 10, 11, 12, 13, 14])])
def test_ring_columns(t, columns):
    """the left edge x1 = 10 of a wide box: o = (t - 1) / 2 columns outside it, the edge, and t - o - 1 inside"""
    index, _, _ = index_of([(1, 10, 10, 50, 50, 0.9)], 64, 64, thickness=t, label_scale=0)
    assert np.flatnonzero(index[30, :30] >= 0).tolist() == columns
    assert np.flatnonzero(index[:30, 30] >= 0).tolist() == columns          # and the top edge likewise
    assert np.flatnonzero(index[30, 30:] >= 0).tolist() == [50 - 30 - (t - (t - 1) // 2 - 1) + k for k in range(t)]


def test_a_box_smaller_than_its_ring_is_filled():
    index, _, _ = index_of([(1, 10, 10, 12, 30, 0.9)], 40, 40, thickness=3, label_scale=0)          # inner columns 12..10: empty
    assert (index[9:32, 9:14] == 1).all() and (index >= 0).sum() == 23 * 5
    index, _, _ = index_of([(1, 10, 10, 13, 30, 0.9)], 40, 40, thickness=3, label_scale=0)          # inner columns 12..11: still empty
    assert (index[9:32, 9:15] == 1).all()
    index, _, _ = index_of([(1, 10, 10, 14, 30, 0.9)], 40, 40, thickness=3, label_scale=0)          # one inner column, 12
    assert (index[12:29, 12] == -1).all() and (index[11, 12] == 1) and (index >= 0).sum() == 23 * 7 - 17
    index, _, _ = index_of([(1, 5, 5, 5, 5, 0.9)], 10, 10, thickness=1, label_scale=0)              # a 1 x 1 box
    assert (index >= 0).sum() == 1 and index[5, 5] == 1


# ---- the label ----------------------------------------------------------------------------------------------------------------------------
def label_rect(row, H, W, **kw):
    _, recs, _ = index_of([row], H, W, **kw)
    return recs[0, 4:8].tolist()


def test_label_placement():
    # "1 0.900": L = 7, z = 2: w = 2 * 43 = 86, h = 18; thickness 3: o = 1, i = 2
    assert label_rect((1, 20, 40, 60, 80, 0.9), 100, 200) == [19, 21, 86, 18]           # above: lx = x1 - o, ly = y1 - o - h
    assert label_rect((1, 20, 18, 60, 80, 0.9), 100, 200) == [19, 20, 86, 18]           # ly = -1 < 0: inside, ly = y1 + i
    assert label_rect((1, 20, 19, 60, 80, 0.9), 100, 200) == [19, 0, 86, 18]            # ly = 0 stays above
    assert label_rect((1, 150, 40, 190, 80, 0.9), 100, 200) == [114, 21, 86, 18]        # lx + w > W: shifted left to W - w
    assert label_rect((1, 114, 40, 190, 80, 0.9), 100, 200) == [113, 21, 86, 18]        # lx + w = 199 fits
    assert label_rect((1, 20, 40, 60, 80, 0.9), 100, 50) == [0, 21, 86, 18]             # wider than the frame: lx = 0, clipped at the right
    assert label_rect((1, -30, 40, 60, 80, 0.9), 100, 200) == [0, 21, 86, 18]           # lx < 0: 0
    index, _, _ = index_of([(1, 20, 40, 60, 80, 0.9)], 100, 50)
    assert (index[21:39, :] >= 0).all() and (index[20, :19] < 0).all()
    assert label_rect((1, 20, 40, 60, 80, 0.9), 100, 200, label_scale=0) == [0, 0, 0, 0]
    assert label_rect((1, 20, 40, 60, 80, 0.9), 100, 200, label_scale=1, with_score=False) == [19, 30, 7, 9]


@pytest.mark.parametrize("z", [1, 3])
@pytest.mark.parametrize("char", ["a", "4", "%"])
def test_a_glyph_is_rendered_as_its_art(z, char):
    names = overlay.name_table(["", char, "", ""], NCLS)
    index, recs, _ = index_of([(1, 10, 40, 30, 50, 0.9)], 64, 64, thickness=1, label_scale=z, with_score=False, names=names)
    lx, ly, w, h = recs[0, 4:8].tolist()
    assert (w, h) == (7 * z, 9 * z) and (lx, ly) == (10, 40 - 9 * z)
    cell = index[ly:ly + h, lx:lx + w]
    art = overlay.GLYPHS[overlay.CHARSET.index(char)]
    want = np.full((9, 7), 1)
    want[1:8, 1:6] = [[NCLS if c == "#" else 1 for c in row] for row in art]
    assert (cell == np.kron(want, np.ones((z, z), int))).all()


@pytest.mark.parametrize("score,text", [(0.0005, "0.001"), (0.1235, "0.124"), (0.9995, "1.000"), (1.0, "1.000"), (0.0004, "0.000"), (12.0, "9.999")])
def test_score_text_at_the_ties(score, text):
    """0.0005 * 1000, 0.1235 * 1000 and 0.9995 * 1000 round to the float64s 0.5, 123.5 and 999.5 exactly: the ties go up"""
    assert float(np.float64(score) * np.float64(1000.0)) in (0.5, 123.5, 999.5, 1000.0, 0.4, 12000.0)
    ch = ref.characters(3, score, 2, True, None)
    assert ch == overlay.glyph_indices("3 " + text)
    _, recs, _ = index_of([(3, 1, 1, 5, 5, score)], 20, 20, thresh=0.0)
    assert recs[0, 9] == 7 and recs[0, 10:12].tolist() == [ch[0] | ch[1] << 8 | ch[2] << 16 | ch[3] << 24, ch[4] | ch[5] << 8 | ch[6] << 16]


def test_names_are_cut_folded_and_ended():
    names = overlay.name_table(["bg", "Red_Panda-Bear!", "", "x"], NCLS)
    assert names[1].tolist() == overlay.glyph_indices("red_panda-be") and names[2].tolist() == [255] * 12
    assert ref.characters(1, 0.5, 1, False, names) == overlay.glyph_indices("red_panda-be")
    assert ref.characters(2, 0.5, 1, False, names) == [] and ref.characters(3, 0.5, 1, True, names) == overlay.glyph_indices("x 0.500")
    assert ref.characters(12, 0.5, 1, False, None) == overlay.glyph_indices("12") and ref.characters(3, 0.5, 0, True, names) == []
    names[3, 0] = 200                                                # an index outside the table reads as '?'
    assert ref.characters(3, 0.5, 1, False, names) == overlay.glyph_indices("?")
    assert overlay.glyph_indices("A z~") == [11, 0, 36, 41]
    with pytest.raises(hip.LsfaError):
        overlay.name_table(["a"], NCLS)


# ---- which rows are drawn, and in which order -----------------------------------------------------------------------------------------------
def test_eligibility_and_skipped_rows():
    rows = [(1, 2, 2, 6, 6, 0.5),                                    # a score exactly equal to thresh is drawn
            (1, 2, 2, 6, 6, 0.4999999),
            (1, np.nan, 2, 6, 6, 0.9), (1, 2, 2, np.inf, 6, 0.9), (1, 2, 2, 6, 6, np.nan), (1, 2, -np.inf, 6, 6, 0.9),
            (2, 6, 2, 5, 6, 0.9), (2, 2, 6, 6, 5, 0.9),              # inverted
            (2, -9, 2, -1, 6, 0.9), (2, 2, -9, 6, -1, 0.9), (2, 16, 2, 20, 6, 0.9), (2, 2, 12, 6, 20, 0.9),          # wholly outside 16 x 12
            (3, -9, 2, 0, 6, 0.9), (3, 15, 11, 20, 20, 0.9),         # touching the frame: drawn
            (3, 5.9, 2, 5.1, 6, 0.9)]                                # x2 < x1 as doubles, equal after trunc(): drawn
    dets, counts = dets_of(rows, R=8)
    recs, n = ref.plan(dets, counts, 0.5, 12, 16, label_scale=0)
    assert n == (4, 4) and recs[:, :4].tolist() == [[2, 2, 6, 6], [-9, 2, 0, 6], [15, 11, 20, 20], [5, 2, 5, 6]] and recs[:, 8].tolist() == [1, 3, 3, 3]
    counts[:] = [5, -3, 0, 100]                                      # class 0 is never drawn; counts below 0 and above R are clamped
    dets[0, :5] = (1, 1, 3, 3, 0.9)
    recs, n = ref.plan(dets, counts, 0.5, 12, 16, label_scale=0)
    assert n == (3, 3) and recs[:, 8].tolist() == [3, 3, 3]


def test_corners_truncate_toward_zero_and_are_clamped_not_clipped():
    dets, counts = dets_of([(1, -0.9, -1.5, 3.99, 1e300, 0.9), (1, -1e300, 0.5, 1e12, 2.0, 0.9)])
    recs, _ = ref.plan(dets, counts, 0.5, 8, 8, label_scale=0)
    assert recs[:, :4].tolist() == [[0, -1, 3, 2 ** 30], [-2 ** 30, 0, 2 ** 30, 2]]
    index = ref.cover(recs, 8, 8, NCLS, FONT, 1, 0)
    assert picture(index)[:4] == ["11111111", "1..1....", "11111111", "1..1...."]          # columns 0 and 3 of the first, rows 0 and 2 of the second


def test_the_later_record_wins():
    index, _, _ = index_of([(2, 2, 2, 9, 9, 0.9), (1, 5, 5, 12, 12, 0.9), (2, 4, 0, 6, 14, 0.8)], 16, 16, thickness=1, label_scale=0)
    assert index[5, 9] == 2 and index[9, 5] == 2          # class 2 is drawn after class 1 whatever the rows' order
    assert index[5, 5] == 1 and index[5, 4] == 2 and index[5, 6] == 2 and index[5, 7] == 1 and index[2, 5] == 2
    # inside a class the later row wins, and a label's background hides what is under it
    index, recs, _ = index_of([(1, 2, 20, 30, 30, 0.9), (1, 2, 12, 30, 40, 0.8)], 48, 48, thickness=1, label_scale=1, with_score=False)
    assert recs[1, 4:8].tolist() == [2, 3, 7, 9] and recs[0, 4:8].tolist() == [2, 11, 7, 9]
    digit = np.where(FONT[2, :7, None] >> np.arange(4, -1, -1) & 1, NCLS, 1)          # the glyph '1': row 0 is ..#..
    assert (index[4:11, 3:8] == digit).all() and (index[13:19, 3:8] == digit[1:]).all()
    assert digit[0, 2] == NCLS and index[12, 5] == 1                # the first label's top text row lies under the second box's top edge


def test_max_boxes_keeps_the_first_rows_and_reports_both_counts():
    rows = [(1, k, k, k + 3, k + 3, 0.9) for k in range(4)] + [(2, 1, 1, 2, 2, 0.1)] + [(3, k, 1, k + 1, 2, 0.9) for k in range(3)]
    dets, counts = dets_of(rows)
    recs, n = ref.plan(dets, counts, 0.5, 16, 16, max_boxes=5)
    assert n == (5, 7) and recs[:, 8].tolist() == [1, 1, 1, 1, 3] and recs[4, :4].tolist() == [0, 1, 1, 2]
    assert ref.plan(dets, counts, 0.5, 16, 16, max_boxes=7)[1] == (7, 7) and ref.plan(dets, counts, 0.95, 16, 16)[1] == (0, 0)
    assert ref.plan(dets, counts, 0.95, 16, 16)[0].shape == (0, ref.REC_INTS)


# ---- the font, the palette, the colour rows -----------------------------------------------------------------------------------------------
def test_the_font_table():
    assert len(overlay.GLYPHS) == len(overlay.CHARSET) == ref.GLYPHS == 42 and FONT.shape == (42, 8) and FONT.nbytes == overlay.GLYPH_BYTES
    assert overlay.CHARSET == " 0123456789abcdefghijklmnopqrstuvwxyz_-.%?"
    assert all(len(g) == 7 and all(len(row) == 5 for row in g) for g in overlay.GLYPHS)
    assert (FONT < 32).all() and (FONT[:, 7] == 0).all()
    assert len(set(bytes(g) for g in FONT)) == 42
    assert [k for k in range(42) if not FONT[k].any()] == [0]
    assert FONT[overlay.CHARSET.index("-")].tolist() == [0, 0, 0, 31, 0, 0, 0, 0] and FONT[overlay.CHARSET.index("1"), 0] == 0b00100
    assert (ref.SPACE, ref.ZERO, ref.DOT, ref.UNKNOWN) == tuple(overlay.CHARSET.index(c) for c in " 0.?")
    assert (overlay.REC_INTS, overlay.NAME_LEN) == (ref.REC_INTS, ref.NAME_LEN)


def test_the_constants_are_the_header_s():
    import re
    text = open(hip._HEADER).read()
    got = {k: int(v) for k, v in re.findall(r"^#define LSFA_OVERLAY_(\w+) (\d+)$", text, flags=re.M)}
    assert got == {"REC_INTS": overlay.REC_INTS, "NAME_LEN": overlay.NAME_LEN, "GLYPHS": 42, "GLYPH_BYTES": overlay.GLYPH_BYTES, "MAX_BOXES": overlay.MAX_BOXES, "MAX_CLASSES": overlay.MAX_CLASSES}


def test_the_palette():
    p = overlay.palette(9)
    assert p.shape == (10, 3) and p.dtype == np.uint8
    assert p[:, ::-1].tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128], [128, 0, 128], [0, 128, 128], [128, 128, 128],
                                   [64, 0, 0], [255, 255, 255]]
    assert len(set(map(tuple, overlay.palette(31)[1:31].tolist()))) == 30


def test_bgr_to_yuv_known_answers():
    bw = np.array([[0, 0, 0], [255, 255, 255]], np.uint8)
    assert overlay.bgr_to_yuv(bw, "bt601").tolist() == [[16, 128, 128], [235, 128, 128]]
    assert overlay.bgr_to_yuv(bw, "bt709").tolist() == [[16, 128, 128], [235, 128, 128]]
    assert overlay.bgr_to_yuv(bw, "jpeg").tolist() == [[0, 128, 128], [255, 128, 128]]
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    for m in ("bt601", "bt709", "jpeg"):
        yuv = overlay.bgr_to_yuv(grey, m)
        assert (yuv[:, 1:] == 128).all() and (np.diff(yuv[:, 0].astype(int)) >= 0).all()
    assert (overlay.bgr_to_yuv(grey, "jpeg")[:, 0] == np.arange(256)).all()
    assert overlay.bgr_to_yuv(np.array([255, 0, 0], np.uint8), "bt601").tolist() == [41, 240, 110]           # blue
    assert overlay.bgr_to_yuv(np.array([0, 0, 255], np.uint8), "jpeg").tolist() == [77, 85, 255]             # red: V = 255.5 clipped
    with pytest.raises(hip.LsfaError):
        overlay.bgr_to_yuv(bw, "bt2020")


def test_yuv_painting_follows_the_intake_s_chroma_rule():
    """the chroma sample (cx, cy) belongs to pixel (2cx, 2cy): a box on odd coordinates colours the luma of its pixels and the chroma of
    the even pixels among them only"""
    index, _, _ = index_of([(1, 1, 1, 3, 3, 0.9)], 5, 7, thickness=1, label_scale=0)
    yuv = overlay.bgr_to_yuv(COLORS, "bt601")
    y, uv = np.full((5, 7), 9, np.uint8), np.full((3, 8), 9, np.uint8)
    u, v = np.full((3, 4), 9, np.uint8), np.full((3, 4), 9, np.uint8)
    ref.paint_yuv420(y, index, yuv, uv=uv)
    ref.paint_yuv420(y.copy(), index, yuv, u=u, v=v)
    assert (y[1:4, 1:4] == [[yuv[1, 0]] * 3, [yuv[1, 0], 9, yuv[1, 0]], [yuv[1, 0]] * 3]).all() and (y == 9).sum() == 35 - 8
    # the ring's pixels have an odd coordinate each but for (2, 2), and that is its hole
    assert index[2, 2] == -1 and (u == 9).all() and (uv == 9).all()          # no covered pixel has two even coordinates
    index, _, _ = index_of([(1, 1, 1, 4, 4, 0.9)], 5, 7, thickness=1, label_scale=0)
    ref.paint_yuv420(y, index, yuv, uv=uv)
    ref.paint_yuv420(y.copy(), index, yuv, u=u, v=v)
    hit = np.zeros((3, 4), bool)
    hit[2, 1] = hit[2, 2] = hit[1, 2] = True                        # pixels (2, 4), (4, 4), (4, 2)
    assert ((u != 9) == hit).all() and (u[hit] == yuv[1, 1]).all() and (v[hit] == yuv[1, 2]).all()
    assert (uv[:, 0::2] == u).all() and (uv[:, 1::2] == v).all()


# ---- Overlay under the spy ------------------------------------------------------------------------------------------------------------------
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
    assert "Overlay" in str(e.value)
    assert not spy.calls, "%s launched %s before refusing" % (fn.__name__, spy.launched())


def test_well_formed_calls_reach_exactly_their_exports(spied):
    ov = overlay.Overlay(NCLS, R, max_boxes=7, thickness=2, label_scale=1, names=["bg", "a", "b", "c"], device=bc.CUDA0, batch=3)
    assert not spied.calls and tuple(ov.records.shape) == (3, 7, 16) and tuple(ov.n.shape) == (3, 2)
    dets, counts = dz()
    frame = z(H, W + 2, 3)[:, :W]
    assert ov.draw_bgr(frame, dets, counts, 0.25) is frame
    assert spied.launched() == ["lsfa_overlay_plan", "lsfa_overlay_paint_bgr"]
    got = spied.values("lsfa_overlay_plan")
    assert (got["N"], got["ncls"], got["R"], got["thresh"], got["H"], got["W"], got["thickness"], got["label_scale"], got["with_score"], got["max_boxes"]) == \
        (1, NCLS, R, 0.25, H, W, 2, 1, 1, 7)
    assert got["names"] is not None and got["records"] == ov.records.data_ptr() and got["n"] == ov.n.data_ptr() and got["dets"] == dets.data_ptr()
    got = spied.values("lsfa_overlay_paint_bgr")
    assert (got["pitch"], got["frame_stride"], got["N"], got["H"], got["W"], got["max_boxes"], got["thickness"], got["label_scale"], got["ncls"]) == \
        (3 * (W + 2), 0, 1, H, W, 7, 2, 1, NCLS)
    assert got["colors"] == ov._bgr.data_ptr() and got["font"] == ov._font.data_ptr() and got["bgr"] == frame.data_ptr()
    del spied.calls[:]
    dets3, counts3 = dz(3)
    ov.draw_bgr(z(3, H + 1, W, 3)[:, :H], dets3, counts3, 0.5)
    got = spied.values("lsfa_overlay_paint_bgr")
    assert (got["pitch"], got["frame_stride"], got["N"]) == (3 * W, 3 * W * (H + 1), 3) and spied.values("lsfa_overlay_plan")["N"] == 3
    del spied.calls[:]
    y = z(H, W + 6)[:, :W]
    assert ov.draw_yuv420(y, dets, counts, 0.5, uv=z(3, 10), matrix="bt709") is y
    assert spied.launched() == ["lsfa_overlay_plan", "lsfa_overlay_paint_yuv420"]
    got = spied.values("lsfa_overlay_paint_yuv420")
    assert (got["y_pitch"], got["c_pitch"], got["y_frame_stride"], got["N"], got["H"], got["W"], got["v"]) == (W + 6, 10, 0, 1, H, W, None)
    assert got["colors"] == ov._yuv["bt709"].data_ptr() and got["ncls"] == NCLS
    del spied.calls[:]
    ov.draw_yuv420(z(2, H, W), dets3[:2].contiguous(), counts3[:2].contiguous(), 0.5, u=z(2, 3, 5), v=z(2, 3, 5))
    got = spied.values("lsfa_overlay_paint_yuv420")
    assert (got["N"], got["y_frame_stride"], got["c_frame_stride"], got["c_pitch"]) == (2, H * W, 15, 5) and got["v"] is not None
    assert got["colors"] == ov._yuv["bt601"].data_ptr()
    assert overlay.Overlay(NCLS, R, device=bc.CUDA0)._names is None
    assert bc.plain(ov._yuv["jpeg"]).numpy().tolist() == overlay.bgr_to_yuv(overlay.palette(NCLS), "jpeg").tolist()
    assert ov.drawn().shape == (3, 2)


def test_the_constructor_refuses_what_the_library_would(spied):
    for kw in (dict(ncls=0), dict(ncls=overlay.MAX_CLASSES + 1), dict(R=0), dict(max_boxes=0), dict(max_boxes=overlay.MAX_BOXES + 1), dict(thickness=0), dict(thickness=9), dict(label_scale=-1),
               dict(label_scale=5), dict(batch=0), dict(thickness=3.0), dict(names=["a"]), dict(colors=np.zeros((NCLS, 3), np.uint8)),
               dict(colors=np.zeros((NCLS + 1, 3), np.int32))):
        with pytest.raises(hip.LsfaError):
            overlay.Overlay(**dict(dict(ncls=NCLS, R=R, device=bc.CUDA0), **kw))
    assert not spied.calls


def test_bad_tensors_are_refused_before_anything_is_launched(spied):
    ov = overlay.Overlay(NCLS, R, device=bc.CUDA0, batch=2)
    dets, counts = dz()
    frame = z(H, W, 3)
    f32 = lambda *s: z(*s, dtype=torch.float32)          # noqa: E731
    fn = ov.draw_bgr
    refused(spied, fn, bc.plain(frame).clone(), dets, counts, 0.5)                  # on the host, in every position
    refused(spied, fn, frame, bc.plain(dets).clone(), counts, 0.5)
    refused(spied, fn, frame, dets, bc.plain(counts).clone(), 0.5)
    refused(spied, fn, f32(H, W, 3), dets, counts, 0.5)                             # dtypes
    refused(spied, fn, frame, f32(NCLS, R, 5), counts, 0.5)
    refused(spied, fn, frame, dets, z(NCLS, dtype=torch.int64), 0.5)
    refused(spied, fn, z(H, W), dets, counts, 0.5)                                  # ranks
    refused(spied, fn, z(1, 1, H, W, 3), dets, counts, 0.5)
    refused(spied, fn, frame, dets[0], counts, 0.5)
    refused(spied, fn, frame, dets, counts[None], 0.5)
    refused(spied, fn, z(H, W, 4), dets, counts, 0.5)                               # shapes
    refused(spied, fn, frame, z(NCLS, R + 1, 5, dtype=torch.float64), counts, 0.5)
    refused(spied, fn, frame, z(NCLS, R, 4, dtype=torch.float64), counts, 0.5)
    refused(spied, fn, frame, dets, z(NCLS + 1, dtype=torch.int32), 0.5)
    refused(spied, fn, z(H, W, 6)[:, :, ::2], dets, counts, 0.5)                    # a last dimension that is not dense
    refused(spied, fn, z(H, W, 4)[:, :, :3], dets, counts, 0.5)                     # pixels that are not packed
    refused(spied, fn, frame, z(NCLS, R, 6, dtype=torch.float64)[:, :, :5], counts, 0.5)
    refused(spied, fn, frame, dets, z(2 * NCLS, dtype=torch.int32)[::2], 0.5)
    refused(spied, fn, torch.as_strided(z(H * W * 3), (H, W, 3), (3 * W - 3, 3, 1)), dets, counts, 0.5)        # a pitch below its row
    refused(spied, fn, z(0, W, 3), dets, counts, 0.5)
    refused(spied, fn, frame, *dz(1), 0.5)                                          # a batch of detections for one frame, and the reverse
    refused(spied, fn, z(2, H, W, 3), dets, counts, 0.5)
    refused(spied, fn, z(2, H, W, 3), *dz(3), 0.5)
    refused(spied, fn, z(3, H, W, 3), *dz(3), 0.5)                                  # more frames than the Overlay was made for
    refused(spied, fn, None, dets, counts, 0.5)
    refused(spied, fn, frame, None, counts, 0.5)
    refused(spied, fn, frame, dets, None, 0.5)
    fn = ov.draw_yuv420
    y, uv, u, v = z(H, W), z(3, 10), z(3, 5), z(3, 5)
    refused(spied, fn, bc.plain(y).clone(), dets, counts, 0.5, uv=uv)
    refused(spied, fn, y, dets, counts, 0.5, uv=bc.plain(uv).clone())
    refused(spied, fn, y, dets, counts, 0.5, u=u, v=bc.plain(v).clone())
    refused(spied, fn, y, bc.plain(dets).clone(), counts, 0.5, uv=uv)
    refused(spied, fn, y, dets, bc.plain(counts).clone(), 0.5, uv=uv)
    refused(spied, fn, f32(H, W), dets, counts, 0.5, uv=uv)
    refused(spied, fn, y, dets, counts, 0.5, uv=z(3, 10, dtype=torch.int16))
    refused(spied, fn, y, f32(NCLS, R, 5), counts, 0.5, uv=uv)
    refused(spied, fn, y, dets, counts, 0.5)                                        # no chroma; both kinds; half of I420
    refused(spied, fn, y, dets, counts, 0.5, uv=uv, u=u, v=v)
    refused(spied, fn, y, dets, counts, 0.5, u=u)
    refused(spied, fn, y, dets, counts, 0.5, uv=z(3, 8))                            # shapes
    refused(spied, fn, y, dets, counts, 0.5, uv=z(2, 10))
    refused(spied, fn, y, dets, counts, 0.5, u=u, v=z(3, 4))
    refused(spied, fn, y, dets, counts, 0.5, uv=z(1, 3, 10))                        # ranks
    refused(spied, fn, z(2, H, W), dets, counts, 0.5, uv=z(2, 3, 10))
    refused(spied, fn, z(H, 2 * W)[:, ::2], dets, counts, 0.5, uv=uv)               # not dense
    refused(spied, fn, y, dets, counts, 0.5, uv=z(3, 20)[:, ::2])
    refused(spied, fn, y, dets, counts, 0.5, u=u, v=z(3, 8)[:, :5])                 # u and v of different pitch
    refused(spied, fn, y, z(NCLS, R, 6, dtype=torch.float64)[:, :, :5], counts, 0.5, uv=uv)
    refused(spied, fn, torch.as_strided(z(H * W), (H, W), (W - 2, 1)), dets, counts, 0.5, uv=uv)
    refused(spied, fn, y, dets, counts, 0.5, uv=uv, matrix="bt2020")
    del spied.calls[:]
    ov.draw_yuv420(y, dets, counts, 0.5, u=u, v=v)
    assert spied.launched() == ["lsfa_overlay_plan", "lsfa_overlay_paint_yuv420"]


# ---- the demo's arguments -------------------------------------------------------------------------------------------------------------------
def test_the_demo_refuses_wrong_combinations(tmp_path, capsys):
    nv12 = tmp_path / "clip.nv12"
    nv12.write_bytes(bytes(8 * 4 * 3 // 2))
    names = tmp_path / "classes.txt"
    names.write_text("cat\ndog\n")
    yuv = ["--yuv", str(nv12), "--size", "8x4"]
    bad = [["--draw-yuv", "out.yuv"],                                               # no --yuv
           ["--frames", "dir", "--draw-yuv", "out.yuv"],
           yuv + ["--yuv-format", "nv21", "--draw-yuv", "out.yuv"],                 # a layout the overlay does not draw into
           yuv + ["--draw-yuv", str(nv12)],                                         # onto its input
           ["--classes", str(names)], ["--draw-thickness", "2"], ["--draw-scale", "1"],          # without --draw / --draw-yuv
           ["--draw", "d", "--draw-thickness", "0"], ["--draw", "d", "--draw-thickness", "9"],
           ["--draw", "d", "--draw-scale", "-1"], ["--draw", "d", "--draw-scale", "5"],
           ["--draw", "d", "--classes", str(tmp_path / "missing.txt")]]
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            demo.parse_args(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
    a = demo.parse_args(yuv + ["--draw", "d", "--draw-yuv", "o.yuv", "--classes", str(names), "--draw-scale", "0"])
    assert (a.draw, a.draw_yuv, a.draw_thickness, a.draw_scale) == ("d", "o.yuv", 3, 0)
    a = demo.parse_args(yuv + ["--yuv-format", "i420", "--draw-yuv", "o.yuv"])
    assert (a.draw_thickness, a.draw_scale, a.draw) == (3, 2, None)
    assert demo.class_names(str(names), 3) == ["background", "cat", "dog"] and demo.class_names(str(names), 2) == ["cat", "dog"]
    with pytest.raises(ValueError):
        demo.class_names(str(names), 5)
    assert "left to the caller" not in demo.__doc__ and "--draw DIR" in demo.__doc__
