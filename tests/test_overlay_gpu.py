"""lsfa_overlay_plan, lsfa_overlay_paint_bgr and lsfa_overlay_paint_yuv420 (lsfa_amd/csrc/overlay.hip) on the GPU against tests/ref_overlay.py,
bit for bit (`==` everywhere): the pixels, the records and n; graph capture; memory ownership; every refusal of the C ABI; the demo's --draw and
--draw-yuv.  tests/test_overlay_cpu.py pins the reference.

Every surface is an allocation that ends with its last sample, its pitch bytes hold 0xA5, and the WHOLE allocation is compared with a numpy
model of it that the reference drew into: a byte the kernel stores outside a covered sample shows wherever it lands.

The sizes are the point of the cases: (1, 1), (2, 2) and (3, 5) are a corner of one tile, (16, 64) is exactly one tile of 64 x 16 pixels,
(17, 65) one pixel beyond it each way, (37, 131) three tiles each way with ragged edges.  A base one byte in and pitches of the row + 1 take
the byte stores; + 0, + 4 and + 16 the dword stores wherever a lane's four pixels are covered."""
import json

import numpy as np
import pytest
import torch

import guarded_arena
import ref_overlay as ref
import ref_yuv

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MATRICES = ("bt601", "bt709", "jpeg")
SIZES = [(1, 1), (2, 2), (3, 5), (16, 64), (17, 65), (37, 131)]
NCLS, R = 5, 12


@pytest.fixture(scope="module")
def overlay(hip):
    from lsfa_amd import overlay as module
    return module


class Surface(object):
    """(n, rows, cols) bytes with rows `pitch` bytes apart, frames `gap` bytes further apart than a frame and the base `offset` bytes into an
    allocation that ends with the last sample, every other byte 0xA5: .host the numpy model (.frames its (n, rows, cols) view) and .view the
    device tensor ((rows, cols) if not batched).  cols = 3 W with pixel=3 gives .view (.., H, W, 3)."""

    def __init__(self, a, extra=0, gap=0, offset=0, batched=True, pixel=1):
        n, rows, cols = a.shape
        pitch = cols + extra
        fs = rows * pitch + gap
        used = (n - 1) * fs + (rows - 1) * pitch + cols
        self.host = np.full(offset + used, 0xA5, np.uint8)
        self.frames = np.lib.stride_tricks.as_strided(self.host[offset:], (n, rows, cols), (fs, pitch, 1))
        self.frames[...] = a
        self.buf = torch.from_numpy(self.host.copy()).to(DEV)
        if pixel == 1:
            view = torch.as_strided(self.buf[offset:], (n, rows, cols), (fs, pitch, 1))
        else:
            view = torch.as_strided(self.buf[offset:], (n, rows, cols // pixel, pixel), (fs, pitch, pixel, 1))
        self.view = view if batched else view[0]

    def check(self, what=""):
        got = self.buf.cpu().numpy()
        bad = np.flatnonzero(got != self.host)
        assert bad.size == 0, "%s: %d bytes differ, the first at %d of %d: %d, expected %d" % (what, bad.size, bad[0], got.size, got[bad[0]], self.host[bad[0]])


def boxes(rs, H, W, ncls=NCLS, rows=R, junk=True):
    """dets (ncls, rows, 5) and counts: boxes inside the frame, across every edge, with negative corners and corners far beyond the frame,
    on fractional coordinates; with `junk` also rows that must not be drawn (NaN, inf, inverted, wholly outside, below the threshold)"""
    dets = np.zeros((ncls, rows, 5))
    counts = rs.randint(rows // 2, rows + 1, ncls).astype(np.int32)
    for j in range(ncls):
        for r in range(rows):
            kind = rs.randint(0, 12)
            x1, y1 = rs.uniform(-0.3 * W - 3, W), rs.uniform(-0.3 * H - 3, H)
            x2, y2 = x1 + rs.uniform(0, 0.8 * W + 3), y1 + rs.uniform(0, 0.8 * H + 3)
            s = rs.uniform(0.5, 1.0)
            if kind == 0:
                x1, x2 = -1e7, 3e9                     # far beyond, clamped to +-2^30
            elif kind == 1:
                y1, y2 = -5e9, H + 0.5
            elif kind == 2:
                x2, y2 = x1, y1                        # one pixel
            if junk and kind == 3:
                s = rs.uniform(0.0, 0.499)
            elif junk and kind == 4:
                v = [x1, y1, x2, y2, s]
                v[rs.randint(0, 5)] = (np.nan, np.inf, -np.inf)[rs.randint(0, 3)]
                x1, y1, x2, y2, s = v
            elif junk and kind == 5:
                x1, x2 = x2 + 1.5, x1
            elif junk and kind == 6:
                x1, x2 = W + rs.uniform(0, 9), W + 20.0
            elif junk and kind == 7:
                y1, y2 = -20.0, -rs.uniform(1.0, 9)
            dets[j, r] = (x1, y1, x2, y2, s)
    dets[0] = (0, 0, W, H, 0.99)                       # class 0 is never drawn
    counts[0] = rows
    return dets, counts


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def expect_bgr(overlay, surf, H, W, dets, counts, thresh, colors=None, **kw):
    """draws the reference into surf's model; dets (N, ncls, R, 5) -> [(records, n)] per frame"""
    font = overlay.font_table()
    out = []
    for b in range(dets.shape[0]):
        colors_b = overlay.palette(dets.shape[1]) if colors is None else colors
        frame = surf.frames[b].reshape(H, W, 3)
        assert np.shares_memory(frame, surf.host)
        _, recs, n = ref.draw_bgr(frame, dets[b], counts[b], thresh, font, colors_b, **kw)
        out.append((recs, n))
    return out


def check_records(ov, want):
    got_n, got = ov.drawn(), ov.records.cpu().numpy()
    for b, (recs, n) in enumerate(want):
        assert tuple(got_n[b]) == n, (b, got_n[b], n)
        np.testing.assert_array_equal(got[b, :n[0]], recs, err_msg="records of image %d" % b)


def plan_kw(ov):
    return dict(thickness=ov.thickness, label_scale=ov.label_scale, with_score=ov.with_score, max_boxes=ov.max_boxes)


# ---- 1: packed BGR --------------------------------------------------------------------------------------------------------------------------
STYLES = [(3, 2), (1, 0), (2, 1), (8, 4), (4, 3)]          # (thickness, label scale)


@pytest.mark.parametrize("H,W", SIZES)
def test_bgr_equals_the_reference_at_every_layout(overlay, H, W):
    rs = np.random.RandomState(100 * H + W)
    for k, (extra, offset) in enumerate([(0, 0), (1, 0), (4, 0), (16, 0), (0, 1)]):
        t_, z_ = STYLES[k % len(STYLES)]
        ov = overlay.Overlay(NCLS, R, max_boxes=64, thickness=t_, label_scale=z_, with_score=k != 2, device=DEV)
        dets, counts = boxes(rs, H, W)
        surf = Surface(rs.randint(0, 256, (1, H, 3 * W)).astype(np.uint8), extra, 0, offset, batched=False, pixel=3)
        want = expect_bgr(overlay, surf, H, W, dets[None], counts[None], 0.5, **plan_kw(ov))
        assert ov.draw_bgr(surf.view, t(dets), t(counts), 0.5) is surf.view
        surf.check("bgr %dx%d pitch +%d offset %d" % (W, H, extra, offset))
        check_records(ov, want)
        assert H * W < 64 or want[0][1][0] > 0


def test_bgr_batch_of_three_pitched_frames_with_different_counts(overlay):
    H, W = 37, 131
    rs = np.random.RandomState(5)
    for gap, extra in ((2, 0), (32, 4)):
        ov = overlay.Overlay(NCLS, R, max_boxes=64, device=DEV, batch=3, names=["bg", "Car", "person", "a_very_long_class_name", "x%"])
        dets, counts = zip(*[boxes(rs, H, W) for _ in range(3)])
        dets, counts = np.stack(dets), np.stack(counts)
        counts[1] = 0                                                  # an image without detections between two with
        counts[2, 1:] = [1, R + 9, -4, 3]                              # above R and below 0
        surf = Surface(rs.randint(0, 256, (3, H, 3 * W)).astype(np.uint8), extra, gap, pixel=3)
        names = overlay.name_table(["bg", "Car", "person", "a_very_long_class_name", "x%"], NCLS)
        want = expect_bgr(overlay, surf, H, W, dets, counts, 0.5, names=names, **plan_kw(ov))
        ov.draw_bgr(surf.view, t(dets), t(counts), 0.5)
        surf.check("gap %d" % gap)
        check_records(ov, want)
        assert want[1][1] == (0, 0) and want[0][1][0] > 3 and want[2][1][0] > 0


# ---- 2: NV12 and I420 -----------------------------------------------------------------------------------------------------------------------
def yuv_case(overlay, rs, H, W, n, nv12, extra, gap, offset, matrix, ov, dets, counts, thresh=0.5, names=None):
    ch, cw = -(-H // 2), -(-W // 2)
    batched = n is not None
    n = n or 1
    ys = Surface(rs.randint(0, 256, (n, H, W)).astype(np.uint8), extra, gap, offset, batched)
    if nv12:
        cs = [Surface(rs.randint(0, 256, (n, ch, 2 * cw)).astype(np.uint8), extra, gap, offset, batched)]
    else:                       # u and v share one pitch and one frame stride
        cs = [Surface(rs.randint(0, 256, (n, ch, cw)).astype(np.uint8), extra, gap, offset, batched) for _ in range(2)]
    colors = overlay.bgr_to_yuv(overlay.palette(dets.shape[1]), matrix)
    want = []
    for b in range(n):
        planes = dict(uv=cs[0].frames[b]) if nv12 else dict(u=cs[0].frames[b], v=cs[1].frames[b])
        _, recs, cnt = ref.draw_yuv420(ys.frames[b], dets[b], counts[b], thresh, overlay.font_table(), colors, names=names, **plan_kw(ov), **planes)
        want.append((recs, cnt))
    d, c = (t(dets), t(counts)) if batched else (t(dets[0]), t(counts[0]))
    planes = dict(uv=cs[0].view) if nv12 else dict(u=cs[0].view, v=cs[1].view)
    assert ov.draw_yuv420(ys.view, d, c, thresh, matrix=matrix, **planes) is ys.view
    what = "%s %dx%d pitch +%d gap %d offset %d %s" % ("nv12" if nv12 else "i420", W, H, extra, gap, offset, matrix)
    ys.check(what + " Y")
    for s in cs:
        s.check(what + " chroma")
    check_records(ov, want)
    return want


@pytest.mark.parametrize("nv12", [True, False], ids=["nv12", "i420"])
@pytest.mark.parametrize("H,W", SIZES)
def test_yuv420_equals_the_reference_at_every_layout(overlay, H, W, nv12):
    rs = np.random.RandomState(100 * H + W + 7)
    for k, (extra, offset) in enumerate([(0, 0), (1, 0), (4, 0), (16, 0), (0, 1)]):
        t_, z_ = STYLES[(k + 1) % len(STYLES)]
        ov = overlay.Overlay(NCLS, R, max_boxes=64, thickness=t_, label_scale=z_, device=DEV)
        dets, counts = boxes(rs, H, W)
        want = yuv_case(overlay, rs, H, W, None, nv12, extra, 0, offset, MATRICES[k % 3], ov, dets[None], counts[None])
        assert H * W < 64 or want[0][1][0] > 0


@pytest.mark.parametrize("nv12", [True, False], ids=["nv12", "i420"])
def test_yuv420_batch_of_three_pitched_frames(overlay, nv12):
    rs = np.random.RandomState(11)
    for (H, W), gap, extra in (((37, 131), 2, 0), ((18, 66), 32, 16)):
        ov = overlay.Overlay(NCLS, R, max_boxes=64, device=DEV, batch=3)
        dets, counts = zip(*[boxes(rs, H, W) for _ in range(3)])
        dets, counts = np.stack(dets), np.stack(counts)
        counts[0, 2:] = 0
        want = yuv_case(overlay, rs, H, W, 3, nv12, extra, gap, 0, "bt709", ov, dets, counts)
        assert want[0][1] != want[1][1]


@pytest.mark.parametrize("nv12", [True, False], ids=["nv12", "i420"])
def test_chroma_takes_the_even_pixels_of_boxes_on_odd_coordinates(overlay, nv12):
    """thin boxes whose edges fall on odd rows and columns colour luma only; on even ones luma and chroma"""
    H, W = 21, 35
    rs = np.random.RandomState(3)
    dets, counts = np.zeros((3, 4, 5)), np.array([0, 3, 2], np.int32)
    dets[1, :3] = [(1, 1, 9, 9, 0.9), (11, 3, 33, 19, 0.9), (13.9, 5.9, 31.2, 17.5, 0.9)]
    dets[2, :2] = [(2, 2, 8, 8, 0.9), (12, 4, 32, 18, 0.9)]
    ov = overlay.Overlay(3, 4, max_boxes=8, thickness=1, label_scale=0, device=DEV)
    yuv_case(overlay, rs, H, W, None, nv12, 3, 0, 0, "bt601", ov, dets[None], counts[None])
    ov = overlay.Overlay(3, 4, max_boxes=8, thickness=2, label_scale=1, device=DEV)
    yuv_case(overlay, rs, H, W, None, nv12, 0, 0, 0, "jpeg", ov, dets[None], counts[None])


# ---- 3: the records -------------------------------------------------------------------------------------------------------------------------
def bgr_case(overlay, H, W, dets, counts, thresh=0.5, seed=0, **kw):
    ov = overlay.Overlay(dets.shape[0], dets.shape[1], device=DEV, **kw)
    surf = Surface(np.random.RandomState(seed).randint(0, 256, (1, H, 3 * W)).astype(np.uint8), 0, 0, 0, batched=False, pixel=3)
    before = surf.host.copy()
    want = expect_bgr(overlay, surf, H, W, dets[None], counts[None], thresh, **plan_kw(ov))
    ov.draw_bgr(surf.view, t(dets), t(counts), thresh)
    surf.check()
    check_records(ov, want)
    return want[0], int((before != surf.host).sum())


def test_no_records_leave_every_byte(overlay):
    dets, counts = boxes(np.random.RandomState(1), 37, 131)
    (recs, n), changed = bgr_case(overlay, 37, 131, dets, counts, thresh=1.5)
    assert n == (0, 0) and changed == 0
    (recs, n), changed = bgr_case(overlay, 37, 131, dets, np.zeros(NCLS, np.int32))
    assert n == (0, 0) and changed == 0


def test_single_boxes(overlay):
    one = lambda *row: (np.array([[[0] * 5], [list(row)]], np.float64), np.array([0, 1], np.int32))          # noqa: E731
    (recs, n), changed = bgr_case(overlay, 17, 65, *one(40, 9, 40, 9, 0.9), thickness=1, label_scale=0)
    assert n == (1, 1) and changed <= 3                              # a 1 x 1 box: one pixel
    (recs, n), changed = bgr_case(overlay, 17, 65, *one(0, 0, 64, 16, 0.9), thickness=1, label_scale=0)
    assert n == (1, 1) and recs[0, :4].tolist() == [0, 0, 64, 16]    # the whole frame: its border
    (recs, n), changed = bgr_case(overlay, 17, 65, *one(0, 0, 64, 16, 0.9), thickness=8, label_scale=4)
    assert n == (1, 1)
    (recs, n), changed = bgr_case(overlay, 17, 65, *one(0.5, 0.5, 3.5, 3.5, 0.9), thickness=8, label_scale=1)          # smaller than its ring: filled
    assert n == (1, 1)
    for row in ((-30, -30, 10, 5, 0.9), (60, 10, 5000, 400, 0.9), (-1e9, 8, 1e9, 8.5, 0.9), (32, -1e12, 33, 1e12, 0.9), (-2e9, -2e9, 2e9, 2e9, 0.9)):
        (recs, n), changed = bgr_case(overlay, 17, 65, *one(*row), thickness=3, label_scale=2)          # across each edge, far beyond the frame
        assert n == (1, 1), row
    (recs, n), changed = bgr_case(overlay, 17, 65, *one(10, 5, 20, 12, 0.5), thresh=0.5)                # a score equal to the threshold is drawn
    assert n == (1, 1) and changed > 0
    for row in ((10, 5, 20, 12, np.nextafter(0.5, 0)), (np.nan, 5, 20, 12, 0.9), (10, 5, np.inf, 12, 0.9), (10, 5, 20, 12, np.nan), (20, 5, 10, 12, 0.9),
                (10, 12, 20, 5, 0.9), (65, 5, 70, 12, 0.9), (10, 17, 20, 30, 0.9), (-9, 5, -1, 12, 0.9), (10, -9, 20, -0.5 - 1, 0.9)):
        (recs, n), changed = bgr_case(overlay, 17, 65, *one(*row), thresh=0.5)
        assert n == (0, 0) and changed == 0, row


@pytest.mark.parametrize("count", [130, 300])
def test_many_boxes_across_one_tile_keep_their_order(overlay, count):
    """every box reaches into the tile at (64, 16) and nearly every outline crosses it: the sift keeps those, over more than one round of its
    prefix at 300 records, and each pixel must still take the LAST of them"""
    H, W = 48, 200
    rs = np.random.RandomState(count)
    ncls, rows = 4, 100
    dets, counts = np.zeros((ncls, rows, 5)), np.array([0, 100, 100, 100], np.int32)
    x1, y1 = rs.uniform(40, 100, (ncls, rows)), rs.uniform(2, 28, (ncls, rows))
    dets[..., 0], dets[..., 1] = x1, y1
    dets[..., 2], dets[..., 3] = np.maximum(x1 + rs.uniform(0, 60, x1.shape), 64.5), np.maximum(y1 + rs.uniform(0, 20, x1.shape), 16.5)
    dets[..., 4] = 0.9
    flat = dets[1:].reshape(-1, 5)
    flat[count:, 4] = 0.1
    (recs, n), changed = bgr_case(overlay, H, W, dets, counts, max_boxes=512, thickness=2, label_scale=1)
    assert n == (count, count) and changed > 0


def test_more_eligible_rows_than_max_boxes_and_a_plan_of_several_rounds(overlay):
    H, W = 37, 131
    dets, counts = boxes(np.random.RandomState(8), H, W, ncls=4, rows=160, junk=True)          # 480 (class, row) pairs: two rounds of the plan's prefix
    (recs, n), _ = bgr_case(overlay, H, W, dets, counts, max_boxes=50)
    assert n[0] == 50 and n[1] > 2 * 50
    (recs, n), _ = bgr_case(overlay, H, W, dets, counts, max_boxes=1)
    assert n[0] == 1
    (recs2, n2), _ = bgr_case(overlay, H, W, dets, counts, max_boxes=512, label_scale=0)
    assert n2[0] == n2[1] == n[1]


# ---- 4: graph capture -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bgr", "nv12"])
def test_plan_and_paint_captured_once_and_replayed_on_new_detections_and_frames(overlay, kind):
    H, W = 37, 131
    ch, cw = -(-H // 2), -(-W // 2)
    rs = np.random.RandomState(21)
    ov = overlay.Overlay(NCLS, R, max_boxes=64, device=DEV)
    font, colors = overlay.font_table(), overlay.palette(NCLS)
    dets, counts = torch.zeros((NCLS, R, 5), dtype=torch.float64, device=DEV), torch.zeros(NCLS, dtype=torch.int32, device=DEV)
    frame = torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV)
    y, uv = torch.zeros((H, W), dtype=torch.uint8, device=DEV), torch.zeros((ch, 2 * cw), dtype=torch.uint8, device=DEV)

    def draw():
        if kind == "bgr":
            ov.draw_bgr(frame, dets, counts, 0.5)
        else:
            ov.draw_yuv420(y, dets, counts, 0.5, uv=uv, matrix="bt709")

    draw()                      # loads the code objects outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        draw()
    for k in range(2):
        d, c = boxes(rs, H, W)
        f, yy, cc = rs.randint(0, 256, (H, W, 3)).astype(np.uint8), rs.randint(0, 256, (H, W)).astype(np.uint8), rs.randint(0, 256, (ch, 2 * cw)).astype(np.uint8)
        for dst, src in ((dets, d), (counts, c), (frame, f), (y, yy), (uv, cc)):
            dst.copy_(t(src))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        if kind == "bgr":
            _, recs, n = ref.draw_bgr(f, d, c, 0.5, font, colors, max_boxes=64)
            np.testing.assert_array_equal(frame.cpu().numpy(), f)
        else:
            _, recs, n = ref.draw_yuv420(yy, d, c, 0.5, font, overlay.bgr_to_yuv(colors, "bt709"), uv=cc, max_boxes=64)
            np.testing.assert_array_equal(y.cpu().numpy(), yy)
            np.testing.assert_array_equal(uv.cpu().numpy(), cc)
        check_records(ov, [(recs, n)])
        assert n[0] > 0


# ---- 5: memory ownership --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", guarded_arena.PATTERNS, ids=["0xFF", "0x7F"])
def test_no_result_depends_on_memory_a_call_does_not_own(overlay, pattern):
    """one call of each export with EVERY tensor - frames, planes, dets, counts and what Overlay makes itself: records, n, font, names, colours -
    between bands of `pattern`: the bands stay intact and the results are those of ordinary tensors, which are the reference's"""
    H, W = 17, 65
    ch, cw = -(-H // 2), -(-W // 2)
    rs = np.random.RandomState(31)
    dets, counts = zip(*[boxes(rs, H, W) for _ in range(2)])
    dets, counts = np.stack(dets), np.stack(counts)
    f, yy, cc = rs.randint(0, 256, (2, H, W, 3)).astype(np.uint8), rs.randint(0, 256, (2, H, W)).astype(np.uint8), rs.randint(0, 256, (2, ch, 2 * cw)).astype(np.uint8)
    u, v = rs.randint(0, 256, (2, ch, cw)).astype(np.uint8), rs.randint(0, 256, (2, ch, cw)).astype(np.uint8)
    names = ["bg", "one", "two", "three", "four"]

    def run(place, make):
        ov = make()
        d, c = place(dets, "dets"), place(counts, "counts")
        out = [ov.draw_bgr(place(f, "frames"), d, c, 0.5), ov.records.clone(), ov.n.clone()]
        py, puv = place(yy, "y"), place(cc, "uv")
        ov.draw_yuv420(py, d, c, 0.5, uv=puv, matrix="jpeg")
        py2, pu, pv = place(yy, "y"), place(u, "u"), place(v, "v")
        ov.draw_yuv420(py2, d, c, 0.5, u=pu, v=pv)
        return out + [py, puv, py2, pu, pv, c]          # (dets holds NaNs, which equal nothing)

    make = lambda: overlay.Overlay(NCLS, R, max_boxes=64, names=names, device=DEV, batch=2)          # noqa: E731
    plain = guarded_arena.host(run(lambda a, role: t(a), make))
    arena = guarded_arena.Arena(pattern)
    with pytest.MonkeyPatch.context() as mp, guarded_arena.guarded_allocations(mp, arena):
        guarded = run(lambda a, role: arena.place(a.shape, torch.from_numpy(a).dtype, role, values=torch.from_numpy(a)), make)
        assert sum(p.role.startswith("torch.") for p in arena.placed) >= 8          # font, names, four colour tables, records, n
    arena.check()
    torch.cuda.synchronize()
    assert guarded_arena.same(plain, guarded_arena.host(guarded))
    want = f.copy()
    name_tab = overlay.name_table(names, NCLS)
    for b in range(2):
        ref.draw_bgr(want[b], dets[b], counts[b], 0.5, overlay.font_table(), overlay.palette(NCLS), names=name_tab, max_boxes=64)
    np.testing.assert_array_equal(plain[0].numpy(), want)
    assert (plain[0].numpy() != f).any()


# ---- 6: the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_c_abi_returns_einval_and_launches_nothing(hip, overlay):
    """the header's list through the three exports: LSFA_EINVAL with the export's name in the message, and frames, planes, records and n
    keep every byte; then the same buffers through well-formed calls, which draw"""
    H, W, MB = 17, 65, 8
    ch, cw = -(-H // 2), -(-W // 2)
    L = hip.lib()
    rs = np.random.RandomState(41)
    d, c = boxes(rs, H, W)
    dets, counts = t(d), t(c)
    font, colors = t(overlay.font_table()), t(overlay.palette(NCLS))
    records, n = torch.full((1, MB, overlay.REC_INTS), 7, dtype=torch.int32, device=DEV), torch.full((1, 2), 7, dtype=torch.int32, device=DEV)
    bufs = dict(bgr=torch.full((H, W + 2, 3), 9, dtype=torch.uint8, device=DEV), y=torch.full((H, W + 3), 9, dtype=torch.uint8, device=DEV),
                uv=torch.full((ch, 2 * cw + 4), 9, dtype=torch.uint8, device=DEV), u=torch.full((ch, cw + 1), 9, dtype=torch.uint8, device=DEV),
                v=torch.full((ch, cw + 1), 9, dtype=torch.uint8, device=DEV))
    P = {k: b.data_ptr() for k, b in bufs.items()}

    def plan(**o):
        a = dict(dets=dets.data_ptr(), counts=counts.data_ptr(), N=1, ncls=NCLS, R=R, thresh=0.5, H=H, W=W, t=3, z=2, ws=1, names=None, mb=MB,
                 records=records.data_ptr(), n=n.data_ptr())
        a.update(o)
        return L.lsfa_overlay_plan(a["dets"], a["counts"], a["N"], a["ncls"], a["R"], a["thresh"], a["H"], a["W"], a["t"], a["z"], a["ws"], a["names"],
                                   a["mb"], a["records"], a["n"], None)

    def tail(a):
        return [a["N"], a["H"], a["W"], a["records"], a["n"], a["mb"], a["t"], a["z"], a["font"], a["colors"], a["ncls"], None]

    def common(**o):
        a = dict(N=1, H=H, W=W, records=records.data_ptr(), n=n.data_ptr(), mb=MB, t=3, z=2, font=font.data_ptr(), colors=colors.data_ptr(), ncls=NCLS)
        a.update(o)
        return a

    def paint_bgr(**o):
        a = common(**dict(dict(bgr=P["bgr"], pitch=3 * (W + 2), fs=0), **o))
        return L.lsfa_overlay_paint_bgr(*([a["bgr"], a["pitch"], a["fs"]] + tail(a)))

    def paint_yuv(i420=False, **o):
        base = dict(y=P["y"], yp=W + 3, yfs=0, c=P["u"] if i420 else P["uv"], v=P["v"] if i420 else None, cp=cw + 1 if i420 else 2 * cw + 4, cfs=0)
        a = common(**dict(base, **o))
        return L.lsfa_overlay_paint_yuv420(*([a["y"], a["yp"], a["yfs"], a["c"], a["v"], a["cp"], a["cfs"]] + tail(a)))

    shared = [dict(N=0), dict(N=-1), dict(N=65536), dict(H=0), dict(H=-17), dict(W=0), dict(W=-65), dict(H=65537), dict(W=65537), dict(mb=0), dict(mb=-1),
              dict(mb=overlay.MAX_BOXES + 1), dict(t=0), dict(t=9), dict(t=-3), dict(z=-1), dict(z=5), dict(records=None), dict(n=None)]
    paint_only = [dict(font=None), dict(colors=None), dict(ncls=0), dict(ncls=-1), dict(ncls=overlay.MAX_CLASSES + 1)]
    bad = [(plan, "lsfa_overlay_plan", o) for o in shared + [dict(dets=None), dict(counts=None), dict(R=0), dict(R=-1), dict(ncls=0), dict(ncls=overlay.MAX_CLASSES + 1), dict(ncls=overlay.MAX_CLASSES, R=1 << 20)]]
    bad += [(paint_bgr, "lsfa_overlay_paint_bgr", o) for o in shared + paint_only + [dict(bgr=None), dict(pitch=3 * W - 1), dict(pitch=0), dict(pitch=-3 * W), dict(fs=-1)]]
    bad += [(paint_yuv, "lsfa_overlay_paint_yuv420", o) for o in shared + paint_only + [dict(y=None), dict(c=None), dict(yp=W - 1), dict(yp=0), dict(cp=2 * cw - 1),
                                                                                     dict(cp=-8), dict(yfs=-1), dict(cfs=-1)]]
    bad += [(lambda **o: paint_yuv(i420=True, **o), "lsfa_overlay_paint_yuv420", o) for o in (dict(cp=cw - 1), dict(c=None), dict(H=0))]
    before = {k: b.clone() for k, b in bufs.items()}
    for fn, name, o in bad:
        assert fn(**o) == -1, (name, o)
        assert name in L.lsfa_last_error().decode(), (name, o)
    torch.cuda.synchronize()
    assert all(torch.equal(bufs[k], before[k]) for k in bufs) and bool((records == 7).all()) and bool((n == 7).all())
    # ... and the same buffers through well-formed calls
    recs, cnt = ref.plan(d, c, 0.5, H, W, max_boxes=MB)
    assert plan() == 0 and paint_bgr() == 0 and paint_yuv() == 0
    torch.cuda.synchronize()
    assert tuple(n.cpu().numpy()[0]) == cnt and cnt[1] > MB == cnt[0]
    np.testing.assert_array_equal(records.cpu().numpy()[0], recs)
    index = ref.cover(recs, H, W, NCLS, overlay.font_table())
    want = np.full((H, W + 2, 3), 9, np.uint8)
    ref.paint_bgr(want[:, :W], index, overlay.palette(NCLS))
    np.testing.assert_array_equal(bufs["bgr"].cpu().numpy(), want)
    wy, wuv = np.full((H, W + 3), 9, np.uint8), np.full((ch, 2 * cw + 4), 9, np.uint8)
    ref.paint_yuv420(wy[:, :W], index, overlay.palette(NCLS), uv=wuv[:, :2 * cw])          # the B, G, R rows as they are: the table is the caller's
    np.testing.assert_array_equal(bufs["y"].cpu().numpy(), wy)
    np.testing.assert_array_equal(bufs["uv"].cpu().numpy(), wuv)
    bufs["y"].fill_(9)
    assert paint_yuv(i420=True) == 0
    wu, wv = np.full((ch, cw + 1), 9, np.uint8), np.full((ch, cw + 1), 9, np.uint8)
    ref.paint_yuv420(wy[:, :W].copy(), index, overlay.palette(NCLS), u=wu[:, :cw], v=wv[:, :cw])
    np.testing.assert_array_equal(bufs["y"].cpu().numpy(), wy)
    np.testing.assert_array_equal(bufs["u"].cpu().numpy(), wu)
    np.testing.assert_array_equal(bufs["v"].cpu().numpy(), wv)


# ---- 7: the demo ----------------------------------------------------------------------------------------------------------------------------
def dets_of_json(frame_dets, ncls):
    """the `dets` list of one frame of --out -> dets (ncls, R, 5), counts (ncls): the demo lists a frame's detections in draw order"""
    rows = max([1] + [sum(1 for d in frame_dets if d["class"] == j) for j in range(ncls)])
    dets, counts = np.zeros((ncls, rows, 5)), np.zeros(ncls, np.int32)
    for d in frame_dets:
        j = d["class"]
        dets[j, counts[j]] = d["box"] + [d["score"]]
        counts[j] += 1
    return dets, counts


def test_demo_draws_the_synthetic_clip_and_an_nv12_file(hip, overlay, tmp_path):
    from PIL import Image
    from lsfa_amd import demo
    from lsfa_amd.config.config import lsfa_test_config
    from lsfa_amd.utils.synthetic import SyntheticClip
    ncls = int(lsfa_test_config().dataset.NUM_CLASSES)
    font, colors = overlay.font_table(), overlay.palette(ncls)
    out = tmp_path / "synthetic.json"
    demo.main(["--num", "2", "--score", "0.05", "--no-graph", "--draw", str(tmp_path / "png"), "--draw-thickness", "2", "--out", str(out)])
    results = json.loads(out.read_text())
    clip = SyntheticClip(0, 2, 600, 1000)
    assert sorted(p.name for p in (tmp_path / "png").iterdir()) == ["000000.png", "000001.png"] and sum(len(r["dets"]) for r in results) > 0
    for i, r in enumerate(results):
        dets, counts = dets_of_json(r["dets"], ncls)
        want, _, n = ref.draw_bgr(clip.frame_u8(i).numpy().copy(), dets, counts, 0.05, font, colors, thickness=2, max_boxes=overlay.MAX_BOXES)
        got = np.asarray(Image.open(str(tmp_path / "png" / ("%06d.png" % i))).convert("RGB"))[:, :, ::-1]
        assert 0 < n[0] <= len(r["dets"]) or not r["dets"]
        np.testing.assert_array_equal(got, want, err_msg="synthetic frame %d" % i)

    W, H, frames = 96, 64, 2
    rs = np.random.RandomState(9)
    planes = [ref_yuv.forward(rs.randint(0, 256, (H // 8, W // 8, 3)).astype(np.uint8).repeat(8, 0).repeat(8, 1)) for _ in range(frames)]
    src = tmp_path / "clip.nv12"
    src.write_bytes(b"".join(ref_yuv.raw_frame_bytes(y, u, v, "nv12") for y, u, v in planes))
    names = tmp_path / "classes.txt"
    names.write_text("".join("Kind_%d\n" % j for j in range(1, ncls)))
    out = tmp_path / "nv12.json"
    demo.main(["--yuv", str(src), "--size", "%dx%d" % (W, H), "--score", "0.05", "--no-graph", "--draw-yuv", str(tmp_path / "out.nv12"), "--draw",
               str(tmp_path / "png2"), "--classes", str(names), "--draw-scale", "1", "--out", str(out)])
    results = json.loads(out.read_text())
    raw = (tmp_path / "out.nv12").read_bytes()
    per = W * H * 3 // 2
    assert len(raw) == frames * per and src.read_bytes() != raw and sum(len(r["dets"]) for r in results) > 0
    table = overlay.name_table(["background"] + ["Kind_%d" % j for j in range(1, ncls)], ncls)
    for i, r in enumerate(results):
        dets, counts = dets_of_json(r["dets"], ncls)
        y, u, v = planes[i]
        y, uv = y.copy(), ref_yuv.interleave(u, v)
        kw = dict(label_scale=1, names=table, max_boxes=overlay.MAX_BOXES)
        bgr = ref_yuv.to_bgr(y, uv=uv, matrix="bt601")
        ref.draw_yuv420(y, dets, counts, 0.05, font, overlay.bgr_to_yuv(colors, "bt601"), uv=uv, **kw)
        assert raw[i * per:(i + 1) * per] == y.tobytes() + uv.tobytes(), "nv12 frame %d" % i
        want, _, _ = ref.draw_bgr(np.ascontiguousarray(bgr), dets, counts, 0.05, font, colors, **kw)
        got = np.asarray(Image.open(str(tmp_path / "png2" / ("%06d.png" % i))).convert("RGB"))[:, :, ::-1]
        np.testing.assert_array_equal(got, want, err_msg="nv12 frame %d as BGR" % i)
