"""lsfa_overlay_paint_yuv (lsfa_amd/csrc/overlay.hip) and overlay.Overlay.draw_yuv on the GPU against tests/ref_overlay_fmt.py, bit for bit
(`==` everywhere), in all 29 formats of the intake: the samples, the records and n; a batch of pitched frames; agreement with
lsfa_overlay_paint_yuv420; track ids; graph capture; memory ownership; every refusal of the C ABI; the demo's --draw-raw.
tests/test_overlay_fmt_cpu.py pins the reference.

Every plane is an allocation that ends with its last sample, pre-filled with random samples, its pitch samples hold 0xA5 bytes, and the WHOLE
allocation is compared with a numpy model of it that the reference drew into: a sample the kernel stores outside a covered one - a
neighbour of a wide store, the ignored bits of an uncovered word, the spare Y byte of an odd packed row - shows wherever it lands.

The sizes are the point of the cases: (1, 1) is a corner of one 64 x 16 tile, (5, 7) odd both ways, (17, 67) one tile boundary each way and
W % 4 = 3, (33, 130) two boundaries each way and W % 4 = 2.  A dense plane at an aligned base takes the wide stores wherever a lane's samples
are all covered; a base one sample in with a pitch of the row plus one sample takes the per-sample stores on every second row."""
import json

import numpy as np
import pytest
import torch

import guarded_arena
import ref_overlay
import ref_overlay_fmt as ref
import ref_tracks
import ref_yuvfmt
from test_overlay_gpu import boxes, check_records, dets_of_json, plan_kw, t

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MATRICES = ("bt601", "bt709", "jpeg")
SIZES = [(1, 1), (5, 7), (17, 67), (33, 130)]
NCLS, R = 5, 12
STYLES = [(3, 2), (1, 0), (2, 1), (4, 3)]          # (thickness, label scale)
# one format per (subsampling x layout class x sample width): planar, interleaved and - 4:2:2 of bytes only - packed
CLASSES = ["i420", "nv21", "yuv420p10le", "p010", "yuv422p", "nv16", "uyvy422", "yuv422p10le", "p210", "yuv444p", "nv42", "yuv444p10le", "p410"]


@pytest.fixture(scope="module")
def overlay(hip):
    from lsfa_amd import overlay as module
    return module


def name_of(c):
    names = sorted(k for k, v in ref_yuvfmt.NAMES.items() if v == c)
    return names[0] if names else "0x%03x" % c


class Plane(object):
    """(n, rows, cols) samples - bytes or 16-bit words - with rows `cols + extra` samples apart, frames `gap` samples further apart than a
    frame and the base `offset` samples into an allocation that ends with the last sample, every other byte 0xA5: .host the numpy model
    (.frames its (n, rows, cols) view) and .view the device tensor ((rows, cols) if not batched; words as int16)."""

    def __init__(self, a, extra=0, gap=0, offset=0, batched=True):
        n, rows, cols = a.shape
        pitch = cols + extra
        fs = rows * pitch + gap
        used = (n - 1) * fs + (rows - 1) * pitch + cols
        b = a.dtype.itemsize
        self.host = np.full(offset + used, 0xA5 if b == 1 else 0xA5A5, a.dtype)
        self.frames = np.lib.stride_tricks.as_strided(self.host[offset:], (n, rows, cols), (fs * b, pitch * b, b))
        self.frames[...] = a
        self.buf = torch.from_numpy(self.host.view(np.uint8 if b == 1 else np.int16).copy()).to(DEV)
        view = torch.as_strided(self.buf[offset:], (n, rows, cols), (fs, pitch, 1))
        self.view = view if batched else view[0]

    def check(self, what=""):
        got = self.buf.cpu().numpy().view(self.host.dtype)
        bad = np.flatnonzero(got != self.host)
        assert bad.size == 0, "%s: %d samples differ, the first at %d of %d: 0x%x, expected 0x%x" % (what, bad.size, bad[0], got.size, got[bad[0]], self.host[bad[0]])


def fmt_case(overlay, rs, c, H, W, n, extra, gap, offset, matrix, ov, dets, counts, ids=None, names=None, thresh=0.5):
    """draws frames of format c (a code) on the device and in the numpy model of every plane and compares the whole allocations, the records
    and n; n None: one unbatched frame; dets (n, ncls, R, 5).  -> [(records, (recorded, eligible))]"""
    batched = n is not None
    n = n or 1
    laid = ref_yuvfmt.lay_out(c, *ref_yuvfmt.random_samples(c, rs, H, W, n))
    planes = {k: Plane(a, extra, gap, offset, batched) for k, a in laid.items()}          # u and v share one pitch and one frame stride
    colors = overlay.bgr_to_yuv(overlay.palette(dets.shape[1]), matrix)
    font = overlay.font_table()
    want = []
    for b in range(n):
        if ids is None:
            recs, cnt = ref_overlay.plan(dets[b], counts[b], thresh, H, W, names=names, **plan_kw(ov))
        else:
            recs, cnt = ref_tracks.plan_ids(dets[b], counts[b], ids[b], thresh, H, W, names=names, **plan_kw(ov))
        index = ref_overlay.cover(recs, H, W, dets.shape[1], font, ov.thickness, ov.label_scale)
        ref.paint(c, index, colors, width=W, **{k: p.frames[b] for k, p in planes.items()})
        want.append((recs, cnt))
    lead = (lambda a: t(a)) if batched else (lambda a: t(a[0]))
    views = {k: p.view for k, p in planes.items()}
    y = views.pop("y")
    got = ov.draw_yuv(c, y, lead(dets), lead(counts), thresh, matrix=matrix, width=W, ids=None if ids is None else lead(ids), **views)
    assert got is y
    what = "%s %dx%d pitch +%d gap %d offset %d %s" % (name_of(c), W, H, extra, gap, offset, matrix)
    for k, p in planes.items():
        p.check("%s plane %s" % (what, k))
    check_records(ov, want)
    return want


# ---- 1: every format, bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("c", ref_yuvfmt.ALL, ids=[name_of(c) for c in ref_yuvfmt.ALL])
def test_every_format_equals_the_reference_dense_and_one_sample_in(overlay, c, H, W):
    rs = np.random.RandomState(1000 * H + W + c)
    for k, (extra, offset) in enumerate([(0, 0), (1, 1)]):
        t_, z_ = STYLES[(c + k) % len(STYLES)]
        ov = overlay.Overlay(NCLS, R, max_boxes=64, thickness=t_, label_scale=z_, device=DEV)
        dets, counts = boxes(rs, H, W)
        want = fmt_case(overlay, rs, c, H, W, None, extra, 0, offset, MATRICES[(c + k) % 3], ov, dets[None], counts[None])
        assert H * W < 64 or want[0][1][0] > 0


@pytest.mark.parametrize("name", ["p010", "yuv444p", "uyvy422"])
def test_a_covered_frame_takes_the_wide_stores_and_its_ragged_edge_does_not(overlay, name):
    """thick outlines and large labels: most lanes have their four pixels covered, at every alignment of the row"""
    c = ref_yuvfmt.NAMES[name]
    rs = np.random.RandomState(c)
    for (H, W), extra in (((33, 130), 0), ((18, 66), 2), ((18, 67), 3), ((16, 64), 8)):
        ov = overlay.Overlay(NCLS, R, max_boxes=64, thickness=8, label_scale=4, device=DEV)
        dets, counts = boxes(rs, H, W, junk=False)
        fmt_case(overlay, rs, c, H, W, None, extra, 0, 0, "bt709", ov, dets[None], counts[None])


# ---- 2: a batch -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CLASSES)
def test_batch_of_three_pitched_frames_with_different_counts(overlay, name):
    c = ref_yuvfmt.NAMES[name]
    rs = np.random.RandomState(11 + c)
    for (H, W), gap, extra in (((33, 130), 2, 0), ((18, 67), 32, 16)):
        ov = overlay.Overlay(NCLS, R, max_boxes=64, device=DEV, batch=3)
        dets, counts = zip(*[boxes(rs, H, W) for _ in range(3)])
        dets, counts = np.stack(dets), np.stack(counts)
        counts[1] = 0                                                  # an image without detections between two with
        counts[2, 1:] = [1, R + 9, -4, 3]                              # above R and below 0
        want = fmt_case(overlay, rs, c, H, W, 3, extra, gap, 0, "bt709", ov, dets, counts)
        assert want[1][1] == (0, 0) and want[0][1][0] > 3 and want[2][1][0] > 0


# ---- 3: the old export ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nv12", "i420"])
def test_the_420_codes_leave_the_bytes_of_the_old_export(overlay, name):
    c = ref_yuvfmt.NAMES[name]
    rs = np.random.RandomState(17)
    for (H, W), extra, offset in (((33, 130), 0, 0), ((17, 67), 1, 1), ((16, 64), 4, 0)):
        ov = overlay.Overlay(NCLS, R, max_boxes=64, device=DEV)
        dets, counts = boxes(rs, H, W)
        laid = ref_yuvfmt.lay_out(c, *ref_yuvfmt.random_samples(c, rs, H, W, 1))
        new, old = ({k: Plane(a, extra, 0, offset, False) for k, a in laid.items()} for _ in range(2))
        d, cn = t(dets), t(counts)
        ov.draw_yuv(name, new["y"].view, d, cn, 0.5, matrix="jpeg", **{k: p.view for k, p in new.items() if k != "y"})
        ov.draw_yuv420(old["y"].view, d, cn, 0.5, matrix="jpeg", **{k: p.view for k, p in old.items() if k != "y"})
        for k in new:
            assert torch.equal(new[k].buf, old[k].buf), (name, k, H, W)
        assert not torch.equal(new["y"].buf.cpu(), torch.from_numpy(new["y"].host))


# ---- 4: track ids ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["yuyv422", "yuv422p10le"])
def test_track_ids_are_drawn_bit_exact(overlay, name):
    c = ref_yuvfmt.NAMES[name]
    H, W = 33, 131
    rs = np.random.RandomState(23 + c)
    names = ["bg", "Car", "person", "a_very_long_class_name", "x%"]
    ov = overlay.Overlay(NCLS, R, max_boxes=64, thickness=2, label_scale=1, names=names, device=DEV, batch=2)
    dets, counts = zip(*[boxes(rs, H, W) for _ in range(2)])
    dets, counts = np.stack(dets), np.stack(counts)
    ids = rs.randint(-1, 5, (2, NCLS, R)).astype(np.int32)
    ids[rs.rand(2, NCLS, R) < 0.2] = 123456
    want = fmt_case(overlay, rs, c, H, W, 2, 1, 2, 0, "bt601", ov, dets, counts, ids=ids, names=overlay.name_table(names, NCLS))
    assert want[0][1][0] > 0 and want[1][1][0] > 0


# ---- 5: graph capture -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p010", "uyvy422"])
def test_plan_and_paint_captured_once_and_replayed_on_new_detections_and_frames(overlay, name):
    c = ref_yuvfmt.NAMES[name]
    H, W = 37, 131
    rs = np.random.RandomState(21)
    ov = overlay.Overlay(NCLS, R, max_boxes=64, device=DEV)
    font, colors = overlay.font_table(), overlay.bgr_to_yuv(overlay.palette(NCLS), "bt709")
    dets, counts = torch.zeros((NCLS, R, 5), dtype=torch.float64, device=DEV), torch.zeros(NCLS, dtype=torch.int32, device=DEV)
    as_dev = lambda a: a.view(np.int16) if a.dtype == np.uint16 else a          # noqa: E731
    planes = {k: t(as_dev(np.zeros_like(a))) for k, a in ref_yuvfmt.lay_out(c, *ref_yuvfmt.random_samples(c, rs, H, W)).items()}

    def draw():
        ov.draw_yuv(name, planes["y"], dets, counts, 0.5, matrix="bt709", width=W, **{k: p for k, p in planes.items() if k != "y"})

    draw()                      # loads the code objects outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        draw()
    for k in range(2):
        d, cn = boxes(rs, H, W)
        laid = ref_yuvfmt.lay_out(c, *ref_yuvfmt.random_samples(c, rs, H, W))
        dets.copy_(t(d))
        counts.copy_(t(cn))
        for key, a in laid.items():
            planes[key].copy_(t(as_dev(a)))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _, recs, n = ref.draw(c, laid["y"], d, cn, 0.5, font, colors, width=W, max_boxes=64, **{key: a for key, a in laid.items() if key != "y"})
        for key, a in laid.items():
            np.testing.assert_array_equal(planes[key].cpu().numpy().view(a.dtype), a, err_msg="%s plane %s, replay %d" % (name, key, k))
        check_records(ov, [(recs, n)])
        assert n[0] > 0


# ---- 6: memory ownership --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", guarded_arena.PATTERNS, ids=["0xFF", "0x7F"])
def test_no_result_depends_on_memory_a_call_does_not_own(overlay, pattern):
    """one call per format with EVERY tensor - planes, dets, counts and what Overlay makes itself - between bands of `pattern`: the bands
    stay intact and the results are those of ordinary tensors, which are the reference's"""
    H, W = 17, 65
    rs = np.random.RandomState(31)
    dets, counts = zip(*[boxes(rs, H, W) for _ in range(2)])
    dets, counts = np.stack(dets), np.stack(counts)
    fmts = ["p010", "yuyv422", "yuv444p"]
    as_dev = lambda a: a.view(np.int16) if a.dtype == np.uint16 else a          # noqa: E731
    laid = {f: ref_yuvfmt.lay_out(ref_yuvfmt.NAMES[f], *ref_yuvfmt.random_samples(ref_yuvfmt.NAMES[f], rs, H, W, 2)) for f in fmts}
    names = ["bg", "one", "two", "three", "four"]

    def run(place, make):
        ov = make()
        d, cn = place(dets, "dets"), place(counts, "counts")
        out = []
        for f in fmts:
            planes = {k: place(np.ascontiguousarray(as_dev(a)), f + " " + k) for k, a in laid[f].items()}
            ov.draw_yuv(f, planes["y"], d, cn, 0.5, matrix="jpeg", width=W, **{k: p for k, p in planes.items() if k != "y"})
            out += [planes[k] for k in sorted(planes)] + [ov.records.clone(), ov.n.clone()]
        return out + [cn]          # (dets holds NaNs, which equal nothing)

    make = lambda: overlay.Overlay(NCLS, R, max_boxes=64, names=names, device=DEV, batch=2)          # noqa: E731
    plain = guarded_arena.host(run(lambda a, role: t(a), make))
    arena = guarded_arena.Arena(pattern)
    with pytest.MonkeyPatch.context() as mp, guarded_arena.guarded_allocations(mp, arena):
        guarded = run(lambda a, role: arena.place(a.shape, torch.from_numpy(a).dtype, role, values=torch.from_numpy(a)), make)
        assert sum(p.role.startswith("torch.") for p in arena.placed) >= 8          # font, names, four colour tables, records, n
    arena.check()
    torch.cuda.synchronize()
    assert guarded_arena.same(plain, guarded_arena.host(guarded))
    name_tab, colors = overlay.name_table(names, NCLS), overlay.bgr_to_yuv(overlay.palette(NCLS), "jpeg")
    at = 0
    for f in fmts:
        want = {k: a.copy() for k, a in laid[f].items()}
        for b in range(2):
            ref.draw(f, want["y"][b], dets[b], counts[b], 0.5, overlay.font_table(), colors, width=W, names=name_tab, max_boxes=64,
                     **{k: a[b] for k, a in want.items() if k != "y"})
        for k in sorted(want):
            np.testing.assert_array_equal(plain[at].numpy().view(want[k].dtype), want[k], err_msg="%s plane %s" % (f, k))
            at += 1
        at += 2
        assert (want["y"] != laid[f]["y"]).any()


# ---- 7: the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_c_abi_returns_einval_and_launches_nothing(hip, overlay):
    """the header's list: LSFA_EINVAL with the export's name in the message, and planes, records and n keep every byte; then the same
    buffers through well-formed calls, which draw"""
    H, W, MB = 17, 65, 8
    cw = -(-W // 2)
    L = hip.lib()
    rs = np.random.RandomState(41)
    d, cn = boxes(rs, H, W)
    dets, counts = t(d), t(cn)
    font, colors = t(overlay.font_table()), t(overlay.bgr_to_yuv(overlay.palette(NCLS)))
    records, n = torch.full((1, MB, overlay.REC_INTS), 7, dtype=torch.int32, device=DEV), torch.full((1, 2), 7, dtype=torch.int32, device=DEV)
    # one pitch with room for every format's rows: Y of words, interleaved 4:4:4 chroma of words, packed rows
    PITCH = 4 * W + 8
    bufs = {k: torch.full((H, PITCH), 9, dtype=torch.uint8, device=DEV) for k in ("y", "c", "v")}
    P = {k: b.data_ptr() for k, b in bufs.items()}
    assert all(p % 4 == 0 for p in P.values())
    F = ref_yuvfmt.NAMES

    def paint(fmt, **o):
        """a well-formed call of format fmt, changed by o"""
        sub, layout, sample = ref_yuvfmt.fields(fmt)
        if layout >= ref_yuvfmt.YUYV:
            a = dict(y=P["y"], yp=PITCH, yfs=0, c=None, v=None, cp=0, cfs=0)
        else:
            a = dict(y=P["y"], yp=PITCH, yfs=0, c=P["c"], v=P["v"] if layout == 0 else None, cp=PITCH, cfs=0)
        a.update(N=1, H=H, W=W, fmt=fmt, records=records.data_ptr(), n=n.data_ptr(), mb=MB, t=3, z=2, font=font.data_ptr(), colors=colors.data_ptr(),
                 ncls=NCLS)
        a.update(o)
        return L.lsfa_overlay_paint_yuv(a["y"], a["yp"], a["yfs"], a["c"], a["v"], a["cp"], a["cfs"], a["N"], a["H"], a["W"], a["fmt"], a["records"],
                                        a["n"], a["mb"], a["t"], a["z"], a["font"], a["colors"], a["ncls"], None)

    shared = [dict(N=0), dict(N=-1), dict(N=65536), dict(H=0), dict(H=-17), dict(W=0), dict(W=-65), dict(H=65537), dict(W=65537), dict(mb=0), dict(mb=-1),
              dict(mb=overlay.MAX_BOXES + 1), dict(t=0), dict(t=9), dict(t=-3), dict(z=-1), dict(z=5), dict(records=None), dict(n=None), dict(font=None),
              dict(colors=None), dict(ncls=0), dict(ncls=-1), dict(ncls=overlay.MAX_CLASSES + 1), dict(y=None), dict(yfs=-2)]
    bad = [(F[f], o) for f in ("nv12", "yuv422p10le", "uyvy422") for o in shared]
    # a format outside the 27 + 2
    bad += [(c, {}) for c in (3, 0x50, 0x300, 1 << 12, -1, ref_yuvfmt.code(0, 3, 0), ref_yuvfmt.code(2, 4, 0), ref_yuvfmt.code(1, 3, 1), ref_yuvfmt.code(1, 4, 2))]
    # v given with layouts 1 and 2 or missing with layout 0; a missing chroma plane
    bad += [(F["nv12"], dict(v=P["v"])), (F["nv21"], dict(v=P["v"])), (F["p210"], dict(v=P["v"])), (F["i420"], dict(v=None)), (F["yuv444p10le"], dict(v=None)),
            (F["nv16"], dict(c=None)), (F["yuv422p"], dict(c=None))]
    # a chroma pointer, pitch or stride with a packed layout
    bad += [(F[f], o) for f in ("yuyv422", "uyvy422") for o in (dict(c=P["c"]), dict(v=P["v"]), dict(cp=4 * cw), dict(cfs=4), dict(c=P["c"], v=P["v"], cp=4 * cw))]
    # for words an odd base, pitch or frame stride
    bad += [(F[f], o) for f in ("p010", "yuv444p10le") for o in (dict(y=P["y"] + 1), dict(c=P["c"] + 1), dict(yp=2 * W + 5), dict(cp=4 * W + 5), dict(yfs=3), dict(cfs=1))]
    bad += [(F["yuv420p10le"], dict(v=P["v"] + 1))]
    # a pitch below its row, per layout and sample width; negative frame strides
    bad += [(F["nv12"], dict(yp=W - 1)), (F["nv12"], dict(cp=2 * cw - 1)), (F["i420"], dict(cp=cw - 1)), (F["nv24"], dict(cp=2 * W - 1)), (F["yuv444p"], dict(cp=W - 1)),
            (F["p010"], dict(yp=2 * W - 2)), (F["p010"], dict(cp=4 * cw - 2)), (F["yuv422p10le"], dict(cp=2 * cw - 2)), (F["p410"], dict(cp=4 * W - 2)),
            (F["yuyv422"], dict(yp=4 * cw - 1)), (F["uyvy422"], dict(yp=2 * W)), (F["nv12"], dict(yp=0)), (F["nv12"], dict(cp=-8)), (F["nv16"], dict(cfs=-1)),
            (F["yuv422p"], dict(yfs=-1))]
    before = {k: b.clone() for k, b in bufs.items()}
    for fmt, o in bad:
        assert paint(fmt, **o) == -1, (hex(fmt), o)
        assert "lsfa_overlay_paint_yuv" in L.lsfa_last_error().decode(), (hex(fmt), o)
    torch.cuda.synchronize()
    assert all(torch.equal(bufs[k], before[k]) for k in bufs) and bool((records == 7).all()) and bool((n == 7).all())
    # ... and the same buffers through well-formed calls
    recs, cnt = ref_overlay.plan(d, cn, 0.5, H, W, max_boxes=MB)
    assert L.lsfa_overlay_plan(dets.data_ptr(), counts.data_ptr(), 1, NCLS, R, 0.5, H, W, 3, 2, 1, None, MB, records.data_ptr(), n.data_ptr(), None) == 0
    index = ref_overlay.cover(recs, H, W, NCLS, overlay.font_table())
    yuv = overlay.bgr_to_yuv(overlay.palette(NCLS))
    for name in ("nv12", "yuv422p10le", "uyvy422", "p410", "yuv444p"):
        for b in bufs.values():
            b.fill_(9)
        assert paint(F[name]) == 0, name
        torch.cuda.synchronize()
        sub, layout, sample = ref_yuvfmt.fields(F[name])
        dt = ref_yuvfmt.dtype(F[name])
        ch, ccw = ref_yuvfmt.chroma_shape(F[name], H, W)
        want = {k: np.full((H, PITCH), 9, np.uint8) for k in bufs}
        row = lambda k, rows, samples: want[k][:rows].view(dt)[:, :samples]          # noqa: E731
        if layout >= ref_yuvfmt.YUYV:
            ref.paint(name, index, yuv, y=row("y", H, 4 * cw), width=W)
        elif layout == 0:
            ref.paint(name, index, yuv, y=row("y", H, W), u=row("c", ch, ccw), v=row("v", ch, ccw))
        else:
            ref.paint(name, index, yuv, y=row("y", H, W), uv=row("c", ch, 2 * ccw))
        for k in bufs:
            np.testing.assert_array_equal(bufs[k].cpu().numpy(), want[k], err_msg="%s buffer %s" % (name, k))
        assert (want["y"] != 9).any()
    assert tuple(n.cpu().numpy()[0]) == cnt and cnt[1] > MB == cnt[0]


# ---- 8: the demo ----------------------------------------------------------------------------------------------------------------------------
def test_demo_draws_a_p010_file_in_its_own_layout(hip, overlay, tmp_path):
    from lsfa_amd import demo
    from lsfa_amd.config.config import lsfa_test_config
    import ref_yuv
    ncls = int(lsfa_test_config().dataset.NUM_CLASSES)
    font, colors = overlay.font_table(), overlay.bgr_to_yuv(overlay.palette(ncls), "bt709")
    W, H, frames = 96, 64, 2
    c = ref_yuvfmt.NAMES["p010"]
    rs = np.random.RandomState(9)
    clip = []
    for _ in range(frames):          # blocky 8-bit frames as ten-bit samples in the high bits of their words
        y, u, v = ref_yuv.forward(rs.randint(0, 256, (H // 8, W // 8, 3)).astype(np.uint8).repeat(8, 0).repeat(8, 1))
        clip.append(tuple((a.astype(np.uint16) << 8).astype(np.uint16) for a in (y, u, v)))
    src = tmp_path / "clip.p010"
    src.write_bytes(b"".join(ref_yuvfmt.raw_frame_bytes(c, *f) for f in clip))
    names = tmp_path / "classes.txt"
    names.write_text("".join("Kind_%d\n" % j for j in range(1, ncls)))
    out = tmp_path / "p010.json"
    demo.main(["--yuv", str(src), "--size", "%dx%d" % (W, H), "--yuv-format", "p010", "--yuv-matrix", "bt709", "--score", "0.05", "--no-graph", "--draw-raw",
               str(tmp_path / "out.p010"), "--classes", str(names), "--draw-scale", "1", "--draw-thickness", "2", "--out", str(out)])
    results = json.loads(out.read_text())
    raw = (tmp_path / "out.p010").read_bytes()
    per = 2 * W * H * 3 // 2
    assert len(raw) == frames * per and src.read_bytes() != raw and sum(len(r["dets"]) for r in results) > 0
    table = overlay.name_table(["background"] + ["Kind_%d" % j for j in range(1, ncls)], ncls)
    for i, r in enumerate(results):
        dets, counts = dets_of_json(r["dets"], ncls)
        p = ref_yuvfmt.lay_out(c, *clip[i])
        ref.draw("p010", p["y"], dets, counts, 0.05, font, colors, uv=p["uv"], thickness=2, label_scale=1, names=table, max_boxes=overlay.MAX_BOXES)
        assert raw[i * per:(i + 1) * per] == p["y"].astype("<u2").tobytes() + p["uv"].astype("<u2").tobytes(), "p010 frame %d" % i
