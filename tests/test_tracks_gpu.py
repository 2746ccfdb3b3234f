"""lsfa_track_steps (lsfa_amd/csrc/tracks.hip) and lsfa_overlay_plan_ids (overlay.hip) on the GPU against tests/ref_tracks.py, bit for bit (`==`
everywhere): tbox as raw 64-bit patterns, tint, issued, ids and n; rows consumed in place from the motion search; garbage in the state
between guard bands; graph capture; the ids variant of the overlay through both paint calls; every refusal of the C ABI and of the wrappers.
tests/test_tracks_cpu.py pins the reference.

The shapes are the smallest at which the kernel can still go wrong: 33 classes are more than the sixteen waves of a workgroup, 70 rows in one
class more than a wave of detections, 70 and 257 slots more than one and four groups of 64, 1 and 4 slots overflow, and 150 rows are no
multiple of 64."""
import numpy as np
import pytest
import torch

import guarded_arena
import ref_overlay
import ref_tracks as ref
import test_overlay_gpu as og
from me_util import clip, t

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
W, H, BLOCKS = 320, 200, 200


@pytest.fixture(scope="module")
def tracks(hip):
    from lsfa_amd import tracks as module
    return module


@pytest.fixture(scope="module")
def overlay(hip):
    from lsfa_amd import overlay as module
    return module


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def scene(rs, frames, ncls, R, crowd=False):
    """one stream: dets (frames, ncls, R, 5), counts (frames, ncls), rows (frames, BLOCKS, 7), row_n (frames).  Integer boxes with jittered
    constant velocities, births, deaths, missed frames, duplicates (which become identical tracks, so the next frame's IoUs tie exactly), rows
    that are not eligible, counts below 0 and above R; crowd: class 1 holds R objects from the first frame on"""
    dets, counts = np.zeros((frames, ncls, R, 5)), np.zeros((frames, ncls), np.int32)
    rows, row_n = np.zeros((frames, BLOCKS, 7), np.int32), np.zeros(frames, np.int32)
    drift = [(int(rs.randint(-12, 13)), int(rs.randint(-8, 9))) for _ in range(3)]

    def new_object():
        x, y = rs.randint(0, W - 40), rs.randint(0, H - 40)
        return [x, y, x + rs.randint(10, 50), y + rs.randint(10, 50)], drift[rs.randint(0, 3)]

    objects = {j: [new_object() for _ in range(R if crowd and j == 1 else rs.randint(0, min(R, 4) + 1))] for j in range(1, ncls)}
    for f in range(frames):
        for k in range(BLOCKS):
            sx, sy = rs.randint(0, W), rs.randint(0, H)
            v = drift[rs.randint(0, 3)] if rs.rand() < 0.8 else (0, 0)
            rows[f, k] = (-1, 16, 16, sx, sy, sx + v[0] + rs.randint(-1, 2), sy + v[1])
        row_n[f] = (0, 1, 150, BLOCKS, BLOCKS + 7)[rs.randint(0, 5)]
        for j in range(1, ncls):
            objs = objects[j]
            for box, v in objs:
                jx, jy = rs.randint(-1, 2), rs.randint(-1, 2)
                box[0] += v[0] + jx; box[2] += v[0] + jx; box[1] += v[1] + jy; box[3] += v[1] + jy          # noqa: E702
            if objs and rs.rand() < 0.15:
                objs.pop(rs.randint(0, len(objs)))
            if len(objs) < R and rs.rand() < 0.3:
                objs.append(new_object())
            out = []
            for box, v in objs:
                if rs.rand() < 0.1:
                    continue                                                       # missed this frame
                out.append(box + [rs.uniform(0.5, 1.0)])
                if rs.rand() < 0.1:
                    out.append(box + [rs.uniform(0.5, 1.0)])                       # a duplicate
                if rs.rand() < 0.1:
                    out.append([(np.nan, 5, 20, 30, 0.9), (5, 5, 20, np.inf, 0.9), (5, 5, 20, 30, 0.2), (30, 5, 20, 30, 0.9)][rs.randint(0, 4)])
            out = [out[i] for i in rs.permutation(len(out))][:R]
            for r, row in enumerate(out):
                dets[f, j, r] = row
            dets[f, j, len(out):] = (1, 1, 30, 30, 0.99)                           # beyond counts: never read as a detection
            counts[f, j] = len(out)
            if not out and rs.rand() < 0.3:
                counts[f, j] = -2
            elif len(out) == R and rs.rand() < 0.3:
                counts[f, j] = R + 3
        dets[f, 0] = (0, 0, W, H, 0.99)
        counts[f, 0] = R
    return dets, counts, rows, row_n


def same_state(tr, want, what):
    tbox, tint, issued = tr.state()
    np.testing.assert_array_equal(tint, want.tint, err_msg="%s: tint" % what)
    np.testing.assert_array_equal(bits(tbox), bits(want.tbox), err_msg="%s: tbox" % what)
    np.testing.assert_array_equal(issued, want.issued, err_msg="%s: issued" % what)


# ---- 1: randomised scenes -----------------------------------------------------------------------------------------------------------------
#        ncls, R,  T,   S, F,  crowd
CASES = [(2,  1,  1,   1, 1,  False),
         (4,  8,  4,   3, 5,  False),
         (33, 8,  70,  1, 12, False),
         (4,  70, 70,  1, 12, True),
         (4,  70, 257, 3, 5,  True),
         (33, 1,  257, 1, 1,  False),
         (2,  70, 4,   1, 5,  True),
         (4,  8,  1,   3, 12, False)]


@pytest.mark.parametrize("ncls,R,T,S,F,crowd", CASES)
def test_randomised_scenes_equal_the_reference(tracks, ncls, R, T, S, F, crowd):
    calls = -(-12 // F)
    rs = np.random.RandomState(1000 * ncls + 10 * R + T + S + F + 1)
    streams = [scene(rs, calls * F, ncls, R, crowd and s == 0) for s in range(S)]
    dets, counts, rows, row_n = (np.stack([st[k] for st in streams]) for k in range(4))
    kw = dict(max_tracks=T, score_thresh=0.5, iou_thresh=0.3, max_age=2, min_hits=2, streams=S)
    tr, want = tracks.Tracker(ncls, R, frames=F, device=DEV, **kw), ref.Tracker(ncls, R, **kw)
    total = np.zeros(4, np.int64)
    for c in range(calls):
        fs = slice(c * F, (c + 1) * F)
        with_rows = c != 1 or calls == 1                   # the second call of several: no rows at all
        got = tr.steps(t(dets[:, fs]), t(counts[:, fs]), t(rows[:, fs]) if with_rows else None, t(row_n[:, fs]) if with_rows else None)
        ids, n = want.steps(dets[:, fs], counts[:, fs], rows[:, fs] if with_rows else None, row_n[:, fs])
        assert got is tr.ids
        np.testing.assert_array_equal(got.cpu().numpy(), ids, err_msg="ids of call %d" % c)
        np.testing.assert_array_equal(tr.stats(), n, err_msg="n of call %d" % c)
        same_state(tr, want, "call %d" % c)
        total += n.reshape(-1, 4).sum(0)
    assert total[0] > 0 and total[2] > 0 and total[1] > 0 and (T >= (ncls - 1) * R or total[3] > 0), total          # fewer slots than rows: drops
    if crowd:
        assert max(int(c) for c in counts[0, :, 1]) >= R and want.tint[0, :, 0].astype(bool).sum() > min(T, 64) - 1


def test_step_is_one_frame_of_one_stream_and_reset_empties_the_tracker(tracks):
    ncls, R = 4, 8
    dets, counts, rows, row_n = scene(np.random.RandomState(5), 6, ncls, R)
    tr, want = tracks.Tracker(ncls, R, max_tracks=16, device=DEV), ref.Tracker(ncls, R, max_tracks=16)
    for f in range(6):
        r = t(rows[f]) if f % 2 else None                  # all the rows of the estimator, or none
        got = tr.step(t(dets[f]), t(counts[f]), r)
        ids, n = want.step(dets[f], counts[f], rows[f] if f % 2 else None, BLOCKS)
        np.testing.assert_array_equal(got.cpu().numpy(), ids)
        np.testing.assert_array_equal(tr.stats()[0, 0], n)
        same_state(tr, want, "frame %d" % f)
    assert want.tint[0, :, 0].any()
    tr.reset()
    assert not any(x.any() for x in tr.state())


# ---- 2: rows consumed in place -----------------------------------------------------------------------------------------------------------
def test_rows_of_the_chain_search_are_read_in_place_through_their_strides(hip, tracks):
    width, height, ncls, R = 96, 64, 3, 8
    clips = [clip(5, width, height, seed=3), clip(5, width, height, seed=4, m=(-4, 5))]
    sme = hip.SegmentMotionEstimator(width, height, frames=4, clips=2, device=DEV, search=8, lam=4)
    sme.segment(t(np.stack([np.stack(c) for c in clips])), 1.0, (0.0, 0.0, 0.0), 1.0)
    assert tuple(sme.rows.shape) == (2, 4, 24, 7)
    host_rows = sme.rows.cpu().numpy()
    assert (host_rows[0, :, :, 5] - host_rows[0, :, :, 3] != 0).any()
    # boxes that move as the texture does: clip 0 by (3, -2), clip 1 by (-4, 5) a frame
    dets, counts = np.zeros((2, 4, ncls, R, 5)), np.zeros((2, 4, ncls), np.int32)
    for c, m in enumerate(((3, -2), (-4, 5))):
        for f in range(4):
            for j in (1, 2):
                x, y = 20 + 10 * j + m[0] * (f + 1), 20 + m[1] * (f + 1)
                dets[c, f, j, 0] = (x, y, x + 40, y + 30, 0.9)
                counts[c, f, j] = 1
    kw = dict(max_tracks=4, iou_thresh=0.3, streams=2)
    for view, host in ((sme.rows, host_rows), (sme.rows[:, :, :17], host_rows[:, :, :17])):          # as it stands, and a strided view of it
        tr, want = tracks.Tracker(ncls, R, frames=4, device=DEV, **kw), ref.Tracker(ncls, R, **kw)
        before = sme.rows.clone()
        got = tr.steps(t(dets), t(counts), view)
        ids, n = want.steps(dets, counts, host, np.full((2, 4), host.shape[2], np.int32))
        np.testing.assert_array_equal(got.cpu().numpy(), ids)
        np.testing.assert_array_equal(tr.stats(), n)
        same_state(tr, want, "rows %s" % (tuple(view.shape),))
        assert torch.equal(sme.rows, before) and n[:, 1:, 1].sum() == 12


# ---- 3: garbage in the state ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", guarded_arena.PATTERNS, ids=["0xFF", "0x7F"])
def test_garbage_in_the_state_and_the_rows_between_guard_bands(tracks, pattern):
    """a slot of class 999, a NaN box, counters at INT_MAX, a free slot that holds values, rows of INT_MIN / INT_MAX: the reference's bits,
    every band intact, and the results of ordinary tensors"""
    ncls, R, T, F = 4, 8, 70, 3
    imax, imin = 2 ** 31 - 1, -2 ** 31
    dets, counts, rows, row_n = scene(np.random.RandomState(77), F, ncls, R)
    rows[:, 0] = (0, 0, 0, imax, imin, imin, imax)
    rows[:, 1] = (0, 0, 0, imin, imax, imax, imin)
    rows[:, 2] = (0, 0, 0, 10, 10, imax, imin)
    row_n[:] = BLOCKS
    tbox, tint = np.zeros((1, T, 5)), np.zeros((1, T, 4), np.int32)
    tbox[0, 0], tint[0, 0] = (5, 5, 60, 60, 0.5), (3, 999, 1, 0)                      # a class that does not exist
    tbox[0, 1], tint[0, 1] = (np.nan, 5, 60, 60, 0.5), (4, 1, imax, imax)             # NaN box, counters that wrap
    tbox[0, 2], tint[0, 2] = (-1e300, -1e300, 1e300, 1e300, 0.5), (5, 2, 1, 0)        # holds every row, INT_MAX ones included
    tbox[0, 3], tint[0, 3] = (7, 7, 9, 9, 0.25), (0, 1, 5, 5)                         # free, with values left in it
    tbox[0, 69], tint[0, 69] = (5, 5, 60, 60, 0.5), (-7, -1, imin, -1)                # a negative id is active
    tbox[0, 4], tint[0, 4] = (100, 100, 140, 140, 0.5), (-2, 3, 1, 0)                 # an id that is matched and reads like no other
    dets[:, 3, 0], counts[:, 3] = (100, 100, 140, 140, 0.9), np.maximum(counts[:, 3], 1)
    kw = dict(max_tracks=T, max_age=1, min_hits=1)
    want = ref.Tracker(ncls, R, **kw)
    want.tbox[:], want.tint[:], want.issued[:] = tbox, tint, imax
    ids, n = want.steps(dets[None], counts[None], rows[None], row_n[None])

    def run(place, make):
        tr = make()
        tr.tbox.copy_(t(tbox)); tr.tint.copy_(t(tint)); tr.issued.fill_(imax)          # noqa: E702
        got = tr.steps(place(dets[None]), place(counts[None]), place(rows[None]), place(row_n[None]))
        return [got, tr.n, tr.tbox.view(torch.int64), tr.tint, tr.issued]

    make = lambda: tracks.Tracker(ncls, R, frames=F, device=DEV, **kw)          # noqa: E731
    plain = guarded_arena.host(run(t, make))
    arena = guarded_arena.Arena(pattern)
    with pytest.MonkeyPatch.context() as mp, guarded_arena.guarded_allocations(mp, arena):
        guarded = run(lambda a: arena.place(a.shape, torch.from_numpy(a).dtype, "input", values=torch.from_numpy(np.ascontiguousarray(a))), make)
        assert sum(p.role.startswith("torch.") for p in arena.placed) >= 5          # tbox, tint, issued, ids, n
    arena.check()
    torch.cuda.synchronize()
    assert guarded_arena.same(plain, guarded_arena.host(guarded))
    np.testing.assert_array_equal(plain[0].numpy(), ids)
    np.testing.assert_array_equal(plain[1].numpy(), n)
    np.testing.assert_array_equal(plain[2].numpy(), bits(want.tbox))
    np.testing.assert_array_equal(plain[3].numpy(), want.tint)
    np.testing.assert_array_equal(plain[4].numpy(), want.issued)
    assert n[0, :, 0].sum() > 0 and (ids[0, :, 3, 0] == -2).all() and (n[0, :, 2] > 0).all() and want.tint[0, 4].tolist() == [-2, 3, 1 + F, 0]


# ---- 4: graph capture -------------------------------------------------------------------------------------------------------------------
def test_a_captured_steps_call_replayed_three_times_advances_three_segments(tracks):
    ncls, R, F = 4, 8, 3
    dets, counts, rows, row_n = (a[None] for a in scene(np.random.RandomState(9), F, ncls, R))
    kw = dict(max_tracks=6, max_age=1, min_hits=2)
    d, c, r, rn = t(dets), t(counts), t(rows), t(row_n)
    tr, eager, want = tracks.Tracker(ncls, R, frames=F, device=DEV, **kw), tracks.Tracker(ncls, R, frames=F, device=DEV, **kw), ref.Tracker(ncls, R, **kw)
    tr.steps(d, c, r, rn)                   # loads the code object outside the capture
    tr.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tr.steps(d, c, r, rn)
    tr.reset()
    torch.cuda.synchronize()
    for k in range(3):
        g.replay()
        eager.steps(d, c, r, rn)
        ids, n = want.steps(dets, counts, rows, row_n)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(tr.ids.cpu().numpy(), ids, err_msg="replay %d" % k)
        assert torch.equal(tr.ids, eager.ids) and torch.equal(tr.n, eager.n)
        same_state(tr, want, "replay %d" % k)
        same_state(eager, want, "eager call %d" % k)
    assert want.issued[0] > 0


def test_tracker_and_overlay_in_one_graph(tracks, overlay):
    ncls, R, fh, fw = 4, 8, 45, 70
    rs = np.random.RandomState(13)
    tr, want = tracks.Tracker(ncls, R, max_tracks=16, device=DEV), ref.Tracker(ncls, R, max_tracks=16)
    ov = overlay.Overlay(ncls, R, max_boxes=32, thickness=1, label_scale=1, device=DEV)
    dets, counts = torch.zeros((ncls, R, 5), dtype=torch.float64, device=DEV), torch.zeros(ncls, dtype=torch.int32, device=DEV)
    frame = torch.zeros((fh, fw, 3), dtype=torch.uint8, device=DEV)

    def run():
        ov.draw_bgr(frame, dets, counts, 0.5, ids=tr.step(dets, counts))

    run()
    tr.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    tr.reset()
    for k in range(3):
        d, c = og.boxes(rs, fh, fw, ncls=ncls, rows=R)
        f = rs.randint(0, 256, (fh, fw, 3)).astype(np.uint8)
        for dst, src in ((dets, d), (counts, c), (frame, f)):
            dst.copy_(t(src))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ids, n = want.step(d, c)
        recs, cnt = ref.plan_ids(d, c, ids, 0.5, fh, fw, thickness=1, label_scale=1, max_boxes=32)
        ref_overlay.paint_bgr(f, ref_overlay.cover(recs, fh, fw, ncls, overlay.font_table(), 1, 1), overlay.palette(ncls))
        np.testing.assert_array_equal(tr.ids[0, 0].cpu().numpy(), ids)
        np.testing.assert_array_equal(frame.cpu().numpy(), f)
        og.check_records(ov, [(recs, cnt)])
        assert cnt[0] > 0


# ---- 5: the ids variant of the overlay ----------------------------------------------------------------------------------------------------
def some_ids(rs, shape):
    ids = rs.randint(1, 9, shape).astype(np.int32)
    kind = rs.randint(0, 6, shape)
    ids[kind == 0], ids[kind == 1], ids[kind == 2] = 0, -1, rs.randint(99990, 2 ** 31 - 1)
    return ids


def test_plan_ids_and_both_paint_calls_equal_the_reference(overlay):
    rs = np.random.RandomState(17)
    ncls, R = og.NCLS, og.R
    names = ["bg", "Car", "person", "a_very_long_class_name", "x%"]
    table, font, colors = overlay.name_table(names, ncls), overlay.font_table(), overlay.palette(ncls)
    for k, (extra, offset) in enumerate([(0, 0), (1, 0), (4, 1)]):
        thick, z = og.STYLES[k]
        fh, fw = 45, 70
        ov = overlay.Overlay(ncls, R, max_boxes=64, thickness=thick, label_scale=z, names=names if k != 1 else None, device=DEV, batch=2)
        kw = dict(names=table if k != 1 else None, **og.plan_kw(ov))
        dets, counts = zip(*[og.boxes(rs, fh, fw) for _ in range(2)])
        dets, counts, ids = np.stack(dets), np.stack(counts), some_ids(rs, (2, ncls, R))
        surf = og.Surface(rs.randint(0, 256, (2, fh, 3 * fw)).astype(np.uint8), extra, 8, offset, pixel=3)
        want = []
        for b in range(2):
            recs, n = ref.plan_ids(dets[b], counts[b], ids[b], 0.5, fh, fw, **kw)
            ref_overlay.paint_bgr(surf.frames[b].reshape(fh, fw, 3), ref_overlay.cover(recs, fh, fw, ncls, font, thick, z), colors)
            want.append((recs, n))
        ov.draw_bgr(surf.view, t(dets), t(counts), 0.5, ids=t(ids))
        surf.check("bgr with ids, style %d" % k)
        og.check_records(ov, want)
        plain = [ref_overlay.plan(dets[b], counts[b], 0.5, fh, fw, **kw)[1] for b in range(2)]
        assert all(0 < w[1][1] < p[1] for w, p in zip(want, plain)) and (z == 0 or max(int(w[0][:, 9].max()) for w in want) > 18)
        # 4:2:0, an odd width: NV12 and I420
        fw = 71
        ch, cw = -(-fh // 2), -(-fw // 2)
        yuv = overlay.bgr_to_yuv(colors, "bt709")
        for nv12 in (True, False):
            dets1, counts1 = og.boxes(rs, fh, fw)
            ids1 = some_ids(rs, (ncls, R))
            ys = og.Surface(rs.randint(0, 256, (1, fh, fw)).astype(np.uint8), extra, 0, offset, batched=False)
            cs = [og.Surface(rs.randint(0, 256, (1, ch, 2 * cw if nv12 else cw)).astype(np.uint8), extra, 0, offset, batched=False) for _ in range(1 if nv12 else 2)]
            recs, n = ref.plan_ids(dets1, counts1, ids1, 0.5, fh, fw, **kw)
            planes = dict(uv=cs[0].frames[0]) if nv12 else dict(u=cs[0].frames[0], v=cs[1].frames[0])
            ref_overlay.paint_yuv420(ys.frames[0], ref_overlay.cover(recs, fh, fw, ncls, font, thick, z), yuv, **planes)
            planes = dict(uv=cs[0].view) if nv12 else dict(u=cs[0].view, v=cs[1].view)
            ov.draw_yuv420(ys.view, t(dets1), t(counts1), 0.5, matrix="bt709", ids=t(ids1), **planes)
            for s_ in [ys] + cs:
                s_.check("%s with ids, style %d" % ("nv12" if nv12 else "i420", k))
            og.check_records(ov, [(recs, n)])
            assert n[0] > 0


def test_draw_bgr_without_ids_gives_the_bytes_it_gives_today(overlay):
    rs = np.random.RandomState(19)
    fh, fw = 45, 70
    ov = overlay.Overlay(og.NCLS, og.R, max_boxes=64, device=DEV)
    dets, counts = og.boxes(rs, fh, fw)
    for kw in (dict(), dict(ids=None)):
        surf = og.Surface(rs.randint(0, 256, (1, fh, 3 * fw)).astype(np.uint8), 4, 0, 0, batched=False, pixel=3)
        want = og.expect_bgr(overlay, surf, fh, fw, dets[None], counts[None], 0.5, **og.plan_kw(ov))
        ov.draw_bgr(surf.view, t(dets), t(counts), 0.5, **kw)
        surf.check("no ids")
        og.check_records(ov, want)
        assert want[0][1][0] > 0


# ---- 6: the C ABI and the wrappers ---------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_c_abi_returns_einval_and_launches_nothing(hip, overlay):
    ncls, R, T, S, F = 4, 8, 16, 2, 2
    L = hip.lib()
    full = lambda shape, dtype: torch.full(shape, 7, dtype=dtype, device=DEV)          # noqa: E731
    bufs = dict(dets=full((S, F, ncls, R, 5), torch.float64), counts=full((S, F, ncls), torch.int32), rows=full((S, F, 10, 7), torch.int32),
                row_n=full((S, F), torch.int32), tbox=full((S, T, 5), torch.float64), tint=full((S, T, 4), torch.int32), issued=full((S,), torch.int32),
                ids=full((S, F, ncls, R), torch.int32), n=full((S, F, 4), torch.int32), records=full((S, 8, overlay.REC_INTS), torch.int32),
                pn=full((S, 2), torch.int32))
    before = {k: b.clone() for k, b in bufs.items()}
    P = {k: b.data_ptr() for k, b in bufs.items()}

    def steps(**o):
        a = dict(dets=P["dets"], counts=P["counts"], S=S, F=F, ncls=ncls, R=R, rows=P["rows"], row_n=P["row_n"], n_max=10, ss=F * 70, fs=70, st=0.5, it=0.3,
                 max_age=2, min_hits=1, T=T, tbox=P["tbox"], tint=P["tint"], issued=P["issued"], ids=P["ids"], n=P["n"])
        a.update(o)
        return L.lsfa_track_steps(a["dets"], a["counts"], a["S"], a["F"], a["ncls"], a["R"], a["rows"], a["row_n"], a["n_max"], a["ss"], a["fs"], a["st"], a["it"],
                                  a["max_age"], a["min_hits"], a["T"], a["tbox"], a["tint"], a["issued"], a["ids"], a["n"], None)

    def plan_ids(**o):
        a = dict(dets=P["dets"], counts=P["counts"], ids=P["ids"], N=S, ncls=ncls, R=R, thresh=0.5, H=45, W=70, t=3, z=2, ws=1, names=None, mb=8,
                 records=P["records"], n=P["pn"])
        a.update(o)
        return L.lsfa_overlay_plan_ids(a["dets"], a["counts"], a["ids"], a["N"], a["ncls"], a["R"], a["thresh"], a["H"], a["W"], a["t"], a["z"], a["ws"],
                                       a["names"], a["mb"], a["records"], a["n"], None)

    nan, inf = float("nan"), float("inf")
    bad = [(steps, "lsfa_track_steps", o) for o in
           [dict(dets=None), dict(counts=None), dict(tbox=None), dict(tint=None), dict(issued=None), dict(ids=None), dict(n=None), dict(S=0), dict(S=-1),
            dict(S=65536), dict(F=0), dict(F=-2), dict(F=4097), dict(R=0), dict(R=-1), dict(T=0), dict(T=-1), dict(T=1025), dict(ncls=0), dict(ncls=-1),
            dict(ncls=4097), dict(ncls=4096, R=1 << 20), dict(n_max=-1), dict(ss=-1), dict(fs=-70), dict(max_age=-1), dict(min_hits=0), dict(min_hits=-1),
            dict(st=nan), dict(st=inf), dict(it=nan), dict(it=-inf)]]
    bad += [(plan_ids, "lsfa_overlay_plan_ids", o) for o in
            [dict(ids=None), dict(ncls=1), dict(ncls=0), dict(dets=None), dict(counts=None), dict(records=None), dict(n=None), dict(N=0), dict(N=65536),
             dict(R=0), dict(ncls=4097), dict(ncls=4096, R=1 << 20), dict(H=0), dict(W=65537), dict(mb=0), dict(mb=overlay.MAX_BOXES + 1), dict(t=0), dict(t=9),
             dict(z=-1), dict(z=5)]]
    for fn, name, o in bad:
        assert fn(**o) == -1, (name, o)
        assert name in L.lsfa_last_error().decode(), (name, o)
    torch.cuda.synchronize()
    assert all(torch.equal(bufs[k], before[k]) for k in bufs)
    # ... and the same buffers through well-formed calls; rows == NULL and row_n == NULL are no refusals
    for k in ("tbox", "tint", "issued"):
        bufs[k].zero_()
    bufs["dets"].copy_(t(np.broadcast_to(np.array((10.0, 10.0, 40.0, 40.0, 0.9)), (S, F, ncls, R, 5))))
    bufs["counts"].fill_(1)
    assert steps(rows=None) == 0 and steps(row_n=None) == 0 and steps(rows=None, row_n=None) == 0 and steps() == 0 and plan_ids() == 0
    torch.cuda.synchronize()
    assert bufs["issued"].tolist() == [ncls - 1] * S and bufs["n"][:, -1].tolist() == [[ncls - 1, ncls - 1, 0, 0]] * S
    assert bufs["pn"].tolist() == [[ncls - 1, ncls - 1]] * S


def test_every_refusal_of_the_wrappers_raises_before_a_launch(hip, tracks, overlay):
    ncls, R, T, S, F = 4, 8, 16, 2, 3
    E = hip.LsfaError
    for kw in (dict(ncls=0), dict(ncls=4097), dict(R=0), dict(max_tracks=0), dict(max_tracks=1025), dict(max_age=-1), dict(min_hits=0), dict(streams=0),
               dict(streams=65536), dict(frames=0), dict(frames=4097), dict(score_thresh=float("nan")), dict(iou_thresh=float("inf")), dict(max_tracks=2.0),
               dict(ncls=4096, R=1 << 20)):
        with pytest.raises(E, match="Tracker"):
            tracks.Tracker(**dict(dict(ncls=ncls, R=R, device=DEV), **kw))
    tr = tracks.Tracker(ncls, R, max_tracks=T, streams=S, frames=F, device=DEV)
    one = tracks.Tracker(ncls, R, max_tracks=T, device=DEV)
    dets, counts = torch.zeros((S, F, ncls, R, 5), dtype=torch.float64, device=DEV), torch.zeros((S, F, ncls), dtype=torch.int32, device=DEV)
    rows, row_n = torch.zeros((S, F, 10, 7), dtype=torch.int32, device=DEV), torch.zeros((S, F), dtype=torch.int32, device=DEV)
    wide = torch.zeros((S, F, 10, 8), dtype=torch.int32, device=DEV)
    bad = [dict(dets=dets.float()), dict(dets=dets.cpu()), dict(dets=dets[:, :2]), dict(dets=dets[..., :4]), dict(dets=dets.transpose(0, 1).contiguous().transpose(0, 1)),
           dict(dets=None), dict(counts=counts.long()), dict(counts=counts.cpu()), dict(counts=counts[0]), dict(rows=rows.long()), dict(rows=rows.cpu()),
           dict(rows=rows[0]), dict(rows=rows[:, :2]), dict(rows=rows[..., :6]), dict(rows=wide[..., :7]), dict(rows=rows.transpose(2, 3).contiguous().transpose(2, 3)),
           dict(rows=rows[:, :, :0]), dict(rows=None), dict(row_n=row_n.long()), dict(row_n=row_n.cpu()), dict(row_n=row_n[0]), dict(row_n=row_n.t().contiguous().t())]
    for o in bad:
        a = dict(dict(dets=dets, counts=counts, rows=rows, row_n=row_n), **o)
        if o == dict(rows=None):
            a["row_n"] = row_n                            # row_n without rows
        with pytest.raises(E, match="Tracker.steps"):
            tr.steps(a["dets"], a["counts"], a["rows"], a["row_n"])
    with pytest.raises(E, match="Tracker.step"):
        tr.step(dets[0, 0], counts[0, 0])                 # made for two streams
    for o in (dict(dets=dets[0]), dict(counts=counts[0, 0].float()), dict(rows=rows[0]), dict(rows=wide[0, 0, :, :7]), dict(row_n=row_n[0])):
        a = dict(dict(dets=dets[0, 0], counts=counts[0, 0], rows=rows[0, 0], row_n=None), **o)
        with pytest.raises(E, match="Tracker.step"):
            one.step(a["dets"], a["counts"], a["rows"], a["row_n"])
    # a state tensor or an output that was replaced by something else
    for name, other in (("tbox", tr.tbox.transpose(1, 2).contiguous().transpose(1, 2)), ("tbox", tr.tbox.float()), ("tint", tr.tint[:, :, :3]),
                        ("issued", tr.issued.cpu()), ("ids", tr.ids[:, :, :, :4]), ("n", tr.n.long())):
        keep = getattr(tr, name)
        setattr(tr, name, other)
        with pytest.raises(E, match=name):
            tr.steps(dets, counts)
        setattr(tr, name, keep)
    for stream in (-1, S, 1.0, True):
        with pytest.raises(E, match="reset"):
            tr.reset(stream)
    torch.cuda.synchronize()
    assert not any(x.any() for x in tr.state()) and not any(x.any() for x in one.state()) and not tr.stats().any()
    tr.steps(dets, counts, rows, row_n)                   # the well-formed call goes through
    tr.reset(1)
    # Overlay: ids of the wrong kind
    ov = overlay.Overlay(ncls, R, device=DEV, batch=2)
    frame = torch.zeros((2, 20, 30, 3), dtype=torch.uint8, device=DEV)
    ids = torch.ones((2, ncls, R), dtype=torch.int32, device=DEV)
    d2, c2 = dets[:, 0].contiguous(), counts[:, 0].contiguous()
    y, uv = torch.zeros((2, 20, 30), dtype=torch.uint8, device=DEV), torch.zeros((2, 10, 30), dtype=torch.uint8, device=DEV)
    for other in (ids.long(), ids.cpu(), ids[0], ids[:, :, :4], ids.transpose(1, 2).contiguous().transpose(1, 2)):
        with pytest.raises(E, match="ids"):
            ov.draw_bgr(frame, d2, c2, 0.5, ids=other)
        with pytest.raises(E, match="ids"):
            ov.draw_yuv420(y, d2, c2, 0.5, uv=uv, ids=other)
    with pytest.raises(E, match="2 classes"):
        overlay.Overlay(1, R, device=DEV).draw_bgr(frame[0], dets[0, 0, :1], counts[0, 0, :1], 0.5, ids=ids[0, :1])
    torch.cuda.synchronize()
    assert not frame.any() and not y.any() and not uv.any() and not ov.drawn().any()


# ---- 7: the demo ----------------------------------------------------------------------------------------------------------------------------
def test_demo_tracks_an_nv12_file(hip, tmp_path):
    import json

    import ref_yuv
    from lsfa_amd import demo
    from lsfa_amd.config.config import lsfa_test_config
    ncls = int(lsfa_test_config().dataset.NUM_CLASSES)
    width, height, frames = 96, 64, 3
    rs = np.random.RandomState(9)
    planes = [ref_yuv.forward(rs.randint(0, 256, (height // 8, width // 8, 3)).astype(np.uint8).repeat(8, 0).repeat(8, 1)) for _ in range(frames)]
    src = tmp_path / "clip.nv12"
    src.write_bytes(b"".join(ref_yuv.raw_frame_bytes(y, u, v, "nv12") for y, u, v in planes))
    common = ["--yuv", str(src), "--size", "%dx%d" % (width, height), "--score", "0.05", "--no-graph", "--track"]
    out = tmp_path / "tracks.json"
    demo.main(common + ["--track-iou", "0.2", "--track-max-age", "1", "--track-slots", "64", "--out", str(out)])
    results = json.loads(out.read_text())
    assert sum(len(r["dets"]) for r in results) > 0
    want = None
    for r in results:
        dets, counts = og.dets_of_json(r["dets"], ncls)
        if want is None or want.R != dets.shape[1]:
            state = None if want is None else want.state()
            want = ref.Tracker(ncls, dets.shape[1], max_tracks=64, score_thresh=0.05, iou_thresh=0.2, max_age=1)
            if state is not None:
                want.tbox[:], want.tint[:], want.issued[:] = state
        ids, _ = want.step(dets, counts)
        seen = np.zeros(ncls, np.int32)
        for d in r["dets"]:
            assert d["track"] == ids[d["class"], seen[d["class"]]], (r["frame"], d)
            seen[d["class"]] += 1
    # with the estimator's rows and the ids drawn: one launch more a frame, the stream in the input's layout
    demo.main(common + ["--estimate-mv", "--draw-yuv", str(tmp_path / "out.nv12"), "--out", str(out)])
    raw = (tmp_path / "out.nv12").read_bytes()
    assert len(raw) == frames * width * height * 3 // 2 and raw != src.read_bytes()
    assert all("track" not in d for r in json.loads(out.read_text()) for d in r["dets"])
    for bad in (["--track-iou", "nan"], ["--track-max-age", "-1"], ["--track-min-hits", "0"], ["--track-slots", "0"], ["--track-slots", "1025"]):
        with pytest.raises(SystemExit):
            demo.parse_args(common + bad)
    with pytest.raises(SystemExit):
        demo.parse_args(common[:-1] + ["--track-slots", "8"])          # belongs to --track
