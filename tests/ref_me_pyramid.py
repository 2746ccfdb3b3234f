"""The numpy statement of the pyramid motion search (include/lsfa_hip.h, lsfa_luma_pyramid / lsfa_mv_refine_chain; DESIGN.md "Pyramid search"),
built on tests/ref_me.py: the top level IS ref_me.estimate on the smallest plane, every level below refines its parent's winner.  It is what
the device kernels are compared with bit for bit; tests/test_me_pyramid_cpu.py pins it by cases with a known answer.  Written for clarity:
one Python iteration per block and candidate, candidates visited in the order of the tie-break so that "strictly smaller cost replaces" is the
lexicographic minimum under (cost, |dx| + |dy|, dy, dx)."""
import numpy as np

import ref_me


def reach(levels, search, refine):
    """the longest vector component the mode can return, in pixels of level 0"""
    return search * 2 ** levels + refine * (2 ** levels - 1)


def down(p):
    """(h, w) uint8 -> (ceil(h / 2), ceil(w / 2)) uint8: (a + b + c + d + 2) >> 2 over the 2 x 2 taps, coordinates clamped to the plane"""
    h, w = p.shape
    ys, xs = 2 * np.arange(-(-h // 2)), 2 * np.arange(-(-w // 2))
    y1, x1 = np.minimum(ys + 1, h - 1), np.minimum(xs + 1, w - 1)
    q = p.astype(np.int32)
    return ((q[ys][:, xs] + q[ys][:, x1] + q[y1][:, xs] + q[y1][:, x1] + 2) >> 2).astype(np.uint8)


def pyramid(p0, levels):
    """[P_0, .., P_levels]: each level from the one below it, never from P_0"""
    out = [np.ascontiguousarray(p0)]
    for _ in range(levels):
        out.append(down(out[-1]))
    return out


def parent_vectors(rows):
    """rows (n, 7) -> (n, 2) int64 (dx, dy) = (src - dst): the winner a row carries"""
    rows = np.asarray(rows).astype(np.int64)
    return np.stack([rows[:, 3] - rows[:, 5], rows[:, 4] - rows[:, 6]], axis=1)


def refine(y_cur, y_ref, parent_rows, refine=2, lam=4, max_sad=0):
    """One refinement step on level k: (H, W) uint8 planes of level k and the rows of level k + 1 ((mbh_{k+1} * mbw_{k+1}, 7), block
    (bx, by)'s parent is (bx >> 1, by >> 1)) -> rows (mbh * mbw, 7) int32, sad (mbh, mbw) int32 of level k.  Candidates (2 pdx + ex,
    2 pdy + ey), (ex, ey) in [-refine, refine]^2, plus (0, 0); valid iff the covered rectangle shifted by the candidate lies inside the
    plane; cost = SAD + lam (|dx| + |dy|) on the absolute vector; max_sad > 0 zeroes a winner whose SAD exceeds it."""
    assert y_cur.dtype == np.uint8 and y_ref.dtype == np.uint8 and y_cur.shape == y_ref.shape and y_cur.ndim == 2
    assert 1 <= refine <= 3 and lam >= 0 and max_sad >= 0
    H, W = y_cur.shape
    r = int(refine)
    mbh, mbw = -(-H // 16), -(-W // 16)
    pmbh, pmbw = -(-(-(-H // 2)) // 16), -(-(-(-W // 2)) // 16)
    pv = parent_vectors(parent_rows)
    assert pv.shape == (pmbh * pmbw, 2), (pv.shape, pmbh, pmbw)
    cur, ref = y_cur.astype(np.int64), y_ref.astype(np.int64)
    rows = np.empty((mbh, mbw, 7), np.int32)
    sads = np.empty((mbh, mbw), np.int32)
    for by in range(mbh):
        for bx in range(mbw):
            x0, y0 = 16 * bx, 16 * by
            x1, y1 = min(x0 + 16, W) - 1, min(y0 + 16, H) - 1
            pdx, pdy = (int(v) for v in pv[(by >> 1) * pmbw + (bx >> 1)])
            cands = set((2 * pdx + ex, 2 * pdy + ey) for ey in range(-r, r + 1) for ex in range(-r, r + 1))
            cands.add((0, 0))
            block = cur[y0:y1 + 1, x0:x1 + 1]
            best = None
            for length, dy, dx in sorted((abs(dx) + abs(dy), dy, dx) for dx, dy in cands):
                if x0 + dx < 0 or x1 + dx > W - 1 or y0 + dy < 0 or y1 + dy > H - 1:
                    continue
                sad = int(np.abs(block - ref[y0 + dy:y1 + dy + 1, x0 + dx:x1 + dx + 1]).sum())
                cost = sad + lam * length
                if best is None or cost < best[0]:
                    best = (cost, sad, dx, dy)
            _, sad, dx, dy = best                   # (0, 0) is always valid
            sads[by, bx] = sad
            if max_sad > 0 and sad > max_sad:
                dx, dy = 0, 0
            rows[by, bx] = (-1, 16, 16, x0 + 8 + dx, y0 + 8 + dy, x0 + 8, y0 + 8)
    return rows.reshape(mbh * mbw, 7), sads


def estimate(y_cur, y_ref, levels=0, search=16, lam=4, max_sad=0, refine_radius=2, return_levels=False):
    """The mode as a whole: (H, W) uint8 planes -> rows (mbh * mbw, 7) int32, sad (mbh, mbw) int32 of level 0.  levels = 0 is
    ref_me.estimate.  With return_levels also [rows of level 0, .., rows of the top level]."""
    assert levels in (0, 1, 2)
    if levels == 0:
        rows, sad = ref_me.estimate(y_cur, y_ref, search, lam, max_sad)
        return (rows, sad, [rows]) if return_levels else (rows, sad)
    pc, pr = pyramid(y_cur, levels), pyramid(y_ref, levels)
    rows, sad = ref_me.estimate(pc[levels], pr[levels], search, lam, 0)
    per_level = [rows]
    for k in range(levels - 1, -1, -1):
        rows, sad = refine(pc[k], pr[k], rows, refine_radius, lam, max_sad if k == 0 else 0)
        per_level.insert(0, rows)
    return (rows, sad, per_level) if return_levels else (rows, sad)


def eligible(width, height, levels, v):
    """(mbh, mbw) bool: the level-0 blocks for which the block itself and its ancestors on levels 1 .. levels all have their covered
    rectangle, shifted by the candidate v / 2^k = (dx, dy) >> k (v a multiple of 2^levels), inside their planes"""
    assert v[0] % 2 ** levels == 0 and v[1] % 2 ** levels == 0
    mbh, mbw = -(-height // 16), -(-width // 16)
    ok = np.ones((mbh, mbw), bool)
    w, h = width, height
    for k in range(levels + 1):
        dx, dy = v[0] // 2 ** k, v[1] // 2 ** k
        for by in range(mbh):
            for bx in range(mbw):
                ax, ay = bx >> k, by >> k
                x0, y0 = 16 * ax, 16 * ay
                x1, y1 = min(x0 + 16, w) - 1, min(y0 + 16, h) - 1
                ok[by, bx] &= x0 + dx >= 0 and x1 + dx <= w - 1 and y0 + dy >= 0 and y1 + dy <= h - 1
        w, h = -(-w // 2), -(-h // 2)
    return ok


def shifted_pair(width, height, m, seed=0):
    """two (H, W) uint8 white-noise planes (ref, cur) cut out of one world; the content moves by m = (mx, my) from ref to cur:
    cur[y, x] = ref[y - my, x - mx] wherever both lie inside, so the block vector src - dst is -m and ref_me.vectors gives m"""
    rs = np.random.RandomState(seed)
    mx, my = m
    world = rs.randint(0, 256, (height + 2 * abs(my), width + 2 * abs(mx))).astype(np.uint8)
    ref = world[abs(my):abs(my) + height, abs(mx):abs(mx) + width]
    cur = world[abs(my) - my:abs(my) - my + height, abs(mx) - mx:abs(mx) - mx + width]
    return np.ascontiguousarray(ref), np.ascontiguousarray(cur)


# the known answer beyond the full search's reach (tests/test_me_pyramid_cpu.py, tests/test_me_pyramid_gpu.py)
KNOWN = dict(width=256, height=192, m=(44, -24), levels=2, search=12, refine=2, lam=4, seed=5)


def known_answer_case():
    """(ref plane, cur plane, eligible (mbh, mbw) bool): white noise translated by m = (44, -24).  Every level is a multiple of 64, so no tap
    is clamped; both shifts are multiples of 4, so away from the frame edge every level of the shifted frame is the shifted level and the true
    candidate has SAD 0 on every level.  The content moves by m, so the block vector src - dst is -m and ref_me.vectors gives m."""
    k = KNOWN
    ref, cur = shifted_pair(k['width'], k['height'], k['m'], seed=k['seed'])
    return ref, cur, eligible(k['width'], k['height'], k['levels'], (-k['m'][0], -k['m'][1]))
