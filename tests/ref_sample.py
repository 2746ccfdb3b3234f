"""An independent statement of the two bilinear samplers, and coordinate fields that sit on their index decisions.

Plain numpy; nothing here goes through the oracle's shared library.  Used by tests/test_sample_edges_{cpu,gpu}.py.

  warp_ref      GridGenerator 'warp' + BilinearSampler as oracle/lsfa_oracle.c states them (orc_warp_bilinear), with the fused epilogue
                in the kernels' order: * mul, + rnet_conv0(res), * bn scale, + bn shift, + add.
  deform_ref    DeformableConvolution's im2col (orc_deform_im2col / dcn_bilinear): zero outside [0, H) x [0, W), the last row and column
                clamped, four weights.

Each has two forms.  `*_f32`: every operation on np.float32 arrays in the order the C text writes them; numpy never fuses a product into
a sum, which is -ffp-contract=off, so the result is comparable bit for bit.  `*_f64`: the sampling itself - corner choice, weights, the
four-term sum, the epilogue - in float64, used only to bound the f32 form.  Both forms sample at the SAME point: the coordinate is
float32 arithmetic in both (warp_coord, deform_coord).  The warp's round trip through the normalised grid moves a coordinate by a few
ulp of the map's width (test_sample_edges_cpu.py bounds that on its own), which times the gradient of a random feature is a hundred
times the rounding of the four-term sum; a float64 round trip would compare two different sample points, not two roundings of one sum.

classify() names the position of a coordinate relative to an axis' index decisions; edge_field() builds flows / offsets whose
coordinates, recomputed in float32, land in every class that can be reached."""
import collections

import numpy as np

F32 = np.float32
_ONE, _TWO = F32(1), F32(2)

CLASSES = ("int_interior", "zero", "neg_zero", "below_zero_1ulp", "band_lo", "minus_one", "below_minus_one", "last", "above_last_1ulp",
           "band_hi", "below_L_1ulp", "at_L", "beyond_L", "frac_interior", "wild", "nonfinite")
# the classes next to an index decision at either end of the axis: every pair of them (x class, y class) gets a cell of its own
BORDER = ("zero", "neg_zero", "below_zero_1ulp", "band_lo", "minus_one", "below_minus_one", "last", "above_last_1ulp", "band_hi",
          "below_L_1ulp", "at_L", "beyond_L")
WILD = 2.0 ** 31


def classify(u, L):
    """The edge class of each float32 coordinate `u` along an axis of length L (an array of names, shaped like u).

    int_interior     an integer in [1, L - 2]                     frac_interior    any other value in (0, L - 1)
    zero / neg_zero  +0.0 / -0.0                                  last             L - 1
    below_zero_1ulp  [-spacing(L), 0): below zero by no more than the spacing of float32 at the axis' own scale - the closest a
                     coordinate formed at that scale comes to zero - down to the smallest subnormal, which is where a flush to zero shows
    band_lo          the rest of (-1, 0)                          band_hi          the rest of (L - 1, L)
    minus_one        -1                                           at_L             L
    below_minus_one  (-2^31, -1)                                  beyond_L         (L, 2^31)
    above_last_1ulp  the float32 after L - 1                      below_L_1ulp     the float32 before L
    wild             finite, |u| >= 2^31 (an int conversion of it is undefined), up to FLT_MAX
    nonfinite        +-inf or NaN"""
    u = np.asarray(u, F32)
    Lf = F32(L)
    with np.errstate(invalid="ignore"):
        integer = np.floor(u) == u
        conds = [
            (~np.isfinite(u), "nonfinite"),
            (np.abs(u) >= F32(WILD), "wild"),
            (u > Lf, "beyond_L"),
            (u == Lf, "at_L"),
            (u == np.nextafter(Lf, F32(-np.inf)), "below_L_1ulp"),
            (u == np.nextafter(Lf - _ONE, F32(np.inf)), "above_last_1ulp"),
            (u > Lf - _ONE, "band_hi"),
            (u == Lf - _ONE, "last"),
            ((u == 0) & ~np.signbit(u), "zero"),
            ((u == 0) & np.signbit(u), "neg_zero"),
            ((u < 0) & (u >= -np.spacing(Lf)), "below_zero_1ulp"),
            ((u < 0) & (u > -_ONE), "band_lo"),
            (u == -_ONE, "minus_one"),
            (u < -_ONE, "below_minus_one"),
            (integer, "int_interior"),
        ]
    out = np.full(u.shape, "frac_interior", dtype="U16")
    for cond, name in reversed(conds):
        out[cond] = name
    return out


# ---- the coordinates: float32 in both forms -------------------------------------------------------------------------------------------------
def warp_coord(p, f, L):
    """x_real of pixel index p moved by the flow f on an axis of length L: the round trip through the normalised grid, float32 throughout
    (oracle/lsfa_oracle.c: gx = (x + fx) / half_w - 1; x_real = (gx + 1) * (W - 1) / 2)."""
    p, f = np.asarray(p, F32), np.asarray(f, F32)
    half = F32((L - 1) / 2.0)
    with np.errstate(all="ignore"):
        g = (p + f) / half - _ONE
        return (g + _ONE) * F32(L - 1) / _TWO


def warp_coord_f64(p, f, L):
    """the same formula in float64 (only to bound warp_coord)"""
    p, f = np.asarray(p, np.float64), np.asarray(f, np.float64)
    with np.errstate(all="ignore"):
        g = (p + f) / ((L - 1) / 2.0) - 1.0
        return (g + 1.0) * (L - 1) / 2.0


def deform_coord(b, f):
    """the tap's coordinate: (float)(ho * stride - pad + i * dilate) + offset, one float32 addition"""
    with np.errstate(all="ignore"):
        return np.asarray(b, F32) + np.asarray(f, F32)


def warp_coords(flow):
    """(x_real, y_real), each (N, H, W) float32"""
    flow = np.asarray(flow, F32)
    N, _, H, W = flow.shape
    xs = np.arange(W, dtype=F32)[None, None, :]
    ys = np.arange(H, dtype=F32)[None, :, None]
    return warp_coord(xs, flow[:, 0], W), warp_coord(ys, flow[:, 1], H)


def deform_bases(L_out, k, pad, stride, dil):
    """(k, L_out) int: the integer part of a tap's coordinate along one axis"""
    return np.arange(L_out)[None, :] * stride - pad + np.arange(k)[:, None] * dil


def deform_coords(offset, H, W, k, pad, stride, dil, dg):
    """offset (N, 2 * k * k * dg, Ho, Wo) -> (h, w), each (N, dg, k*k, Ho, Wo) float32"""
    offset = np.asarray(offset, F32)
    N, _, Ho, Wo = offset.shape
    off = offset.reshape(N, dg, k * k, 2, Ho, Wo)
    bh = np.repeat(deform_bases(Ho, k, pad, stride, dil), k, axis=0)           # tap = i * k + j: i changes slowest
    bw = np.tile(deform_bases(Wo, k, pad, stride, dil), (k, 1))
    h = deform_coord(bh.astype(F32)[None, None, :, :, None], off[:, :, :, 0])
    w = deform_coord(bw.astype(F32)[None, None, :, None, :], off[:, :, :, 1])
    return h, w


# ---- the warp -----------------------------------------------------------------------------------------------------------------------------------
def _corner(real, L, dt):
    """floor, the clamped integer index, the two weights and the two validity masks of one axis"""
    real = real.astype(dt)
    with np.errstate(all="ignore"):
        f0 = np.floor(real)
        # clamped to [-2, L] before the integer conversion, as the kernels do: outside the map either way, and defined for every float
        # (fmax / fmin drop a NaN, like fmaxf / fminf: NaN -> -2)
        i0 = np.fmin(np.fmax(f0, dt(-2)), dt(L)).astype(np.int64)
        w0 = dt(1) - (real - f0)
        w1 = dt(1) - w0
    v0 = (i0 >= 0) & (i0 <= L - 1)
    v1 = (i0 + 1 >= 0) & (i0 + 1 <= L - 1)
    return i0, w0, w1, v0, v1


def warp_ref(feat, flow, mul=None, add=None, res=None, bn=None, dtype=F32):
    """feat (feat_n, C, H, W): map n samples feature n mod feat_n; flow (N, 2, H, W); mul, add (N, C, H, W); res = (res (N, rc, H, W),
    res_w (C, rc), res_b (C)); bn = (scale (C), shift (C)) -> (N, C, H, W) in `dtype`."""
    dt = dtype
    feat, flow = np.asarray(feat, F32), np.asarray(flow, F32)
    N, _, H, W = flow.shape
    feat_n, C = feat.shape[:2]
    x_real, y_real = warp_coords(flow)
    x0, wx0, wx1, vx0, vx1 = _corner(x_real, W, dt)
    y0, wy0, wy1, vy0, vy1 = _corner(y_real, H, dt)
    fsel = feat[np.arange(N) % feat_n].astype(dt)                              # (N, C, H, W)
    n_idx = np.arange(N)[:, None, None]

    def tap(yi, xi, valid):
        v = fsel[n_idx, :, np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)]       # (N, H, W, C)
        return np.where(valid[..., None], v, dt(0)).transpose(0, 3, 1, 2)
    tl, tr = tap(y0, x0, vy0 & vx0), tap(y0, x0 + 1, vy0 & vx1)
    bl, br = tap(y0 + 1, x0, vy1 & vx0), tap(y0 + 1, x0 + 1, vy1 & vx1)
    wx0, wx1, wy0, wy1 = (a[:, None] for a in (wx0, wx1, wy0, wy1))
    with np.errstate(all="ignore"):
        v = tl * wy0 * wx0 + tr * wy0 * wx1 + bl * wy1 * wx0 + br * wy1 * wx1
        if mul is not None:
            v = v * np.asarray(mul, F32).astype(dt)
        if res is not None:
            r, rw, rb = (np.asarray(a, F32).astype(dt) for a in res)
            rw = rw.reshape(C, -1)
            q = rw[None, :, 0, None, None] * r[:, None, 0]
            for k in range(1, r.shape[1]):
                q = q + rw[None, :, k, None, None] * r[:, None, k]
            q = q + rb[None, :, None, None]
            v = v + q
        if bn is not None:
            s, t = (np.asarray(a, F32).astype(dt) for a in bn)
            v = v * s[None, :, None, None]
            v = v + t[None, :, None, None]
        if add is not None:
            v = v + np.asarray(add, F32).astype(dt)
    assert v.dtype == dt
    return v


def warp_ref_f32(feat, flow, **kw):
    return warp_ref(feat, flow, dtype=F32, **kw)


def warp_ref_f64(feat, flow, **kw):
    return warp_ref(feat, flow, dtype=np.float64, **kw)


def warp_zero_sample(shape, mul=None, add=None, res=None, bn=None):
    """what the epilogue makes of a sample that is exactly zero, (N, C, H, W) float32"""
    N, C, H, W = shape
    return warp_ref_f32(np.zeros((1, C, H, W), F32), np.zeros((N, 2, H, W), F32), mul=mul, add=add, res=res, bn=bn)


# ---- the deformable sampler ---------------------------------------------------------------------------------------------------------------------
def deform_ref(data, offset, k, pad, stride, dil, dg, dtype=F32):
    """data (N, C, H, W), offset (N, 2 * k * k * dg, Ho, Wo) -> col (N, C * k * k, Ho * Wo) in `dtype`"""
    dt = dtype
    data, offset = np.asarray(data, F32), np.asarray(offset, F32)
    N, C, H, W = data.shape
    Ho, Wo = offset.shape[2:]
    KK, cpg = k * k, C // dg
    h32, w32 = deform_coords(offset, H, W, k, pad, stride, dil, dg)              # (N, dg, KK, Ho, Wo)
    with np.errstate(invalid="ignore"):
        inside = (h32 >= 0) & (w32 >= 0) & (h32 < H) & (w32 < W)                  # false for NaN: the guard runs before any conversion
    h, w = np.where(inside, h32, F32(0)).astype(dt), np.where(inside, w32, F32(0)).astype(dt)
    h_low, w_low = np.floor(h).astype(np.int64), np.floor(w).astype(np.int64)
    # the last row / column: both corners on it, and the coordinate moved onto it
    ch, cw = h_low >= H - 1, w_low >= W - 1
    h_low, w_low = np.where(ch, H - 1, h_low), np.where(cw, W - 1, w_low)
    h_high, w_high = np.where(ch, H - 1, h_low + 1), np.where(cw, W - 1, w_low + 1)
    h, w = np.where(ch, h_low.astype(dt), h), np.where(cw, w_low.astype(dt), w)
    lh, lw = h - h_low.astype(dt), w - w_low.astype(dt)
    hh, hw = dt(1) - lh, dt(1) - lw
    w1, w2, w3, w4 = hh * hw, hh * lw, lh * hw, lh * lw
    d = data.astype(dt).reshape(N, dg, cpg, H, W)
    n_idx, g_idx = np.arange(N)[:, None, None, None, None], np.arange(dg)[None, :, None, None, None]

    def tap(hi, wi):
        return d[n_idx, g_idx, :, hi, wi]                                         # (N, dg, KK, Ho, Wo, cpg)
    e = lambda a: a[..., None]
    val = e(w1) * tap(h_low, w_low) + e(w2) * tap(h_low, w_high) + e(w3) * tap(h_high, w_low) + e(w4) * tap(h_high, w_high)
    val = np.where(e(inside), val, dt(0))
    assert val.dtype == dt
    return np.ascontiguousarray(val.transpose(0, 1, 5, 2, 3, 4)).reshape(N, C * KK, Ho * Wo)


def deform_ref_f32(data, offset, k, pad, stride, dil, dg):
    return deform_ref(data, offset, k, pad, stride, dil, dg, dtype=F32)


def deform_ref_f64(data, offset, k, pad, stride, dil, dg):
    return deform_ref(data, offset, k, pad, stride, dil, dg, dtype=np.float64)


# ---- fdiv24 (lsfa_amd/csrc/dcn.hip) ---------------------------------------------------------------------------------------------------------------
def fdiv24(n, d):
    """n / d as the power-of-two deformable kernel forms it: a float32 product with the host's 1.0f / d, then one correction step either
    way from the remainder.  n: an int32 array of values in [0, 2^24)."""
    n = np.asarray(n, np.int32)
    inv = F32(1) / F32(d)
    q = (n.astype(F32) * inv).astype(np.int32)
    r = n - q * np.int32(d)
    q = q + (r >= d).astype(np.int32)
    q = q - (r < 0).astype(np.int32)
    return q


# ---- fields on the edges ------------------------------------------------------------------------------------------------------------------------
def _steps(f, n=4):
    """f and the n float32 values on either side of it"""
    out, lo, hi = [F32(f)], F32(f), F32(f)
    for _ in range(n):
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
        out += [lo, hi]
    return np.array(out, F32)


_NONFINITE = (np.inf, -np.inf, np.nan, np.finfo(F32).max, -np.finfo(F32).max)
_WILD = (3e9, -3e9, 2.0 ** 31, -2.0 ** 31, 1e20, -1e30, 1.5e38, -1.5e38, 3e38, -3e38)


def _targets(cls, L, rs):
    """coordinates to aim at for one class, the first the preferred one"""
    Lf = F32(L)
    if cls == "int_interior":
        return [float(rs.randint(1, L - 1))] if L >= 3 else []
    if cls == "frac_interior":
        return [float(rs.uniform(0.05, L - 1.05)) if L > 2 else float(rs.uniform(0.05, 0.95)), (L - 1) / 2.0 + 0.25]
    return {"zero": [0.0], "neg_zero": [-0.0], "below_zero_1ulp": [-2.0 ** -149, -float(np.spacing(Lf)) / 2, -float(np.spacing(Lf))],
            "band_lo": [-float(rs.uniform(0.1, 0.9))], "minus_one": [-1.0],
            "below_minus_one": [-1.0 - float(rs.uniform(0.1, 3.0)), -float(np.nextafter(_ONE, F32(2)))], "last": [L - 1.0],
            "above_last_1ulp": [float(np.nextafter(Lf - _ONE, F32(np.inf)))], "band_hi": [L - 1.0 + float(rs.uniform(0.1, 0.9))],
            "below_L_1ulp": [float(np.nextafter(Lf, F32(-np.inf)))], "at_L": [float(L)],
            "beyond_L": [L + float(rs.uniform(0.1, 3.0)), float(np.nextafter(Lf, F32(np.inf)))]}[cls]


def solve(chain, cls, p, L, rs):
    """A float32 f with classify(chain(p, f), L) == cls, or None.  For each coordinate aimed at, the candidates are the float32 values within
    4 steps of (target - p); the chain is recomputed in float32 for each and the first that lands in the class is kept."""
    if cls in ("wild", "nonfinite"):
        pool = _WILD if cls == "wild" else _NONFINITE
        cands = np.array([pool[i] for i in rs.permutation(len(pool))], F32)
    else:
        ts = _targets(cls, L, rs)
        if not ts:
            return None
        with np.errstate(all="ignore"):
            cands = np.concatenate([_steps(F32(np.float64(t) - np.float64(p))) for t in ts])
    hit = np.nonzero(classify(chain(np.full(cands.shape, p, F32), cands), L) == cls)[0]
    return cands[hit[0]] if hit.size else None


def _pairs_wanted():
    """(x class, y class): every pair of border classes, and every class against both interior classes on either side"""
    want = [(a, b) for a in BORDER for b in BORDER]
    for c in CLASSES:
        for i in ("int_interior", "frac_interior"):
            want += [(c, i), (i, c)]
    want += [("wild", "wild"), ("wild", "nonfinite"), ("nonfinite", "wild"), ("nonfinite", "nonfinite"), ("wild", "zero"), ("last", "wild"),
             ("nonfinite", "last"), ("zero", "nonfinite")]
    return want


def _counts(cu, cv):
    return {"x": collections.Counter(cu.ravel().tolist()), "y": collections.Counter(cv.ravel().tolist()),
            "pairs": set(zip(cu.ravel().tolist(), cv.ravel().tolist()))}


def warp_edge_field(H, W, rs, nonfinite=True):
    """flow (K, 2, H, W) float32, K even, and the counts of the classes its coordinates fall in ({'x': Counter, 'y': Counter, 'pairs':
    set of (x class, y class)}), recomputed from the flow.  Every class the round trip can reach at this width / height stands on each
    axis, each reachable pair of _pairs_wanted() in a cell of its own; the other cells hold whole-pixel flows in [-2, 2] (the lattice).
    nonfinite=False: the cells that would hold a non-finite coordinate hold a wild one."""
    chain = {0: lambda p, f: warp_coord(p, f, W), 1: lambda p, f: warp_coord(p, f, H)}
    size = (W, H)

    def table(axis):
        return {c: {p: solve(chain[axis], c, p, size[axis], rs) for p in range(size[axis])} for c in CLASSES}
    tx, ty = table(0), table(1)
    maps, used = [], []

    def new_map():
        maps.append(rs.randint(-2, 3, (2, H, W)).astype(F32))
        used.append(np.zeros((H, W), bool))
    new_map()
    for cx, cy in _pairs_wanted():
        if not nonfinite:
            cx, cy = ("wild" if c == "nonfinite" else c for c in (cx, cy))
        xs = [p for p, f in tx[cx].items() if f is not None]
        ys = [p for p, f in ty[cy].items() if f is not None]
        if not xs or not ys:
            continue
        for m in range(len(maps) + 1):
            if m == len(maps):
                new_map()
            free = [(y, x) for y in ys for x in xs if not used[m][y, x]]
            if free:
                y, x = free[rs.randint(len(free))]
                maps[m][0, y, x], maps[m][1, y, x] = tx[cx][x], ty[cy][y]
                used[m][y, x] = True
                break
    if len(maps) % 2:
        new_map()
    flow = np.stack(maps).astype(F32)
    xr, yr = warp_coords(flow)
    return flow, _counts(classify(xr, W), classify(yr, H))


def deform_edge_field(H, W, rs, k, pad, stride, dil, dg):
    """offset (N, 2 * k * k * dg, Ho, Wo) float32 on the convolution's output grid and the counts as in warp_edge_field, with 'by_tap' and
    'by_group': class -> the set of taps / deformable groups it occurs in (either axis).  The offset of a cell is target - base in float32,
    kept only if base + offset, recomputed in float32, lands in the class (so a class is placed where its base lets it be hit: the
    smallest subnormal below zero only where the base is 0).  The wanted pairs are laid out twice, in taps [0, 4) of group 0 and in taps
    [4, k * k) of the last group; the other cells hold whole-pixel offsets in [-2, 2]."""
    span = dil * (k - 1) + 1
    Ho, Wo = (H + 2 * pad - span) // stride + 1, (W + 2 * pad - span) // stride + 1
    KK = k * k
    bh, bw = deform_bases(Ho, k, pad, stride, dil), deform_bases(Wo, k, pad, stride, dil)       # (k, Ho), (k, Wo)
    memo = {}

    def sol(cls, b, L):
        if (cls, b, L) not in memo:
            memo[(cls, b, L)] = solve(deform_coord, cls, b, L, rs)
        return memo[(cls, b, L)]
    imgs, used = [], []

    def new_img():
        imgs.append(rs.randint(-2, 3, (dg, KK, 2, Ho, Wo)).astype(F32))
        used.append(np.zeros((dg, KK, Ho, Wo), bool))
    new_img()
    for taps, g in ((range(0, 4), 0), (range(4, KK), dg - 1)):
        for cw_, ch_ in _pairs_wanted():
            cells = []
            for tap in taps:
                i, j = divmod(tap, k)
                hs = [ho for ho in range(Ho) if sol(ch_, int(bh[i, ho]), H) is not None]
                ws = [wo for wo in range(Wo) if sol(cw_, int(bw[j, wo]), W) is not None]
                cells += [(tap, ho, wo) for ho in hs for wo in ws]
            if not cells:
                continue
            for m in range(len(imgs) + 1):
                if m == len(imgs):
                    new_img()
                free = [c for c in cells if not used[m][g, c[0], c[1], c[2]]]
                if free:
                    tap, ho, wo = free[rs.randint(len(free))]
                    i, j = divmod(tap, k)
                    imgs[m][g, tap, 0, ho, wo] = sol(ch_, int(bh[i, ho]), H)
                    imgs[m][g, tap, 1, ho, wo] = sol(cw_, int(bw[j, wo]), W)
                    used[m][g, tap, ho, wo] = True
                    break
        # one step below zero in the strictest sense: the smallest subnormal, where the tap's integer part is 0, on either axis (the other
        # axis keeps its whole-pixel offset)
        for axis, base in ((0, bh), (1, bw)):
            at0 = [(tap, ho, wo) for tap in taps for ho in range(Ho) for wo in range(Wo)
                   if (base[tap // k, ho] if axis == 0 else base[tap % k, wo]) == 0]
            for m in range(len(imgs) + 1 if at0 else 0):
                if m == len(imgs):
                    new_img()
                free = [c for c in at0 if not used[m][g, c[0], c[1], c[2]]]
                if free:
                    tap, ho, wo = free[rs.randint(len(free))]
                    imgs[m][g, tap, axis, ho, wo] = F32(-2.0 ** -149)
                    used[m][g, tap, ho, wo] = True
                    break
    offset = np.stack(imgs).astype(F32).reshape(len(imgs), 2 * KK * dg, Ho, Wo)
    h, w = deform_coords(offset, H, W, k, pad, stride, dil, dg)
    ch, cw = classify(h, H), classify(w, W)
    counts = _counts(cw, ch)
    counts["by_tap"] = collections.defaultdict(set)
    counts["by_group"] = collections.defaultdict(set)
    for g in range(dg):
        for tap in range(KK):
            for c in set(ch[:, g, tap].ravel().tolist()) | set(cw[:, g, tap].ravel().tolist()):
                counts["by_tap"][c].add(tap)
                counts["by_group"][c].add(g)
    return offset, counts


def edge_field(H, W, rs, sampler="warp", **cfg):
    """(field, counts): warp_edge_field(H, W, rs, **cfg) or deform_edge_field(H, W, rs, k=, pad=, stride=, dil=, dg=)"""
    return warp_edge_field(H, W, rs, **cfg) if sampler == "warp" else deform_edge_field(H, W, rs, **cfg)


# ---- the cases both test files use: built once per shape, never written to ------------------------------------------------------------------------
SHAPES = ((7, 5), (9, 16), (2, 2), (6, 63))             # smallest general case; width a multiple of 4; all border; the network's odd width
CHANNELS = (16, 12)                                      # power-of-two channels-last kernel and staged warp; the general channels-last kernel
DEFORM_CFGS = ((1, 1, 1, 1), (2, 1, 2, 4), (1, 2, 1, 4))  # (pad, stride, dilate, deformable groups), k = 3
_cases = {}


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def warp_case(hw, C):
    """flow (K, 2, H, W) of warp_edge_field, the same field with its non-finite cells made wild ('flow_wild'), two features and the
    epilogue's operands for K maps"""
    if ("warp", hw, C) not in _cases:
        H, W = hw
        flow, counts = warp_edge_field(H, W, np.random.RandomState(1000 * H + 10 * W))              # (the field does not depend on C)
        flow_wild, counts_wild = warp_edge_field(H, W, np.random.RandomState(1000 * H + 10 * W), nonfinite=False)
        rs = np.random.RandomState(1000 * H + 10 * W + C)
        K = max(flow.shape[0], flow_wild.shape[0])
        f = lambda *s: rs.randn(*s).astype(F32)
        _cases[("warp", hw, C)] = _frozen(dict(
            flow=flow, counts=counts, flow_wild=flow_wild, counts_wild=counts_wild, feat=f(2, C, H, W), mul=(1 + 0.1 * f(K, C, H, W)).astype(F32),
            add=f(K, C, H, W), res=(4 * f(K, 3, H, W)).astype(F32), res_w=(0.01 * f(C, 3)).astype(F32), res_b=(0.01 * f(C)).astype(F32),
            bn_s=(rs.rand(C) + 0.5).astype(F32), bn_t=f(C)))
    return _cases[("warp", hw, C)]


def warp_classes(flow):
    """(x class, y class) of every cell, and the masks `nonfinite` (either axis) and `zero_sample` (no NaN weight, and no tap inside the map
    on at least one axis: the sample is exactly zero)"""
    _, _, H, W = flow.shape
    xr, yr = warp_coords(flow)
    cx, cy = classify(xr, W), classify(yr, H)
    nonfinite = (cx == "nonfinite") | (cy == "nonfinite")
    out = ("below_minus_one", "at_L", "beyond_L", "wild")
    zero_sample = ~nonfinite & (np.isin(cx, out) | np.isin(cy, out))
    return cx, cy, nonfinite, zero_sample


def warp_operands(case, subset, sl=slice(None)):
    """the keyword operands of warp_ref for a subset name made of 'mul', 'add', 'res', 'bn' joined by '+', or 'plain'; sl: the maps taken"""
    kw = {}
    for name in ([] if subset == "plain" else subset.split("+")):
        if name in ("mul", "add"):
            kw[name] = case[name][sl]
        elif name == "res":
            kw["res"] = (case["res"][sl], case["res_w"], case["res_b"])
        elif name == "bn":
            kw["bn"] = (case["bn_s"], case["bn_t"])
    return kw


def deform_case(hw, C, cfg):
    if ("deform", hw, C, cfg) not in _cases:
        H, W = hw
        pad, stride, dil, dg = cfg
        offset, counts = deform_edge_field(H, W, np.random.RandomState(1000 * H + 10 * W + 7 * pad + dg), 3, pad, stride, dil, dg)
        rs = np.random.RandomState(1000 * H + 10 * W + C + 7 * pad + dg)                              # (the field does not depend on C)
        _cases[("deform", hw, C, cfg)] = _frozen(dict(offset=offset, counts=counts, data=rs.randn(offset.shape[0], C, H, W).astype(F32)))
    return _cases[("deform", hw, C, cfg)]
