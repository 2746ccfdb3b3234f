"""The shapes and the inputs of tests/test_stem_edges_gpu.py, made on the CPU from fixed seeds, so that tests/test_stem_edges_cpu.py
can hold the reference's own emulation to the bound on the same inputs and the geometry predicates are stated once (ref_stem.geometry).
Every generator returns a dict of float32 numpy arrays: x (N, 3, H, W), w (64, 3, 7, 7), bias (64), in_scale / in_shift (3),
accum (N, Ho, Wo, 64)."""
import numpy as np

import ref_stem

f32 = ref_stem.f32

# ---- 1. borders and ragged tiles: (N, H, W).  H covers Ho % 4 = 1, 1, 2, 3, 0, 0, 1 (odd and even rows), W gives Wo = 1, 1, 4, 31, 32,
# 32, 33, 33, 35; the widths 62..70 put the right image border inside the patch columns 64..69 that threads t < 252 stage
BORDER_H = (1, 2, 4, 6, 7, 8, 9)
BORDER_W = (1, 2, 7, 62, 63, 64, 65, 66, 70)
BORDER_SHAPES = [(1, 1, 1), (2, 1, 70), (1, 9, 1), (1, 2, 2), (2, 4, 7), (1, 6, 62), (2, 7, 63), (1, 8, 64), (1, 9, 65), (2, 6, 66),
                 (1, 7, 70), (1, 4, 64), (2, 8, 65)]

# ---- 3. the tile walk: name -> (N, H, W); the predicates are walk_predicate()
WALK_SHAPES = {
    "a_unused_slot_ragged": (37, 32, 400),
    "b_parity_returns_whole_row_end": (74, 24, 448),
    "c_tpw_divides_xt": (43, 47, 256),
}


def walk_predicate(name):
    """what the shape was chosen for, on ref_stem.geometry: asserted by both test files"""
    g = ref_stem.geometry(*WALK_SHAPES[name])
    assert g.xt * g.yt * g.N >= 1024 and g.tpw >= 2, (name, vars(g))
    assert g.N * g.Ho * g.Wo * 64 <= 16 << 20, (name, vars(g))
    last = g.xt - 1
    if name == "a_unused_slot_ragged":
        assert (g.xt, g.yt, g.tpw, g.grid_x) == (7, 4, 2, 4) and g.slots == g.xt + 1 and not g.whole(last), vars(g)
        assert g.walk(last)[1] == 0 and not g.more(last)              # the ragged tile opens a walk whose second slot breaks
    elif name == "b_parity_returns_whole_row_end":
        assert g.tpw >= 3 and g.Wo % 32 == 0 and g.slots > g.xt, vars(g)
        assert g.whole(last) and g.walk(last)[1] + 1 < g.tpw and not g.more(last)      # more == false by the row's end, on a whole tile
        assert any(g.walk(t)[1] == 2 for t in range(g.xt))            # a third tile of a walk: the exchange parity is 0 again
    else:
        assert g.xt % g.tpw == 0 and g.slots == g.xt, vars(g)
        assert g.walk(last)[1] + 1 == g.tpw and g.whole(last) and not g.more(last)     # more == false by t + 1 == tpw
    return g


def _weights(rs, decades):
    w = f32(rs.randn(64, 3, 7, 7) * 0.05)
    if decades:
        w = w * f32(np.exp(rs.uniform(-6, 6, 64)))[:, None, None, None]      # output channels five decades apart
    return f32(w)


def random_case(shape, seed, decades=False, per_image=False):
    """an image-like input (0..255) with bn_data's affine, bias and a map to accumulate onto; per_image: every image at a brightness
    of its own, over eight decades"""
    N, H, W = shape
    rs = np.random.RandomState(seed)
    x = f32(rs.rand(N, 3, H, W) * 255)
    if per_image:
        x = x * f32(np.exp(rs.uniform(-18, 0, N)))[:, None, None, None]
    g = ref_stem.geometry(N, H, W)
    return dict(x=f32(x), w=_weights(rs, decades), bias=f32(rs.randn(64)), in_scale=f32(rs.uniform(0.01, 0.03, 3)),
                in_shift=f32(rs.uniform(-3, -1, 3)), accum=f32(rs.randn(N, g.Ho, g.Wo, 64)))


# ---- 4. own scale.  A tile's bright or dark values sit in input rows [8 r + 3, 8 r + 5) and columns [64 t + 8, 64 t + 56): the only part
# of a tile's input that no other tile's patch reaches (rows: the patch of tile row r + 1 starts at 8 r + 5, that of r - 1 ends at
# 8 r + 3), so that a dark tile's WHOLE patch is dark and a zero tile's is zero (asserted by own_scale_case on ref_stem.geometry).
OWN_ROWS, OWN_COLS = (3, 5), (8, 56)
BRIGHT, DARK = 6.0e4, 2.0 ** -40
ORDERS = {"bright_dark_zero": "BDZ", "dark_bright_zero": "DBZ"}


def own_scale_case(shape, order, seed=4):
    """tiles bright (up to 6e4), dark (the same kind of pattern times 2^-40) and all-zero in turn along every row of tiles, the turn
    shifted by one per tile row and per image -> the case and kinds (N, yt, xt) of 'B', 'D', 'Z'"""
    N, H, W = shape
    g = ref_stem.geometry(N, H, W)
    rs = np.random.RandomState(seed)
    pattern = f32(rs.rand(N, 3, H, W) * BRIGHT)
    n, r, t = np.meshgrid(np.arange(N), np.arange(g.yt), np.arange(g.xt), indexing="ij")
    kinds = np.array(list(ORDERS[order]))[(n + r + t) % 3]
    factor = np.zeros((N, 1, H, W), np.float32)
    for rr in range(g.yt):
        for tt in range(g.xt):
            f = np.where(kinds[:, rr, tt] == "B", 1.0, np.where(kinds[:, rr, tt] == "D", DARK, 0.0)).astype(np.float32)
            factor[:, 0, 8 * rr + OWN_ROWS[0]:8 * rr + OWN_ROWS[1], 64 * tt + OWN_COLS[0]:64 * tt + OWN_COLS[1]] = f[:, None, None]
    x = f32(pattern * factor)
    mb = ref_stem.patch_max_bits(x, g).view(np.float32)
    assert (mb[kinds == "Z"] == 0).all() and (mb[kinds == "D"] > 0).all() and (mb[kinds == "D"] <= BRIGHT * DARK).all()
    assert (mb[kinds == "B"] > 0.5 * BRIGHT).all()
    return dict(x=x, w=_weights(rs, True), bias=f32(rs.randn(64))), kinds


def zeroed_dark(x, kinds, shape):
    """x with the dark tiles' values replaced by zeros"""
    g = ref_stem.geometry(*shape)
    x = x.copy()
    for rr in range(g.yt):
        for tt in range(g.xt):
            sel = kinds[:, rr, tt] == "D"
            x[sel, :, 8 * rr + OWN_ROWS[0]:8 * rr + OWN_ROWS[1], 64 * tt + OWN_COLS[0]:64 * tt + OWN_COLS[1]] = 0
    return x


# scale_of's edges: the biased exponent of the patch maximum, a tile each
EDGE_SHAPE = (1, 8, 256)
EDGE_EXPONENTS = (31, 32, 240, 241)


def exponent_edge_case(seed=5):
    N, H, W = EDGE_SHAPE
    rs = np.random.RandomState(seed)
    x = np.zeros((N, 3, H, W), np.float32)
    for tt, be in enumerate(EDGE_EXPONENTS):
        unit = np.float32(2.0) ** (be - 127)
        v = f32(rs.rand(3, OWN_ROWS[1] - OWN_ROWS[0], OWN_COLS[1] - OWN_COLS[0])) * unit      # below the exponent: [0, 1) * 2^e
        v[tt % 3, 1, 7 + tt] = np.float32(1.75) * unit
        x[0, :, OWN_ROWS[0]:OWN_ROWS[1], 64 * tt + OWN_COLS[0]:64 * tt + OWN_COLS[1]] = v
    got = (ref_stem.patch_max_bits(x)[0, 0] >> 23) & 255
    assert tuple(int(b) for b in got) == EDGE_EXPONENTS, got
    return dict(x=x, w=_weights(rs, False))


# ---- 2. impulses and 5. non-finite pixels: a 3 x 3 grid of tiles, the last column and row ragged
POINT_SHAPE = (1, 20, 140)
IMPULSE_AT = [(0, 0), (0, 139), (19, 0), (19, 139), (10, 70), (7, 63), (8, 64), (7, 65), (8, 66), (12, 64), (8, 100)]      # (row, column)
IMPULSE_VALUES = (0x3F800000, 0x3FD55FFF)              # 1.0, and a value whose low mantissa bits are all set


def impulse_weights(seed=2):
    """all 64 x 147 weights distinct in magnitude (0.02 .. 0.1 in shuffled equal steps, random signs), their low eight mantissa bits set"""
    rs = np.random.RandomState(seed)
    n = 64 * 147
    w = f32((0.02 + 0.08 * rs.permutation(n) / n) * np.where(rs.rand(n) < 0.5, -1.0, 1.0)).reshape(64, 3, 7, 7)
    w = (w.view(np.uint32) | np.uint32(0xFF)).view(np.float32)
    assert len(np.unique(np.abs(w))) == w.size
    return f32(w)


NONFINITE_AT = {"interior": (1, 12, 96), "seam": (2, 8, 64)}       # (channel, row, column): inside tile (1, 1); on the corner of four tiles


def tiles_whose_patch_holds(g, y, x):
    return [(r, t) for r in range(g.yt) for t in range(g.xt) if g.patch(r, t)[0] <= y < g.patch(r, t)[1] and g.patch(r, t)[2] <= x < g.patch(r, t)[3]]
