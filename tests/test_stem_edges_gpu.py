"""stem_conv_kernel (lsfa_amd/csrc/stem.hip) against tests/ref_stem.py, tile by tile: every comparison is |got - conv_ref| / bound <= 1
PER ELEMENT (the bound is local: a dark tile beside a bright one is held to the dark tile's own magnitude; ref_stem's docstring derives
it), amax_out is max|y| exactly, a second launch reproduces the bits.  Shapes and inputs come from tests/stem_cases.py, where
tests/test_stem_edges_cpu.py holds the reference's own emulation to the same bound and shows which input kills which mutant; every
shape's geometry predicate is asserted here as well.  The non-finite rule: a NaN or an infinity in the input must not become finite
output silently - every output whose window holds it is non-finite or the launch's amax_out holds a non-finite bit pattern.
The worst err / bound per family is written with parity_util.record('stem_edges', ...)."""
import numpy as np
import pytest
import torch

import parity_util
import ref_stem
import stem_cases as SC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_worst = {}


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(x):
    return x.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all().item())


def flagged_nonfinite(am):
    """an amax_out row holds the bit pattern of an infinity or a NaN: what trips the consumer's status word"""
    return bool(((am & 0x7FFFFFFF) >= 0x7F800000).any().item())


def note(family, tag, value):
    rec = _worst.setdefault(family, {"err_over_bound": 0.0, "worst_at": None, "comparisons": 0})
    rec["comparisons"] += 1
    if value >= rec["err_over_bound"]:
        rec["err_over_bound"], rec["worst_at"] = float(value), repr(tag)
    parity_util.record("stem_edges", _worst)


def launch(hip, x, wl, bias=None, in_scale=None, in_shift=None, accum=None, act=1, in_place=False):
    """two launches with amax_out: the same bits, amax_out == max|y| exactly -> y (N, Ho, Wo, 64) on the device"""
    outs = []
    for _ in range(2):
        am = hip.amax_slots(1, DEV)[0]
        out = accum.clone() if in_place else None
        y = hip.stem_conv(x, wl, bias, in_scale, in_shift, out=out, accum=out if in_place else accum, act=act, amax_out=am)
        assert float(am.view(torch.float32).max()) == float(y.abs().max())
        outs.append(y)
    assert same_bits(outs[0], outs[1])
    return outs[0]


def held(family, tag, got, xa, w, bias=None, accum=None, act=1, where=None):
    """err / bound <= 1 on every element (of `where`) -> the ratios"""
    got = got.cpu().numpy()
    r = ref_stem.ratio(got, ref_stem.conv_ref(xa, w, bias, accum, act), ref_stem.bound(xa, w, bias, accum, act))
    sel = r if where is None else r[where]
    assert np.isfinite(got if where is None else got[where]).all(), (family, tag)
    worst = float(sel.max()) if sel.size else 0.0
    print("%s %r: err / bound %.4f" % (family, tag, worst))
    note(family, tag, worst)
    assert worst <= 1.0, "%s %r: err / bound = %.4f" % (family, tag, worst)
    return r


def per_output(tiles, g):
    """(N, yt, xt) -> (N, Ho, Wo)"""
    return np.repeat(np.repeat(tiles, ref_stem.TILE_ROWS, 1), ref_stem.TILE_COLS, 2)[:, :g.Ho, :g.Wo]


# ------------------------------------------------------------------ 1. borders and ragged tiles ----
@pytest.mark.parametrize("shape", SC.BORDER_SHAPES)
def test_borders_and_ragged_tiles(hip, shape):
    """plain; with bn_data's affine (in_shift != 0: the outermost outputs show that the padding is zero AFTER it); without bias; and
    LeakyReLU with accum in place (the ragged epilogue together with arow)"""
    g = ref_stem.geometry(*shape)
    assert g.tpw == 1 and (g.H in SC.BORDER_H) and (g.W in SC.BORDER_W)
    c = SC.random_case(shape, sum(shape))
    x, w, b, sc, sh, acc = c["x"], c["w"], c["bias"], c["in_scale"], c["in_shift"], c["accum"]
    wl = hip.stem_weight_layout(t(w))
    held("borders", (shape, "plain"), launch(hip, t(x), wl, t(b)), x, w, b)
    xa = ref_stem.operands(x, sc, sh)
    held("borders", (shape, "affine"), launch(hip, t(x), wl, t(b), t(sc), t(sh)), xa, w, b)
    held("borders", (shape, "nobias"), launch(hip, t(x), wl, None), x, w, None)
    got = launch(hip, t(x), wl, t(b), t(sc), t(sh), accum=t(acc), act=2, in_place=True)
    held("borders", (shape, "accum_leaky"), got, xa, w, b, acc, 2)
    assert same_bits(got, launch(hip, t(x), wl, t(b), t(sc), t(sh), accum=t(acc), act=2))      # in place = into a fresh map


# ------------------------------------------------------------------ 2. impulses ----
@pytest.mark.parametrize("value", SC.IMPULSE_VALUES)
def test_impulses_pin_every_tap(hip, value):
    """one non-zero pixel, all weights distinct: every output is ONE product x * w[co, ci, iy + 3 - 2 oy, ix + 3 - 2 ox], to 2^-22
    relative, and exactly act(bias) where no tap meets the pixel (the zero-weight slots included)"""
    N, H, W = SC.POINT_SHAPE
    g = ref_stem.geometry(N, H, W)
    w = SC.impulse_weights()
    wl = hip.stem_weight_layout(t(w))
    xv = np.array([value], np.uint32).view(np.float32)[0]
    bias = ref_stem.f32(np.random.RandomState(8).randn(64))
    worst = 0.0
    for i, (iy, ix) in enumerate(SC.IMPULSE_AT):
        ci = i % 3
        x = np.zeros((N, 3, H, W), np.float32)
        x[0, ci, iy, ix] = xv
        want = np.zeros((g.Ho, g.Wo, 64), np.float64)
        hit = np.zeros((g.Ho, g.Wo), bool)
        for oy in range(g.Ho):
            for ox in range(g.Wo):
                ky, kx = iy + 3 - 2 * oy, ix + 3 - 2 * ox
                if 0 <= ky < 7 and 0 <= kx < 7:
                    want[oy, ox], hit[oy, ox] = np.float64(xv) * w[:, ci, ky, kx].astype(np.float64), True
        assert 4 <= hit.sum() <= 16
        got = launch(hip, t(x), wl, None, act=0).cpu().numpy()[0]
        assert (got[~hit] == 0).all(), (iy, ix)
        rel = np.abs(got[hit] - want[hit]) / np.abs(want[hit])
        worst = max(worst, float(rel.max()) / 2.0 ** -22)
        assert rel.max() <= 2.0 ** -22, ((iy, ix), rel.max() / 2.0 ** -22)
        for act in (1, 2):
            gb = launch(hip, t(x), wl, t(bias), act=act).cpu().numpy()[0]
            slope = np.float32(0.0 if act == 1 else ref_stem.SLOPE)
            act_bias = np.maximum(bias, np.float32(0)) + slope * np.minimum(bias, np.float32(0))
            assert np.array_equal(gb[~hit].view(np.uint32), np.broadcast_to(act_bias, gb.shape)[~hit].view(np.uint32)), (iy, ix, act)
    print("impulses %#x: largest relative error / 2^-22 = %.4f" % (value, worst))
    note("impulses_rel_err_over_2^-22", hex(value), worst)


# ------------------------------------------------------------------ 3. the tile walk ----
@pytest.mark.parametrize("name", sorted(SC.WALK_SHAPES))
def test_tile_walk(hip, name):
    """tiles_per_wg >= 2: an unused last slot (the break), a third tile (the parity back at 0), `more` false on a whole tile at the
    row's end and by t + 1 == tpw; every image alone (tiles_per_wg = 1) gives the bits it has inside the batch"""
    g = SC.walk_predicate(name)
    shape = SC.WALK_SHAPES[name]
    c = SC.random_case(shape, 3, decades=True, per_image=True)
    x, w, b, sc, sh = c["x"], c["w"], c["bias"], c["in_scale"], c["in_shift"]
    wl = hip.stem_weight_layout(t(w))
    got = launch(hip, t(x), wl, t(b), t(sc), t(sh))
    held("walk", name, got, ref_stem.operands(x, sc, sh), w, b)
    xd = t(x)
    assert ref_stem.geometry(1, g.H, g.W).tpw == 1
    for n in range(g.N):
        alone = hip.stem_conv(xd[n:n + 1], wl, t(b), t(sc), t(sh))
        assert same_bits(alone[0], got[n]), (name, n)


# ------------------------------------------------------------------ 4. own scale ----
@pytest.mark.parametrize("order", sorted(SC.ORDERS))
@pytest.mark.parametrize("name", ["a_unused_slot_ragged", "b_parity_returns_whole_row_end"])
def test_own_scale_bright_dark_and_zero_tiles(hip, name, order):
    """bright, dark (x 2^-40) and all-zero tiles in turn along the walk, between tile rows and between images: the dark tiles inside
    the LOCAL bound, the zero tiles exactly act(bias), the bright tiles' bits the same when the dark tiles are zeros"""
    g = SC.walk_predicate(name)
    shape = SC.WALK_SHAPES[name]
    c, kinds = SC.own_scale_case(shape, order)
    x, w, b = c["x"], c["w"], c["bias"]
    wl = hip.stem_weight_layout(t(w))
    kind = per_output(kinds, g)
    got = launch(hip, t(x), wl, None, act=0)
    r = held("own_scale", (name, order), got, x, w, None, None, 0)
    for k in "BDZ":
        note("own_scale_" + {"B": "bright", "D": "dark", "Z": "zero"}[k], (name, order), float(r[kind == k].max()))
    assert (got.cpu().numpy()[kind == "Z"] == 0).all()
    gb = launch(hip, t(x), wl, t(b), act=2)
    slope = ref_stem.SLOPE
    act_bias = np.maximum(b, np.float32(0)) + slope * np.minimum(b, np.float32(0))
    gz = gb.cpu().numpy()[kind == "Z"]
    assert np.array_equal(gz.view(np.uint32), np.broadcast_to(act_bias, gz.shape).view(np.uint32))
    g0 = launch(hip, t(SC.zeroed_dark(x, kinds, shape)), wl, t(b), act=2)
    sel = torch.from_numpy(kind == "B").to(DEV)
    assert same_bits(gb[sel], g0[sel])


def test_scale_of_edges(hip):
    """patch maxima with biased exponents 31, 32, 240 and 241, a tile each: 32 and 240 inside the bound, 31 inside its flush floor;
    241 (fp16 overflows under s = 1) falls under the non-finite rule: the outputs that read the tile's values are non-finite"""
    c = SC.exponent_edge_case()
    x, w = c["x"], c["w"]
    g = ref_stem.geometry(*SC.EDGE_SHAPE)
    wl = hip.stem_weight_layout(t(w))
    am = hip.amax_slots(1, DEV)[0]
    y = hip.stem_conv(t(x), wl, None, act=0, amax_out=am)
    assert same_bits(y, hip.stem_conv(t(x), wl, None, act=0))
    got = y.cpu().numpy()
    r = ref_stem.ratio(got, ref_stem.conv_ref(x, w, None, None, 0), ref_stem.bound(x, w, None, None, 0))
    reads = ref_stem.pre_activation(np.where(x != 0, np.float32(np.nan), np.float32(0)), w)      # NaN where the window holds a value
    for tt, be in enumerate(SC.EDGE_EXPONENTS):
        cols = slice(32 * tt, 32 * tt + 32)
        if be == 241:
            sel = np.isnan(reads[:, :, cols])
            shown = ~np.isfinite(got[:, :, cols][sel])
            print("exponent 241: %d of %d outputs non-finite, amax_out %#x" % (shown.sum(), shown.size, int(am.max().item())))
            assert shown.all() or flagged_nonfinite(am)
            assert (got[:, :, cols][~sel] == 0).all()
        else:
            assert np.isfinite(got[:, :, cols]).all()
            worst = float(r[:, :, cols].max())
            print("exponent %d: err / bound %.4f" % (be, worst))
            note("scale_of_edges", be, worst)
            assert worst <= 1.0, (be, worst)


# ------------------------------------------------------------------ 5. non-finite pixels ----
@pytest.mark.parametrize("where", sorted(SC.NONFINITE_AT))
@pytest.mark.parametrize("value", ["nan", "inf", "-inf"])
def test_nonfinite_pixel_stays_visible(hip, value, where):
    """one NaN / +inf / -inf pixel, act 0 / 1 / 2, with and without amax_out: every output whose window holds it is non-finite or
    amax_out holds a non-finite bit pattern; tiles whose PATCH does not hold it keep the clean run's bits"""
    N, H, W = SC.POINT_SHAPE
    g = ref_stem.geometry(N, H, W)
    c = SC.random_case(SC.POINT_SHAPE, 11)
    x, w, b = c["x"], c["w"], c["bias"]
    ci, iy, ix = SC.NONFINITE_AT[where]
    bad = x.copy()
    bad[0, ci, iy, ix] = np.float32(value)
    holds = ref_stem.window_holds_nonfinite(bad)
    assert holds.sum() >= 9
    tiles = np.zeros((N, g.yt, g.xt), bool)
    for r_, t_ in SC.tiles_whose_patch_holds(g, iy, ix):
        tiles[0, r_, t_] = True
    assert tiles.sum() == (1 if where == "interior" else 4)
    clean_tile = torch.from_numpy(~per_output(tiles, g)).to(DEV)
    assert not (holds & clean_tile.cpu().numpy()).any()
    wl = hip.stem_weight_layout(t(w))
    for act in (0, 1, 2):
        clean = hip.stem_conv(t(x), wl, t(b), act=act)
        for with_amax in (False, True):
            am = hip.amax_slots(1, DEV)[0] if with_amax else None
            y = hip.stem_conv(t(bad), wl, t(b), act=act, amax_out=am)
            assert same_bits(y[clean_tile], clean[clean_tile]), (act, with_amax)
            shown = ~np.isfinite(y.cpu().numpy()[holds])
            flagged = with_amax and flagged_nonfinite(am)
            assert shown.all() or flagged, "act %d, amax_out %s: %d of %d outputs that read the %s pixel are finite and nothing flags it" % (
                act, with_amax, (~shown).sum(), shown.size, value)
            if with_amax:
                assert flagged, "act %d: amax_out = %#x does not show the %s pixel" % (act, int(am.max().item()), value)


def test_maxpool_keeps_a_nan_visible(hip):
    """lsfa_maxpool3x3s2_nhwc on a map with one NaN: every output whose window holds it shows it in y and y2, and amax_out flags it"""
    rs = np.random.RandomState(6)
    x = ref_stem.f32(rs.randn(1, 9, 11, 8))
    x[0, 4, 5, 3] = np.nan
    s2, t2 = ref_stem.f32(rs.uniform(0.5, 1.5, 8)), ref_stem.f32(rs.randn(8))
    holds = np.zeros((5, 6), bool)
    for oy in range(5):
        for ox in range(6):
            holds[oy, ox] = 2 * oy - 1 <= 4 <= 2 * oy + 1 and 2 * ox - 1 <= 5 <= 2 * ox + 1
    assert holds.sum() == 2
    clean = np.where(np.isnan(x), -np.inf, x)
    want = np.full((1, 5, 6, 8), -np.inf, np.float32)
    for oy in range(5):
        for ox in range(6):
            want[0, oy, ox] = clean[0, max(2 * oy - 1, 0):2 * oy + 2, max(2 * ox - 1, 0):2 * ox + 2].reshape(-1, 8).max(0)
    for second in (False, True):
        am = hip.amax_slots(1, DEV)[0]
        out = hip.maxpool3x3s2_nhwc(t(x), scale2=t(s2) if second else None, shift2=t(t2) if second else None, amax_out=am)
        ys = [o.cpu().numpy() for o in (out if second else (out,))]
        nan_at = np.zeros((1, 5, 6, 8), bool)
        nan_at[0, holds, 3] = True
        for y in ys:
            assert np.isnan(y[nan_at]).all() and np.isfinite(y[~nan_at]).all()
        assert np.array_equal(ys[0][~nan_at], want[~nan_at])
        if second:
            assert np.array_equal(ys[1][~nan_at], np.maximum(want * s2 + t2, np.float32(0))[~nan_at])
        assert flagged_nonfinite(am)


# ------------------------------------------------------------------ average pooling, image tables ----
@pytest.mark.parametrize("shape,k", [((1, 5, 9, 7), 2), ((2, 3, 37, 50), 4), ((1, 2, 5, 6), 1), ((1, 2, 3, 9), 4)])
def test_avgpool_nchw_bit_for_bit_in_the_stated_order(hip, shape, k):
    """avgpool_kernel: the clipped window's pixels row by row onto 0, one division by their number; k = 1; k > H"""
    x = ref_stem.f32(np.random.RandomState(shape[2]).rand(*shape) * 255)
    want = ref_stem.avgpool_full_f32_in_order(x, k)
    got = hip.avgpool_nchw(t(x), k)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    tbl = scattered_table(hip, x)
    assert same_bits(hip.avgpool_nchw(tbl, k), got)


def scattered_table(hip, x):
    """the images of x (N, C, H, W) as an ImageTable: each in a place of its own inside one buffer of garbage, in scrambled order,
    with garbage of varying length between them"""
    N, C, H, W = x.shape
    n = C * H * W
    order = np.random.RandomState(N).permutation(N)
    gaps = [17 + 5 * i for i in range(N + 1)]
    buf = torch.full((N * n + sum(gaps),), float("nan"), dtype=torch.float32, device=DEV)
    buf[::3] = 1.0e30
    images, at = [None] * N, gaps[0]
    for slot, i in enumerate(order):
        images[i] = buf[at:at + n].view(C, H, W)
        images[i].copy_(t(x[i]))
        at += n + gaps[slot + 1]
    return hip.ImageTable(N, C, H, W, DEV).set(images)


@pytest.mark.parametrize("shape", [SC.WALK_SHAPES["a_unused_slot_ragged"], (2, 9, 65)])
def test_image_table_gives_the_dense_bits(hip, shape):
    """stem_conv on separately placed images (lsfa_stem_conv7x7s2_tbl): the bits of the dense call, walked tiles included"""
    c = SC.random_case(shape, 9)
    wl = hip.stem_weight_layout(t(c["w"]))
    args = (wl, t(c["bias"]), t(c["in_scale"]), t(c["in_shift"]))
    dense = hip.stem_conv(t(c["x"]), *args)
    assert same_bits(hip.stem_conv(scattered_table(hip, c["x"]), *args), dense)
    am = hip.amax_slots(1, DEV)[0]
    acc = t(c["accum"])
    got = hip.stem_conv(scattered_table(hip, c["x"]), *args, accum=acc, act=2, amax_out=am)
    assert same_bits(got, hip.stem_conv(t(c["x"]), *args, accum=acc, act=2))
    assert float(am.view(torch.float32).max()) == float(got.abs().max())
