"""tests/ref_stem.py held to itself on the CPU, on the inputs of tests/test_stem_edges_gpu.py (tests/stem_cases.py):
the faithful emulation of stem_conv_kernel's arithmetic stays inside the per-element bound everywhere, every mutant of it leaves the
bound on a named input, the geometry helper gives the launch arithmetic stem.hip quotes, and every listed shape reaches its path."""
import numpy as np
import pytest

import ref_stem
import stem_cases as SC

CH = np.arange(0, 64, 4)            # the output channels the large cases are emulated at (the emulation costs 441 products per output)
IMAGES = 6                          # ... and the images: two full turns of bright / dark / zero


def _run(case, mode, mutant=None, channels=None, images=None):
    """-> (worst err / bound, old map-wide criterion, got, ref) of the emulation in one of the GPU test's four modes"""
    x, w = case["x"][:images], case["w"]
    kw = dict(bias=case.get("bias"), accum=None, act=1)
    xa = x
    if mode == "affine":
        xa = ref_stem.operands(x, case["in_scale"], case["in_shift"])
    elif mode == "nobias":
        kw["bias"] = None
    elif mode == "accum_leaky":
        kw.update(accum=case["accum"][:images], act=2)
    elif mode == "linear_nobias":
        kw.update(bias=None, act=0)
    else:
        assert mode == "plain"
    ch = np.arange(64) if channels is None else channels
    got = ref_stem.emulate(xa, w, mutant=mutant, channels=ch, **kw)
    ref = ref_stem.conv_ref(xa, w, **kw)[..., ch]
    bnd = ref_stem.bound(xa, w, **kw)[..., ch]
    r = ref_stem.ratio(got, ref, bnd)
    return float(np.nanmax(np.where(np.isnan(got), np.inf, r))), ref_stem.old_criterion(np.nan_to_num(got, nan=np.inf), ref), got, ref


def _impulse_case(at=(8, 64), bits=SC.IMPULSE_VALUES[1]):
    x = np.zeros((1, 3) + SC.POINT_SHAPE[1:], np.float32)
    x[0, 1, at[0], at[1]] = np.array([bits], np.uint32).view(np.float32)[0]
    return dict(x=x, w=SC.impulse_weights())


def _inputs():
    """name -> (case, mode, channels, images): one entry per input generator of the GPU test"""
    d = {}
    for shape in SC.BORDER_SHAPES:
        for mode in ("plain", "affine", "nobias", "accum_leaky"):
            d["border %s %s" % (shape, mode)] = (SC.random_case(shape, sum(shape)), mode, None, None)
    d["impulse"] = (_impulse_case(), "linear_nobias", None, None)
    for name, shape in SC.WALK_SHAPES.items():
        d["walk " + name] = (SC.random_case(shape, 3, decades=True, per_image=True), "affine", CH, IMAGES)
    for name in ("a_unused_slot_ragged", "b_parity_returns_whole_row_end"):
        for order in SC.ORDERS:
            d["own scale %s %s" % (name, order)] = (SC.own_scale_case(SC.WALK_SHAPES[name], order)[0], "linear_nobias", CH, IMAGES)
    return d


def test_faithful_emulation_stays_inside_the_bound():
    """the reference alone: err / bound <= 1 per element on every input of the GPU test (measured: at most 0.17, on a walk
    shape, where the bias addition's own rounding is the whole bound)"""
    worst = {}
    for name, (case, mode, ch, images) in _inputs().items():
        r, _, got, _ = _run(case, mode, None, ch, images)
        assert np.isfinite(got).all(), name
        worst[name] = r
    top = max(worst, key=worst.get)
    print("largest err / bound of the faithful emulation: %.4f at %s" % (worst[top], top))
    assert worst[top] <= 1.0, (top, worst[top])
    # the edges of scale_of: exponents 32 and 240 inside the bound, 31 inside the flush floor; 241 overflows fp16 (no bound: NaN)
    case = SC.exponent_edge_case()
    got = ref_stem.emulate(case["x"], case["w"], act=0)
    r = ref_stem.ratio(got, ref_stem.conv_ref(case["x"], case["w"], act=0), ref_stem.bound(case["x"], case["w"], act=0))
    for tt, be in enumerate(SC.EDGE_EXPONENTS):
        rt = r[:, :, 32 * tt:32 * tt + 32]
        if be == 241:
            assert np.isnan(rt).all() and not np.isfinite(got[:, :, 32 * tt + 4:32 * tt + 28]).any()
        else:
            assert rt.max() <= 1.0, (be, rt.max())
        if be == 31:
            assert (got[:, :, 32 * tt:32 * tt + 32] == 0).all()


# which input kills which mutant (err / bound > 1); the table DESIGN.md quotes
KILLS = {
    "drop_lo_hi": ["border (1, 9, 65) plain", "own scale a_unused_slot_ragged bright_dark_zero"],
    "neighbour_scale": ["own scale a_unused_slot_ragged bright_dark_zero", "own scale b_parity_returns_whole_row_end bright_dark_zero"],
    "zero_tap_kx": ["impulse", "border (1, 9, 65) plain"],
    "zero_tap_ky": ["impulse", "border (1, 9, 65) plain"],
}


def test_every_mutant_is_killed_and_the_old_criterion_misses_the_neighbour_scale():
    inputs = _inputs()
    assert set(KILLS) == set(ref_stem.MUTANTS)
    for mutant, names in KILLS.items():
        for name in names:
            case, mode, ch, images = inputs[name]
            r, old, _, _ = _run(case, mode, mutant, ch, images)
            print("%-16s on %-60s err / bound %.3g, map-wide criterion %.3g" % (mutant, name, r, old))
            assert r > 1.0, (mutant, name, r)
            if mutant == "neighbour_scale":
                # ... and this is why the file exists: a dark tile cut with its bright neighbour's scale is far below the map's maximum
                assert old < 1.0, (name, old)
                faithful_old = _run(case, mode, None, ch, images)[1]
                assert faithful_old < 1.0
    # a dropped lo hi product on a dark map passes the map-wide criterion as well
    case = SC.random_case((1, 9, 65), 1)
    case["x"] = case["x"] * np.float32(2.0 ** -30)
    r, old, _, _ = _run(case, "linear_nobias", "drop_lo_hi")
    assert r > 1.0 and old < 1.0, (r, old)


def test_geometry_restates_the_launch_arithmetic():
    """hand-worked cases, the two stem.hip quotes (one 600 x 1000 image: no walk; six: eight tiles per workgroup) among them"""
    def facts(N, H, W):
        g = ref_stem.geometry(N, H, W)
        return g.Ho, g.Wo, g.xt, g.yt, g.want, g.gx, g.tpw, g.grid_x
    assert facts(1, 600, 1000) == (300, 500, 16, 75, 2, 8, 2, 8)
    assert facts(6, 600, 1000) == (300, 500, 16, 75, 14, 2, 8, 2)
    assert facts(9, 150, 250) == (75, 125, 4, 19, 1, 4, 1, 4)
    assert facts(1, 1, 1) == (1, 1, 1, 1, 1, 1, 1, 1)
    assert facts(37, 32, 400) == (16, 200, 7, 4, 2, 4, 2, 4)
    assert facts(74, 24, 448) == (12, 224, 7, 3, 3, 3, 3, 3)
    assert facts(43, 47, 256) == (24, 128, 4, 6, 2, 2, 2, 2)
    g = ref_stem.geometry(1, 20, 140)
    assert g.patch(0, 0) == (0, 11, 0, 66) and g.patch(1, 1) == (5, 19, 60, 130) and g.patch(2, 2) == (13, 20, 124, 140)
    assert SC.tiles_whose_patch_holds(g, 12, 96) == [(1, 1)]
    assert SC.tiles_whose_patch_holds(g, 8, 64) == [(0, 0), (0, 1), (1, 0), (1, 1)]


def test_every_gpu_shape_reaches_the_path_it_is_listed_under():
    for name in SC.WALK_SHAPES:
        SC.walk_predicate(name)
    geos = [ref_stem.geometry(*s) for s in SC.BORDER_SHAPES]
    assert {g.H for g in geos} == set(SC.BORDER_H) and {g.W for g in geos} == set(SC.BORDER_W)
    assert {g.Ho % 4 for g in geos} == {0, 1, 2, 3} and {g.Wo % 32 for g in geos} >= {0, 1, 31}
    assert {g.Wo for g in geos} >= {1, 31, 32, 33} and {g.N for g in geos} == {1, 2}
    assert any(g.H == 1 and g.W == 1 for g in geos) and any(g.H == 1 and g.W > 1 for g in geos) and any(g.W == 1 and g.H > 1 for g in geos)
    assert all(g.tpw == 1 for g in geos)
    # the right border inside the patch columns 64..69 of tile 0 (image columns 60..65)
    assert {g.W for g in geos if 60 < g.W <= 66} >= {62, 63, 64, 65, 66}
    g = ref_stem.geometry(*SC.POINT_SHAPE)
    assert (g.xt, g.yt, g.tpw) == (3, 3, 1) and not g.whole(2) and g.Ho % 4 != 0
    g = ref_stem.geometry(*SC.EDGE_SHAPE)
    assert (g.xt, g.yt) == (len(SC.EDGE_EXPONENTS), 1)


@pytest.mark.parametrize("shape,k", [((1, 5, 9, 7), 2), ((2, 3, 37, 50), 4), ((1, 2, 5, 6), 1), ((1, 2, 3, 9), 4)])
def test_avgpool_in_order_restatement_is_the_average(shape, k):
    """avgpool_full_f32_in_order against a float64 loop: within fp32 round-off of the clipped window's mean, exact for k = 1"""
    x = (np.random.RandomState(k).rand(*shape) * 255).astype(np.float32)
    got = ref_stem.avgpool_full_f32_in_order(x, k)
    N, C, H, W = shape
    for oy in range(got.shape[2]):
        for ox in range(got.shape[3]):
            win = x[:, :, oy * k:oy * k + k, ox * k:ox * k + k].astype(np.float64)
            want = win.mean(axis=(2, 3))
            assert np.abs(got[:, :, oy, ox] - want).max() <= ref_stem.gamma(k * k + 1) * np.abs(win).mean(axis=(2, 3)).max()
    if k == 1:
        assert np.array_equal(got, x)
