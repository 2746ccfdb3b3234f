"""The two bilinear samplers on the coordinates where their index decisions are made - the part that needs no GPU.

tests/ref_sample.py states both samplers in plain numpy and builds the fields; here the fields are shown to cover every edge class
(a condition, with the classes that cannot be reached listed and proven unreachable), the numpy statement is pinned to the C oracle bit
for bit, its float32 form is bounded by its float64 form, the oracle's hardened index conversion is pinned on wild coordinates, and the
float-reciprocal division of the power-of-two deformable kernel (fdiv24, lsfa_amd/csrc/dcn.hip) is checked over its whole domain.
tests/test_sample_edges_gpu.py runs the same fields through every kernel."""
import numpy as np
import pytest

import oracle
import ref_sample as R

HW_IDS = lambda hw: "%dx%d" % hw
CFG_IDS = lambda c: "pad%d-s%d-d%d-dg%d" % c

# ---- classes a coordinate cannot fall in ------------------------------------------------------------------------------------------------------------
# -0.0 is no coordinate of either sampler, at any size.
#   warp: x_real = (gx + 1.0f) * (W - 1) / 2.0f.  gx + 1.0f is exactly zero only for gx = -1, and x + (-x) is +0 in round-to-nearest; a
#         non-zero gx + 1.0f is at least 2^-24 in size, so the product does not underflow to -0 either.
#   deformable: h = (float)(int) + offset, and a sum is -0 only when both terms are; (float) of an int is never -0.
# test_minus_zero_is_no_coordinate probes both chains.
NEVER = {"neg_zero"}
# an axis of two samples has no integer strictly between 0 and L - 1
TOO_SHORT = {2: {"int_interior"}}
# The warp's round trip cannot produce these coordinates at these axis lengths (L = W or H): x_real is a float32 multiple of (L - 1) / 2
# rounded once more, and e.g. -1 = (gx + 1) * (L - 1) / 2 needs gx + 1 = -2 / (L - 1) to be a float32 on the 2^-23 grid of [-2, -1) + 1,
# which it is for L - 1 a power of two only.  test_the_skipped_warp_classes_are_unreachable proves each entry by walking every float32
# value of x + fx across the class; each class is present at some tested width AND some tested height
# (test_every_skipped_warp_class_is_present_at_another_length).
WARP_UNREACHABLE = {
    2: set(), 5: set(), 9: set(),
    6: {"minus_one"},
    7: {"minus_one", "above_last_1ulp", "below_L_1ulp"},
    16: {"minus_one", "above_last_1ulp"},
    63: {"minus_one", "above_last_1ulp", "below_L_1ulp"},
}


def warp_absent(L):
    return NEVER | TOO_SHORT.get(L, set()) | WARP_UNREACHABLE[L]


def deform_absent(L):
    return NEVER | TOO_SHORT.get(L, set())


def test_classify_names_every_edge_of_an_axis():
    L, f = 5, np.float32
    up, down = lambda v: np.nextafter(f(v), f(np.inf)), lambda v: np.nextafter(f(v), f(-np.inf))
    cases = [(2.0, "int_interior"), (1.0, "int_interior"), (3.0, "int_interior"), (0.0, "zero"), (-0.0, "neg_zero"), (down(0), "below_zero_1ulp"),
             (-np.spacing(f(5)), "below_zero_1ulp"), (down(-np.spacing(f(5))), "band_lo"), (-0.5, "band_lo"), (up(-1), "band_lo"), (-1.0, "minus_one"),
             (down(-1), "below_minus_one"), (-80.0, "below_minus_one"), (-2.0 ** 31, "wild"), (up(-2.0 ** 31), "below_minus_one"), (4.0, "last"),
             (up(4), "above_last_1ulp"), (up(up(4)), "band_hi"), (4.5, "band_hi"), (down(down(5)), "band_hi"), (down(5), "below_L_1ulp"), (5.0, "at_L"),
             (up(5), "beyond_L"), (1e9, "beyond_L"), (2.0 ** 31, "wild"), (np.finfo(f).max, "wild"), (-3e38, "wild"), (np.inf, "nonfinite"),
             (-np.inf, "nonfinite"), (np.nan, "nonfinite"), (up(0), "frac_interior"), (0.5, "frac_interior"), (down(4), "frac_interior"),
             (up(1), "frac_interior")]
    got = R.classify(np.array([c[0] for c in cases], f), L)
    assert got.tolist() == [c[1] for c in cases]
    assert set(c[1] for c in cases) == set(R.CLASSES)
    assert R.classify(np.array([0.5, 1.0, 0.0], f), 2).tolist() == ["frac_interior", "last", "zero"]


# ---- coverage of the inputs is a condition ---------------------------------------------------------------------------------------------------------
def _check_axes(counts, absent_x, absent_y, what):
    for axis, absent in (("x", absent_x), ("y", absent_y)):
        for c in R.CLASSES:
            if c in absent:
                assert counts[axis][c] == 0, "%s: %s on %s is listed as unreachable but the field holds it: take it off the list" % (what, c, axis)
            else:
                assert counts[axis][c] >= 1, "%s: no cell of class %s on the %s axis" % (what, c, axis)
    for cx in R.BORDER:
        for cy in R.BORDER:
            if cx not in absent_x and cy not in absent_y:
                assert (cx, cy) in counts["pairs"], "%s: no cell with x in %s and y in %s" % (what, cx, cy)


@pytest.mark.parametrize("C", R.CHANNELS)
@pytest.mark.parametrize("hw", R.SHAPES, ids=HW_IDS)
def test_the_warp_field_holds_every_reachable_class_and_border_pair(hw, C):
    H, W = hw
    case = R.warp_case(hw, C)
    assert case["flow"].shape[0] % 2 == 0 and case["flow_wild"].shape[0] % 2 == 0
    _check_axes(case["counts"], warp_absent(W), warp_absent(H), "warp %dx%d" % hw)
    for axis in "xy":
        assert case["counts"][axis]["wild"] >= 1 and case["counts"][axis]["nonfinite"] >= 1
    # the field for the amax check: the same, with no non-finite coordinate
    _check_axes(case["counts_wild"], warp_absent(W) | {"nonfinite"}, warp_absent(H) | {"nonfinite"}, "warp %dx%d without non-finite cells" % hw)
    # whole-pixel flows: most of the other cells sit on the lattice
    assert case["counts"]["x"]["int_interior"] + case["counts"]["x"]["zero"] + case["counts"]["x"]["last"] >= 3


def test_every_skipped_warp_class_is_present_at_another_length():
    widths, heights = set(w for _, w in R.SHAPES), set(h for h, _ in R.SHAPES)
    assert widths | heights == set(WARP_UNREACHABLE)
    for lengths in (widths, heights):
        for c in set().union(*WARP_UNREACHABLE.values()) | set().union(*TOO_SHORT.values()):
            assert any(c not in warp_absent(L) for L in lengths), c


def _floats_between(lo, hi):
    """every float32 in [lo, hi] (same sign, both non-zero)"""
    a, b = np.float32(lo).view(np.int32), np.float32(hi).view(np.int32)
    return np.arange(min(a, b), max(a, b) + 1, dtype=np.int32).view(np.float32)


@pytest.mark.parametrize("L", sorted(L for L, s in WARP_UNREACHABLE.items() if s))
def test_the_skipped_warp_classes_are_unreachable(L):
    """x_real depends on the pixel and the flow through a = x + fx alone, and every step of the chain is monotone in a.  So walk EVERY
    float32 a from one that lands strictly below the class' coordinate to one that lands strictly above it: none lands on it."""
    f = np.float32
    point = {"minus_one": f(-1), "above_last_1ulp": np.nextafter(f(L - 1), f(np.inf)), "below_L_1ulp": np.nextafter(f(L), f(-np.inf))}
    for c in sorted(WARP_UNREACHABLE[L]):
        t = point[c]
        a = _floats_between(t * f(1 - 2e-5), t * f(1 + 2e-5))
        assert a.size > 100
        x = R.warp_coord(np.zeros_like(a), a, L)
        assert (np.diff(x) >= 0).all() or (np.diff(x) <= 0).all()
        assert x.min() < t < x.max(), "the walk does not cross %s" % c
        assert not (x == t).any() and not (R.classify(x, L) == c).any(), "%s is reachable at L = %d: take it off the list" % (c, L)


def test_minus_zero_is_no_coordinate():
    f = np.float32
    tiny = np.concatenate([[f(0), f(-0.0)], f(2.0) ** np.arange(-149, -18).astype(f), -(f(2.0) ** np.arange(-149, -18).astype(f))]).astype(f)
    for L in sorted(WARP_UNREACHABLE):
        for p in (0, 1, L - 1):
            for a in (tiny, tiny - f(p)):                     # flows around 0 and around -p: x + fx at and around zero
                x = R.warp_coord(np.full(a.shape, p, f), a, L)
                assert not ((x == 0) & np.signbit(x)).any()
    for b in (-2, -1, 0, 1):
        h = R.deform_coord(f(b), tiny - f(b))
        assert not ((h == 0) & np.signbit(h)).any()


@pytest.mark.parametrize("cfg", R.DEFORM_CFGS, ids=CFG_IDS)
@pytest.mark.parametrize("hw", R.SHAPES, ids=HW_IDS)
def test_the_deform_field_holds_every_class_in_two_taps_and_two_groups(hw, cfg):
    H, W = hw
    pad, stride, dil, dg = cfg
    for C in R.CHANNELS:
        case = R.deform_case(hw, C, cfg)
        counts = case["counts"]
        _check_axes(counts, deform_absent(W), deform_absent(H), "deform %dx%d %s" % (H, W, CFG_IDS(cfg)))
        for c in R.CLASSES:
            if c in deform_absent(W) and c in deform_absent(H):
                continue
            assert len(counts["by_tap"][c]) >= 2, "%s occurs in taps %s only" % (c, sorted(counts["by_tap"][c]))
            if dg > 1:
                assert len(counts["by_group"][c]) >= 2, "%s occurs in groups %s only" % (c, sorted(counts["by_group"][c]))
        # one ulp below zero in the strictest sense, the smallest subnormal (where the tap's integer part is 0), on both axes
        h, w = R.deform_coords(case["offset"], H, W, 3, pad, stride, dil, dg)
        sub = np.float32(-2.0 ** -149)
        assert (h == sub).any() and (w == sub).any()


# ---- the numpy statement is the oracle's ----------------------------------------------------------------------------------------------------------------
def oracle_warp(case, flow, subset):
    """the C oracle for a subset; bn, which it has no argument for, is applied to its result as two float32 roundings (tests/test_hip_ops.py
    warp_want_bn does the same)"""
    K = flow.shape[0]
    kw = {}
    names = [] if subset == "plain" else subset.split("+")
    for name in names:
        if name in ("mul", "add") and not (name == "add" and "bn" in names):
            kw[name] = case[name][:K]
        elif name == "res":
            kw.update(res=case["res"][:K], res_w=case["res_w"], res_b=case["res_b"])
    out = oracle.warp_bilinear(case["feat"][:1], flow, **kw)
    if "bn" in names:
        with np.errstate(all="ignore"):
            out = (out * case["bn_s"][None, :, None, None]).astype(np.float32) + case["bn_t"][None, :, None, None]
            if "add" in names:
                out = out + case["add"][:K]
    return out.astype(np.float32)


@pytest.mark.parametrize("subset", ["plain", "mul", "add", "res", "bn", "res+bn+add"])
@pytest.mark.parametrize("hw", R.SHAPES, ids=HW_IDS)
def test_warp_ref_f32_is_the_oracle_bit_for_bit(hw, subset):
    """on every cell whose coordinates are finite and below 2^31 - where the oracle was defined before its index conversion was clamped"""
    case = R.warp_case(hw, 16)
    flow = case["flow"]
    cx, cy, nonfinite, _ = R.warp_classes(flow)
    tame = ~nonfinite & (cx != "wild") & (cy != "wild")
    assert tame.sum() > tame.size // 2
    got = R.warp_ref_f32(case["feat"][:1], flow, **R.warp_operands(case, subset, slice(0, flow.shape[0])))
    want = oracle_warp(case, flow, subset)
    m = np.broadcast_to(tame[:, None], got.shape)
    np.testing.assert_array_equal(got[m], want[m])
    assert np.isfinite(got[m]).all()


@pytest.mark.parametrize("hw", R.SHAPES, ids=HW_IDS)
def test_the_oracle_is_defined_on_wild_coordinates(hw):
    """orc_warp_bilinear clamps before its (int), as the kernels do: on cells with a finite coordinate at or beyond 2^31 it equals the numpy
    statement, and the sample is exactly zero; wherever no coordinate is non-finite the two agree, and where one is, both give NaN or agree."""
    case = R.warp_case(hw, 16)
    for flow in (case["flow"], case["flow_wild"]):
        cx, cy, nonfinite, zero_sample = R.warp_classes(flow)
        wild = ~nonfinite & ((cx == "wild") | (cy == "wild"))
        assert wild.any() and (zero_sample | ~wild).all()
        for subset in ("plain", "mul+res+add"):
            kw = R.warp_operands(case, subset, slice(0, flow.shape[0]))
            got, want = oracle_warp(case, flow, subset), R.warp_ref_f32(case["feat"][:1], flow, **kw)
            m = np.broadcast_to(~nonfinite[:, None], got.shape)
            np.testing.assert_array_equal(got[m], want[m])
            np.testing.assert_array_equal(got, want)                      # (NaN == NaN here: a non-finite cell is NaN in both or equal)
            z = np.broadcast_to(zero_sample[:, None], got.shape)
            np.testing.assert_array_equal(got[z], R.warp_zero_sample(got.shape, **kw)[z])
            if subset == "plain":
                assert (got[z] == 0).all()


@pytest.mark.parametrize("cfg", R.DEFORM_CFGS, ids=CFG_IDS)
@pytest.mark.parametrize("hw", R.SHAPES, ids=HW_IDS)
def test_deform_ref_f32_is_the_oracle_bit_for_bit_everywhere(hw, cfg):
    """the guard runs before the conversion, so wild and non-finite offsets are defined: exactly 0"""
    H, W = hw
    pad, stride, dil, dg = cfg
    for C in R.CHANNELS:
        case = R.deform_case(hw, C, cfg)
        got = R.deform_ref_f32(case["data"], case["offset"], 3, pad, stride, dil, dg)
        want = oracle.deform_im2col(case["data"], case["offset"], 3, 3, pad, stride, dil, dg)
        assert np.isfinite(got).all()
        np.testing.assert_array_equal(got, want)
        h, w = R.deform_coords(case["offset"], H, W, 3, pad, stride, dil, dg)                  # (N, dg, KK, Ho, Wo)
        ch, cw = R.classify(h, H), R.classify(w, W)
        out = np.isin(ch, ["wild", "nonfinite", "below_zero_1ulp", "band_lo", "minus_one", "below_minus_one", "at_L", "beyond_L"])
        out |= np.isin(cw, ["wild", "nonfinite", "below_zero_1ulp", "band_lo", "minus_one", "below_minus_one", "at_L", "beyond_L"])
        N, Ho, Wo = h.shape[0], h.shape[3], h.shape[4]
        g6 = got.reshape(N, dg, C // dg, 9, Ho, Wo)
        assert out.any() and (g6[np.broadcast_to(out[:, :, None], g6.shape)] == 0).all()


# ---- the float32 form against the float64 form -------------------------------------------------------------------------------------------------------
def _four_ulp(feat):
    """4 ulp of max|feat|: each of the four terms tap * weight * weight of the sum is at most max|feat| in size and carries roundings of
    about an ulp of that - a bound from the form of the sum, not from a measurement"""
    return 4.0 * float(np.spacing(np.float32(np.abs(feat).max())))


@pytest.mark.parametrize("hw", R.SHAPES, ids=HW_IDS)
def test_warp_ref_f32_is_within_4_ulp_of_the_float64_form(hw):
    case = R.warp_case(hw, 16)
    flow = case["flow"]
    _, _, nonfinite, _ = R.warp_classes(flow)
    a, b = R.warp_ref_f32(case["feat"], flow), R.warp_ref_f64(case["feat"], flow)
    m = np.broadcast_to(~nonfinite[:, None], a.shape)
    assert np.abs(a[m].astype(np.float64) - b[m]).max() <= _four_ulp(case["feat"])


@pytest.mark.parametrize("cfg", R.DEFORM_CFGS, ids=CFG_IDS)
@pytest.mark.parametrize("hw", R.SHAPES, ids=HW_IDS)
def test_deform_ref_f32_is_within_4_ulp_of_the_float64_form(hw, cfg):
    pad, stride, dil, dg = cfg
    case = R.deform_case(hw, 16, cfg)
    a = R.deform_ref_f32(case["data"], case["offset"], 3, pad, stride, dil, dg)
    b = R.deform_ref_f64(case["data"], case["offset"], 3, pad, stride, dil, dg)
    assert np.abs(a.astype(np.float64) - b).max() <= _four_ulp(case["data"])


@pytest.mark.parametrize("hw", R.SHAPES, ids=HW_IDS)
def test_the_warp_round_trip_moves_a_coordinate_by_a_few_ulp(hw):
    """Why the two forms of warp_ref share their float32 coordinate.  With u = 2^-24 and b = gx + 1: x + fx carries u relative, the division
    makes it 2u, - 1 and + 1 add u(|b| + 1) and u|b|, the product with L - 1 one more u: |x_real - exact| <= u (5 |x_real| + (L - 1) / 2) to
    first order - up to 1e-5 pixels at L = 63, against 4 ulp of a feature value for the sum."""
    case = R.warp_case(hw, 16)
    H, W = hw
    flow = case["flow"]
    u = 2.0 ** -24
    for axis, L in ((0, W), (1, H)):
        p = np.arange(L, dtype=np.float32)[None, None, :] if axis == 0 else np.arange(L, dtype=np.float32)[None, :, None]
        x32, x64 = R.warp_coord(p, flow[:, axis], L), R.warp_coord_f64(p, flow[:, axis], L)
        tame = np.isfinite(x32) & (np.abs(x64) < 2.0 ** 31)
        bound = u * (5.0 * np.abs(x64) + (L - 1) / 2.0) * (1 + 1e-6)
        assert (np.abs(x32[tame].astype(np.float64) - x64[tame]) <= bound[tame]).all()


# ---- fdiv24 ----------------------------------------------------------------------------------------------------------------------------------------------
# KK = 9 and, at the shapes above and the network's own (38 x 63 maps, 1000 x 600 frames), every Wo and Ho * Wo the kernel divides by
@pytest.mark.parametrize("d", [1, 3, 9, 25, 49, 5, 7, 21, 63, 125, 35, 2394, 9375])
def test_fdiv24_is_the_integer_quotient_on_its_whole_domain(d):
    """dcn.hip: 'the float product is off by at most one, the remainder fixes it' - for every n in [0, 2^24)"""
    n = np.arange(1 << 24, dtype=np.int32)
    np.testing.assert_array_equal(R.fdiv24(n, d), n // np.int32(d))
