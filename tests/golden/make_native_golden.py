"""Generates tests/golden/ref_native.npz from the reference's own native code (oracle/_ref).

Runs only where the reference tree is (LSFA_REFERENCE, default as in make_golden.py):

    python tests/golden/make_native_golden.py            # rebuilds oracle/_ref, writes the npz, prints the counts

Every output comes from the `on` build of oracle/_ref (a*b + c fuses inside one expression).  For every
PSROI, Proposal and anchor output K the npz also holds K__off and K__fast: how many of its values the
-ffp-contract=off and =fast builds of the same slices change (the motion vectors are integer work).  Those counts are measurements (DESIGN.md quotes them); nothing asserts them
against a number chosen in advance, only that regenerating gives them again.

Inputs are listed by class, not drawn at random, wherever the class is the point (ROIs, block rows); feature
maps, scores and deltas are seeded noise.  PSROI feature maps are stored as float16 (every value is exactly
representable in float32, the file stays small); everything else has the type the operators take.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "ref_native.npz")

# ---------------------------------------------------------------- PSROI pooling -----------------------------
PSROI_MAP = (2, 5, 10, 13)                       # N, D, H, W
PSROI_SETS = [                                   # name, spatial_scale, P, G
    ("net", 0.0625, 7, 7),                       # the network's
    ("g3", 0.125, 3, 3),                         # small groups
    ("p6g3", 0.1, 6, 3),                         # unequal, and a scale that is no power of two: bin edges round
]
SEARCH_PX = (-64, 600)                           # corners searched for a bin edge that fusing moves


def edge_flips(scale, P, px_range):
    """Integer corner pairs (lo, hi) within px_range at which the fused and the unfused bin edge, p * bin + start, fall
    on different sides of an integer: [(lo, hi, p)].  The ROI's corners are rounded before anything else, so
    integer pairs are all there is.  float32(float64(p) * bin + start) is the fused value: the product has at
    most 27 significant bits and the sum of it and a nearby float32 is exact in float64."""
    s = np.float32(scale)
    lo = np.arange(*px_range, dtype=np.float32)[:, None]
    hi = np.arange(*px_range, dtype=np.float32)[None, :]
    start = lo * s
    end = (hi.astype(np.float64) + 1.0).astype(np.float32) * s
    size = np.maximum((end - start).astype(np.float64), 0.1).astype(np.float32)
    bin_ = size / np.float32(P)
    found = []
    for p in range(P + 1):
        fused = (np.float64(p) * bin_.astype(np.float64) + start.astype(np.float64)).astype(np.float32)
        plain = (np.float32(p) * bin_).astype(np.float32) + start
        flip = (np.floor(fused) != np.floor(plain)) | (np.ceil(fused) != np.ceil(plain))
        flip &= hi >= lo - 1
        found += [(int(a) + px_range[0], int(b) + px_range[0], p) for a, b in zip(*np.nonzero(flip))]
    return found


def psroi_rois(scale, P, H, W):
    """~100 ROIs [batch, x1, y1, x2, y2] for a map of H x W at `scale`, class by class; returns (rois, n_flips,
    n_flips among corner pairs that are both >= 0, which is all that Proposal's clipped boxes can be)."""
    im_w, im_h = int(round(W / scale)), int(round(H / scale))
    below = lambda v: float(np.nextafter(np.float32(v), np.float32(0)))
    r = []
    # integer corners; the last is the whole image
    r += [[0, 0, 0, 15, 15], [0, 16, 32, 63, 95], [0, 3, 5, 100, 77], [0, 17, 9, 18, 10], [0, 1, 1, 2, 2],
          [0, 31, 47, 32, 48], [0, 0, 0, im_w - 1, im_h - 1]]
    # corners at x.5 (round() goes away from zero where rint goes to even: 0.5 and 2.5), and the float just below
    r += [[0, 0.5, 2.5, 40.5, 30.5], [0, 2.5, 0.5, 16.5, 24.5], [0, 1.5, 3.5, 33.5, 19.5], [0, 4.5, 6.5, 8.5, 10.5],
          [0, below(0.5), below(2.5), below(40.5), below(30.5)], [0, below(2.5), below(0.5), below(16.5), below(24.5)],
          [0, 12.5, 14.5, below(28.5), below(62.5)], [0, 0.5, 0.5, 0.5, 0.5], [0, 2.5, 2.5, 2.5, 2.5]]
    # negative corners
    r += [[0, -0.5, -3.2, 30, 40], [0, -3.2, -0.5, 50, 20], [0, -0.5, -0.5, -0.5, -0.5], [0, -10, -10, -2, -2],
          [0, -1.5, -2.5, 12.5, 13.5], [0, -40, 8, 24, 40]]
    # x2 < x1, x2 == x1, x2 == x1 - 1: the 0.1 floor of the ROI's size
    r += [[0, 50, 40, 20, 10], [0, 30, 30, 30, 30], [0, 30, 30, 29, 29], [0, 64, 16, 10, 80], [0, 20, 70, 90, 20],
          [0, 7, 7, 7, 40], [0, 7, 7, 40, 7]]
    # wholly right of / below the map (empty bins give 0), partly outside
    r += [[0, im_w + 20, 10, im_w + 60, 50], [0, 10, im_h + 5, 50, im_h + 40], [0, im_w + 1, im_h + 1, im_w + 9, im_h + 9],
          [0, im_w - 30, im_h - 30, im_w + 40, im_h + 40], [0, im_w - 8, 0, im_w + 100, im_h - 1], [0, 0, im_h - 3, im_w - 1, im_h + 300],
          [0, im_w - 1, im_h - 1, im_w - 1, im_h - 1], [0, im_w, im_h, im_w, im_h]]
    # corners where the fused and the unfused bin edge differ: first those that reach into the map, then any in SEARCH_PX
    flips = edge_flips(scale, P, SEARCH_PX)
    inside = [f for f in flips if 0 <= f[1] < min(im_w, im_h)]
    for lo, hi, _ in (inside + flips)[:8]:
        r += [[0, lo, 3, hi, 40], [0, 5, lo, 60, hi]]
    # general position: fractional corners on a lattice that covers the image and its surroundings
    i = 0
    while len(r) < 88:
        x1, y1 = (i * 37.3) % (im_w + 16) - 8, (i * 23.7) % (im_h + 16) - 8
        r.append([0, x1, y1, x1 + 3 + (i * 11.9) % (im_w * 0.8), y1 + 2 + (i * 7.1) % (im_h * 0.8)])
        i += 1
    # batch index 1: one ROI of every class above again
    r += [[1] + row[1:] for row in r[::7]]
    return np.array(r, np.float32), len(flips), len([f for f in flips if f[0] >= 0 and f[1] >= 0])


# ---------------------------------------------------------------- Proposal ----------------------------------
def rpn_inputs(rs, B, H, W, A=9, frac_pos=0.1):
    logit = rs.randn(B, 2, A * H, W).astype(np.float32) * 2
    logit[:, 1] += np.log(frac_pos / (1 - frac_pos))
    e = np.exp(logit - logit.max(1, keepdims=True))
    prob = (e / e.sum(1, keepdims=True)).astype(np.float32).reshape(B, 2 * A, H, W)
    deltas = (rs.randn(B, 4 * A, H, W) * np.tile([0.1, 0.1, 0.4, 0.4], A)[None, :, None, None]).astype(np.float32)
    return prob, deltas


def proposal_cases():
    """name -> (inputs name, prob, deltas, im_info, dict(min_size, pre, post, threshold))"""
    H, W, A = 8, 10, 9
    cases = {}
    # (a) decode edges: two images of different real size and scale, one row of deltas x 6, an exp that overflows
    # float32 and one that underflows; boxes clip to the image
    rs = np.random.RandomState(101)
    prob, deltas = rpn_inputs(rs, 2, H, W)
    deltas[:, :, 3, :] *= 6
    deltas[0, 4 * 2 + 2, 3, 4] = 89.0           # exp -> inf
    deltas[1, 4 * 5 + 3, 3, 2] = -104.0         # exp -> 0
    im_info = np.array([[100, 140, 1.3], [128, 160, 1.0]], np.float32)
    cases["a"] = ("a", prob, deltas, im_info, dict(min_size=16, pre=300, post=50, threshold=0.7))
    # (b) ties and padding: 21 score values and a few signed zeros, identical boxes per anchor shape, most cells
    # beyond the real image (-1), pre above the anchor count, post above the survivors
    rs = np.random.RandomState(102)
    prob, deltas = rpn_inputs(rs, 1, H, W)
    prob = (np.round(prob * 20) / 20).astype(np.float32)
    fg = prob[0, A:]
    fg[0, 0, 0], fg[3, 1, 2], fg[8, 2, 3] = 0.0, 0.0, 0.0
    fg[1, 0, 1], fg[4, 2, 0], fg[7, 1, 3] = -0.0, -0.0, -0.0
    deltas[:] = 0
    im_info = np.array([[60, 70, 1.0]], np.float32)
    cases["b"] = ("b", prob, deltas, im_info, dict(min_size=0, pre=6000, post=300, threshold=0.7))
    # (c) pre = 200: the last 64-box block of the mask is partly filled; two thresholds on the same inputs
    rs = np.random.RandomState(103)
    prob, deltas = rpn_inputs(rs, 1, H, W)
    im_info = np.array([[128, 160, 1.0]], np.float32)
    cases["c07"] = ("c", prob, deltas, im_info, dict(min_size=16, pre=200, post=50, threshold=0.7))
    cases["c03"] = ("c", prob, deltas, im_info, dict(min_size=16, pre=200, post=50, threshold=0.3))
    return cases


# ---------------------------------------------------------------- motion vectors ----------------------------
MV_SIZES = [(37, 23), (96, 64)]
MV_FRAMES = 5


def synthetic_block_mvs(rs, width, height, n_extra=40):
    """as tests/test_hip_ops.py: the 16x16 macroblock grid with small motions, then scattered partitions"""
    rows = []
    for by in range(0, height, 16):
        for bx in range(0, width, 16):
            dx, dy = rs.randint(-9, 10), rs.randint(-9, 10)
            if rs.rand() < 0.2:
                dx = dy = 0
            rows.append([-1, 16, 16, bx + 8 - dx, by + 8 - dy, bx + 8, by + 8])
    for _ in range(n_extra):
        w, h = [(8, 8), (16, 8), (8, 16), (5, 7), (16, 16)][rs.randint(0, 5)]
        x, y = rs.randint(-4, width + 4), rs.randint(-4, height + 4)
        rows.append([-1, w, h, x - rs.randint(-20, 21), y - rs.randint(-20, 21), x, y])
    return rows


def edge_rows(width, height):
    cx, cy = width // 2, height // 2
    return [
        [-1, 1, 16, cx - 3, cy - 2, cx, cy], [-1, 16, 1, cx - 3, cy - 2, cx, cy],     # w or h = 1: covers nothing
        [-1, 5, 7, cx + 1, cy - 4, cx + 4, cy - 1],                                     # odd: covers 4 x 6
        [-1, 255, 4, cx - 3, cy + 1, cx, cy],                                           # w = 255
        [-1, 4, 255, cx + 2, cy - 1, cx, cy],
        [-1, 16, 16, width + 30, height + 30, width + 40, height + 40],                 # wholly outside
        [-1, 16, 16, -30, -30, 4, 4],                                                   # destination in, source out
        [-1, 16, 16, 6, 5, -20, -20],                                                   # source in, destination out
        [-1, 16, 16, 20, 12, 20, 12],                                                   # zero displacement
        [-1, 8, 8, 3, 3, 12, 10], [-1, 8, 8, 20, 5, 12, 10], [-1, 8, 8, 9, 15, 12, 10],  # one destination, three sources
        [-1, 16, 8, 1, 2, 0, 0], [-1, 8, 16, width - 9, height - 7, width - 1, height - 1],   # straddling the corners
    ]


def mv_frames(width, height):
    rs = np.random.RandomState(1000 + width)
    frames = []
    for f in range(MV_FRAMES):
        rows = synthetic_block_mvs(rs, width, height)
        if f in (1, 4):
            rows = rows + edge_rows(width, height)
        if f == 2:
            rows = edge_rows(width, height) + rows          # the edge rows first: later blocks write over them
        if f == 3:
            rows = []                                        # a frame with no rows
        frames.append(np.array(rows, np.int32).reshape(-1, 7))
    bgr = rs.randint(0, 256, (2, height, width, 3)).astype(np.uint8)
    return frames, bgr


# ---------------------------------------------------------------- the fixture -------------------------------
def _changed(a, b):
    return np.int64(np.count_nonzero(~((a == b) | ((a != a) & (b != b)))))


def generate(verbose=False):
    import oracle
    from oracle import ref_native
    assert ref_native.available(), "no reference tree at %s" % ref_native.reference_root()
    oracle.build()
    ref_native.build(force=True)
    ops = {m: ref_native.Ops(m) for m in ref_native.MODES}
    out = {}
    say = print if verbose else (lambda *a: None)

    def record(prefix, results):
        """results: mode -> {name: array}; stores the `on` arrays and, for each, how many values off / fast change"""
        for name, val in results["on"].items():
            out["%s_%s" % (prefix, name)] = val
            for m in ("off", "fast"):
                out["%s_%s__%s" % (prefix, name, m)] = _changed(val, results[m][name])
        say("%-10s %s" % (prefix, "  ".join("%s: off %d fast %d of %d" % (n, out["%s_%s__off" % (prefix, n)], out["%s_%s__fast" % (prefix, n)],
                                                                         v.size) for n, v in results["on"].items())))

    out["anchors"] = ops["on"].generate_anchors()
    for m in ("off", "fast"):
        out["anchors__%s" % m] = _changed(out["anchors"], ops[m].generate_anchors())

    N, D, H, W = PSROI_MAP
    for name, scale, P, G in PSROI_SETS:
        rs = np.random.RandomState(7 * P + G)
        data = rs.randn(N, D * G * G, H, W).astype(np.float16)
        rois, n_flips, n_flips_nonneg = psroi_rois(scale, P, H, W)
        out["psroi_%s_params" % name] = np.array([scale, D, P, G], np.float64)
        out["psroi_%s_data" % name] = data
        out["psroi_%s_rois" % name] = rois
        out["psroi_%s_edge_flips_nonneg" % name] = np.int64(n_flips_nonneg)
        out["psroi_%s_edge_flips" % name] = np.int64(n_flips)     # (corner pair, edge) triples in SEARCH_PX where fusing moves a floor / ceil
        res = {}
        for m, o in ops.items():
            pooled, mc = o.psroi_pool(data.astype(np.float32), rois, scale, D, P, G)
            res[m] = dict(out=pooled, map=mc)
        assert res["on"]["map"].max() < 256
        say("psroi_%s: %d ROIs, %d bin edges of integer corner pairs in [%d, %d) px that fusing moves across an integer, %d of them with both corners >= 0" %
            ((name, len(rois), n_flips) + SEARCH_PX + (n_flips_nonneg,)))
        record("psroi_%s" % name, res)
        out["psroi_%s_map" % name] = res["on"]["map"].astype(np.uint8)

    for name, (inputs, prob, deltas, im_info, par) in proposal_cases().items():
        out["prop_%s_prob" % inputs], out["prop_%s_deltas" % inputs], out["prop_%s_im_info" % inputs] = prob, deltas, im_info
        out["prop_%s_params" % name] = np.array([par["min_size"], par["pre"], par["post"], par["threshold"]], np.float64)
        res = {m: o.proposal(prob, deltas, im_info, rpn_pre_nms_top_n=par["pre"], rpn_post_nms_top_n=par["post"],
                             threshold=par["threshold"], rpn_min_size=par["min_size"]) for m, o in ops.items()}
        record("prop_%s" % name, res)
    # the fixture must be able to tell the contraction rule
    assert out["prop_a_decode__off"] > 0, "case (a): the unfused build changes nothing in the decode output"

    for width, height in MV_SIZES:
        frames, bgr = mv_frames(width, height)
        accu, mv, res = ref_native.coviar_gop(frames, width, height, bgr[0], bgr[1])
        key = "mv_%dx%d" % (width, height)
        out[key + "_rows"] = np.concatenate(frames)
        out[key + "_counts"] = np.array([len(f) for f in frames], np.int32)
        out[key + "_bgr"] = bgr                        # [0] the GOP's first frame, [1] the last frame
        out[key + "_accu"] = accu.astype(np.int16)     # coordinates: they fit
        out[key + "_mv"] = mv.astype(np.int16)
        out[key + "_res"] = res.astype(np.int16)
        assert np.array_equal(out[key + "_accu"], accu) and np.array_equal(out[key + "_res"], res)
        say("%s: %s rows per frame, %d of %d pixels moved" % (key, out[key + "_counts"].tolist(), int((mv != 0).any(-1).sum()), width * height))
    return out


def main():
    out = generate(verbose=True)
    np.savez_compressed(OUT, **out)
    print("%s: %d bytes, %d arrays" % (os.path.relpath(OUT, ROOT), os.path.getsize(OUT), len(out)))


if __name__ == "__main__":
    main()
