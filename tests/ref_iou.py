"""numpy statement of lsfa_amd/csrc/iou_test.h: "does this pair of boxes suppress?" in float32 and float64.

The kernels decide `fl(inter / uni) > thresh` (float32) and `not (inter / uni <= thresh)` (float64) from the sign of
d = fma(-thresh, uni, inter) and take the division only when they cannot tell.  This file restates every step in the
kernel's operation order and sorts each pair of a box list into one of five kinds:

  plain_keep / plain_suppress    the fast test answers (`unsure` stays false)
  sliver_keep / sliver_suppress  0 < d < thresh * 2^-22 * uni (2^-51 in float64): the division answers, keep / suppress
  degenerate                     !(uni > 0): zero, negative or NaN union, the division answers

With a threshold outside the fast range (`fast` is False) every pair divides: `unsure` is all True and the two sliver
kinds are empty.  d is computed exactly (fractions.Fraction) wherever a float64 estimate of it is not far from both 0 and
the sliver's upper edge, and rounded to the format once, as an fma does.

The sweeps are greedy NMS over boxes already in score order, on a pair matrix: `sweep(c.div)` is a second reference
beside oracle.nms_sorted / oracle.nms_f64; `sign_only_answer` and `never_redo_answer` are the two wrong kernels the tests
must be able to tell from the right one.
"""
from fractions import Fraction

import numpy as np

TILE = 64


class Classified(object):
    """Per-pair (n, n) arrays; every one is symmetric (see iou_test.h: max, min and + of two areas are symmetric)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def box_area(boxes):
    """(x2 - x1 + 1) * (y2 - y1 + 1) in the dtype of `boxes`."""
    one = boxes.dtype.type(1)
    return (boxes[:, 2] - boxes[:, 0] + one) * (boxes[:, 3] - boxes[:, 1] + one)


def inter_uni(boxes):
    """inter (n, n), uni (n, n) = (Sa + Sb) - inter in the dtype of `boxes`.  fmax / fmin are C's (a NaN operand loses),
    as on the device and in the oracle."""
    one, zero = boxes.dtype.type(1), boxes.dtype.type(0)
    with np.errstate(invalid="ignore", over="ignore"):
        S = box_area(boxes)
        left = np.fmax(boxes[:, None, 0], boxes[None, :, 0])
        right = np.fmin(boxes[:, None, 2], boxes[None, :, 2])
        top = np.fmax(boxes[:, None, 1], boxes[None, :, 1])
        bottom = np.fmin(boxes[:, None, 3], boxes[None, :, 3])
        width = np.fmax(right - left + one, zero)
        height = np.fmax(bottom - top + one, zero)
        inter = width * height
        uni = S[:, None] + S[None, :] - inter
    assert inter.dtype == boxes.dtype and uni.dtype == boxes.dtype
    return inter, uni


def make_iou_test(thresh, dtype):
    """(thresh, thresh_eps, fast) of make_iou_test / make_iou_test64, in `dtype`."""
    ty = np.dtype(dtype).type
    t = ty(thresh)
    if ty is np.float32:
        return t, t * np.float32(2.0 ** -22), bool(t > np.float32(1e-30) and t < np.float32(1e30))
    return t, t * np.float64(2.0 ** -51), bool(t > 1e-300 and t < 1e300)


def round_to_format(v, bits):
    """The Fraction nearest to the Fraction `v` with a `bits`-bit significand, ties to even (no under- or overflow: the
    callers' values are far from both)."""
    if v == 0:
        return Fraction(0)
    sign, a = (-1 if v < 0 else 1), abs(v)
    e = a.numerator.bit_length() - a.denominator.bit_length()       # 2^(e-1) < a < 2^(e+1)
    if a < Fraction(2) ** e:
        e -= 1                                                          # now 2^e <= a < 2^(e+1)
    ulp = Fraction(2) ** (e - bits + 1)
    q, r = divmod(a, ulp)
    q = int(q)
    if r * 2 > ulp or (r * 2 == ulp and (q & 1)):
        q += 1
    return sign * q * ulp


def exact_d(inter, uni, thresh, bits):
    """fma(-thresh, uni, inter) of finite operands: (the exact value, the value rounded once) as Fractions."""
    v = Fraction(float(inter)) - Fraction(float(thresh)) * Fraction(float(uni))
    return v, round_to_format(v, bits)


def classify(boxes, thresh, dtype):
    dtype = np.dtype(dtype)
    boxes = np.ascontiguousarray(np.asarray(boxes)[:, :4], dtype=dtype)
    n = boxes.shape[0]
    bits = 24 if dtype == np.float32 else 53
    t, eps, fast = make_iou_test(thresh, dtype)
    inter, uni = inter_uni(boxes)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        quo = inter / uni
        div = (quo > t) if dtype == np.float32 else ~(quo <= t)
        degenerate = ~(uni > 0)
        eps_uni = eps * uni                                   # the kernel's rounded product
        # float64 estimate of d: for float32 operands the product is exact and the sum is off by 2^-53 of the larger
        # term; for float64 operands product and sum are each off by 2^-53.  Pairs whose estimate is further from 0
        # than `near` are decided by it (the sliver ends at 2^-22 resp. 2^-51 of thresh * uni), the others exactly.
        t64, uni64, inter64 = np.float64(t), uni.astype(np.float64), inter.astype(np.float64)
        est = inter64 - t64 * uni64
        near = np.abs(t64 * uni64) * (2.0 ** -18 if bits == 24 else 2.0 ** -45)
        pos = est > 0
        clear = est >= near                                   # far above the sliver
        todo = np.isfinite(uni64) & np.isfinite(inter64) & (np.abs(est) <= near)
    if fast:
        for i, j in zip(*np.nonzero(todo)):
            v, d = exact_d(inter[i, j], uni[i, j], t, bits)
            pos[i, j] = d > 0
            clear[i, j] = d >= Fraction(float(eps_uni[i, j]))
    fast_answer = pos & clear                                 # what iou_exceeds_fast returns (a NaN d compares false)
    if fast:
        sliver = pos & ~clear & ~degenerate
        unsure = degenerate | sliver
    else:
        sliver = np.zeros((n, n), bool)
        unsure = np.ones((n, n), bool)
    plain = ~degenerate & ~sliver
    if fast:      # the fast test's own claim: where it is sure, it equals the division
        assert np.array_equal(fast_answer[~unsure], div[~unsure]), "iou_test.h's proof fails on these boxes"
    c = Classified(n=n, dtype=dtype, thresh=t, fast=fast, inter=inter, uni=uni, div=div, pos=pos, clear=clear,
                   fast_answer=fast_answer, unsure=unsure, degenerate=degenerate,
                   sliver_keep=sliver & ~div, sliver_suppress=sliver & div,
                   plain_keep=plain & ~div, plain_suppress=plain & div)
    for name in ("div", "pos", "clear", "unsure", "degenerate", "sliver_keep", "sliver_suppress", "plain_keep", "plain_suppress"):
        a = getattr(c, name)
        assert np.array_equal(a, a.T), "%s is not symmetric in row and column" % name
    return c


def sweep(answer, max_keep=None):
    """Greedy NMS over boxes in score order: box i survives iff no earlier survivor k has answer[k, i]."""
    n = answer.shape[0]
    removed = np.zeros(n, bool)
    later = np.arange(n)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        if max_keep is not None and len(keep) >= max_keep:
            break
        removed |= answer[i] & (later > i)
    return np.array(keep, np.int32)


def _tiles_with(flag):
    """(n, n) bool: the pair's 64 x 64 tile of sorted positions holds a pair with `flag` set."""
    n = flag.shape[0]
    nb = (n + TILE - 1) // TILE
    out = np.zeros_like(flag)
    for rb in range(nb):
        for cb in range(nb):
            sl = (slice(rb * TILE, (rb + 1) * TILE), slice(cb * TILE, (cb + 1) * TILE))
            out[sl] = flag[sl].any()
    return out


def sign_only_answer(c, tile_redo=False):
    """A fast test that answers from the sign of d alone and never calls the sliver unsure.  Degenerate unions (and
    every pair when the threshold is outside the fast range) still divide; with `tile_redo` so does every pair that
    shares a 64 x 64 tile with one, as in the kernels that redo a whole tile."""
    if not c.fast:
        return c.div.copy()
    redo = _tiles_with(c.degenerate) if tile_redo else c.degenerate
    return np.where(redo, c.div, c.pos)


def never_redo_answer(c):
    """`unsure` is ignored: the fast test's answer stands for every pair."""
    return c.fast_answer.copy()


def flip(answer, i, j):
    a = answer.copy()
    a[i, j] = a[j, i] = not a[i, j]
    return a
