"""hip._fp16_exponent, the Python statement of the fp16 two-piece form's exponent rule (weights: one exponent per tensor or per output
channel), against a plain integer restatement on math.frexp, at the edges of float32's exponent range.

The rule: e = 13 - floor(log2(amax)), so that amax * 2^e lies in [2^13, 2^14); 0 for a zero or non-finite maximum; clamped to +-100, which
binds for a maximum below 2^-87 (e would be > 100) and from 2^114 up (e would be < -100)."""
import math

import numpy as np
import pytest
import torch

from lsfa_amd import hip

F32_MAX = (2.0 - 2.0 ** -23) * 2.0 ** 127
BELOW_2_14 = 2.0 ** 14 - 2.0 ** -10                # the float32 just below 2^14 (spacing 2^-10 in [2^13, 2^14))

# (name, maximum, the exponent the rule gives without its clamp or None, the exponent it must return)
EDGES = [
    ("zero", 0.0, None, 0),
    ("smallest subnormal", 2.0 ** -149, 162, 100),
    ("smallest normal", 2.0 ** -126, 139, 100),
    ("2^-87: the last unclamped", 2.0 ** -87, 100, 100),
    ("2^-88: the first clamped", 2.0 ** -88, 101, 100),
    ("2^113: the last unclamped", 2.0 ** 113, -100, -100),
    ("2^114: the first clamped", 2.0 ** 114, -101, -100),
    ("2^13 exactly", 2.0 ** 13, 0, 0),
    ("just below 2^14", BELOW_2_14, 0, 0),
    ("largest finite float32", F32_MAX, -114, -100),
    ("inf", float("inf"), None, 0),
    ("nan", float("nan"), None, 0),
]


def restated(amax):
    """-> (the exponent without the clamp or None for zero / non-finite, the clamped exponent): integers only, from math.frexp
    (amax = m * 2^ex with m in [0.5, 1), so floor(log2(amax)) = ex - 1)"""
    if amax == 0.0 or math.isinf(amax) or math.isnan(amax):
        return None, 0
    raw = 13 - (math.frexp(amax)[1] - 1)
    return raw, max(-100, min(100, raw))


def check(amax, e):
    raw, want = restated(amax)
    assert e == want, (amax, e, want)
    if raw is None:
        assert e == 0
    elif raw == want:                                   # the clamp does not bind: the maximum lands in fp16's top binades
        assert 2.0 ** 13 <= math.ldexp(amax, e) < 2.0 ** 14, (amax, e)
    else:
        assert abs(e) == 100 and (e > 0) == (raw > 0), (amax, e, raw)


def test_the_table_is_the_restatement():
    """the expectations written out above are what the frexp restatement gives (the table is no third opinion)"""
    for name, amax, raw, want in EDGES:
        assert restated(amax) == (raw, want), name
    assert float(torch.tensor(BELOW_2_14, dtype=torch.float32)) == BELOW_2_14 and float(torch.tensor(F32_MAX, dtype=torch.float32)) == F32_MAX
    assert float(np.nextafter(np.float32(BELOW_2_14), np.float32(np.inf))) == 2.0 ** 14


@pytest.mark.parametrize("name,amax,raw,want", EDGES, ids=[e[0] for e in EDGES])
def test_fp16_exponent_scalar(name, amax, raw, want):
    """the per-tensor use: a 0-d float64 tensor -> an int32 exponent"""
    e = hip._fp16_exponent(torch.tensor(amax, dtype=torch.float64))
    assert e.dtype == torch.int32 and e.shape == ()
    assert int(e.item()) == want
    check(amax, int(e.item()))


def test_fp16_exponent_vector_mixes_all_edges():
    """the per-channel use: every edge in one vector, each entry judged on its own (no entry's zero / inf / NaN leaks into a neighbour)"""
    amax = torch.tensor([e[1] for e in EDGES], dtype=torch.float64)
    got = hip._fp16_exponent(amax)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(EDGES),)
    assert got.tolist() == [e[3] for e in EDGES]
    for a, e in zip(amax.tolist(), got.tolist()):
        check(a, e)


def test_fp16_exponent_every_binade_of_float32():
    """both ends of every binade of float32, subnormals included, as one vector: the scaled maximum lies in [2^13, 2^14) wherever the clamp does
    not bind, and the clamped value is returned elsewhere"""
    vals = []
    for ex in range(-149, 128):
        vals.append(2.0 ** ex)
        if ex >= -126:
            vals.append((2.0 - 2.0 ** -23) * 2.0 ** ex)          # the float32 just below 2^(ex + 1)
    got = hip._fp16_exponent(torch.tensor(vals, dtype=torch.float64)).tolist()
    for a, e in zip(vals, got):
        check(a, e)
