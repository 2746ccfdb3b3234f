"""The specification of stem_conv_kernel (lsfa_amd/csrc/stem.hip), in numpy / torch-on-CPU float64, for tests/test_stem_edges_cpu.py
and tests/test_stem_edges_gpu.py: the operands the convolution really sees, a float64 convolution of them, the launch arithmetic
restated, a PER-ELEMENT worst-case error bound derived from the kernel's stated arithmetic, and an emulation of that arithmetic with
switches for three mutants (what the bound has to tell from the kernel).

The kernel's arithmetic, as stem.hip states it.  An input value is x' = fl32(fl32(x * in_scale) + in_shift) (two roundings: the library
is built with -ffp-contract=off, lsfa_amd/build.py), zero in the padding.  A 4 x 32 tile of outputs reads a 3 x 14 x 70 patch, rows
[8 r - 3, 8 r + 11) and columns [64 t - 4, 64 t + 66) of the image.  With m the largest |x'| of the PATCH, s = 2^(13 - floor(log2 m))
(scale_of; 1 when m's biased exponent is below 32 or above 240), a = x' s is cut into hi = fp16(a), lo = fp16(a - hi).  The weights of
output channel co are cut the same way with the scale of the channel's largest |w|.  Per tap three products, lo hi + hi lo + hi hi, are
added in fp32 (the lo lo product is dropped); the sum is multiplied by 1 / (s_x s_w), then + bias, + accum, activation.

The bound (bound()), per output element, four terms, derived here and not fitted to any run:

  cut + sum   (3.01 * 2^-22 + 1.01 * gamma(441)) * A, A = sum |x'| |w| over the window, gamma(n) = n u / (1 - n u), u = 2^-24.
              hi is within 2^-11 |a| of a and the residual a - hi is exact in fp32, so lo is within 2^-11 of the residual: the pair is
              within 2^-22 |a| of a, for either operand: 2 * 2^-22 |x'| |w| for the two kept cross terms, and |lo_x lo_w| <= 2^-22
              |x'| |w| (1 + 2^-10) for the dropped one: 3.01 * 2^-22.  The products of fp16 values are exact in fp32.  147 real taps x 3
              products are added in fp32 in an order the hardware does not state; every term passes through at most 440 additions,
              each ASSUMED to have a relative error of at most u: gamma(441) on the sum of the absolute products, which is at most
              (1 + 2^-10)^2 A: 1.01.  (The 45 padded taps multiply by exact zeros.)
  fp16 floor  2^-36 * (X wmax[co] + m sum |w[co]|), X = sum |x'| over the window.  Where a piece falls into fp16's subnormal range its
              error is absolute, 2^-25 in the scaled domain; a s >= 2^13 for a = m, so 2^-25 / s <= 2^-38 m per input value, and
              2^-38 wmax per weight.  Summed over the window against the other operand, with a factor 4 for the second piece, the cross
              terms and the dropped product.
  flush       a patch whose m has a biased exponent below 32 (m < 2^-95) is cut with s = 1: every value is below fp16's smallest
              subnormal and the convolution is lost whole: |x'| <= m < 2^-95, so the loss is at most 2^-95 sum |w[co]| (this replaces
              the two terms above).  Everywhere, 4 * 2^-149 for results in fp32's own subnormal range.
  epilogue    u * (|c + bias| + |c + bias + accum| + |0.1 v|), c the exact convolution, each term only where the kernel performs the
              operation: the additions of bias and of accum and LeakyReLU's product, one rounding each, on the value they produce
              (the multiplication by 1 / (s_x s_w) is exact).  At most u * (2 |v| + |accum| + |0.1 v|).

The bound is not defined (NaN) where the window or the patch holds a non-finite value or the patch maximum's biased exponent is above
240 (s = 1 and fp16 overflows): the tests treat those elements by the non-finite rule instead.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
TILE_ROWS, TILE_COLS = 4, 32
PATCH_ROWS, PATCH_COLS = 14, 70
SLOPE = np.float32(0.1)            # the kernel's LeakyReLU slope, an fp32 constant


def gamma(n, u=U):
    return n * u / (1.0 - n * u)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def operands(x, in_scale=None, in_shift=None):
    """x (N, 3, H, W) -> the map the convolution sees, float32: fl32(fl32(x * sc) + sh) per channel (x itself without an affine)"""
    x = f32(x)
    if in_scale is None:
        assert in_shift is None
        return x
    prod = x * f32(in_scale).reshape(1, 3, 1, 1)                # first rounding
    return prod + f32(in_shift).reshape(1, 3, 1, 1)             # second rounding


def activate(v, act):
    """0 none, 1 ReLU, 2 LeakyReLU(0.1f); NaN stays NaN"""
    if act == 1:
        return np.where(v < 0, 0.0, v)
    if act == 2:
        return np.where(v < 0, v * np.float64(SLOPE), v)
    assert act == 0
    return v


def _conv64(x, w):
    y = F.conv2d(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)), torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)), None, 2, 3)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def window_holds_nonfinite(xa):
    """(N, Ho, Wo) bool: the 7 x 7 x 3 window of the output holds a NaN or an infinity"""
    bad = (~np.isfinite(f32(xa))).astype(np.float64)
    return _conv64(bad, np.ones((1, 3, 7, 7)))[..., 0] > 0


def pre_activation(xa, w, bias=None, accum=None):
    """float64 (N, Ho, Wo, 64): conv 7x7 / stride 2 / pad 3 of xa (N, 3, H, W) with w (64, 3, 7, 7) + bias + accum (channels-last);
    NaN wherever the window holds a non-finite value"""
    xa = f32(xa)
    v = _conv64(np.where(np.isfinite(xa), xa, 0), w)
    if bias is not None:
        v = v + np.asarray(bias, np.float64)
    if accum is not None:
        v = v + np.asarray(accum, np.float64)
    v[window_holds_nonfinite(xa)] = np.nan
    return v


def conv_ref(xa, w, bias=None, accum=None, act=1):
    return activate(pre_activation(xa, w, bias, accum), act)


class Geometry(object):
    """stem_launch's arithmetic for (N, 3, H, W): Ho, Wo, xt, yt (tiles per row, tile rows), want, gx, tpw (tiles a workgroup walks),
    grid_x (workgroups per row of tiles), slots = grid_x * tpw (>= xt; the walk breaks at the unused ones)"""

    def __init__(self, N, H, W):
        self.N, self.H, self.W = N, H, W
        self.Ho, self.Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
        self.xt, self.yt = (self.Wo + TILE_COLS - 1) // TILE_COLS, (self.Ho + TILE_ROWS - 1) // TILE_ROWS
        self.want = max((self.xt * self.yt * N) // 512, 1)
        self.gx = (self.xt + self.want - 1) // self.want
        self.tpw = (self.xt + self.gx - 1) // self.gx
        self.grid_x = (self.xt + self.tpw - 1) // self.tpw
        self.slots = self.grid_x * self.tpw

    def patch(self, r, t):
        """(y0, y1, x0, x1): the patch of tile (row r, column t), clipped to the image"""
        return max(8 * r - 3, 0), min(8 * r - 3 + PATCH_ROWS, self.H), max(64 * t - 4, 0), min(64 * t - 4 + PATCH_COLS, self.W)

    def whole(self, t):
        return (t + 1) * TILE_COLS <= self.Wo

    def walk(self, t):
        """(workgroup, position in its walk) of tile column t"""
        return t // self.tpw, t % self.tpw

    def more(self, t):
        """the kernel's `more` at tile column t: another patch is loaded while this tile multiplies"""
        return self.walk(t)[1] + 1 < self.tpw and (t + 1) * TILE_COLS < self.Wo


def geometry(N, H, W):
    return Geometry(N, H, W)


def patch_max_bits(xa, g=None):
    """(N, yt, xt) uint32: the bit pattern of the largest |xa| of every tile's patch (a NaN ranks above everything, as in the kernel)"""
    xa = f32(xa)
    N, _, H, W = xa.shape
    g = g or geometry(N, H, W)
    bits = np.abs(xa).view(np.uint32)
    out = np.zeros((N, g.yt, g.xt), np.uint32)
    for r in range(g.yt):
        for t in range(g.xt):
            y0, y1, x0, x1 = g.patch(r, t)
            out[:, r, t] = bits[:, :, y0:y1, x0:x1].reshape(N, -1).max(1)
    return out


def _per_output(tiles, g):
    """(N, yt, xt) -> (N, Ho, Wo): every output gets its tile's value"""
    return np.repeat(np.repeat(tiles, TILE_ROWS, 1), TILE_COLS, 2)[:, :g.Ho, :g.Wo]


def scale_of(bits):
    """scale_of of stem.hip on bit patterns: (s, 1 / s) float32, 1 where the biased exponent is outside [32, 240]"""
    be = ((np.asarray(bits, np.uint32) >> 23) & 255).astype(np.int64)
    ok = (be >= 32) & (be <= 240)
    s = np.where(ok, (np.where(ok, 267 - be, 127) << 23).astype(np.uint32).view(np.float32), np.float32(1))
    inv = np.where(ok, (np.where(ok, be - 13, 127) << 23).astype(np.uint32).view(np.float32), np.float32(1))
    return s.astype(np.float32), inv.astype(np.float32)


def bound(xa, w, bias=None, accum=None, act=1):
    """(N, Ho, Wo, 64) float64: the worst-case |kernel - conv_ref| per element (module docstring); NaN where it is not defined"""
    xa, w = f32(xa), f32(w)
    N, _, H, W = xa.shape
    g = geometry(N, H, W)
    fin = np.where(np.isfinite(xa), xa, 0)
    aw = np.abs(w).astype(np.float64)
    A = _conv64(np.abs(fin), aw)
    X = _conv64(np.abs(fin), np.ones((1, 3, 7, 7)))
    wmax, wsum = aw.reshape(64, -1).max(1), aw.reshape(64, -1).sum(1)
    mb = _per_output(patch_max_bits(xa, g), g)
    be = (mb >> 23) & 255
    m = np.where(be < 255, mb.view(np.float32), 0).astype(np.float64)[..., None]
    b = (3.01 * 2.0 ** -22 + 1.01 * gamma(441)) * A + 2.0 ** -36 * (X * wmax + m * wsum)
    b = np.where((be < 32)[..., None], 2.0 ** -95 * wsum, b) + 4 * 2.0 ** -149
    v = _conv64(fin, w)
    e = np.zeros_like(v)
    if bias is not None:
        v = v + np.asarray(bias, np.float64)
        e = e + np.abs(v)
    if accum is not None:
        v = v + np.asarray(accum, np.float64)
        e = e + np.abs(v)
    if act == 2:
        e = e + np.abs(np.float64(SLOPE) * v)
    b = b + U * e
    b[window_holds_nonfinite(xa) | (be > 240)] = np.nan
    return b


def ratio(got, ref, bnd):
    """|got - ref| / bound per element (0 where both are 0, inf where only the bound is); NaN where the bound is not defined"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), np.where(np.isnan(bnd), np.nan, np.where(err > 0, np.inf, 0.0)))


def old_criterion(got, ref):
    """max err / (2e-6 sqrt(147) max(max|ref|, 1)): the map-wide criterion of tests/test_hip_ops.py::test_stem_conv_pool_vs_torch (< 1)"""
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / (2e-6 * np.sqrt(147) * max(float(np.abs(ref).max()), 1.0)))


def _cut(a):
    with np.errstate(over="ignore", invalid="ignore"):
        hi = a.astype(np.float16)
        lo = (a - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float32), lo.astype(np.float32)


MUTANTS = ("drop_lo_hi", "neighbour_scale", "zero_tap_kx", "zero_tap_ky")


def emulate(xa, w, bias=None, accum=None, act=1, mutant=None, channels=None):
    """The kernel's arithmetic in numpy float32, tile by tile: every output's inputs are cut with the scale of ITS tile's patch (an input
    value under two patches is cut twice, as in the kernel), the weights per output channel; lo hi, hi lo and hi hi are three fp32
    matrix products added in that order; * (inv_x * inv_w); + bias; + accum; max(v, 0) + slope min(v, 0).
    mutant: None, or
      'drop_lo_hi'       the lo(x) hi(w) product is left out
      'neighbour_scale'  tile column t > 0 is cut with the scale of tile t - 1 of its row (a slip of the exchange slots' parity)
      'zero_tap_kx'      the zero-weight tap sits behind the seven kx taps instead of in front: tap kx reads the column one to the left
      'zero_tap_ky'      the zero-weight row sits in front of the seven ky rows instead of behind: tap ky reads the row above
    channels: the output channels to compute (all 64 by default) -> (N, Ho, Wo, len(channels)) float32"""
    assert mutant is None or mutant in MUTANTS
    xa, w = f32(xa), f32(w)
    N, _, H, W = xa.shape
    g = geometry(N, H, W)
    ch = np.arange(64) if channels is None else np.asarray(channels)
    tb = patch_max_bits(xa, g)
    if mutant == "neighbour_scale":
        tb = np.concatenate([tb[:, :, :1], tb[:, :, :-1]], 2)
    sx, inv_x = scale_of(_per_output(tb, g))                    # (N, Ho, Wo)
    wsel = w[ch]
    sw, inv_w = scale_of(np.abs(wsel).reshape(len(ch), -1).max(1).view(np.uint32))
    wh, wl = _cut(wsel * sw[:, None, None, None])
    dy, dx = (-1 if mutant == "zero_tap_ky" else 0), (-1 if mutant == "zero_tap_kx" else 0)
    xp = np.zeros((N, 3, H + 8, W + 8), np.float32)             # padding 4: the mutants read one further
    xp[:, :, 4:4 + H, 4:4 + W] = xa
    cols = np.empty((N, g.Ho, g.Wo, 147), np.float32)
    for ci in range(3):
        for ky in range(7):
            for kx in range(7):
                y0, x0 = ky - 3 + dy + 4, kx - 3 + dx + 4
                cols[..., (ci * 7 + ky) * 7 + kx] = xp[:, ci, y0:y0 + 2 * g.Ho:2, x0:x0 + 2 * g.Wo:2]
    with np.errstate(over="ignore", invalid="ignore"):
        ah, al = _cut(cols * sx[..., None])
        ah, al = ah.reshape(-1, 147), al.reshape(-1, 147)
        bh, bl = wh.reshape(len(ch), 147).T.copy(), wl.reshape(len(ch), 147).T.copy()
        acc = np.zeros((ah.shape[0], len(ch)), np.float32)
        if mutant != "drop_lo_hi":
            acc = acc + al @ bh
        acc = acc + ah @ bl
        acc = acc + ah @ bh
        inv = inv_x.reshape(-1, 1) * inv_w.reshape(1, -1)
        v = acc * inv
        v = v + (f32(bias)[ch] if bias is not None else np.float32(0))
        v = v.reshape(N, g.Ho, g.Wo, len(ch))
        if accum is not None:
            v = v + f32(accum)[..., ch]
        slope = np.float32(0.0 if act == 1 else (SLOPE if act == 2 else 1.0))
        out = np.maximum(v, np.float32(0)) + slope * np.minimum(v, np.float32(0))
    return out.astype(np.float32)                               # numpy's maximum / minimum keep a NaN


def avgpool_full_f32_in_order(x, k):
    """avgpool_kernel's statement in numpy float32: (N, C, H, W) -> (N, C, ceil(H / k), ceil(W / k)); the pixels of the window clipped to
    the image are added row by row onto 0, then one division by the number of pixels the clipped window holds"""
    x = f32(x)
    N, C, H, W = x.shape
    Ho, Wo = -(-H // k), -(-W // k)
    s = np.zeros((N, C, Ho, Wo), np.float32)
    cnt = np.zeros((Ho, Wo), np.float32)
    for dy in range(k):
        for dx in range(k):
            v = x[:, :, dy::k, dx::k]
            s[:, :, :v.shape[2], :v.shape[3]] = s[:, :, :v.shape[2], :v.shape[3]] + v
            cnt[:v.shape[2], :v.shape[3]] += 1
    return s / cnt
