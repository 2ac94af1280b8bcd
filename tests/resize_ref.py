"""Exact-arithmetic reference of the crop resize (cv::resize INTER_AREA, 8UC3).

Plain numpy and `fractions`; no project code.  One weight matrix per axis,
Wy (dh x sh) and Wx (dw x sw), is built in exact rationals and converted to
float64 at the end; the result is

    einsum('ys,stc,xt->yxc', Wy, img.astype(float64), Wx)

and is NOT rounded.  The float64 evaluation adds less than 1e-9 (weights in
[0, 1] that sum to 1, bytes, at most a few thousand terms).

Axis rules (ssize -> dsize, scale = ssize / dsize, inv = dsize / ssize)

* box axis: the weight of source s for destination d is the length of
  [s, s + 1) n [d * scale, min((d + 1) * scale, ssize)), normalised to sum 1:
  the area integral of a piecewise-constant image.  Used for both axes when
  neither is upscaled (kinds 0, 1, 2) and for an upscaled (or equal) axis of
  kind 3, where OpenCV's "area mode" linear tap f = (d + 1) - (s + 1) * inv
  is exactly this overlap fraction (box_equals_two_tap checks it).
* two-tap axis: a downscaled axis of kind 3, the published formula
  s = floor(d * scale), f = (d + 1) - (s + 1) * inv, f = 0 if f <= 0 else
  f - floor(f), s clamped to the last source index with f = 0.

Knife edges.  Both floors act on values that can be exact integers
(d * ssize / dsize for d > 0, and f); in double precision the product lands
on either side and the implementation then takes one neighbour outright.
For such indices the reference also builds the row for the lower one-sided
limit of each floor, so an axis of kind 3 has up to four variants (three
distinct ones: the exact row, all weight on s - 1, all weight on s); a
pixel passes when it is within the bound of any combination.  The box
weights are continuous in the cell's edges, so kinds 0-2 have one variant.

Bounds (|implementation - exact|, in grey levels)

area_bound(sh, sw, dh, dw) = 0.5 + eps_f32 + eps_sliver + 1e-9   (cap 0.75)
  0.5         the final rint of the float32 sum.
  eps_f32     the float32 evaluation.  Every partial sum is < 256 (bytes
              times weights that sum to 1 + O(2^-20)), so each float32
              product or sum rounds by at most half an ulp of [128, 256),
              2^-17, and later factors (weights <= 1) do not grow it.  A
              pixel with nx x ny taps takes nx products + nx sums per source
              row, one product + one sum per row into the total, and the
              float32 roundings of the weights themselves add
              255 * 2^-24 per axis (< 2 * 2^-17 together):
              eps_f32 = (2 nx ny + 2 ny + 4) * 2^-17, nx = ceil(scale_x) + 1.
              The integer-scale branch (int sum * float(1 / area)) has two
              roundings and is covered by the same expression.
  eps_sliver  computeResizeAreaTab drops a partial tap whose overlap is
              <= 1e-3 source pixels and does not renormalise, so the dropped
              weight (overlap / cell width) times 255 is lost.  Overlaps are
              multiples of 1 / dsize, so for dsize < 1000 nothing is
              dropped; otherwise the largest dropped weight per axis is
              computed in rationals from the sizes alone.

LINEAR_BOUND = 0.75 + A + B + 2e-4 = 1.0066                      (cap 1.5)
  Q11 coefficients c0 = rn((1 - f) * 2048), c1 = rn(f * 2048): each is off
  by at most 2^-12 (+ 2^-23 for f and 1 - f in float32, the 2e-4 term).
  A  horizontal: |p0 e0 + p1 e1| <= 255 * 2 * 2^-12 = 0.12451, and the
     `>> 4` truncation of h (units of 1/128): (15/16) / 128 = 0.00733.
  B  vertical coefficients on a row value <= 255 * 2049 / 2048:
     2 * 2^-12 * 255.125 = 0.12457.
  0.75  x = m0 + m1 loses [0, 2) quarter-levels to the two `>> 16`
     truncations, i.e. x / 4 is low by [0, 0.5); (x + 2) >> 2 on an integer
     x lies in [x / 4 - 0.25, x / 4 + 0.5].  Together the result lies in
     (-0.75, +0.5] around the Q11 value.  The scalar tail
     ((.. + 2^21) >> 22) is a plain rounding, 0.5, and is covered.
"""
import functools
import math
from fractions import Fraction as F

import numpy as np

AREA_CAP = 0.75
LINEAR_CAP = 1.5
_A = 255 * 2 * 2.0 ** -12 + (15 / 16) / 128
_B = 2 * 2.0 ** -12 * (255 * 2049 / 2048)
LINEAR_BOUND = 0.75 + _A + _B + 2e-4
assert LINEAR_BOUND < LINEAR_CAP


def kind_of(sh, sw, dh, dw):
    """0 copy, 1 integer scales, 2 area (no axis upscaled), 3 otherwise."""
    if (sh, sw) == (dh, dw):
        return 0
    if sw >= dw and sh >= dh:
        return 1 if sw % dw == 0 and sh % dh == 0 else 2
    return 3


def box_row(ssize, dsize, d):
    lo, hi = F(d * ssize, dsize), min(F((d + 1) * ssize, dsize), F(ssize))
    row = {}
    for s in range(math.floor(lo), math.ceil(hi)):
        ov = min(hi, F(s + 1)) - max(lo, F(s))
        if ov > 0:
            row[s] = ov / (hi - lo)
    return row


def two_tap_rows(ssize, dsize, d):
    """The published two-tap row of destination d, then the rows of the lower
    one-sided limits of its floors (only where a floor acts on an integer)."""
    x, inv = F(d * ssize, dsize), F(dsize, ssize)
    ss = [math.floor(x)]
    if x.denominator == 1 and d > 0:
        ss.append(math.floor(x) - 1)
    rows = []
    for s in ss:
        f = (d + 1) - (s + 1) * inv
        if f <= 0:
            fs = [F(0)]
        else:
            fs = [f - math.floor(f)]
            if f.denominator == 1:
                fs.append(f - (math.floor(f) - 1))
        for f in fs:
            s0 = s
            if s0 >= ssize - 1:
                s0, f = ssize - 1, F(0)
            row = {s0: 1 - f}
            if f:
                row[s0 + 1] = f
            row = {k: v for k, v in row.items() if v}
            if row not in rows:
                rows.append(row)
    return rows


def _dense(rows, ssize):
    W = np.zeros((len(rows), ssize), np.float64)
    for d, row in enumerate(rows):
        assert sum(row.values()) == 1 and min(row) >= 0 and max(row) < ssize
        for s, w in row.items():
            W[d, s] = float(w)
    return W


@functools.lru_cache(maxsize=None)
def axis_weights(ssize, dsize, linear):
    """Weight matrices (dsize x ssize) of one axis: [exact, variants...]
    (cached: callers do not write to them)."""
    if not linear:
        return [_dense([box_row(ssize, dsize, d) for d in range(dsize)], ssize)]
    var = [two_tap_rows(ssize, dsize, d) for d in range(dsize)]
    if ssize <= dsize:
        first = [box_row(ssize, dsize, d) for d in range(dsize)]
    else:
        first = [v[0] for v in var]
    mats = [_dense(first, ssize)]
    for n in range(1, max(len(v) for v in var)):
        mats.append(_dense([v[min(n, len(v) - 1)] if len(v) > 1 else first[d] for d, v in enumerate(var)], ssize))
    return mats


def box_equals_two_tap(ssize, dsize):
    """On an upscaled axis the exact two-tap row is the box row."""
    return all(two_tap_rows(ssize, dsize, d)[0] == box_row(ssize, dsize, d) for d in range(dsize))


def apply(Wy, img, Wx):
    return np.einsum('ys,stc,xt->yxc', Wy, np.asarray(img, np.float64), Wx, optimize=True)  # (one axis at a time)


def resize_exact(img, dh, dw):
    """(kind, [outputs]): the exact result first, then the knife-edge variant
    combinations (kind 3 only)."""
    sh, sw = img.shape[:2]
    k = kind_of(sh, sw, dh, dw)
    Wys, Wxs = axis_weights(sh, dh, k == 3), axis_weights(sw, dw, k == 3)
    return k, [apply(Wy, img, Wx) for Wy in Wys for Wx in Wxs]


@functools.lru_cache(maxsize=None)
def _sliver(ssize, dsize):
    """Largest weight computeResizeAreaTab may drop from one cell."""
    if dsize < 999:
        return 0.0
    lim = F(1001, 1000000)
    worst = F(0)
    for d in range(dsize):
        lo, hi = F(d * ssize, dsize), min(F((d + 1) * ssize, dsize), F(ssize))
        a, b = math.ceil(lo) - lo, hi - math.floor(hi)
        worst = max(worst, ((a if a <= lim else 0) + (b if b <= lim else 0)) / (hi - lo))
    return float(worst)


def area_bound(sh, sw, dh, dw):
    nx, ny = -(-sw // dw) + 1, -(-sh // dh) + 1
    eps_f32 = (2 * nx * ny + 2 * ny + 4) * 2.0 ** -17
    b = 0.5 + eps_f32 + 255 * (_sliver(sw, dw) + _sliver(sh, dh)) + 1e-9
    assert b < AREA_CAP, (sh, sw, dh, dw, b)
    return b


def bound_of(sh, sw, dh, dw):
    return LINEAR_BOUND if kind_of(sh, sw, dh, dw) == 3 else area_bound(sh, sw, dh, dw)


def compare(got, img, dh=None, dw=None):
    """got (dh, dw, 3) against the exact resize of img.  Returns (worst error
    after the knife-edge rule, worst error against the exact row alone,
    pixels that needed a variant, variant combinations, bound)."""
    dh, dw = got.shape[:2] if dh is None else (dh, dw)
    sh, sw = img.shape[:2]
    _, refs = resize_exact(img, dh, dw)
    bound = bound_of(sh, sw, dh, dw)
    g = np.asarray(got, np.float64)
    e0 = np.abs(g - refs[0]).max(-1)
    best = e0
    for r in refs[1:]:
        best = np.minimum(best, np.abs(g - r).max(-1))
    needed = int(((e0 > bound) & (best <= bound)).sum())
    return float(best.max()), float(e0.max()), needed, len(refs), bound
