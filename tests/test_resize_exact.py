"""The resize is pinned to exact arithmetic (CPU only).

Every GPU resize test compares bit for bit with the oracle's restatement of
cv::resize(INTER_AREA); here the oracle itself, and the product library's
host `resize`, are compared with tests/resize_ref.py: per-axis weight
matrices in exact rationals (area integral; the published two-tap formula
on a downscaled axis of the linear kind), unrounded.  A tap, weight or row
range misread in BOTH restatements would pass every bit-exact test and
fails here.

Bounds (derived in resize_ref.py, never taken from the code under test)

  area kinds 0-2   0.5 + eps_f32 + eps_sliver, per shape; cap 0.75.
                   eps_f32 = (2 nx ny + 2 ny + 4) * 2^-17 (float32 sums of
                   values < 256), eps_sliver = 255 * the weight the 1e-3
                   sliver rule of computeResizeAreaTab may drop (0 for
                   outputs under 1000 px).  Largest value in this file:
                   0.5 + 0.125 at 89x89 -> 1x1 (90 x 90 taps).
  linear kind 3    0.75 + 0.13184 + 0.12457 + 2e-4 = 1.0066; cap 1.5
                   (two Q11 coefficient roundings of 2^-12 per axis, the
                   >> 4 and the two >> 16 truncations, (t + 2) >> 2).

Observed against the oracle over this file's table (not asserted):
  area kinds 0.5000000000002, linear kind 0.8068 (the host library: the same);
  350 of 685,314 pixels (0.051 %) needed a knife-edge variant, 440 of the 638
  shapes are coprime on both axes.

Knife edges: where d * ssize / dsize is an integer the implementation may
take either neighbour; the reference offers the one-sided limits as
variants.  Over the table at most 1 % of pixels may need one; shapes whose
axes both have gcd(ssize, dsize) == 1 (at least half of the table) have no
such index and must pass on the exact rows alone.
"""
import math

import numpy as np
import pytest

from ffcv_amd.synthetic import natural_image
from tests import resize_ref as R

# (sh, sw, dh, dw); the class of each row is computed, see test_table_covers_every_kind
TABLE = [
    # copy
    (1, 1, 1, 1), (7, 5, 7, 5), (33, 20, 33, 20),
    # integer scales: 2x, 3x, 2x3 (either way), 1 x n
    (8, 10, 4, 5), (20, 30, 10, 15), (9, 12, 3, 4), (6, 9, 3, 3), (12, 8, 4, 4), (89, 89, 1, 1), (5, 21, 5, 7),
    # area, both scales in (1, 2)
    (7, 9, 5, 7), (31, 45, 17, 29), (50, 41, 37, 23), (89, 88, 69, 67), (12, 18, 8, 12),
    # area, one or both scales >= 2 (and sources 1 px high / wide)
    (20, 30, 7, 20), (45, 50, 9, 7), (64, 17, 3, 17), (1, 40, 1, 7), (40, 1, 9, 1), (88, 89, 3, 2), (30, 45, 10, 31),
    # kind 3, both axes up
    (5, 7, 11, 13), (1, 1, 5, 7), (10, 9, 33, 20), (1, 6, 4, 13), (6, 1, 13, 4), (8, 12, 16, 18),
    # kind 3, x up and y down
    (40, 9, 16, 32), (23, 5, 7, 19), (64, 3, 5, 16), (12, 8, 8, 16), (40, 1, 9, 3),
    # kind 3, x down and y up
    (9, 40, 32, 16), (5, 23, 19, 7), (8, 12, 16, 8), (1, 50, 3, 7), (3, 64, 16, 5),
]


def _class(sh, sw, dh, dw):
    k = R.kind_of(sh, sw, dh, dw)
    if k == 0:
        return 'copy'
    if k == 1:
        return 'int'
    if k == 2:
        return 'area<2' if sw < 2 * dw and sh < 2 * dh else 'area>=2'
    if sw <= dw and sh <= dh:
        return 'lin-up-up'
    return 'lin-xup-ydown' if sw <= dw else ('lin-xdown-yup' if sh <= dh else 'lin-other')


def _coprime(s):
    return math.gcd(s[0], s[2]) == 1 and math.gcd(s[1], s[3]) == 1


def _shapes():
    rng = np.random.default_rng(20240)
    out = list(TABLE)
    for k in range(600):  # source sides 1-89, output sides 1-69; every second one redrawn until coprime
        while True:
            s = (int(rng.integers(1, 90)), int(rng.integers(1, 90)), int(rng.integers(1, 70)), int(rng.integers(1, 70)))
            if k % 2 or _coprime(s):
                break
        out.append(s)
    return out


def _content(rng, k, h, w):
    if k % 3 == 0:
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if k % 3 == 1:
        return natural_image(rng, h, w)
    return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)


_CASES = None


def _cases():
    """[(shape, image)], built once; the images sit inside a larger source so
    the crop offsets are exercised too."""
    global _CASES
    if _CASES is None:
        rng = np.random.default_rng(7)
        _CASES = []
        for k, s in enumerate(_shapes()):
            sh, sw = s[:2]
            i, j = k % 3, (k // 3) % 4
            src = _content(rng, k, sh + i + 1, sw + j + 2)
            _CASES.append((s, src, i, j))
    return _CASES


def _sweep(resize):
    """Worst error per kind group, knife-edge pixel count, total pixels."""
    worst = {'area': 0.0, 'linear': 0.0}
    needed = total = 0
    for (sh, sw, dh, dw), src, i, j in _cases():
        got = resize(src, i, i + sh, j, j + sw, dh, dw)
        err, _, n, nvar, bound = R.compare(got, src[i:i + sh, j:j + sw])
        assert err <= bound, ((sh, sw, dh, dw), err, bound)
        if _coprime((sh, sw, dh, dw)):
            assert nvar == 1 and n == 0, (sh, sw, dh, dw)
        key = 'linear' if R.kind_of(sh, sw, dh, dw) == 3 else 'area'
        worst[key] = max(worst[key], err)
        needed += n
        total += dh * dw
    return worst, needed, total


def _report(name, worst, needed, total):
    shapes = [c[0] for c in _cases()]
    ncop = sum(_coprime(s) for s in shapes)
    print(f'\n{name}: max |got - exact| area kinds {worst["area"]:.13f}, linear kind {worst["linear"]:.4f}; '
          f'knife-edge pixels {needed} of {total} ({100 * needed / total:.3f} %); '
          f'coprime shapes {ncop} of {len(shapes)} (no variant needed in any)')
    assert needed <= 0.01 * total
    assert 2 * ncop >= len(shapes)


def test_table_covers_every_kind():
    n = {}
    for s in TABLE:
        n[_class(*s)] = n.get(_class(*s), 0) + 1
    for c in ['copy', 'int', 'area<2', 'area>=2', 'lin-up-up', 'lin-xup-ydown', 'lin-xdown-yup']:
        assert n.get(c, 0) >= 3, (c, n)
    assert any(s[0] == 1 for s in TABLE) and any(s[1] == 1 for s in TABLE) and any(s[2:] == (1, 1) for s in TABLE)
    for scales in [(2, 2), (3, 3), (2, 3)]:
        assert any(R.kind_of(*s) == 1 and (s[0] // s[2], s[1] // s[3]) == scales for s in TABLE)
    for s in _shapes():
        R.bound_of(*s)  # asserts the cap
    assert R.LINEAR_BOUND < R.LINEAR_CAP


def test_reference_axes_agree_where_both_apply():
    """On an upscaled axis OpenCV's area-mode tap is the overlap fraction: the
    exact two-tap row equals the box row, so the linear kind's reference is
    the area integral there and not a restatement of the tap formula."""
    for s, d in [(1, 5), (5, 7), (7, 13), (9, 33), (12, 16), (3, 64), (20, 20), (63, 64)]:
        assert R.box_equals_two_tap(s, d), (s, d)
    # rows are distributions; a constant image is reproduced exactly
    img = np.full((9, 13, 3), 201, np.uint8)
    for dh, dw in [(9, 13), (3, 13), (4, 5), (20, 30), (20, 5), (4, 30)]:
        for r in R.resize_exact(img, dh, dw)[1]:
            assert np.abs(r - 201).max() < 1e-9


def test_oracle_matches_exact(oracle):
    worst, needed, total = _sweep(oracle.resize_crop)
    _report('oracle', worst, needed, total)


def test_host_library_matches_exact(hip_lib):
    from ffcv_amd import libffcv as L

    def resize(src, r0, r1, c0, c1, dh, dw):
        out = np.zeros((dh, dw, 3), np.uint8)
        L.resize_crop(src, r0, r1, c0, c1, out)
        return out
    worst, needed, total = _sweep(resize)
    _report('libffcv_hip host resize', worst, needed, total)


TEETH = [(8, 10, 4, 5), (20, 30, 10, 10), (31, 45, 17, 29), (20, 30, 7, 20), (10, 9, 33, 20), (40, 9, 16, 32),
         (9, 40, 32, 16), (12, 8, 8, 16), (33, 20, 33, 20)]


def _fails(got, img):
    err, _, _, _, bound = R.compare(got, img)
    return err > bound


def test_reference_has_teeth(oracle):
    """The oracle's output against a reference that is off by one column, by
    one row, or has its axes' weights exchanged must miss the bound, for
    every kind.  Only the reference side is perturbed."""
    rng = np.random.default_rng(99)
    for sh, sw, dh, dw in TEETH:
        img = natural_image(rng, sh, sw)
        got = oracle.resize_crop(img, 0, sh, 0, sw, dh, dw)
        assert not _fails(got, img)
        assert _fails(got, np.roll(img, 1, axis=1)), ('column', sh, sw, dh, dw)
        assert _fails(got, np.roll(img, 1, axis=0)), ('row', sh, sw, dh, dw)
    # Wy built for the x sizes and Wx for the y sizes: a square source and a
    # non-square output keep the shapes compatible (the result is transposed)
    for s, dh, dw in [(24, 12, 16), (24, 9, 20), (20, 31, 26), (20, 33, 12), (20, 12, 33)]:
        img = natural_image(rng, s, s)
        got = oracle.resize_crop(img, 0, s, 0, s, dh, dw).astype(np.float64)
        k = R.kind_of(s, s, dh, dw)
        bound = R.bound_of(s, s, dh, dw)
        best = None
        for Wy in R.axis_weights(s, dw, k == 3):       # the x sizes, applied to rows
            for Wx in R.axis_weights(s, dh, k == 3):   # the y sizes, applied to columns
                e = np.abs(got - R.apply(Wy, img, Wx).transpose(1, 0, 2)).max(-1)
                best = e if best is None else np.minimum(best, e)
        assert best.max() > bound, ('swapped', s, dh, dw)
        assert not _fails(got.astype(np.uint8), img)
