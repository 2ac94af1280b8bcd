"""Writes tests/golden/blur_order.npz: neighbourhoods on which the blur's
pinned arithmetic (tests/blur_ref.py: float32, every product and sum rounded,
taps in ascending order) differs from a fused multiply-add accumulation or from
the taps taken in descending order.  Random images alone change only a few
bytes per megapixel under either, so they do not pin the order; these do.

    python tests/golden/make_blur_order.py

Seeded: the same file every run.  For each kernel size k in (3, 5, 23) random
512 x 512 images are blurred three ways; wherever the centre of a full
(2r + 1)^2 window comes out differently, the window is kept as a tile of its
own (the centre's result depends on nothing outside it), with the image's
weights, the pinned centre bytes and the two other results.  The search stops
at 16 tiles per kernel size or 16 M bytes in all.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import blur_ref as R  # noqa: E402

KSIZES = (3, 5, 23)
PER_K = 16
CAP_BYTES = 16 * 1000 * 1000
SIDE = 512


def _variant_pass(a, w, ksize, axis, fma, reverse):
    r = (ksize - 1) // 2
    n = a.shape[axis]
    pos = np.arange(n)
    acc = None
    for j in (range(ksize - 1, -1, -1) if reverse else range(ksize)):
        v = np.take(a, R._reflect(pos - r + j, n), axis=axis)
        if acc is None:
            acc = np.float32(w[j]) * v
        elif fma:   # one rounding: float32(w v + acc), the product and the sum in float64
            acc = (np.float64(w[j]) * v.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
        else:
            acc = acc + np.float32(w[j]) * v
    return acc


def variant(img, ksize, w, fma=False, reverse=False):
    a = _variant_pass(img.astype(np.float32), w, ksize, 1, fma, reverse)
    a = _variant_pass(a, w, ksize, 0, fma, reverse)
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def main():
    rng = np.random.default_rng(20240611)
    out = {}
    searched = 0
    for ksize in KSIZES:
        r = (ksize - 1) // 2
        tiles, weights, want, fused, rev = [], [], [], [], []
        while len(tiles) < PER_K and searched + SIDE * SIDE * 3 <= CAP_BYTES * (KSIZES.index(ksize) + 1) // len(KSIZES):
            img = rng.integers(0, 256, (SIDE, SIDE, 3), dtype=np.uint8)
            w = R.weights_f32(ksize, rng.uniform(0.3, 2.0))
            searched += img.size
            a, b, c = R.blur(img, ksize, w), variant(img, ksize, w, fma=True), variant(img, ksize, w, reverse=True)
            assert np.array_equal(a, variant(img, ksize, w))   # the two statements of the contract agree
            hit = ((a != b) | (a != c)).any(axis=2)
            hit[:r], hit[SIDE - r:], hit[:, :r], hit[:, SIDE - r:] = False, False, False, False
            for y, x in zip(*np.nonzero(hit)):
                if len(tiles) == PER_K:
                    break
                tile = img[y - r:y + r + 1, x - r:x + r + 1].copy()
                assert np.array_equal(R.blur(tile, ksize, w)[r, r], a[y, x])
                tiles.append(tile)
                weights.append(w)
                want.append(a[y, x])
                fused.append(b[y, x])
                rev.append(c[y, x])
        out[f'tiles_{ksize}'] = np.stack(tiles)
        out[f'weights_{ksize}'] = np.stack(weights)
        out[f'want_{ksize}'] = np.stack(want)
        out[f'fma_{ksize}'] = np.stack(fused)
        out[f'reversed_{ksize}'] = np.stack(rev)
        print(ksize, len(tiles), 'tiles;', searched, 'bytes searched so far')
    assert sum(len(out[f'tiles_{k}']) for k in KSIZES) >= 32
    np.savez_compressed(os.path.join(HERE, 'blur_order.npz'), **out)


if __name__ == '__main__':
    main()
