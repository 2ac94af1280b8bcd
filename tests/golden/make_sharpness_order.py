"""Writes tests/golden/sharpness_order.npz: 3 x 3 neighbourhoods, found by
search, on which Pillow's ImageEnhance.Sharpness differs from a twin of the
pinned arithmetic (tests/sharpness_ref.py) with the blend contracted to a fused
multiply-add.  Needs Pillow; no GPU.

    python tests/golden/make_sharpness_order.py

Seeded: the same file every run.  Two searches:

  1. the blend.  For each factor k / 100, k = 0 .. 200, every pair (d, i) of a
     smoothed byte and a centre byte that a neighbourhood can produce
     (0 <= 13 d - 5 i <= 2040, the sum of the eight neighbours) is blended
     both ways; where the bytes differ, a neighbourhood with that centre and
     that smoothed value is built, one hit per channel, and run through Pillow
     itself, whose centre bytes become `want`.  At most PER_FACTOR tiles per
     factor, TILES in all.
  2. the smooth.  SMOOTH_SIDE^2 random neighbourhoods (three channels each)
     and every constant-plus-one-outlier neighbourhood are smoothed four ways:
     as pinned, with the row sum contracted to fma, with the nine products
     summed flat, and with the rows taken bottom first.  None differs, and none
     can: the exact sum 0.5 + S / 13, S an integer, lies at least 1 / 26 from
     every integer, while the roundings of any of these evaluations move it by
     less than 2^-11.  The count is printed for DESIGN.md; the fixture holds
     no tiles for these variants.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import sharpness_ref as R  # noqa: E402

TILES = 48
PER_FACTOR = 6
SMOOTH_SIDE = 1024


def neighbourhood(rng, d, i):
    """A 3 x 3 plane with centre i whose eight neighbours sum to 13 d - 5 i."""
    n = 13 * d - 5 * i
    assert 0 <= n <= 2040
    nb = np.full(8, n // 8)
    nb[:n % 8] += 1
    for _ in range(16):                 # move mass between pairs: the sum stays
        a, b = rng.choice(8, 2, replace=False)
        m = int(rng.integers(0, min(nb[a], 255 - nb[b]) + 1))
        nb[a] -= m
        nb[b] += m
    plane = np.insert(nb, 4, i).reshape(3, 3)
    assert plane.min() >= 0 and plane.max() <= 255
    return plane.astype(np.uint8)


def search_blend(rng):
    d, i = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    n = 13 * d - 5 * i
    reach = (n >= 0) & (n <= 2040)
    d8, i8 = d.astype(np.uint8), i.astype(np.uint8)
    tiles, factors, want, fused = [], [], [], []
    pairs = 0
    for k in range(201):
        factor = k / 100
        a, b = R.blend(d8, i8, factor), R.blend(d8, i8, factor, fma=True)
        pairs += int(reach.sum())
        hits = np.argwhere(reach & (a != b))
        rng.shuffle(hits)
        for t in range(min(PER_FACTOR, len(hits) // 3)):
            if len(tiles) == TILES:
                break
            tile = np.stack([neighbourhood(rng, *hits[3 * t + c]) for c in range(3)], axis=2)
            got = R.pillow_sharpen(tile, factor)
            assert np.array_equal(got, R.sharpen(tile, factor)), (factor, tile)
            f = R.sharpen(tile, factor, fma=True)[1, 1]
            assert (got[1, 1] != f).all()
            tiles.append(tile)
            factors.append(factor)
            want.append(got[1, 1])
            fused.append(f)
    print(len(tiles), 'blend tiles from', pairs, '(factor, d, i) triples')
    return dict(tiles=np.stack(tiles), factor=np.array(factors, np.float32), want=np.stack(want),
                fma=np.stack(fused))


def search_smooth(rng):
    tried = 0
    imgs = [rng.integers(0, 256, (SMOOTH_SIDE + 2, SMOOTH_SIDE + 2, 3), dtype=np.uint8)]
    # a constant with one outlier, every pair of values, at the nine positions
    v, o = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    for pos in range(9):
        img = np.repeat(np.repeat(v[:, :, None], 3, 0), 3, 1).astype(np.uint8)       # 3 x 3 blocks of v
        img[pos // 3::3, pos % 3::3] = o[:, :, None]
        imgs.append(np.repeat(img, 3, 2))
    for img in imgs:
        a = R.smooth(img)
        for kw in (dict(fma=True), dict(flat=True), dict(rows=(2, 1, 0))):
            assert np.array_equal(a, R.smooth(img, **kw)), kw
        tried += (img.shape[0] - 2) * (img.shape[1] - 2) * 3
    print('smooth: no neighbourhood of', tried, 'differs under fma, the flat sum or the reversed rows')


def main():
    rng = np.random.default_rng(20241021)
    out = search_blend(rng)
    search_smooth(rng)
    assert len(out['tiles']) >= 32
    np.savez_compressed(os.path.join(HERE, 'sharpness_order.npz'), **out)


if __name__ == '__main__':
    main()
