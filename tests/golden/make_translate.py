"""Generate tests/golden/translate.npz by running the REFERENCE's own
RandomTranslate (ffcv/transforms/translate.py) with the compiler disabled,
under ``np.random.seed(seed)``, through the stub modules of make_golden.py
(this container only; no test imports this file).  Only the OUTPUTS are saved:

  rows    int64 (N, 6): seed, H, W, padding, y, x.  The window origin (y, x)
          is read off a probe image whose pixels encode their own position;
          where the window misses the image entirely (padding >= H or W can do
          that) nothing is left to read, and the row carries the two values
          the reference's ``randint`` returned, recorded as it ran (every
          other row asserts that both agree).
  pairs   a few dozen (input, output) image pairs on small non-constant images
          with a non-zero fill: in_k, out_k, and meta (K, 5) = seed, padding,
          fill R, G, B.

Run:  python tests/golden/make_translate.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import install_stubs, REF  # noqa: E402


def run_reference(mod, images, padding, fill, seed):
    """The reference's translate() on a copy of images; returns the output
    and the (y, x) its randint calls returned, in call order."""
    op = mod.RandomTranslate(padding, fill)
    fn = op.generate_code()
    n, h, w, c = images.shape
    dst = np.zeros((n, h + 2 * padding, w + 2 * padding, c), images.dtype)
    drawn = []
    real = mod.randint

    def recording(*a, **k):
        v = real(*a, **k)
        drawn.append(int(v))
        return v
    mod.randint = recording
    try:
        np.random.seed(seed)
        out = fn(images.copy(), dst)
    finally:
        mod.randint = real
    return out, drawn


def probe(h, w):
    """Pixel (r, c) holds (r + 1, c + 1, 0) for sizes up to 64; fill is 0."""
    img = np.zeros((1, h, w, 3), np.uint8)
    img[0, :, :, 0] = (np.arange(h) + 1)[:, None]
    img[0, :, :, 1] = (np.arange(w) + 1)[None, :]
    return img


def gen_rows(mod):
    rng = np.random.default_rng(404)
    rows = []
    for k in range(2000):
        if k < 64:
            h = w = k + 1
        else:
            h, w = int(rng.integers(1, 65)), int(rng.integers(1, 65))
        kind = k % 5
        if kind == 0:
            p = int(rng.integers(0, 4))
        elif kind == 1:
            p = int(rng.integers(0, min(h, w) + 1))
        elif kind == 2:
            p = max(h, w) + int(rng.integers(0, 40))   # beyond both sides
        elif kind == 3:
            p = min(h, w) + int(rng.integers(0, 3))    # at / just past the short side
        else:
            p = int(rng.integers(0, 2 * max(h, w) + 1))
        seed = int(rng.integers(0, 2 ** 32))
        out, drawn = run_reference(mod, probe(h, w), p, (0, 0, 0), seed)
        assert len(drawn) == 2
        y, x = drawn
        ys, xs = np.nonzero(out[0, :, :, 0])
        if ys.size:  # out[r, c] = in[r + y - p, c + x - p]: read (y, x) off one visible pixel
            r, c = int(ys[0]), int(xs[0])
            py = int(out[0, r, c, 0]) - 1 - r + p
            px = int(out[0, r, c, 1]) - 1 - c + p
            assert (py, px) == (y, x), (k, py, px, y, x)
        rows.append((seed, h, w, p, y, x))
    return np.array(rows, np.int64)


def gen_pairs(mod):
    rng = np.random.default_rng(405)
    out = {}
    meta = []
    for k in range(40):
        h, w = int(rng.integers(1, 17)), int(rng.integers(1, 17))
        p = [0, 1, 2, 3, 5, max(h, w), 20][k % 7]
        fill = tuple(int(v) for v in rng.integers(1, 256, 3))
        seed = int(rng.integers(0, 2 ** 32))
        img = rng.integers(0, 256, (1, h, w, 3), dtype=np.uint8)
        res, _ = run_reference(mod, img, p, fill, seed)
        out[f'in_{k}'] = img[0]
        out[f'out_{k}'] = np.asarray(res[0], np.uint8)
        meta.append((seed, p) + fill)
    out['meta'] = np.array(meta, np.int64)
    return out


def main():
    install_stubs()
    sys.path.insert(0, REF)
    import ffcv  # noqa: F401
    from ffcv.transforms import translate as mod
    from ffcv.pipeline.compiler import Compiler
    Compiler.set_enabled(False)
    rows = gen_rows(mod)
    pairs = gen_pairs(mod)
    np.savez_compressed(os.path.join(HERE, 'translate.npz'), rows=rows, **pairs)
    print('translate.npz:', rows.shape, len(pairs['meta']), 'pairs')


if __name__ == '__main__':
    main()
