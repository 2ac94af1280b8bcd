"""Generate tests/golden/color_jitter.npz by running the REFERENCE's own
RandomBrightness / RandomContrast / RandomSaturation
(ffcv/transforms/color_jitter.py) with the compiler disabled, on a batch of
one image under ``np.random.seed(seed)``, through the stub modules of
make_golden.py (this container only; no test imports this file).  With a batch
of one the reference's ``rand(1)`` then ``uniform(lo, hi, 1)`` are the first
draws of RandomState(seed): the per-sample stream of the seeding contract.
Only the OUTPUTS are saved:

  rows    a few hundred decisions, as parallel arrays: rows_op (1 brightness,
          2 contrast, 3 saturation), rows_seed, rows_magnitude, rows_p,
          rows_apply (the reference's ``rand(1) < p``) and rows_ratio_bits
          (the uint64 bits of the float64 its ``uniform`` returned), recorded
          as the reference ran.
  pairs   a few dozen (input, output) image pairs per operation on small
          non-constant images, and the 24 x 71 image of the 1,704 RGB triples
          whose float64 gray sum lies within 1e-9 of an integer: in_k, out_k,
          meta_op / meta_seed / meta_magnitude / meta_p (K,).

Run:  python tests/golden/make_color_jitter.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import install_stubs, REF  # noqa: E402

NAMES = {1: 'RandomBrightness', 2: 'RandomContrast', 3: 'RandomSaturation'}


def near_integer_image():
    """The RGB triples whose gray sum (0.2989 r + 0.587 g) + 0.114 b, in
    float64, lies within 1e-9 of an integer, in (r, g, b) order, as 24 x 71."""
    g, b = np.meshgrid(np.arange(256.0), np.arange(256.0), indexing='ij')
    found = []
    for r in range(256):
        s = 0.2989 * r + 0.587 * g + 0.114 * b
        gi, bi = np.nonzero(np.abs(s - np.rint(s)) < 1e-9)
        found += [(r, int(x), int(y)) for x, y in zip(gi, bi)]
    assert len(found) == 1704, len(found)
    return np.array(found, np.uint8).reshape(24, 71, 3)


def run_reference(mod, kind, image, magnitude, p, seed):
    """The reference's operation on a batch holding a copy of image; returns
    the output image, rand(1) < p and the float64 uniform() returned."""
    fn = getattr(mod, NAMES[kind])(magnitude, p).generate_code()
    drawn = {}
    rand, uniform = np.random.rand, np.random.uniform

    def rec_rand(*a):
        v = rand(*a)
        drawn['rand'] = v.copy()
        return v

    def rec_uniform(*a):
        v = uniform(*a)
        drawn['uniform'] = v.copy()
        return v
    np.random.rand, np.random.uniform = rec_rand, rec_uniform
    try:
        np.random.seed(seed)
        out = fn(image[None].copy())
    finally:
        np.random.rand, np.random.uniform = rand, uniform
    assert drawn['rand'].shape == (1,) and drawn['uniform'].shape == (1,) and drawn['uniform'].dtype == np.float64
    return np.asarray(out[0], np.uint8), bool(drawn['rand'][0] < p), drawn['uniform'][0]


def gen_rows(mod):
    rng = np.random.default_rng(505)
    probe = rng.integers(0, 256, (3, 4, 3), dtype=np.uint8)
    mags = [0.0, 0.1, 0.25, 0.5, 0.9, 1.0, 1.5, 3.0, 10.0]
    cols = {k: [] for k in ('op', 'seed', 'magnitude', 'p', 'apply', 'ratio_bits')}
    for k in range(600):
        kind = k % 3 + 1
        m = mags[(k // 3) % len(mags)] if k % 2 else float(rng.uniform(0, 2))
        p = [0.0, 0.5, 1.0, 0.3][(k // 3) % 4] if k % 5 else float(rng.uniform(0, 1))
        seed = int(rng.integers(0, 2 ** 32))
        _, apply, ratio = run_reference(mod, kind, probe, m, p, seed)
        cols['op'].append(kind)
        cols['seed'].append(seed)
        cols['magnitude'].append(m)
        cols['p'].append(p)
        cols['apply'].append(apply)
        cols['ratio_bits'].append(np.float64(ratio).view(np.uint64))
    return {'rows_op': np.array(cols['op'], np.int64), 'rows_seed': np.array(cols['seed'], np.int64),
            'rows_magnitude': np.array(cols['magnitude'], np.float64), 'rows_p': np.array(cols['p'], np.float64),
            'rows_apply': np.array(cols['apply'], np.uint8),
            'rows_ratio_bits': np.array(cols['ratio_bits'], np.uint64)}


def gen_pairs(mod):
    rng = np.random.default_rng(506)
    near = near_integer_image()
    out, meta = {}, []
    k = 0
    for kind in (1, 2, 3):
        for j in range(36):
            if j < 4:
                img = near
            else:
                h, w = int(rng.integers(1, 17)), int(rng.integers(1, 17))
                img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
                if j % 6 == 0:    # dark / bright images: contrast means near the ends
                    img = (img // 8 + (0 if j % 12 else 224)).astype(np.uint8)
            m = [0.0, 0.3, 0.5, 0.9, 1.0, 2.0, 6.0][j % 7]
            p = 1.0 if j % 9 else 0.5
            seed = int(rng.integers(0, 2 ** 32))
            res, _, _ = run_reference(mod, kind, img, m, p, seed)
            out[f'in_{k}'] = img
            out[f'out_{k}'] = res
            meta.append((kind, seed, m, p))
            k += 1
    out['meta_op'] = np.array([r[0] for r in meta], np.int64)
    out['meta_seed'] = np.array([r[1] for r in meta], np.int64)
    out['meta_magnitude'] = np.array([r[2] for r in meta], np.float64)
    out['meta_p'] = np.array([r[3] for r in meta], np.float64)
    return out


def main():
    install_stubs()
    sys.path.insert(0, REF)
    import ffcv  # noqa: F401
    from ffcv.transforms import color_jitter as mod
    from ffcv.pipeline.compiler import Compiler
    Compiler.set_enabled(False)
    rows = gen_rows(mod)
    pairs = gen_pairs(mod)
    path = os.path.join(HERE, 'color_jitter.npz')
    np.savez_compressed(path, **rows, **pairs)
    print('color_jitter.npz:', len(rows['rows_op']), 'rows,', len(pairs['meta_op']), 'pairs,',
          os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
