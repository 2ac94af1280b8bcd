"""numpy statement of RandomAdjustSharpness, shared by
test_sharpness*.py: Pillow's ImageEnhance.Sharpness(img).enhance(factor),
that is Image.blend(img.filter(ImageFilter.SMOOTH), img, factor), restated as
float32 arithmetic in which every product and every sum is rounded on its own.
Written over whole arrays (shifted views, tap by tap), not the way the kernel
or the host twin walk an image.

The variants (fma, flat, the other row order) exist for the order fixture
only (tests/golden/make_sharpness_order.py): `sharpen` with its defaults is
the contract."""
import numpy as np

from ffcv_amd.transforms.rng import contract_seed

OP_SHARPNESS = 19
COPY, SHARPEN, LEAVE = 0, 1, 2            # the apply codes of ffcv_sharpness_batch
FACTORS = (0, 0.01, 0.3, 0.9, 1, 1.5, 1.99, 2)
F32 = np.float32
W1 = F32(1) / F32(13)
W5 = F32(5) / F32(13)
# the rows of a 3 x 3 neighbourhood in the order their sums join the running
# sum: the top row first.  No input can tell this order from another (see
# make_sharpness_order.py): the exact sum lies at least 1 / 26 from an integer.
ROWS = (0, 1, 2)


def _fma(a, b, c):
    """float32(a * b + c) with one rounding (the product of two float32 values
    and the sum are exact enough in float64 for every value met here: 24 + 24
    bits of product, an addend within 2^11 of it)."""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(F32)


def draw(seed, epoch, sid, p):
    """The decision of sample sid: rand() < p."""
    return bool(np.random.RandomState(contract_seed(seed, epoch, int(sid), OP_SHARPNESS)).rand() < p)


def smooth(img, rows=ROWS, fma=False, flat=False):
    """ImageFilter.SMOOTH on a uint8 (H, W, 3) image."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    out = img.copy()
    if h < 3 or w < 3:
        return out
    f = img.astype(F32)
    tap = lambda r, c: f[r:h - 2 + r, c:w - 2 + c]  # noqa: E731
    wt = lambda r, c: W5 if (r, c) == (1, 1) else W1  # noqa: E731
    s = np.full((h - 2, w - 2, 3), F32(0.5))
    for r in rows:
        if flat:            # the nine products join the running sum one by one
            for c in range(3):
                s = s + tap(r, c) * wt(r, c)
        elif fma:           # the row sum contracted: fma(p2, w, fma(p1, w, p0 w))
            rs = tap(r, 0) * wt(r, 0)
            rs = _fma(tap(r, 1), wt(r, 1), rs)
            rs = _fma(tap(r, 2), wt(r, 2), rs)
            s = s + rs
        else:
            s = s + ((tap(r, 0) * wt(r, 0) + tap(r, 1) * wt(r, 1)) + tap(r, 2) * wt(r, 2))
        assert s.dtype == F32
    out[1:h - 1, 1:w - 1] = np.clip(s, 0, 255).astype(np.uint8)      # truncation
    return out


def blend(d, i, factor, fma=False):
    """Image.blend(d, i, factor) on uint8 arrays."""
    a = F32(factor)
    df, jf = d.astype(F32), i.astype(F32)
    diff = jf - df
    t = _fma(diff, a, df) if fma else df + a * diff
    assert t.dtype == F32
    if 0 <= factor <= 1:
        assert t.min() >= 0 and t.max() <= 255
        return t.astype(np.uint8)
    return np.clip(t, 0, 255).astype(np.uint8)


def sharpen(img, factor, rows=ROWS, fma=False, flat=False):
    """One uint8 (H, W, 3) image at `factor`: the contract with the defaults."""
    img = np.asarray(img, np.uint8)
    return blend(smooth(img, rows, fma, flat), img, factor, fma)


def sharpen_batch(imgs, apply, factor, dst):
    """apply codes per image: 0 copy, 1 sharpen, 2 leave dst alone, else copy."""
    out = np.array(dst, np.uint8)
    for k, im in enumerate(imgs):
        if apply[k] == SHARPEN:
            out[k] = sharpen(im, factor[k])
        elif apply[k] != LEAVE:
            out[k] = im
    return out


def pillow_sharpen(img, factor):
    from PIL import Image, ImageEnhance
    return np.asarray(ImageEnhance.Sharpness(Image.fromarray(np.asarray(img, np.uint8), 'RGB')).enhance(factor))


def make_inputs(rng, shape, batch=7):
    """Random images, all-0, all-255, a 0 / 255 checkerboard, random again."""
    imgs = rng.integers(0, 256, (batch,) + tuple(shape) + (3,), dtype=np.uint8)
    imgs[batch - 4] = 0
    imgs[batch - 3] = 255
    yy, xx = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing='ij')
    imgs[batch - 2] = (((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None]
    return imgs


def mixed_apply(batch=7):
    """Codes 0 / 1 / 2 and one unknown code (treated as 0)."""
    apply = np.ones(batch, np.uint8)
    apply[0], apply[1], apply[2] = LEAVE, COPY, 7
    return apply[:batch]
