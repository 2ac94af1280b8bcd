"""The statement of RandomPosterize / RandomAutocontrast / RandomEqualize /
RandomInvert: the four tables as plain Python over a channel's
256-bin histogram, written from the contract (and checked against Pillow's
ImageOps in tests/test_tone.py), a program of steps applied one after the
other, each on the previous step's bytes, and the image families the tests
draw from."""
import numpy as np

from ffcv_amd.transforms.rng import contract_seed

POSTERIZE, AUTOCONTRAST, EQUALIZE, INVERT = 1, 2, 3, 4
KINDS = (POSTERIZE, AUTOCONTRAST, EQUALIZE, INVERT)
OP_ID = {POSTERIZE: 15, AUTOCONTRAST: 16, EQUALIZE: 17, INVERT: 18}
FAMILIES = ('noise', 'band', 'constant_channel', 'two_valued', 'normal')


def invert_table():
    return [255 - v for v in range(256)]


def posterize_table(bits):
    return [v & (0xFF & ~(2 ** (8 - bits) - 1)) for v in range(256)]


def autocontrast_table(h):
    occupied = [v for v in range(256) if h[v] > 0]
    lo, hi = occupied[0], occupied[-1]
    if hi <= lo:
        return list(range(256))
    scale = 255.0 / (hi - lo)           # Python floats: float64, every operation rounded on its own
    offset = -lo * scale
    return [min(max(int(v * scale + offset), 0), 255) for v in range(256)]


def equalize_raw(h):
    """Equalize's entries before the min(255, .), or None where the table is
    the identity; and the step."""
    h = [int(x) for x in h]
    occupied = [v for v in range(256) if h[v] > 0]
    if len(occupied) < 2:
        return None, None
    step = (sum(h) - h[occupied[-1]]) // 255
    if step == 0:
        return None, 0
    raw, below = [], 0                                   # below = sum(h[:v])
    for v in range(256):
        raw.append((step // 2 + below) // step)
        below += h[v]
    return raw, step


def equalize_table(h):
    raw, _ = equalize_raw(h)
    return list(range(256)) if raw is None else [min(255, e) for e in raw]


def histogram(channel):
    return np.bincount(np.asarray(channel).reshape(-1), minlength=256)


def step_np(image, kind, bits=8):
    """One step on one uint8 (H, W, 3) image: a new array."""
    out = np.empty_like(image)
    for c in range(3):
        if kind == POSTERIZE:
            table = posterize_table(bits)
        elif kind == INVERT:
            table = invert_table()
        elif kind == AUTOCONTRAST:
            table = autocontrast_table(histogram(image[..., c]))
        else:
            table = equalize_table(histogram(image[..., c]))
        out[..., c] = np.asarray(table, dtype=np.uint8)[image[..., c]]
    return out


def apply_program_batch(images, steps, bits, apply):
    """steps[i] on image k where apply[i][k], one after the other: a new array."""
    out = np.array(images, copy=True)
    for k in range(len(out)):
        for i, kind in enumerate(steps):
            if apply[i][k]:
                out[k] = step_np(out[k], kind, bits)
    return out


def draw(seed, epoch, sample, kind, p):
    return bool(np.random.RandomState(contract_seed(seed, epoch, int(sample), OP_ID[kind])).rand() < p)


def family(rng, name, h, w):
    """One uint8 (h, w, 3) image of a family."""
    shape = (h, w, 3)
    if name == 'noise':
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if name == 'band':                                   # 16 adjacent values
        return (rng.integers(0, 256, shape) // 16 + rng.integers(0, 240)).astype(np.uint8)
    if name == 'constant_channel':
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        img[..., rng.integers(0, 3)] = rng.integers(0, 256)
        return img
    if name == 'two_valued':
        a, b = rng.integers(0, 256, 3), rng.integers(0, 256, 3)
        return np.where(rng.random(shape) < 0.5, a, b).astype(np.uint8)
    if name == 'normal':
        return np.clip(rng.normal(128.0, rng.uniform(2.0, 60.0), shape), 0, 255).astype(np.uint8)
    if name == 'flat':                                   # every byte of a channel in one bin
        return np.broadcast_to(rng.integers(0, 256, 3).astype(np.uint8), shape).copy()
    raise ValueError(name)


def image_set(shapes=50, per_shape=8, seed=2024):
    """A list of uint8 (per_shape, h, w, 3) batches, shapes 1 x 1 to 39 x 39,
    the five families in turn: 400 images by default."""
    rng = np.random.default_rng(seed)
    hw = [(1, 1), (39, 39), (1, 39), (39, 1), (16, 16)]
    while len(hw) < shapes:
        hw.append((int(rng.integers(1, 40)), int(rng.integers(1, 40))))
    out, j = [], 0
    for h, w in hw:
        batch = []
        for _ in range(per_shape):
            batch.append(family(rng, FAMILIES[j % len(FAMILIES)], h, w))
            j += 1
        out.append(np.stack(batch))
    return out
