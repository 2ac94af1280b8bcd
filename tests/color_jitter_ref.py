"""numpy statement of RandomBrightness / RandomContrast / RandomSaturation
under the seeding contract, shared by test_color_jitter.py and
test_color_jitter_gpu.py.  Written the reference's way (float64 blends of
whole arrays, ``gray.mean()``), not the way the package's host path (tables)
or the kernels compute it."""
import numpy as np

from ffcv_amd.transforms.rng import contract_seed

BRIGHTNESS, CONTRAST, SATURATION = 1, 2, 3
OP_ID = {BRIGHTNESS: 5, CONTRAST: 6, SATURATION: 7}


def gray_np(img):
    r, g, b = img[:, :, 0], img[:, :, 1], img[:, :, 2]
    return (0.2989 * r + 0.587 * g + 0.114 * b).astype(np.uint8)


def blend_np(img, other, ratio):
    ratio = np.float64(ratio)
    return (ratio * img + (1 - ratio) * other).clip(0, 255).astype(np.uint8)


def jitter_np(img, kind, ratio):
    """One operation on one uint8 (H, W, 3) image (a new array)."""
    if kind == BRIGHTNESS:
        return blend_np(img, 0, ratio)
    if kind == CONTRAST:
        return blend_np(img, gray_np(img).mean(), ratio)
    if kind == SATURATION:
        return blend_np(img, np.repeat(gray_np(img)[:, :, None], 3, axis=2), ratio)
    raise ValueError(kind)


def jitter_draw(seed, epoch, sid, kind, p, magnitude):
    """(apply, ratio) of sample sid: rand() < p, then uniform(lo, hi)."""
    rs = np.random.RandomState(contract_seed(seed, epoch, int(sid), OP_ID[kind]))
    apply = bool(rs.rand() < p)
    return apply, rs.uniform(max(0, 1 - magnitude), 1 + magnitude)


def apply_program(img, kinds, applies, ratios):
    """The steps (in pipeline order) with the given decisions, one after another."""
    out = np.array(img, np.uint8)
    for kind, a, r in zip(kinds, applies, ratios):
        if a:
            out = jitter_np(out, kind, r)
    return out


def apply_program_batch(imgs, kinds, apply, ratio):
    """apply (n, B), ratio (n, B) -> (B, H, W, 3)."""
    return np.stack([apply_program(imgs[k], kinds, apply[:, k], ratio[:, k]) for k in range(len(imgs))])


def near_integer_triples():
    """The RGB triples whose float64 gray sum lies within 1e-9 of an integer,
    in (r, g, b) order: (N, 3) uint8."""
    g, b = np.meshgrid(np.arange(256.0), np.arange(256.0), indexing='ij')
    found = []
    for r in range(256):
        s = 0.2989 * r + 0.587 * g + 0.114 * b
        gi, bi = np.nonzero(np.abs(s - np.rint(s)) < 1e-9)
        found.append(np.stack([np.full(gi.size, r), gi, bi], 1))
    return np.concatenate(found).astype(np.uint8)
