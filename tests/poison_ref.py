"""The Poison / ReplaceLabel semantics stated in numpy, independent of the
package: the five statements on a float32 temp.  Shared by test_poison.py
(CPU) and test_poison_gpu.py, with the input builders and the case lists."""
import numpy as np

# opacities at which a float32-only evaluation, a float64 evaluation without
# the intermediate float32 roundings, and one with a single final rounding
# each differ from the statement on the all-pairs image
ALPHAS = (0.0, 1.0, 0.5, 0.3, 0.7, 1 / 3, 0.1, 0.9999999, 1e-12, -0.25, 1.5)

SHAPES = [(1, 1, 3), (3, 5, 3), (32, 32, 3), (37, 29, 3), (40, 35, 3)]
BATCHES = (1, 2, 3, 5, 67)
CLAMPS = [(0, 255), (10, 200), (0.5, 100.5)]
INDEX_SETS = ('empty', 'all', 'every_other', 'first', 'last', 'absent', 'duplicates')


def alpha3_of(alpha):
    return np.repeat(alpha[:, :, None], 3, axis=2)


def chosen(sample_ids, indices):
    """Positions of the batch whose dataset index is in indices."""
    want = set(int(i) for i in np.asarray(indices).reshape(-1))
    return [k for k, s in enumerate(np.asarray(sample_ids).reshape(-1)) if int(s) in want]


def poison_np(images, mask, alpha, sample_ids, indices, clamp=(0, 255)):
    """A poisoned copy of images (n, H, W, 3), any dtype."""
    out = np.array(images, copy=True)
    alpha3 = alpha3_of(alpha)
    for k in chosen(sample_ids, indices):
        temp = np.empty(images.shape[1:], np.float32)
        temp[:] = images[k]
        temp *= 1 - alpha3
        temp += mask.astype(float) * alpha3
        np.clip(temp, clamp[0], clamp[1], out=temp)
        out[k] = temp
    return out


def replace_label_np(labels, sample_ids, indices, new_label):
    out = np.array(labels, copy=True)
    for k in chosen(sample_ids, indices):
        out[k] = new_label
    return out


def all_pairs(alpha_dtype):
    """image (1, 11 * 256, 256, 3), mask, alpha: pixel (256 * a + v, m) holds
    the byte v in all channels against mask byte m under opacity ALPHAS[a], so
    the sample holds every (v, m) pair under every opacity."""
    rows = len(ALPHAS) * 256
    r = np.arange(rows)
    image = np.broadcast_to((r % 256).astype(np.uint8)[:, None, None], (rows, 256, 3)).copy()[None]
    mask = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (rows, 256, 3)).copy()
    alpha = np.broadcast_to(np.array(ALPHAS, np.float64)[r // 256][:, None], (rows, 256)).astype(alpha_dtype)
    return image, mask, alpha


def other_forms(image, mask, alpha, clamp=(0, 255)):
    """The cheaper relatives of the statement on one uint8 image: float32
    only; float64 with no intermediate float32 rounding; float64 with one
    float32 rounding at the end."""
    alpha3 = alpha3_of(alpha)
    lo, hi = np.float32(clamp[0]), np.float32(clamp[1])
    k32, a32 = (1 - alpha3).astype(np.float32), (mask.astype(float) * alpha3).astype(np.float32)
    f32 = np.clip(image.astype(np.float32) * k32 + a32, lo, hi).astype(np.uint8)
    exact = image.astype(np.float64) * np.float64(1 - alpha3) + mask.astype(float) * alpha3
    f64 = np.clip(exact, np.float64(lo), np.float64(hi)).astype(np.uint8)
    f64_once = np.clip(exact.astype(np.float32), lo, hi).astype(np.uint8)
    return f32, f64, f64_once


def random_case(rng, shape, n, alpha_dtype):
    """images (n, *shape) uint8, mask, alpha with values in and outside [0, 1]
    and some of ALPHAS, and the batch's dataset indices (distinct, unordered)."""
    images = rng.integers(0, 256, (n,) + tuple(shape), dtype=np.uint8)
    mask = rng.integers(0, 256, shape, dtype=np.uint8)
    alpha = rng.random(shape[:2]) * 1.5 - 0.25
    flat = alpha.reshape(-1)
    flat[::3] = rng.choice(ALPHAS, flat[::3].shape)
    sample_ids = rng.permutation(4 * n + 8)[:n].astype(np.uint64) + np.uint64(3)
    return images, mask, alpha.astype(alpha_dtype), sample_ids


def index_set(kind, sample_ids):
    s = np.asarray(sample_ids).astype(np.int64)
    if kind == 'empty':
        return []
    if kind == 'all':
        return s.tolist()
    if kind == 'every_other':
        return s[::2].tolist()
    if kind == 'first':
        return [int(s[0])]
    if kind == 'last':
        return [int(s[-1])]
    if kind == 'absent':
        return [0, 1, 2, int(s.max()) + 1, int(s.max()) + 1000]       # sample ids start at 3
    if kind == 'duplicates':
        return [int(s[0]), int(s[-1]), int(s[0]), 1, int(s[-1]), 1]
    raise ValueError(kind)
