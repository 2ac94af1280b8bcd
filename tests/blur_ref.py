"""numpy statement of GaussianBlur, RandomGrayscale and RandomSolarization
under the seeding contract, shared by test_blur*.py and
test_gray_solarize*.py.  Written over whole arrays (np.take along an axis, tap
by tap), not the way the kernel or the host twin walk an image."""
import itertools

import numpy as np

from ffcv_amd.transforms.rng import contract_seed
from tests import color_jitter_ref as CR

GRAYSCALE, SOLARIZE = 4, 5
OP_GRAYSCALE, OP_SOLARIZE, OP_BLUR = 9, 10, 11
WROW = 32
FLT_MIN = np.float64(2.0) ** -126


def uniform_draw(seed, epoch, sid, op_id, p, lo, hi):
    """(apply, value) of sample sid: rand() < p, then uniform(lo, hi)."""
    rs = np.random.RandomState(contract_seed(seed, epoch, int(sid), op_id))
    apply = bool(rs.rand() < p)
    return apply, np.float64(rs.uniform(lo, hi))


def weights_f64(ksize, sigma):
    """e_j / s in float64, s added in ascending j."""
    sigma = np.float64(sigma)
    x = np.arange(ksize, dtype=np.float64) - np.float64(ksize - 1) / np.float64(2)
    t = x / sigma
    e = np.exp(np.float64(-0.5) * (t * t))
    s = np.float64(0)
    for v in e:
        s = s + v
    return e / s


def weights_f32(ksize, sigma):
    """The 32-float row of one sample: float32(e_j / s), below 2^-126 -> +0."""
    w = weights_f64(ksize, sigma).astype(np.float32)
    w[w.astype(np.float64) < FLT_MIN] = 0
    row = np.zeros(WROW, np.float32)
    row[:ksize] = w
    return row


def guard_holds(ksize, sigma):
    """True when no float64 weight lies within 2^-44 (relative) of a float32
    rounding boundary: implementations whose exp differs in the last bits then
    round to the same float32 weights."""
    w = weights_f64(ksize, sigma)
    eps = np.float64(2.0) ** -44
    return bool(np.array_equal((w * (1 - eps)).astype(np.float32), (w * (1 + eps)).astype(np.float32)))


def _reflect(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def _pass(a, w, ksize, axis):
    """One separable pass over float32 `a`: w_0 a[.. - r] first, then the taps
    added in ascending order, every product and sum rounded to float32."""
    r = (ksize - 1) // 2
    n = a.shape[axis]
    pos = np.arange(n)
    acc = None
    for j in range(ksize):
        term = np.float32(w[j]) * np.take(a, _reflect(pos - r + j, n), axis=axis)
        acc = term if acc is None else acc + term
        assert acc.dtype == np.float32
    return acc


def blur(img, ksize, w):
    """One uint8 (H, W, 3) image with the float32 weights w[0 .. ksize)."""
    h, wd = img.shape[:2]
    assert (ksize - 1) // 2 < min(h, wd)
    a = _pass(img.astype(np.float32), w, ksize, 1)
    a = _pass(a, w, ksize, 0)
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def blur_batch(imgs, ksize, apply, weights):
    return np.stack([blur(im, ksize, weights[k]) if apply[k] else im.copy() for k, im in enumerate(imgs)])


def solarize(img, threshold):
    return np.where(img >= threshold, 255 - img, img).astype(np.uint8)


def step_np(img, kind, value):
    """One colour step (the three jitter kinds, grayscale, solarize)."""
    if kind == GRAYSCALE:
        return np.repeat(CR.gray_np(img)[:, :, None], 3, axis=2)
    if kind == SOLARIZE:
        return solarize(img, int(value))
    return CR.jitter_np(img, kind, value)


def apply_program_batch(imgs, kinds, apply, value):
    """apply (n, B), value (n, B) -> (B, H, W, 3)."""
    out = []
    for k, im in enumerate(imgs):
        im = np.array(im, np.uint8)
        for i, kind in enumerate(kinds):
            if apply[i][k]:
                im = step_np(im, kind, value[i][k])
        out.append(im)
    return np.stack(out)


def programs_with_new_kind():
    """Every program of 1-3 distinct steps of the five kinds with a new kind."""
    kinds = (CR.BRIGHTNESS, CR.CONTRAST, CR.SATURATION, GRAYSCALE, SOLARIZE)
    return [p for n in (1, 2, 3) for p in itertools.permutations(kinds, n) if GRAYSCALE in p or SOLARIZE in p]
