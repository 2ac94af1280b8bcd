"""The RandomErasing semantics stated in numpy, independent of the package.
Shared by test_erase.py (CPU) and test_erase_gpu.py.

Draws, per sample, from its own MT19937 under the seeding contract, op id 21::

    rs = np.random.RandomState(contract_seed(seed, epoch, sample, 21))
    apply = rs.random_sample() < p                   # always drawn first
    box = none
    for _ in range(10):
        ea = (H * W) * rs.uniform(scale[0], scale[1])            # float64
        ar = exp(rs.uniform(log(ratio[0]), log(ratio[1])))       # float64
        h = int(round(sqrt(ea * ar))); w = int(round(sqrt(ea / ar)))   # half to even (rint)
        if 0 < h < H and 0 < w < W:
            y = rs.randint(H - h + 1); x = rs.randint(W - w + 1)       # legacy masked rejection
            box = (y, x, h, w); break
    erased  <=>  apply and box is not none

The loop runs whether or not ``apply`` holds, so the words consumed do not
depend on ``p``.

Fill of ``[y:y+h, x:x+w]`` of every channel: a number, one number per channel,
or (``'pixel'``) per-element noise without floating point::

    T[k] = statistics.NormalDist().inv_cdf((k + 0.5) / 4096), k = 0..4095      # float64, once
    table = (mean + std * T) converted once to the tensor's dtype:
            float16/float32: numpy astype (round to nearest even);  uint8: clip(rint(.), 0, 255)
    K = splitmix64(splitmix64(splitmix64(seed ^ (22 << 56)) ^ epoch) ^ sample)  # full 64 bits, op id 22
    e = the element's index inside its sample, in STORAGE order (elements, not bytes)
    word = splitmix64(K ^ (e >> 2));   idx = (word >> (16 * (e & 3) + 4)) & 0xFFF
    element = table[idx]
"""
import math
import statistics

import numpy as np

M64 = (1 << 64) - 1
TRIES = 10
DEFAULT_SCALE = (0.02, 0.33)
DEFAULT_RATIO = (0.3, 3.3)


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def hash3(seed, epoch, sample, op_id):
    h = splitmix64((int(seed) & M64) ^ ((int(op_id) << 56) & M64))
    h = splitmix64(h ^ (int(epoch) & M64))
    return splitmix64(h ^ (int(sample) & M64))


def draw(seed, epoch, sample, p, scale, ratio, H, W):
    """(apply, tries, box): tries = the number of the accepted try (1..10), 0
    when all ten failed; box = (y, x, h, w) of that try, or None."""
    rs = np.random.RandomState(hash3(seed, epoch, sample, 21) & 0xFFFFFFFF)
    apply = rs.random_sample() < p
    for t in range(TRIES):
        ea = (H * W) * rs.uniform(scale[0], scale[1])
        ar = math.exp(rs.uniform(math.log(ratio[0]), math.log(ratio[1])))
        h = int(round(math.sqrt(ea * ar)))
        w = int(round(math.sqrt(ea / ar)))
        if 0 < h < H and 0 < w < W:
            y = rs.randint(H - h + 1)
            x = rs.randint(W - w + 1)
            return apply, t + 1, (int(y), int(x), h, w)
    return apply, 0, None


def draws(ids, seed, epoch, p, scale, ratio, H, W):
    """(boxes int32 (n, 4) with h = w = 0 where nothing is erased, keys uint64
    (n,), applied bool (n,), tries int (n,))."""
    n = len(ids)
    boxes = np.zeros((n, 4), np.int32)
    keys = np.zeros(n, np.uint64)
    applied = np.zeros(n, bool)
    tries = np.zeros(n, np.int64)
    for k, s in enumerate(ids):
        applied[k], tries[k], box = draw(seed, epoch, int(s), p, scale, ratio, H, W)
        if applied[k] and box is not None:
            boxes[k] = box
        keys[k] = hash3(seed, epoch, int(s), 22)
    return boxes, keys, applied, tries


_T = None


def table(mean, std, dtype):
    global _T
    if _T is None:
        nd = statistics.NormalDist()
        _T = np.array([nd.inv_cdf((k + 0.5) / 4096) for k in range(4096)], np.float64)
    t = mean + std * _T
    if np.dtype(dtype) == np.uint8:
        return np.clip(np.rint(t), 0, 255).astype(np.uint8)
    return t.astype(dtype)


def _splitmix64_np(x):
    z = x + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def noise_indices(key, n_elements):
    """The table index of every element 0 .. n_elements - 1 of a sample."""
    e = np.arange(n_elements, dtype=np.uint64)
    with np.errstate(over='ignore'):
        word = _splitmix64_np(np.uint64(key) ^ (e >> np.uint64(2)))
    return ((word >> (np.uint64(16) * (e & np.uint64(3)) + np.uint64(4))) & np.uint64(0xFFF)).astype(np.int64)


def clamp(box, H, W):
    """(y1, y2, x1, x2) of a (y, x, h, w) box inside the image, or None."""
    y, x, h, w = (int(v) for v in box)
    if h <= 0 or w <= 0:
        return None
    y1, y2 = min(max(y, 0), H), min(max(y + h, 0), H)
    x1, x2 = min(max(x, 0), W), min(max(x + w, 0), W)
    return (y1, y2, x1, x2) if y1 < y2 and x1 < x2 else None


def erase(images, boxes, layout, value=None, tab=None, keys=None):
    """A copy of images, (n, H, W, C) for layout 'hwc' or planar (n, C, H, W)
    for 'chw', with the (y, x, h, w) boxes (clamped here) filled: with
    ``value`` (a scalar or C values of the images' dtype), or with entries of
    ``tab`` chosen by ``keys`` and the element's index in storage order."""
    images = np.asarray(images)
    out = images.copy()
    n = images.shape[0]
    H, W = images.shape[1:3] if layout == 'hwc' else images.shape[2:4]
    C = images.shape[3] if layout == 'hwc' else images.shape[1]
    for i in range(n):
        b = clamp(boxes[i], H, W)
        if b is None:
            continue
        y1, y2, x1, x2 = b
        region = (slice(y1, y2), slice(x1, x2)) if layout == 'hwc' else (slice(None), slice(y1, y2), slice(x1, x2))
        if tab is not None:
            fill = np.asarray(tab)[noise_indices(keys[i], images[i].size)].reshape(images[i].shape)
            out[i][region] = fill[region]
        else:
            v = np.broadcast_to(np.asarray(value, images.dtype).reshape(-1), (C,))
            out[i][region] = v if layout == 'hwc' else v[:, None, None]
    return out


# ---- the cases shared by the CPU and the GPU tests ----
# (H, W, scale) with the default ratio, for ids 0..255, seed 7, epoch 1, p = 0.5
DRAW_CASES = ((32, 32, DEFAULT_SCALE), (7, 5, DEFAULT_SCALE), (2, 2, DEFAULT_SCALE), (3, 50, DEFAULT_SCALE),
              (32, 32, (0.85, 1.0)), (224, 224, DEFAULT_SCALE))
DRAW_IDS = np.arange(256, dtype=np.uint64)
DRAW_SEED, DRAW_EPOCH, DRAW_P = 7, 1, 0.5
MODES = ('scalar', 'channel', 'noise')
FILL_DTYPES = {1: np.uint8, 2: np.float16, 4: np.float32}       # what a table of an itemsize holds
NOISE = {1: (128.0, 64.0), 2: (0.0, 1.0), 4: (0.0, 1.0)}


def hand_boxes(H, W):
    """(y, x, h, w): empty, one element, a full row minus one column, a full
    column minus one row, the whole image, boxes out of range on every side,
    and x swept over 0..W-1 (to the row's end and one pixel wide)."""
    b = [(0, 0, 0, 0), (1, 1, 0, 5), (2, 2, -3, 4), (H // 2, W // 2, 1, 1), (0, 0, 1, 1), (H - 1, W - 1, 1, 1),
         (H // 2, 0, 1, W - 1), (H // 2, 1, 1, W - 1), (0, W // 2, H - 1, 1), (1, W // 2, H - 1, 1), (0, 0, H, W),
         (-7, -9, H + 14, W + 18), (-3, 2, 5, 3), (H - 2, 1, 9, 2), (1, -4, 2, 6), (1, W - 2, 3, 40),
         (H + 1, W + 1, 4, 4), (-20, 0, 5, 5), (-2**31, -2**31, 2**31 - 1, 2**31 - 1), (2**31 - 1, 2**31 - 1, 2**31 - 1,
                                                                                       2**31 - 1)]
    b += [(1, x, max(H - 2, 1), W - x) for x in range(W)]
    b += [(0, x, H, 1) for x in range(W)]
    return np.array(b, np.int64).astype(np.int32)


def fill_case(rng, mode, itemsize, C):
    """What one fill needs: (value in the images' unsigned dtype or None, the
    table viewed in it or None, keys or None) -- the fills move bytes, so the
    tests run them on unsigned integers of the itemsize."""
    udt = {1: np.uint8, 2: np.uint16, 4: np.uint32}[itemsize]
    if mode == 'noise':
        return None, table(*NOISE[itemsize], FILL_DTYPES[itemsize]).view(udt), True
    top = int(np.iinfo(udt).max)
    value = rng.integers(0, top, 1 if mode == 'scalar' else C, dtype=np.uint64).astype(udt)
    return value, None, False
