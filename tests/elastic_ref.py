"""The ElasticTransform contract as plain numpy: the sample's
64-bit key, the per-pixel hash noise, the integer Gaussian with a reflect
border, the displacement, and the integer sample of tests/affine_ref.py."""
import numpy as np

from ffcv_amd.transforms.rng import M64, splitmix64
from tests import affine_ref as A

OP_ELASTIC = 27


def key(seed, epoch, sid):
    h = splitmix64((int(seed) & M64) ^ (OP_ELASTIC << 56))
    return splitmix64(splitmix64(h ^ (int(epoch) & M64)) ^ (int(sid) & M64))


def _splitmix64(x):
    """splitmix64 on a uint64 array (the arithmetic wraps)."""
    z = x + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def noise(k, H, W):
    """int64 (2, H, W): axis x, axis y, Q15 of [-1, 1)."""
    e = 2 * np.arange(H * W, dtype=np.uint64).reshape(1, H, W) + np.arange(2, dtype=np.uint64).reshape(2, 1, 1)
    word = _splitmix64(np.uint64(k) ^ (e >> np.uint64(2)))
    return ((word >> (np.uint64(16) * (e & np.uint64(3)))) & np.uint64(0xFFFF)).astype(np.int64) - 32768


def weights(sigma):
    """int64 (2 R + 1,) summing to 65536."""
    k = int(8 * float(sigma) + 1)
    k += k % 2 == 0
    R = (k - 1) // 2
    x = [np.float64(i) / np.float64(sigma) for i in range(R + 1)]
    g = [float(np.exp(np.float64(-0.5) * (v * v))) for v in x]
    total = 0.0
    for i in range(-R, R + 1):
        total += g[abs(i)]
    w = [int(np.floor(65536.0 * g[abs(i)] / total + 0.5)) for i in range(-R, R + 1)]
    w[R] += 65536 - sum(w)
    return np.array(w, np.int64)


def _blur(a, w, axis):
    R = len(w) // 2
    pad = [(0, 0)] * a.ndim
    pad[axis] = (R, R)
    p = np.pad(a, pad, mode='reflect')
    n = a.shape[axis]
    return sum(int(w[i]) * np.take(p, np.arange(i, i + n), axis=axis) for i in range(2 * R + 1))


def coordinates(k, H, W, alpha, sigma):
    """(X, Y), int64 (H, W), Q16."""
    w = weights(sigma)
    h16 = (_blur(noise(k, H, W), w, 2) + 32768) >> 16
    v = _blur(h16, w, 1)
    assert np.abs(v).max() < 2 ** 31
    d = (int(np.floor(float(alpha) * 128 + 0.5)) * v + (1 << 22)) >> 23
    r, c = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing='ij')
    return (c << 16) + d[0], (r << 16) + d[1]


def warp(img, k, alpha, sigma, mode, fill=(0, 0, 0)):
    """One uint8 (H, W, 3) image under key k."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape[:2]
    fill = np.broadcast_to(np.asarray(fill).astype(np.uint8).reshape(-1), (3,)).astype(np.int64)
    Xq, Yq = coordinates(k, H, W, alpha, sigma)
    if mode == A.NEAREST:
        return A._taps(img, (Yq + 32768) >> 16, (Xq + 32768) >> 16, fill).astype(np.uint8)
    ix, iy = Xq >> 16, Yq >> 16
    fx, fy = ((Xq & 0xFFFF) >> 8)[:, :, None], ((Yq & 0xFFFF) >> 8)[:, :, None]
    top = (256 - fx) * A._taps(img, iy, ix, fill) + fx * A._taps(img, iy, ix + 1, fill)
    bot = (256 - fx) * A._taps(img, iy + 1, ix, fill) + fx * A._taps(img, iy + 1, ix + 1, fill)
    return (((256 - fy) * top + fy * bot + 32768) >> 16).astype(np.uint8)


def warp_batch(imgs, seed, epoch, ids, alpha, sigma, mode, fill=(0, 0, 0)):
    return np.stack([warp(im, key(seed, epoch, i), alpha, sigma, mode, fill) for im, i in zip(imgs, ids)])
