"""The mixup semantics stated in numpy, independent of the package: per batch,
in float64, with the RandomState draw.  Shared by test_mixup.py (CPU) and
test_mixup_gpu.py."""
import numpy as np

# lambdas at which a float32 evaluation, a lerp evaluation and a fused
# multiply-add each differ from the float64 statement on the all-pairs image
FIXED_LAMBDAS = (0.0, 1.0, 0.5, 0.3, 0.7, 1 / 3, 0.1, 0.9999999, 1e-12)


def draw_lambdas(last_index, alpha, same_lambda, n):
    """One batch's lambdas: float64 scalar (same_lambda) or float64 (n,)."""
    rs = np.random.RandomState(int(last_index))
    return rs.beta(alpha, alpha) if same_lambda else rs.beta(alpha, alpha, n)


def mix_one_batch(images, lam):
    """images (B, ...) of any dtype, lam a scalar or (B,): the mixed batch in
    the images' dtype (astype truncates into integers and rounds to nearest
    even into float32)."""
    images = np.asarray(images)
    B = images.shape[0]
    lam = np.broadcast_to(np.asarray(lam, np.float64), (B,))
    out = np.empty_like(images)
    for i in range(B):
        l = np.float64(lam[i])
        a = images[i].astype(np.float64)
        b = images[i - 1].astype(np.float64)    # i = 0: the batch's last sample
        out[i] = (l * a + (1 - l) * b).astype(images.dtype)
    return out


def segments(n, batch_size):
    return [(lo, min(n, lo + batch_size)) for lo in range(0, n, batch_size)]


def mix_segments(images, lam, batch_size, same_lambda):
    """A launch of several batches with given lambdas (one per batch when
    same_lambda, else one per sample)."""
    out = np.empty_like(images)
    for s, (lo, hi) in enumerate(segments(len(images), batch_size)):
        out[lo:hi] = mix_one_batch(images[lo:hi], lam[s] if same_lambda else lam[lo:hi])
    return out


def image_mixup(images, indices, alpha, same_lambda, batch_size=None):
    """ImageMixup of a launch: batches of batch_size (default: one batch),
    each drawn from its own last index."""
    n = len(images)
    out = np.empty_like(images)
    for lo, hi in segments(n, batch_size or n):
        out[lo:hi] = mix_one_batch(images[lo:hi], draw_lambdas(indices[hi - 1], alpha, same_lambda, hi - lo))
    return out


def label_mixup(labels, indices, alpha, same_lambda, batch_size=None):
    """float32 (n, 3): [label_i, label_{i-1}, lam_i] per batch."""
    labels = np.asarray(labels).reshape(len(indices), -1)[:, 0]
    n = len(labels)
    out = np.empty((n, 3), np.float32)
    for lo, hi in segments(n, batch_size or n):
        seg = labels[lo:hi]
        out[lo:hi, 0] = seg
        out[lo:hi, 1] = np.roll(seg, 1)
        out[lo:hi, 2] = draw_lambdas(indices[hi - 1], alpha, same_lambda, hi - lo)
    return out


def one_hot(labels3, num_classes):
    """float32 (n, num_classes): zeros, [a] = lam, then [b] = float32(1) - lam."""
    labels3 = np.asarray(labels3, np.float32)
    out = np.zeros((len(labels3), num_classes), np.float32)
    for i, (a, b, lam) in enumerate(labels3):
        out[i, int(a)] = lam
        out[i, int(b)] = np.float32(1) - lam
    return out


def all_pairs():
    """(2, 65536) uint8: element j of sample 0 is j >> 8, of sample 1 j & 255,
    so the two samples hold every (a, b) byte pair."""
    j = np.arange(65536)
    return np.stack([(j >> 8).astype(np.uint8), (j & 255).astype(np.uint8)])


def all_pairs_lambdas():
    """The fixed set plus 16 beta draws."""
    rs = np.random.RandomState(1234)
    draws = np.concatenate([rs.beta(a, a, 4) for a in (0.2, 0.5, 1.0, 2.0)])
    return np.concatenate([np.array(FIXED_LAMBDAS, np.float64), draws])


# ---- the shape / segmentation cases shared by the CPU and the GPU tests ----
def random_inputs(rng, n, elems, dtype):
    """(n, elems) uint8, or float32 over 33 decades with negative and large values."""
    if dtype == np.uint8:
        return rng.integers(0, 256, (n, elems), dtype=np.uint8)
    x = (rng.standard_normal((n, elems)) * 10.0 ** rng.integers(-3, 30, (n, elems))).astype(np.float32)
    x.reshape(-1)[::7] = -np.abs(x.reshape(-1)[::7])
    x.reshape(-1)[:1] = np.float32(3.0e38)
    return x


def random_lambdas(rng, n, batch_size, same):
    m = -(-n // batch_size) if same else n
    lam = rng.beta(0.5, 0.5, m)
    lam[::3] = rng.choice(FIXED_LAMBDAS, lam[::3].shape)
    return lam


SEGMENT_CASES = [(1, 1), (2, 2), (3, 3), (67, 67), (10, 4), (10, 10), (10, 16), (10, 1)]   # (n, batch_size)
ELEMS = (1, 3, 7, 3072, 4095, 4096, 4097)
